"""The MOT layer's restatement (tests/mot_py.py) against the reference's own code
(tests/golden/mot_kat.npz, written by make_mot_golden.py from mot-data.cpp compiled where it
lies, under the address and undefined-behaviour sanitizers), the host motAssembler
(host/msc_consumers.cpp, through tests/cpp/mot_wrap.cpp) against both, the rules where the
reference is undefined or unbounded on cases outside the golden file, and what the library and
the binding export."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mot_py as mp
import packet_py as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sdr-j-dab_amd")
WRAP = os.path.join(ROOT, "tests", "cpp", "build", "libmotwrap.so")
KAT = os.path.join(ROOT, "tests", "golden", "mot_kat.npz")


@pytest.fixture(scope="module")
def kat():
    z = np.load(KAT)
    out = []
    for i, name in enumerate(z["names"]):
        ev, names, bodies = z["events_%d" % i], z["event_names_%d" % i].tobytes(), z["event_bodies_%d" % i].tobytes()
        events, npos, bpos = [], 0, 0
        for g, kind, sub, nl, bl in ev.tolist():
            events.append(dict(group=g, kind=kind, subtype=sub, name=names[npos:npos + nl], body=bodies[bpos:bpos + bl]))
            npos, bpos = npos + nl, bpos + bl
        out.append(dict(name=str(name), groups=np.frombuffer(z["groups_%d" % i].tobytes(), pp.GROUP_DTYPE),
                        bytes=z["bytes_%d" % i], events=events))
    return out


@pytest.fixture(scope="module")
def wrap():
    # built here when build()'s copy is not there (as test_consumers_cpu builds its library)
    subprocess.run(["make", "-s", "-f", os.path.join(ROOT, "tests", "cpp", "Makefile.mot"), WRAP], check=True)
    l = C.CDLL(WRAP)
    l.mw_new.restype = C.c_void_p
    l.mw_new.argtypes = [C.c_int]
    l.mw_free.argtypes = [C.c_void_p]
    l.mw_group.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    l.mw_count.argtypes = [C.c_void_p]
    l.mw_object.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    l.mw_counters.argtypes = [C.c_void_p, C.c_void_p]
    return l


def host_run(l, groups, cap=mp.BODY_BYTES):
    """the host motAssembler over whole groups (as bytes) -> (objects as dicts, counters)"""
    h = l.mw_new(cap)
    try:
        for g in groups:
            l.mw_group(h, bytes(g), len(g))
        out = []
        for i in range(l.mw_count(h)):
            info = np.zeros(7, np.int32)
            name, body = np.zeros(max(1, 1 << 12), np.uint8), np.zeros(max(1, 1 << 17), np.uint8)
            assert l.mw_object(h, i, info.ctypes.data, name.ctypes.data, name.size, body.ctypes.data, body.size) == 0
            assert info[5] <= name.size and info[6] <= body.size
            out.append(dict(group=int(info[0]), kind=int(info[1]), transportId=int(info[2]), contentType=int(info[3]),
                            contentsubType=int(info[4]), name=name[:info[5]].tobytes(), body=body[:info[6]].tobytes()))
        cnt = np.zeros(4, np.int32)
        l.mw_counters(h, cnt.ctypes.data)
        return out, cnt.tolist()
    finally:
        l.mw_free(h)


def restated(groups, cap=mp.BODY_BYTES):
    rec, arena = mp.pack(groups)
    a = mp.Assembler(cap)
    a.feed(rec, arena)
    return a


def test_golden_file_holds_the_fixtures(kat):
    fx = mp.fixtures()
    assert [f["name"] for f in fx] == [k["name"] for k in kat] and len(kat) == 12
    for f, k in zip(fx, kat):
        rec, arena = mp.pack(f["groups"])
        assert rec.tobytes() == k["groups"].tobytes() and np.array_equal(arena, k["bytes"]), f["name"]
    assert os.path.getsize(KAT) < 200 * 1024


def test_fixtures_keep_the_reference_inside_its_arrays(kat):
    """what the sanitizer run proved, restated: segment numbers < 100, bodies <= 32767 bytes,
    segmentSize + 2 <= data length, header size <= segment size for a combined header; and no
    delivered body holds the 0xEE the stub's resize fills with except where a fixture put it"""
    for k in kat:
        a = mp.Assembler()
        a.feed(k["groups"], k["bytes"])
        assert a.malformed == 0 and a.bad_segment == 0, k["name"]
        for r in k["groups"]:
            if r["flags"] & (pp.ACCEPTED | pp.TID) != (pp.ACCEPTED | pp.TID) or r["groupType"] not in (3, 4):
                continue
            d = k["bytes"][r["offset"] + r["data_offset"]:][:r["data_nbytes"]]
            size = (int(d[0]) & 0x1F) << 8 | int(d[1])
            assert r["segmentNumber"] < 100 and size + 2 <= len(d)
            if r["groupType"] == 3 and r["segmentNumber"] == 0:
                assert (int(d[2]) << 20 | int(d[3]) << 12 | int(d[4]) << 4 | int(d[5]) >> 4) <= 32767
                if not r["flags"] & pp.LAST:
                    assert ((int(d[5]) & 15) << 9 | int(d[6]) | int(d[7]) >> 7) <= size


def test_restatement_equals_reference(kat):
    """every fixture: each slide and file the reference delivered -- during which group, the
    contentsubType the_picture got, the name, the body byte for byte -- and nothing else but
    the EPG objects, which the reference completes and drops"""
    shown = {}
    for k in kat:
        a = mp.Assembler()
        objs = a.feed(k["groups"], k["bytes"])
        mine = [o for o in objs if o["kind"] != mp.EPG]
        assert len(mine) == len(k["events"]), k["name"]
        for o, e in zip(mine, k["events"]):
            assert (o["group"], o["kind"], o["body"]) == (e["group"], e["kind"], e["body"]), k["name"]
            assert o["name_len"] == len(e["name"]) and o["name"] == e["name"][:mp.NAME_BYTES], k["name"]
            if o["kind"] == mp.SLIDE:
                assert o["contentsubType"] == e["subtype"], k["name"]
        shown[k["name"]] = [(o["kind"], o["transportId"]) for o in objs]
    S, E, F = mp.SLIDE, mp.EPG, mp.FILE
    assert shown["in_order"] == [(S, 0x0101)] and shown["combined"] == [(S, 0x0202)]
    assert shown["last_first"] == [(S, 0x0303)]
    assert shown["repeats"] == [(S, 0x0404), (S, 0x0405), (S, 0x0405)]      # the first slide once, the second twice
    assert shown["interleaved"] == [(S, 0x0501)]                            # the other lacks a segment
    ev = shown["evict"]
    assert 0x0600 not in [t for _, t in ev[:16]] and ev[16] == (S, 0x0600) and len(ev) == 17
    assert [t for _, t in ev].count(0x0601) == 1                            # its second tenant inherits marks
    assert F in [k for k, _ in ev]
    assert shown["duplicate"] == [(S, 0x0707)] and shown["size_check"] == [(S, 0x0808)]
    assert shown["epg"] == [(E, 0x0909)] and shown["file"] == [(F, 0x0A0A)]
    assert shown["other_types"] == [(S, 0x0B0B)] and shown["filtered"] == [(S, 0x0C0C)]


def test_restatement_details(kat):
    by = {k["name"]: k for k in kat}
    a = mp.Assembler()
    o = a.feed(by["combined"]["groups"], by["combined"]["bytes"])[0]
    assert o["nbytes"] == 432 and o["name"] == b"combined.png" and o["contentsubType"] == 3
    assert a.table[0].segmentSize == 465 - 133          # the reference's header size, not the field's 265
    a = mp.Assembler()
    o = a.feed(by["file"]["groups"], by["file"]["bytes"])[0]
    assert o["name"] == b"dir_file.html" and o["contentType"] == 1
    a = mp.Assembler()
    a.feed(by["duplicate"]["groups"], by["duplicate"]["bytes"])
    assert a.objects[0]["name"] == b"one" and a.objects[0]["nbytes"] == 200
    # other_types is the layer's own rule 6, not the reference's: the golden generator keeps the
    # type 6 groups from the reference (its directory code reads entries nothing initialised), so
    # the golden file pins only that the objects around them are delivered as if they were not there
    a = mp.Assembler()
    a.feed(by["other_types"]["groups"], by["other_types"]["bytes"])
    assert a.other_types == 4
    a = mp.Assembler()
    a.feed(by["evict"]["groups"], by["evict"]["bytes"])
    assert a.created == 19 and a.run_record()["entries"] == 16


def test_host_assembler_equals_restatement_and_reference(kat, wrap):
    for f in mp.fixtures() + mp.rule_cases():
        cap = f.get("cap", mp.BODY_BYTES)
        a = restated(f["groups"], cap)
        got, cnt = host_run(wrap, f["groups"], cap)
        want = [dict(group=o["group"], kind=o["kind"], transportId=o["transportId"], contentType=o["contentType"],
                     contentsubType=o["contentsubType"], name=a_name, body=o["body"])
                for o, a_name in zip(a.objects, _full_names(f["groups"], a))]
        assert got == want, f["name"]
        r = a.run_record()
        assert cnt == [r["malformed"], r["bad_segment"], r["other_types"], r["entries"]], f["name"]
    for k in kat:                                       # and the reference directly
        got, _ = host_run(wrap, [g for g in mp.fixtures() if g["name"] == k["name"]][0]["groups"])
        got = [o for o in got if o["kind"] != mp.EPG]
        assert [(o["group"], o["kind"], o["name"], o["body"]) for o in got] == \
            [(e["group"], e["kind"], e["name"], e["body"]) for e in k["events"]], k["name"]


def _full_names(groups, a):
    """the full names of a's objects (the record keeps 128 bytes; the entry keeps all)"""
    full = {}
    b = mp.Assembler(a.cap)
    rec, arena = mp.pack(groups)
    orig = b.complete

    def spy(e, g, cif):
        full[len(b.objects)] = e.name
        orig(e, g, cif)
    b.complete = spy
    b.feed(rec, arena)
    return [full[i] for i in range(len(b.objects))]


def test_restatement_rules_outside_the_golden_file():
    """pins the restatement mot_py.Assembler, the yardstick of the GPU tests, on rules 1 to 5 --
    not the product code: the host motAssembler is held to these cases through its equality with
    the restatement (test_host_assembler_equals_restatement_and_reference runs rule_cases()
    too), the GPU layer in test_gpu_mot"""
    cases = {c["name"]: c for c in mp.rule_cases()}
    # 1: a one-byte data field and a segment size past the data are dropped and counted; header
    #    fields past the end read 0 (an entry with contentType 0 and body size 25600)
    a = restated(cases["rule1"]["groups"])
    assert a.malformed == 2 and [o["transportId"] for o in a.objects] == [0x1111]
    e = a.handle(0x1112)
    assert e is not None and (e.bodySize, e.contentType, e.contentsubType, e.name) == (25600, 0, 0, b"")
    # 2: segment numbers >= 100 are dropped and counted; 0..99 complete the object
    a = restated(cases["rule2"]["groups"])
    assert a.bad_segment == 2 and len(a.objects) == 1 and a.objects[0]["nbytes"] == 101
    assert a.objects[0]["body"][100:] == b"\x00" and a.handle(0x2222).numofSegments == 100
    # 3: a 40 000-byte body completes (the reference's int16_t size would be negative) ...
    c = cases["rule3_big"]
    a = restated(c["groups"])
    want = b"".join(pp.parse_group(g)["stored"][pp.parse_group(g)["data_offset"] + 2:-2] for g in c["groups"][1:])
    assert len(a.objects) == 1 and a.objects[0]["body"] == want and len(want) == 40000
    # ... and one above max_body_bytes gets a flagged entry whose segments are ignored, while
    # one of exactly max_body_bytes is delivered
    a = restated(cases["rule3_too_large"]["groups"], 4096)
    assert [o["transportId"] for o in a.objects] == [0x3335] and a.handle(0x3334).flags == mp.TOO_LARGE
    assert a.created == 2 and not a.handle(0x3334).marked[0]
    # 4: unwritten bytes read 0; a combined header whose header size exceeds its segment
    #    creates the entry and drops the body part
    a = restated(cases["rule4"]["groups"])
    assert [o["transportId"] for o in a.objects] == [0x4444, 0x4446]
    assert a.objects[1]["body"][40:] == bytes(40) and a.objects[1]["nbytes"] == 80
    e = a.handle(0x4445)
    assert e.segmentSize == -1 and not any(e.marked)
    # 5: the record keeps 128 name bytes, name_len counts them all
    a = restated(cases["rule5"]["groups"])
    o = a.objects[0]
    assert o["name_len"] == 304 and len(o["name"]) == 128 and o["name"] == bytes(65 + i % 26 for i in range(128))
    assert o["kind"] == mp.FILE
    # the output arena: an object that does not fit is recorded without bytes
    rec, arena = mp.pack(cases["rule4"]["groups"])
    a = mp.Assembler()
    a.feed(rec, arena, out_arena=320)
    assert [(o["flags"], o["nbytes"]) for o in a.run_objects] == [(0, 300), (mp.OVERFLOW, 0)]


def test_state_is_carried_across_feeds(kat):
    """split at every group boundary: two feeds deliver what one does"""
    for k in kat:
        whole = mp.Assembler()
        whole.feed(k["groups"], k["bytes"])
        for cut in range(len(k["groups"]) + 1):
            a = mp.Assembler()
            a.feed(k["groups"][:cut], k["bytes"])
            a.feed(k["groups"][cut:], k["bytes"])
            assert [(o["transportId"], o["body"]) for o in a.objects] == \
                [(o["transportId"], o["body"]) for o in whole.objects], (k["name"], cut)


def test_fib_subchannels_flag_mot_components():
    """tests/cpp/test_fib_mot.cpp: the transmitter's FIBs with DSCTy 60 components, what
    ensembleDecoder's auto_layout asks fib_processor::subchannels for when on_mot_object is set"""
    import subprocess
    exe = os.path.join(ROOT, "tests", "cpp", "build", "test_fib_mot")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(PKG, "host"),
                    "-I" + os.path.join(PKG, "synth"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_fib_mot.cpp"),
                    os.path.join(PKG, "host", "fib_processor.cpp"), "-L" + os.path.join(PKG, "lib"), "-ldabsynth",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FIB MOT OK" in r.stdout, r.stdout + r.stderr


def test_library_and_binding_export_the_layer():
    import sys
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import dabamd
    l = dabamd.lib()
    for name in ("dabgpu_mot_groups", "dabgpu_mot_state_bytes", "dabgpu_pipe_mot", "dabgpu_pipe_mot_caps"):
        assert hasattr(l, name), name
    assert dabamd.SUBCH_MOT == 16 and dabamd.MOT_OBJECT_DTYPE == mp.OBJECT_DTYPE and dabamd.MOT_RUN_DTYPE == mp.RUN_DTYPE
    assert dabamd.MOT_OBJECT_DTYPE.itemsize == 156 and dabamd.MOT_RUN_DTYPE.itemsize == 32 and mp.ENTRY_DTYPE.itemsize == 184
    for cap in (0, 1, 4096, 40000, 65536):
        assert dabamd.mot_state_bytes(cap) == mp.state_bytes(cap or mp.BODY_BYTES)
    assert dabamd.mot_state_bytes(-1) == 0 and dabamd.mot_state_bytes((1 << 24) + 1) == 0
    assert dabamd.mot_arena_bytes(7, 100) == mp.arena_bytes(7, 100) == 112 + 7 * 144
    assert callable(dabamd.mot_groups) and callable(dabamd.Pipeline.mot) and callable(dabamd.Pipeline.mot_caps)
    hdr = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    for word in ("#define DABGPU_SUBCH_MOT     16", "DABGPU_MOT_BODY_BYTES 65536", "DABGPU_MOT_NAME_BYTES 128",
                 "(group_slots) * 144", "#define DABGPU_ABI_VERSION 7"):
        assert word in hdr, word
