"""The IP layer's restatement (tests/ip_py.py) against the reference's own code
(tests/golden/ip_kat.npz, written by make_ip_golden.py from ip-datahandler.cpp compiled where it
lies, under the address and undefined-behaviour sanitizers), the host ipAssembler
(host/msc_consumers.cpp, through tests/cpp/ip_wrap.cpp and as a stand-alone program under the
sanitizers) against both, the rules where the reference is undefined on cases outside the golden
file, the synthesiser's IP content, and what the library and the binding export."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ip_py as ip
import packet_py as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sdr-j-dab_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
WRAP = os.path.join(BUILD, "libipwrap.so")
SANITIZE = os.path.join(BUILD, "ip_sanitize")
MAKEFILE = os.path.join(ROOT, "tests", "cpp", "Makefile.ip")
KAT = os.path.join(ROOT, "tests", "golden", "ip_kat.npz")
SEEDS = range(200)


@pytest.fixture(scope="module")
def kat():
    z = np.load(KAT)
    out = []
    for i, name in enumerate(z["names"]):
        data, pos, events = z["event_bytes_%d" % i].tobytes(), 0, []
        for g, kind, value in z["events_%d" % i].tolist():
            events.append((g, kind, value, data[pos:pos + value] if kind == 0 else b""))
            pos += value if kind == 0 else 0
        out.append(dict(name=str(name), groups=np.frombuffer(z["groups_%d" % i].tobytes(), pp.GROUP_DTYPE),
                        bytes=z["bytes_%d" % i], events=events))
    return out


@pytest.fixture(scope="module")
def wrap():
    # built here when build()'s copy is not there (as test_mot_cpu builds its library)
    subprocess.run(["make", "-s", "-f", MAKEFILE, WRAP], check=True)
    l = C.CDLL(WRAP)
    l.iw_new.restype = C.c_void_p
    l.iw_new.argtypes = [C.c_int, C.c_int]
    l.iw_free.argtypes = [C.c_void_p]
    l.iw_group.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    l.iw_counters.argtypes = [C.c_void_p, C.c_void_p]
    return l


@pytest.fixture(scope="module")
def random_slots():
    """(groups, handled, crc_errors) per seed: the handlers start anywhere in their window"""
    out = []
    for seed in SEEDS:
        rng = np.random.default_rng(10_000 + seed)
        out.append((ip.random_groups(seed), int(rng.integers(0, 100)), int(rng.integers(0, 20))))
    return out


def restated(groups, handled=0, crc_errors=0):
    """ip_py over whole groups -> ([(status, quality, ip_bytes, payload or None)], handler, run)"""
    rec, arena = ip.pack(groups)
    h = ip.Handler(handled, crc_errors)
    res, out, run = h.feed(rec, arena)
    rows = [(int(r["status"]), int(r["quality"]), int(r["ip_bytes"]),
             out[r["offset"]:r["offset"] + r["nbytes"]].tobytes() if r["status"] == ip.DELIVERED else None) for r in res]
    return rows, h, run


def host_run(l, groups, handled=0, crc_errors=0):
    """the host ipAssembler over whole groups (as bytes) -> (rows as restated(), counters)"""
    h = l.iw_new(handled, crc_errors)
    try:
        rows = []
        for g in groups:
            info, pay = np.zeros(5, np.int32), np.zeros(1 << 16, np.uint8)
            n = l.iw_group(h, bytes(g), len(g), info.ctypes.data, pay.ctypes.data, pay.size)
            assert n == (1 if info[0] == ip.DELIVERED else 0) and info[4] == info[1]
            rows.append((int(info[0]), int(info[1]), int(info[2]), pay[:info[3]].tobytes() if n else None))
        cnt = np.zeros(9, np.int32)
        l.iw_counters(h, cnt.ctypes.data)
        return rows, cnt.tolist()
    finally:
        l.iw_free(h)


def test_golden_file_holds_the_fixtures(kat):
    fx = ip.fixtures()
    assert [f["name"] for f in fx] == [k["name"] for k in kat] and len(kat) == 9
    for f, k in zip(fx, kat):
        rec, arena = ip.pack(f["groups"])
        assert rec.tobytes() == k["groups"].tobytes() and np.array_equal(arena, k["bytes"]), f["name"]
    assert os.path.getsize(KAT) < 200 * 1024


def test_fixtures_keep_the_reference_inside_its_arrays(kat):
    """what the sanitizer run proved, restated: every group the reference went on with holds its
    length field, and every datagram it copied lies inside the group and holds the bytes
    process_ipVector reads (the header, byte 9)"""
    for k in kat:
        for r in k["groups"]:
            if not r["flags"] & pp.ACCEPTED:
                continue
            nb, nxt = int(r["nbytes"]), int(r["data_offset"])
            assert nxt + 4 <= nb, k["name"]
            d = k["bytes"][r["offset"]:r["offset"] + nb]
            ln = int(d[nxt + 2]) << 8 | int(d[nxt + 3])
            if ln < nb:
                assert 0 < ln and nxt + ln <= nb, k["name"]
                if d[nxt] >> 4 == 4:
                    assert ln >= 10 and ln >= 4 * (int(d[nxt]) & 15), k["name"]


def test_restatement_equals_reference(kat):
    """every fixture: each writeDatagram (during which group, the bytes) and each show_ipErrors
    (during which group, the value) of the reference, in order, and nothing else"""
    seen = {}
    for k in kat:
        h = ip.Handler()
        res, out, run = h.feed(k["groups"], k["bytes"])
        mine = []
        for g, r in enumerate(res):
            if r["quality"] >= 0:
                mine.append((g, 1, int(r["quality"]), b""))
            if r["status"] == ip.DELIVERED:
                mine.append((g, 0, int(r["nbytes"]), out[r["offset"]:r["offset"] + r["nbytes"]].tobytes()))
        assert mine == k["events"], k["name"]
        seen[k["name"]] = (res["status"].tolist(), h)
    D, NA, TL, V4, CS, UDP = ip.DELIVERED, ip.NOT_ACCEPTED, ip.TOO_LONG, ip.NOT_V4, ip.CHECKSUM, ip.NOT_UDP
    assert seen["plain"][0] == [D] * 8 and seen["group_crc"][0] == [D, NA, D]
    assert seen["lengths"][0] == [D, TL, D, TL]                  # nbytes - 2 taken, nbytes refused
    assert seen["versions"][0] == [V4, V4, D, V4, V4, D]         # 6, 0xC, 4, 0, 5, 4
    assert seen["header_sizes"][0] == [CS, D, D, D, D, D]        # 0 sums to 0 and fails; 5 .. 8 and 15
    assert seen["checksums"][0] == [CS, CS, D, CS]               # the first: only a second fold would give 0xFFFF or not
    assert seen["protocols"][0] == [UDP, D, UDP, D]
    assert seen["crc_overlap"][0] == [D, D]
    h = seen["window"][1]
    assert h.qualities == [97, 97] and (h.handled, h.crc_errors) == (30, 1)


def test_crc_overlap_reads_the_complement(kat):
    """rule 1's second half, pinned on the reference: the payload's last two bytes are the group's
    CRC bytes inverted, not as the packet layer stores them"""
    k = [k for k in kat if k["name"] == "crc_overlap"][0]
    datagrams = [e for e in k["events"] if e[1] == 0]
    assert len(datagrams) == 2
    for (g, _, n, data), tail in zip(datagrams, (2, 1)):
        r = k["groups"][g]
        stored = k["bytes"][r["offset"]:r["offset"] + r["nbytes"]]
        crc = stored[-2:][:tail]
        assert data[-tail:] == bytes(int(b) ^ 0xFF for b in crc) and data[-tail:] != crc.tobytes()


def test_restatement_rules_outside_the_golden_file():
    """pins the restatement ip_py.Handler, the yardstick of the GPU tests, on rules 1 to 6 -- not the
    product code: the host ipAssembler is held to these cases through its equality with the
    restatement, the GPU layer in test_gpu_ip"""
    cases = {c["name"]: c for c in ip.rule_cases()}
    # 1: a length field past or across the group's end reads 0 there
    rows = restated(cases["short"]["groups"])[0]
    assert [r[0] for r in rows] == [ip.NOT_V4, ip.NOT_V4, ip.TOO_LONG, ip.CHECKSUM, ip.NOT_V4] and rows[2][2] == 256
    #    a datagram that runs past the group's end is zero-filled there, over the CRC complemented
    rows = restated(cases["overhang"]["groups"])[0]
    g = [pp.parse_group(x) for x in cases["overhang"]["groups"]]
    assert [r[0] for r in rows] == [ip.DELIVERED] * 3
    assert rows[0][3] == g[0]["stored"][2 + 28:] + b"\x00"
    assert rows[1][3] == g[1]["stored"][2 + 28:-2] + bytes(b ^ 0xFF for b in g[1]["stored"][-2:]) + b"\x00"
    assert rows[2][3][-4:] == bytes(4) and len(rows[2][3]) == 34
    # 2: ipLength 0 is no IPv4 and does not step the window
    rows, h, _ = restated(cases["zero_length"]["groups"])
    assert [r[0] for r in rows] == [ip.NOT_V4, ip.DELIVERED] and h.handled == 1
    # 3: the sum past ipLength reads 0; a negative payload length is counted after the window and
    #    checksum steps; payload length 0 is delivered
    rows, h, _ = restated(cases["header_past_length"]["groups"])
    assert [r[0] for r in rows] == [ip.MALFORMED, ip.MALFORMED, ip.CHECKSUM] and (h.handled, h.crc_errors) == (3, 1)
    rows, h, _ = restated(cases["negative_payload"]["groups"], handled=98)
    assert [r[:2] for r in rows] == [(ip.MALFORMED, -1), (ip.MALFORMED, 100), (ip.DELIVERED, -1)] and h.handled == 1
    assert restated([pp.group(ip.datagram(b""))])[0][0] == (ip.DELIVERED, -1, 28, b"")
    # 5: a record outside its arena
    rec, arena = ip.pack(cases["zero_length"]["groups"])
    rec[1]["offset"] = len(arena) - int(rec[1]["nbytes"]) + 1
    assert ip.Handler().feed(rec, arena)[0]["status"].tolist() == [ip.NOT_V4, ip.NOT_ACCEPTED]
    # 6: the output arena; offsets are multiples of 16 in group order
    rec, arena = ip.pack(ip.fixtures()[0]["groups"])
    res, out, run = ip.Handler().feed(rec, arena, out_arena=160)
    assert res["nbytes"].tolist() == [40, 33, 1, 17, 0, 0, 0, 0] and res["offset"].tolist() == [0, 48, 96, 112, 0, 0, 0, 0]
    assert res["status"].tolist() == [0, 0, 0, 0, 6, 6, 6, 6] and run["counts"][ip.MALFORMED] == 4 and run["n_bytes"] == 91


def test_state_is_carried_across_feeds(kat):
    """split at every tenth group boundary: two feeds deliver what one does"""
    k = [k for k in kat if k["name"] == "window"][0]
    whole = ip.Handler()
    want = whole.feed(k["groups"], k["bytes"])[0]
    for cut in range(0, len(k["groups"]) + 1, 10):
        a = ip.Handler()
        r1 = a.feed(k["groups"][:cut], k["bytes"])[0]
        r2 = a.feed(k["groups"][cut:], k["bytes"])[0]
        got = np.concatenate([r1, r2])
        for f in ("status", "quality", "nbytes", "ip_bytes"):
            assert np.array_equal(got[f], want[f]), (cut, f)
        assert a.datagrams == whole.datagrams and a.state() == whole.state()


def test_random_generator_reaches_every_status(random_slots):
    """per seed, on ip_py alone: at least a quarter of the groups delivered and every status met, so
    that the comparisons below cannot pass on refusals alone"""
    for seed, (groups, handled, crc) in zip(SEEDS, random_slots):
        rows, h, run = restated(groups, handled, crc)
        counts = run["counts"].tolist()
        assert counts[ip.DELIVERED] * 4 >= len(groups) and min(counts) >= 1, (seed, counts)
        assert sum(counts) == len(groups) and 60 <= len(groups) <= 130


def test_host_assembler_equals_restatement_and_reference(kat, wrap, random_slots):
    for f in ip.fixtures() + ip.rule_cases():
        rows, h, run = restated(f["groups"])
        got, cnt = host_run(wrap, f["groups"])
        assert got == rows, f["name"]
        assert cnt == [h.handled, h.crc_errors] + run["counts"].tolist(), f["name"]
    for seed, (groups, handled, crc) in zip(SEEDS, random_slots):
        rows, h, run = restated(groups, handled, crc)
        got, cnt = host_run(wrap, groups, handled, crc)
        assert got == rows and cnt == [h.handled, h.crc_errors] + run["counts"].tolist(), seed
    for k, f in zip(kat, ip.fixtures()):                # and the reference directly
        got, _ = host_run(wrap, f["groups"])
        ev = []
        for g, r in enumerate(got):
            if r[1] >= 0:
                ev.append((g, 1, r[1], b""))
            if r[0] == ip.DELIVERED:
                ev.append((g, 0, len(r[3]), r[3]))
        assert ev == k["events"], k["name"]


def test_host_assembler_under_the_sanitizers(tmp_path, random_slots):
    """the stand-alone program (its own main, -fsanitize=address,undefined) over every fixture, the
    rule cases and the random slots, each group as bits and as a heap block of exactly its length"""
    subprocess.run(["make", "-s", "-f", MAKEFILE, SANITIZE], check=True)
    slots = [(f["groups"], 0, 0) for f in ip.fixtures() + ip.rule_cases()] + list(random_slots)
    with open(tmp_path / "in.bin", "wb") as w:
        w.write(np.int32(len(slots)).tobytes())
        for groups, handled, crc in slots:
            w.write(np.array([handled, crc, len(groups)], np.int32).tobytes())
            for g in groups:
                w.write(np.int32(len(g)).tobytes() + bytes(g))
    r = subprocess.run([SANITIZE, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    raw, pos = open(tmp_path / "out.bin", "rb").read(), 0
    for groups, handled, crc in slots:
        rows, h, _ = restated(groups, handled, crc)
        for want in rows:
            st, q, ipb, n = np.frombuffer(raw, np.int32, 4, pos).tolist()
            pos += 16
            pay = raw[pos:pos + n] if n >= 0 else None
            pos += max(n, 0)
            assert (st, q, ipb, pay) == want
        assert np.frombuffer(raw, np.int32, 2, pos).tolist() == [h.handled, h.crc_errors]
        pos += 8
    assert pos == len(raw)


def test_synth_ip_content_decodes_to_its_datagrams():
    """DABSYNTH_IP through the host packet path (packet_py.Assembler on the transmitter's MSC bits)
    and ip_py: the groups are the carousel's in order, and the datagrams are the ones it was built
    from -- every seventh with a bad checksum, every eleventh TCP, options on every fifth"""
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from dabamd.synth import Ensemble, IP, ip_carousel
    assert IP == 7
    seed, br, F = 77, 64, 24
    e = Ensemble(F, subch=[(0, 48, br, 0o103, 0, 0, IP)])
    msc = e.generate(seed)["msc"]
    rows = np.packbits(msc[16:, 0, :24 * br], axis=1)
    a = pp.Assembler(br)
    for q, row in enumerate(rows):
        a.cif(q, row)
    car = ip_carousel(seed, 0)
    assert len(car) == 44 and len(a.delivered) >= 50          # more than one round
    first = car.index(a.delivered[0])
    assert a.delivered == [car[(first + i) % 44] for i in range(len(a.delivered))]
    res, out, run = ip.Handler().feed(a.group_records(), np.frombuffer(bytes(a.arena), np.uint8))
    for i, (g, r) in enumerate(zip(a.delivered, res)):
        k = (first + i) % 44
        hs = g[2] & 15
        assert (hs in (6, 7, 8)) == (k % 5 == 3) and (hs == 5) == (k % 5 != 3) and bool(g[0] & 0x40) == (k % 3 != 0)
        want = ip.CHECKSUM if k % 7 == 6 else ip.NOT_UDP if k % 11 == 10 else ip.DELIVERED
        assert r["status"] == want, (i, k)
        if want == ip.DELIVERED:
            end = len(g) - (2 if g[0] & 0x40 else 0)
            assert out[r["offset"]:r["offset"] + r["nbytes"]].tobytes() == g[2 + 4 * hs + 8:end] and 8 <= r["nbytes"] < 200
    assert run["counts"][ip.CHECKSUM] >= 6 and run["counts"][ip.NOT_UDP] >= 3


def test_fib_subchannels_flag_ip_components():
    """tests/cpp/test_fib_ip.cpp: the transmitter's FIBs with a DSCTy 59 component, what
    ensembleDecoder's auto_layout asks fib_processor::subchannels for when on_datagram is set; only
    when asked"""
    exe = os.path.join(BUILD, "test_fib_ip")
    os.makedirs(BUILD, exist_ok=True)
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(PKG, "host"),
                    "-I" + os.path.join(PKG, "synth"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_fib_ip.cpp"),
                    os.path.join(PKG, "host", "fib_processor.cpp"), "-L" + os.path.join(PKG, "lib"), "-ldabsynth",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FIB IP OK" in r.stdout, r.stdout + r.stderr


def test_library_and_binding_export_the_layer():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import dabamd
    l = dabamd.lib()
    for name in ("dabgpu_ip_groups", "dabgpu_pipe_ip", "dabgpu_pipe_ip_state"):
        assert hasattr(l, name), name
    assert l.dabgpu_abi_version() == 7
    assert dabamd.SUBCH_IP == 64 and dabamd.IP_RESULT_DTYPE == ip.RESULT_DTYPE and dabamd.IP_RUN_DTYPE == ip.RUN_DTYPE
    assert dabamd.IP_STATE_DTYPE == ip.STATE_DTYPE
    assert (dabamd.IP_STATE_DTYPE.itemsize, dabamd.IP_RESULT_DTYPE.itemsize, dabamd.IP_RUN_DTYPE.itemsize) == (8, 16, 48)
    assert dabamd.ip_arena_bytes(7, 100) == ip.arena_bytes(7, 100) == 100 + 7 * 16
    assert (dabamd.IP_DELIVERED, dabamd.IP_NOT_ACCEPTED, dabamd.IP_TOO_LONG, dabamd.IP_NOT_V4, dabamd.IP_CHECKSUM, dabamd.IP_NOT_UDP,
            dabamd.IP_MALFORMED) == tuple(range(7))
    assert callable(dabamd.ip_groups) and callable(dabamd.Pipeline.ip)
    hdr = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    for word in ("#define DABGPU_SUBCH_IP      64", "#define DABGPU_IP_ARENA_FOR(group_slots, arena_bytes) ((arena_bytes) + 16 * (group_slots))",
                 "} dabgpu_ip_state;", "} dabgpu_ip_result;", "} dabgpu_ip_run;", "#define DABGPU_IP_MALFORMED    6",
                 "int dabgpu_ip_groups(dabgpu_ctx *ctx, dabgpu_ip_state *state_d, int n_slots,",
                 "int dabgpu_pipe_ip(dabgpu_pipe *p, uint8_t *bytes_d, dabgpu_ip_result *results_d, dabgpu_ip_run *run_d);",
                 "#define DABGPU_ABI_VERSION 7"):
        assert word in hdr, word
    slots = open(os.path.join(PKG, "csrc", "layer_slots.h")).read()
    assert "enum { DABPLUS = 0, MP2, PACKET, MOT, PAD, NKIND };" in slots       # the IP layer rides on the packet slot
