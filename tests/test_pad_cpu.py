"""The PAD layer's restatement (tests/pad_py.py) against the reference's own code
(tests/golden/pad_kat.npz, written by make_pad_golden.py from pad-handler.cpp compiled where it
lies, under the address and undefined-behaviour sanitizers, every fixture in a process of its
own and from two fills of the handler's storage), the host padAssembler
(host/msc_consumers.cpp, through tests/cpp/pad_wrap.cpp) against both, the rules where the
reference is undefined or unbounded on cases outside the golden file, and what the library and
the binding export."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pad_py as P
import packet_py as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sdr-j-dab_amd")
WRAP = os.path.join(ROOT, "tests", "cpp", "build", "libpadwrap.so")
KAT = os.path.join(ROOT, "tests", "golden", "pad_kat.npz")


@pytest.fixture(scope="module")
def kat():
    return P.load_kat()


@pytest.fixture(scope="module")
def wrap():
    # built here when build()'s copy is not there (as test_consumers_cpu builds its library)
    subprocess.run(["make", "-s", "-f", os.path.join(ROOT, "tests", "cpp", "Makefile.pad"), WRAP], check=True)
    l = C.CDLL(WRAP)
    l.pw_new.restype = C.c_void_p
    l.pw_free.argtypes = [C.c_void_p]
    l.pw_au.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    l.pw_labels.argtypes = [C.c_void_p]
    l.pw_groups.argtypes = [C.c_void_p]
    l.pw_label.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    l.pw_group.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    l.pw_counters.argtypes = [C.c_void_p, C.c_void_p]
    return l


def host_run(l, aus):
    """the host padAssembler over AUs -> (labels, groups, counters) in the model's terms"""
    h = l.pw_new()
    try:
        for a in aus:
            l.pw_au(h, bytes(a[0]), len(a[0]), a[1])
        labels, groups = [], []
        for i in range(l.pw_labels(h)):
            info, pl, text = np.zeros(5, np.int32), np.zeros(64, np.uint8), np.zeros(256, np.uint8)
            assert l.pw_label(h, i, info.ctypes.data, pl.ctypes.data, text.ctypes.data) == 0
            labels.append(dict(au=int(info[0]), charset=int(info[1]), nbytes=int(info[2]), n_pieces=int(info[3]),
                               truncated=int(info[4]), piece_len=pl.tobytes(), text=text.tobytes()))
        for i in range(l.pw_groups(h)):
            info, b = np.zeros(9, np.int32), np.zeros(8192, np.uint8)
            assert l.pw_group(h, i, info.ctypes.data, b.ctypes.data, b.size) == 0
            groups.append(dict(zip(("au", "nbytes", "data_offset", "data_nbytes", "flags", "segmentNumber", "transportId",
                                    "groupType", "lengthInd"), info.tolist()), stored=b[:info[1]].tobytes()))
        cnt = np.zeros(11, np.int32)
        l.pw_counters(h, cnt.ctypes.data)
        return labels, groups, cnt.tolist()
    finally:
        l.pw_free(h)


def model(aus):
    return P.Handler().feed(aus)


def accepted(h):
    return [g for g in h.groups if g["flags"] & pp.ACCEPTED]


def test_golden_file_holds_the_fixtures(kat):
    fx = P.fixtures()
    assert [f["name"] for f in fx] == [k["name"] for k in kat] and len(kat) == 22
    for f, k in zip(fx, kat):
        assert [(bytes(a[0]), a[1]) for a in f["aus"]] == k["aus"] and len(k["aus"]) <= 64, f["name"]
    assert os.path.getsize(KAT) < 200 * 1024
    assert sum(len(k["labels"]) for k in kat) >= 25 and sum(len(k["calls"]) for k in kat) >= 25


def test_no_fixture_pad_touches_a_rule():
    """the share of the fixtures' PADs kept from the reference is zero: none meets rules 1-4"""
    for f in P.fixtures():
        h = model(f["aus"])
        assert not any(h.touched) and h.c["undefined"] == [0, 0, 0, 0], f["name"]


def test_restatement_equals_reference(kat):
    """every fixture: each label the reference showed -- during which AU, charSet, the pieces it
    converted and their bytes -- and each process_mscGroup call -- AU, type, last flag, segment
    number, transport id, where its data pointer stood and the group's bytes"""
    for k in kat:
        h = model(k["aus"])
        got = [dict(au=l["au"], charset=l["charset"], pieces=l["pieces"], text=l["text"]) for l in h.labels]
        assert got == k["labels"], k["name"]
        calls = [dict(au=g["au"], groupType=g["groupType"], last=int(bool(g["flags"] & pp.LAST)), segmentNumber=g["segmentNumber"],
                      transportId=g["transportId"], index=g["data_offset"], bytes=g["stored"]) for g in accepted(h)]
        assert calls == k["calls"], k["name"]


def _same(h, host, what):
    labels, groups, cnt = host
    want = h.label_records()
    assert len(labels) == len(want), what
    for l, w in zip(labels, want):
        assert (l["au"], l["charset"], l["nbytes"], l["n_pieces"], l["truncated"]) == \
            (w["au"], w["charset"], w["nbytes"], w["n_pieces"], w["flags"]), what
        assert l["piece_len"] == w["piece_len"].tobytes() and l["text"] == w["text"].tobytes(), what
    assert len(groups) == len(h.groups), what
    for g, w in zip(groups, h.groups):
        for key in ("au", "nbytes", "data_offset", "data_nbytes", "flags", "segmentNumber", "transportId", "groupType",
                    "lengthInd", "stored"):
            assert g[key] == w[key], (what, key, g[key], w[key])
    c = h.c
    assert cnt == [len(h.labels), len(h.groups), c["aus"], c["pads"], c["unhandled"]] + c["undefined"] + \
        [c["crc_failed"], c["guard_dropped"]], (what, cnt, c)


def test_host_assembler_equals_reference_and_restatement(kat, wrap):
    for k in kat:
        host = host_run(wrap, k["aus"])
        _same(model(k["aus"]), host, k["name"])
        labels, groups, _ = host
        assert [(l["au"], l["charset"], l["text"][:l["nbytes"]]) for l in labels] == \
            [(l["au"], l["charset"], l["text"]) for l in k["labels"]], k["name"]
        assert [(g["au"], g["stored"], g["data_offset"]) for g in groups if g["flags"] & pp.ACCEPTED] == \
            [(c["au"], c["bytes"], c["index"]) for c in k["calls"]], k["name"]


def test_rules_where_the_reference_is_undefined(wrap):
    """one case per rule: the PADs are marked, counted, and the host assembler does the same"""
    cases = P.rule_cases()
    assert sorted({c["rule"] for c in cases}) == [1, 2, 3, 4]
    for c in cases:
        h = model(c["aus"])
        assert h.c["undefined"][c["rule"] - 1] >= 1 and any(c["rule"] in t for t in h.touched), c["name"]
        _same(h, host_run(wrap, c["aus"]), c["name"])
    by = {c["name"]: model(c["aus"]) for c in cases}
    assert by["rule1"].c["undefined"] == [2, 0, 0, 0] and [l["text"] for l in by["rule1"].labels] == [b"ok"]
    assert by["rule2"].c["undefined"][1] == 6                    # count 6 is whole, the six after it are not
    assert by["rule2"].labels[0]["text"] == b"s" and by["rule2"].labels[1]["text"] == b"\0"     # the byte below reads 0
    assert by["rule3"].c["undefined"][2] == 4 and by["rule3"].c["crc_failed"] == 2   # both one-byte groups carry the CRC flag
    lab = by["rule4_bytes"].label_records()[-1]
    assert (lab["nbytes"], lab["n_pieces"], lab["flags"]) == (257, 17, P.LABEL_TRUNCATED)
    assert lab["text"].tobytes() == b"x" * 16 + b"y" * 240       # the 257th byte, z, is not kept
    lab = by["rule4_pieces"].label_records()[-1]
    assert (lab["nbytes"], lab["n_pieces"], lab["flags"]) == (65, 65, P.LABEL_TRUNCATED)
    assert lab["piece_len"].tolist() == [1] * 64 and lab["text"][:65].tobytes() == b"a" + b"b" * 63 + b"c"


def test_fixture_slide_travels_as_xpad_groups(kat):
    """the slide fixture's accepted groups are the MOT groups it was built from, twice"""
    k = [x for x in kat if x["name"] == "slide"][0]
    groups, body = P.slide()
    assert [c["bytes"] for c in k["calls"]] == groups + groups
    import mot_py
    a = mot_py.Assembler()
    a.feed(*mot_py.pack(groups + groups))
    assert [o["body"] for o in a.objects] == [body]


def test_sizes_and_exports():
    assert P.LABEL_DTYPE.itemsize == 344 and P.RUN_DTYPE.itemsize == 64
    assert P.au_slots(24) == 126 and P.arena_bytes(0) == 8192 + 6 * 192 and P.arena_bytes(24) % 16 == 0
    import sys
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import dabamd
    l = dabamd.lib()
    for name in ("dabgpu_pad_aus", "dabgpu_pad_state_bytes", "dabgpu_pipe_pad", "dabgpu_pipe_pad_caps"):
        assert hasattr(l, name), name
    assert dabamd.pad_state_bytes() == 64 + 64 + 256 + 8192
    assert dabamd.SUBCH_PAD == 32 and dabamd.PAD_LABEL_DTYPE == P.LABEL_DTYPE and dabamd.PAD_RUN_DTYPE == P.RUN_DTYPE
    assert dabamd.pad_au_slots(24) == P.au_slots(24) and dabamd.pad_arena_bytes(24) == P.arena_bytes(24)
    assert callable(dabamd.pad_aus)
    hdr = " ".join(open(os.path.join(ROOT, "include", "dabgpu.h")).read().split())
    for word in ("DABGPU_SUBCH_PAD 32", "DABGPU_PAD_LABEL_BYTES 256", "DABGPU_PAD_LABEL_PIECES 64", "dabgpu_pad_label",
                 "dabgpu_pad_run", "DABGPU_PAD_ARENA_BYTES"):
        assert word in hdr, word


# ---- the synthesiser's DABSYNTH_PAD content ------------------------------------------------------
# (startAddr, CUs, bitRate, protLevel, uep, dabplus, content)
OLD_CONTENTS = [(0, 48, 64, 0o103, 0, 1, 0), (48, 24, 32, 0o103, 0, 2, 4), (96, 48, 64, 0o103, 0, 0, 2),
                (144, 48, 64, 0o103, 0, 0, 3), (192, 48, 64, 0o103, 0, 0, 5), (240, 96, 128, 3, 1, 0, 0)]
OLD_HASH = "801ae86683433ca93ee1b08856fde56d1f32d5632297ce66ce708bede5cfe2a0"   # from the library before DABSYNTH_PAD


def _synth():
    import sys
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import dabamd.synth as sy
    return sy


def test_existing_synth_contents_generate_identical_streams():
    """random DAB+, AU_MIX on a shifted grid, MP2, PACKET, MOT and random bits: IQ, FIC and MSC
    truth hash as they did before the PAD content was added"""
    import hashlib
    g = _synth().Ensemble(6, subch=OLD_CONTENTS, snr_db=25.0).generate(4242)
    h = hashlib.sha256()
    for k in ("iq", "fic", "msc"):
        h.update(np.ascontiguousarray(g[k]).tobytes())
    assert h.hexdigest() == OLD_HASH


def synth_aus(msc, s, bitrate):
    """the AUs of DAB+ subchannel s from the transmitter's MSC truth [ncif, NS, bits]: superframes
    of five CIFs on the grid where the AU CRCs hold, layout 0 (four AUs); (bytes, length, cif, au)"""
    rs = bitrate // 8
    rows = np.packbits(msc[:, s, :24 * bitrate], axis=1)
    best = []
    for off in range(5):
        out = []
        for c in range(off, len(rows) - 4, 5):
            sf = rows[c:c + 5].reshape(-1)[:110 * rs].tobytes()
            au = [8] + [int.from_bytes(sf[3:8], "big") >> (40 - 12 * (i + 1)) & 0xFFF for i in range(3)] + [110 * rs]
            if any(b <= a + 2 or b > 110 * rs for a, b in zip(au, au[1:])):
                continue
            for i in range(4):
                a = sf[au[i]:au[i + 1]]
                if pp.crc_good(a):
                    out.append((a[:-2], len(a) - 2, c + 4, i))
        if len(out) > len(best):
            best = out
    return best


def test_synth_pad_programme_matches_the_restatement(wrap):
    """DABSYNTH_PAD truth through the model: the label carousel (three segments over several AUs
    in charset 15, short PADs, the clear command, charset 0) and the slide as X-PAD groups; no
    PAD meets a rule; the host padAssembler delivers the same"""
    import mot_py
    sy = _synth()
    assert sy.PAD == 6
    sub = [(0, 24, 32, 0o103, 0, 1, sy.PAD), (24, 24, 32, 0o103, 0, 1, 0)]
    seed = 77
    g = sy.Ensemble(12, subch=sub, snr_db=25.0).generate(seed)
    aus = synth_aus(g["msc"], 0, 32)
    assert len(aus) >= 32 and all((a[0][0] >> 5) & 7 == 4 for a in aus)
    h = P.Handler().feed(aus)
    # the truth begins four CIFs into the programme's first superframe, as a receiver tuning in would: until
    # the first `first` segment charSet is unset (rule 3); nothing else meets a rule
    start = min(i for i, a in enumerate(aus) if P.Handler().feed(aus[i:i + 1]).cs_set)
    assert not any(h.touched[start:]) and all(t <= {3} for t in h.touched[:start]) and start < 29
    assert h.c["pads"] == len(aus) and h.c["crc_failed"] == 0 and h.c["unhandled"] == 0
    first = b"DABSYNTH s0 - now playing: track %d" % (seed % 90 + 10)
    got = [(l["charset"], l["text"]) for l in h.labels]
    k = got.index((15, first))
    assert got[k:k + 3] == [(15, first), (0, b"ABC"), (0, b"sub 0 charset 0")], got
    assert h.labels[k]["pieces"] == [6, 8, 2] * 2 + [3]         # each 16-byte segment over three AUs
    acc = [x["stored"] for x in accepted(h)]
    assert len(acc) >= 8
    a = mot_py.Assembler()
    a.feed(*mot_py.pack(acc))
    assert len(a.objects) >= 1 and a.objects[0]["transportId"] == 0x1000 and len(a.objects[0]["body"]) == 230
    assert a.objects[0]["name"] == b"s0_0.jpg"
    _same(P.Handler().feed([x[:2] for x in aus]), host_run(wrap, aus), "synth")
    # the random-content subchannel: about one AU in eight reaches processPAD
    rnd = P.Handler().feed(synth_aus(g["msc"], 1, 32))
    assert 0 < rnd.c["pads"] < rnd.c["aus"]
