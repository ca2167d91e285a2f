"""The packet-mode data layer's restatement (tests/packet_py.py) against the reference's own
code (tests/golden/packet_kat.npz, written by make_packet_golden.py from msc-datagroup.cpp
and mot-databuilder.cpp compiled where they lie) and against the bit-level restatement
oracle_py.Datagroups; the three rules where the reference is undefined; what the library and
the binding export; fib_processor::subchannels(..., packet_data)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_py as orc
import packet_py as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sdr-j-dab_amd")


@pytest.fixture(scope="module")
def kat():
    z = np.load(os.path.join(ROOT, "tests", "golden", "packet_kat.npz"))
    out = []
    for i, name in enumerate(z["names"]):
        ends = np.cumsum(z["group_len_%d" % i])
        data = z["group_bytes_%d" % i].tobytes()
        out.append(dict(name=str(name), bitrate=int(z["bitrate_%d" % i]), rows=z["rows_%d" % i],
                        groups=[data[e - n:e] for e, n in zip(ends, z["group_len_%d" % i])],
                        qualities=z["quality_%d" % i].tolist(), mot=z["mot_%d" % i].tolist()))
    return out


def _feed(f, cap=pp.GROUP_BYTES):
    a = pp.Assembler(f["bitrate"], cap)
    infos = np.array([a.cif(q, row) for q, row in enumerate(f["rows"])], pp.INFO_DTYPE)
    return a, infos


def test_golden_file_holds_the_fixtures(kat):
    fx = pp.fixtures()
    assert [f["name"] for f in fx] == [k["name"] for k in kat] and len(kat) >= 8
    for f, k in zip(fx, kat):
        assert f["bitrate"] == k["bitrate"] and np.array_equal(f["rows"], k["rows"]), f["name"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "packet_kat.npz")) < 200 * 1024


def test_restatement_equals_reference(kat):
    """every fixture: the groups handed to the data handler byte for byte, the show_mscErrors
    values, and what the MOT builder passes to process_mscGroup (the accepted groups with a
    transport id: group type, last segment, segment number, transport id)"""
    seen = set()
    for k in kat:
        a, infos = _feed(k)
        assert a.delivered == k["groups"], k["name"]
        assert a.qualities == k["qualities"] == infos["quality"][infos["quality"] >= 0].tolist(), k["name"]
        mot = [[g["groupType"], (g["flags"] >> 4) & 1, g["segmentNumber"], g["transportId"]] for g in a.groups
               if g["flags"] & pp.ACCEPTED and g["flags"] & pp.TID]
        assert mot == k["mot"], k["name"]
        seen |= {g["flags"] & 15 for g in a.groups}
        if k["name"] == "window":
            assert infos["packets"].sum() >= 1000 and infos["crc_errors"].sum() >= 50 and len(a.qualities) == 2
        if k["name"] == "headers":
            assert {g["lengthInd"] for g in a.groups} >= {0, 3, 15}
            assert min(g["nbytes"] for g in a.groups) == 1 and max(g["nbytes"] for g in a.groups) == 4000
            assert sum(1 for g in a.groups if g["flags"] & pp.CRCF and not g["flags"] & pp.ACCEPTED) >= 3
        if k["name"] == "useful":
            assert {len(g) for g in a.delivered} >= set(range(92, 128))
        if k["name"] == "overrun":
            assert infos["packets"].tolist() == [1, 4] and not a.delivered
        if k["name"].startswith("lengths"):
            assert len(a.delivered) == (3 if k["bitrate"] == 8 else 12)
    assert seen == set(range(16))                              # every combination of the four header flags


def test_byte_level_equals_bit_level(kat):
    """Assembler against oracle_py.Datagroups (unchanged) on the same rows, one bit per byte"""
    for f in kat + [x for x in pp.extra_fixtures() if x["name"] != "clip"]:
        a, infos = _feed(f)
        d = orc.Datagroups(60, 0)
        for row in f["rows"]:
            d.add(np.unpackbits(row))
        assert [bytes(np.packbits(g)) for g in d.groups] == a.delivered, f["name"]
        assert d.crc_errors == infos["crc_errors"].sum() and d.state == a.state and d.addr == a.addr


def test_rules_where_the_reference_is_undefined():
    """the three rules and the clip at the CIF's end, stated as numbers for the restatement
    alone: this test runs no library code (it pins packet_py, and passes without the layer);
    test_gpu_packet holds the kernels to packet_py on these same fixtures"""
    fx = {f["name"]: f for f in pp.extra_fixtures()}
    # the copy stops at the CIF's end: 3 * 19 bytes, then bytes 75..95 of the 96
    a, _ = _feed(fx["clip"])
    assert [g["nbytes"] for g in a.groups] == [78, 60] and a.delivered[0][57:] == bytes(fx["clip"]["rows"][0][75:94]) + \
        bytes(fx["clip"]["rows"][0][94:96] ^ 0xFF)
    # rule 1: fields past the end read 0
    a, _ = _feed(fx["short"])
    g = a.groups
    assert [x["nbytes"] for x in g] == [1, 3, 5, 1, 3]
    assert (g[0]["flags"], g[0]["data_offset"], g[0]["data_nbytes"], g[0]["segmentNumber"], g[0]["lengthInd"]) == \
        (pp.EXT | pp.SEG | pp.UA | pp.ACCEPTED, 7, 0, 0, 0)
    assert g[1]["CI"] == 5 and g[1]["flags"] == pp.EXT | pp.SEG | pp.UA | pp.ACCEPTED and g[1]["data_offset"] == 7
    assert g[2]["flags"] == pp.EXT | pp.CRCF | pp.SEG | pp.UA | pp.LAST and g[2]["segmentNumber"] == 0x1300
    assert g[3]["flags"] == pp.CRCF and g[3]["data_nbytes"] == 0          # CRC flag, one byte: bad CRC, not accepted
    assert g[4]["flags"] == pp.SEG | pp.UA | pp.LAST | pp.ACCEPTED and g[4]["data_offset"] == 5
    # rule 2: int32 lengths
    a, _ = _feed(fx["big"])
    (g,) = a.groups
    assert g["nbytes"] == 4509 and g["flags"] & pp.ACCEPTED and g["data_nbytes"] == 4500 and g["data_offset"] == 7
    # rule 3: the cap
    a, _ = _feed(fx["cap"], 256)
    assert [x["nbytes"] for x in a.groups] == [104, 704, 254, 255]
    assert [bool(x["flags"] & pp.TRUNCATED) for x in a.groups] == [False, True, False, False]
    assert [bool(x["flags"] & pp.ACCEPTED) for x in a.groups] == [True, False, True, True]
    assert [x["offset"] for x in a.groups] == [0, 104, 360, 614] and a.run_record() == (4, 869, 0, 0)
    assert a.groups[1]["stored"] == a.delivered[1][:256]


def test_library_exports_packet_layer():
    """fails on a library without the layer: the entry points, the flag, the record sizes and
    the two sizing macros as the header, the binding and the restatement state them"""
    import dabamd
    l = dabamd.lib()
    assert l.dabgpu_abi_version() == 7
    for name in ("dabgpu_pipe_packet", "dabgpu_pipe_packet_caps"):
        assert hasattr(l, name), name
    hdr = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    assert int(re.search(r"#define\s+DABGPU_SUBCH_PACKET\s+(\d+)", hdr).group(1)) == dabamd.SUBCH_PACKET == 8
    assert (dabamd.PACKET_INFO_DTYPE.itemsize, dabamd.PACKET_RUN_DTYPE.itemsize, dabamd.DATAGROUP_DTYPE.itemsize) == (12, 16, 32)
    assert (dabamd.PACKET_INFO_DTYPE, dabamd.PACKET_RUN_DTYPE, dabamd.DATAGROUP_DTYPE) == (pp.INFO_DTYPE, pp.RUN_DTYPE, pp.GROUP_DTYPE)
    assert int(re.search(r"#define\s+DABGPU_PKT_GROUP_BYTES\s+(\d+)", hdr).group(1)) == dabamd.PKT_GROUP_BYTES == pp.GROUP_BYTES
    # the two macros, evaluated by the C preprocessor's own arithmetic rules (integers only)
    for macro, fn, args in (("DABGPU_PKT_GROUP_SLOTS", dabamd.pkt_group_slots, [(6, 128), (24, 384), (1, 12)]),
                            ("DABGPU_PKT_ARENA_BYTES", dabamd.pkt_arena_bytes, [(6, 128, 8216), (24, 64, 256), (3, 20, 1)])):
        m = re.search(r"#define\s+%s\(([^)]*)\)\s*((?:.*\\\n)*.*)" % macro, hdr)
        names, body = [x.strip() for x in m.group(1).split(",")], m.group(2).replace("\\\n", " ").replace("/", "//")
        for a in args:
            assert eval(body, {}, dict(zip(names, a))) == fn(*a), (macro, a)
    assert C.sizeof(dabamd.PipeCaps) == 16
    for name, bit in (("EXTENSION", 1), ("CRC", 2), ("SEGMENT", 4), ("USER_ACCESS", 8), ("LAST", 16), ("TRANSPORT", 32),
                      ("ACCEPTED", 64), ("TRUNCATED", 128)):
        assert int(re.search(r"#define\s+DABGPU_DG_%s\s+(\d+)" % name, hdr).group(1)) == bit


def test_fib_subchannels_flag_packet_components():
    """tests/cpp/test_fib_packet.cpp: the transmitter's FIBs with a PACKET subchannel"""
    exe = os.path.join(ROOT, "tests", "cpp", "build", "test_fib_packet")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(PKG, "host"),
                    "-I" + os.path.join(PKG, "synth"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_fib_packet.cpp"),
                    os.path.join(PKG, "host", "fib_processor.cpp"), "-L" + os.path.join(PKG, "lib"), "-ldabsynth",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FIB PACKET OK" in r.stdout, r.stdout + r.stderr
