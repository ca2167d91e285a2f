"""MPEG layer II without a GPU: the numpy restatement (mp2_py) against the golden file the
reference's own decoder wrote (tests/golden/mp2_kat.npz, make_mp2_golden.py), the frame
writer against the parser, and the C ABI's new surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mp2_py
import oracle_py as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kat():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mp2_kat.npz"))
    out = []
    for i, name in enumerate(z["names"]):
        nb = int(z["nbits_%d" % i])
        out.append(dict(name=str(name), bitrate=int(z["bitrate_%d" % i]), bits=np.unpackbits(z["bits_%d" % i])[:nb],
                        pcm=z["pcm_%d" % i], rate=z["rate_%d" % i]))
    return out


def sync_frames(bits, bitrate):
    """oracle_py.MP2 over CIF-sized pieces: [(frame bytes, rate)]"""
    m = orc.MP2(bitrate)
    for c in range(0, len(bits) - 24 * bitrate + 1, 24 * bitrate):
        m.add([int(x) for x in bits[c:c + 24 * bitrate]])
    return m.frames


def test_restatement_equals_reference(kat):
    """every fixture stream: the frames the synchroniser restatement finds, decoded by the
    decoder restatement, are sample for sample what the reference handed its sink, at the
    same rate; rejected headers hand over nothing"""
    assert len(kat) >= 7
    for s in kat:
        frames = sync_frames(s["bits"], s["bitrate"])
        ret, pcm, _ = mp2_py.decode_chain([f for f, _ in frames])
        dec = [k for k in range(len(frames)) if ret[k]]
        assert len(dec) == len(s["pcm"]) >= 3, s["name"]
        assert [frames[k][1] for k in dec] == list(s["rate"]), s["name"]
        for n, k in enumerate(dec):
            assert np.array_equal(pcm[k], s["pcm"][n]), (s["name"], k)
    names = [s["name"] for s in kat]
    rej = kat[names.index("stereo128")]
    assert len(sync_frames(rej["bits"], 128)) == len(rej["pcm"]) + 3      # three rejected headers in mid-stream
    assert set(kat[names.index("lsf64")]["rate"]) == {24000}


def test_fixtures_are_the_golden_streams_and_cover_the_tables(kat):
    """fixtures() regenerates the golden file's input bits, and the frames between them use
    every allocation value of every allocation row (so all 17 quantisers), all four scfsi
    values, scale factor 63, every joint-stereo bound, dual channel, mono, the CRC word and
    the LSF table; no intermediate of any of them leaves int32; V wraps int16 in the stream
    built for that (illegal code words) and, as the bound says, in no other"""
    fx = mp2_py.fixtures()
    assert [f["name"] for f in fx] == [s["name"] for s in kat]
    seen = {r: set() for r in range(6)}
    quant, scfsi, modes, bounds, crc, sf63, lsf = set(), set(), set(), set(), False, False, False
    for f, s in zip(fx, kat):
        assert np.array_equal(f["bits"], s["bits"]), f["name"]
        nbytes = 3 * f["bitrate"] * (2 if f["lsf"] else 1)
        for spec in f["specs"]:
            h = mp2_py.Decoder().parse(mp2_py.write_frame(spec, nbytes))
            if h is None:
                continue
            assert h["used"] <= 8 * nbytes                               # well-formed: inside lf bits
            layout = mp2_py.table_of(h["lsf"], h["mode"], mp2_py.BITRATES[h["lsf"]][h["br_index"] - 1], h["fs"])[0]
            for sb in range(h["sblimit"]):
                row = mp2_py.band_of(layout, sb)[1]
                for ch in range(2):
                    seen[row].add(int(h["alloc"][ch, sb]))
                    if h["q"][ch, sb]:
                        quant.add(int(h["q"][ch, sb]))
                        scfsi.add(int(h["scfsi"][ch, sb]))
                        sf63 |= 63 in h["scf"][ch, sb]
            modes.add(h["mode"])
            if h["mode"] == mp2_py.JOINT:
                bounds.add(h["bound"])
            crc |= h["crc"]
            lsf |= bool(h["lsf"])
        frames = [mp2_py.write_frame(spec, nbytes) for spec in f["specs"]]
        d = mp2_py.Decoder(check=True)
        for fr in frames:
            d.decode(fr)
        # rule 1 (V is int16) is exercised by the stream built for it, and only by it: legal
        # code words keep |V| <= 30720 however loud (see mp2_py.fixtures)
        assert (d.wrapped > 0) == (f["name"] == "wrap384"), f["name"]
    assert seen == {0: set(range(4)), 1: set(range(8)), 2: set(range(16)), 3: set(range(16)), 4: set(range(16)),
                    5: set(range(16))}
    assert quant == set(range(1, 18)) and scfsi == {0, 1, 2, 3} and sf63 and crc and lsf
    assert modes == {0, 1, 2, 3} and bounds == {4, 8, 12, 16}


def test_frame_writer_round_trips():
    rng = np.random.default_rng(11)
    cases = [(0, 8, 1, mp2_py.STEREO, 0, False, 384), (0, 10, 1, mp2_py.JOINT, 2, True, 576),
             (0, 4, 1, mp2_py.MONO, 0, False, 192), (0, 2, 2, mp2_py.MONO, 0, True, 216),
             (1, 8, 1, mp2_py.DUAL, 0, False, 384), (0, 14, 0, mp2_py.STEREO, 0, False, 1253)]
    for lsf, bri, fs, mode, ext, crc, nbytes in cases:
        want = {r: set(range(16)) for r in range(6)}
        spec = mp2_py.make_spec(rng, lsf, bri, fs, mode, ext, crc, nbytes, want)
        frame = mp2_py.write_frame(spec, nbytes)
        assert len(frame) == nbytes
        h = mp2_py.Decoder().parse(frame)
        for key in ("lsf", "br_index", "fs", "padding", "private", "mode", "mode_ext", "tail", "crc", "crc_word"):
            assert h[key] == spec[key], key
        for key in ("alloc", "scfsi", "scf", "codes"):
            assert np.array_equal(h[key], spec[key]), key
        assert h["frame_size"] == 144000 * mp2_py.BITRATES[lsf][bri - 1] // mp2_py.SAMPLE_RATES[lsf][fs]
    # the three rejections of mp2decodeFrame
    for bri, fs in ((0, 1), (15, 1), (8, 3)):
        bad = dict(lsf=0, br_index=bri, fs=fs, mode=0, mode_ext=0, crc=False)
        assert mp2_py.Decoder().decode(mp2_py.write_frame(bad, 384)) == (0, None)


def test_library_exports_the_layer():
    """fails on a library without the layer: the two entry points, and the state size the
    header, the binding and the restatement agree on"""
    import dabamd
    l = dabamd.lib()
    assert l.dabgpu_abi_version() == 7
    for name in ("dabgpu_mp2_decode", "dabgpu_pipe_mp2"):
        assert hasattr(l, name), name
    hdr = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    assert int(re.search(r"#define\s+DABGPU_MP2_STATE_BYTES\s+(\d+)", hdr).group(1)) == dabamd.MP2_STATE_BYTES
    assert dabamd.MP2_STATE_BYTES == mp2_py.Decoder().state().nbytes
    assert int(re.search(r"#define\s+DABGPU_SUBCH_MP2\s+(\d+)", hdr).group(1)) == dabamd.SUBCH_MP2 == 4
    assert C.sizeof(dabamd.PipeCaps) == 16 and dabamd.PipeCaps._fields_[3][0] == "max_mp2"
    assert dabamd.MP2_INFO_DTYPE.itemsize == 12
