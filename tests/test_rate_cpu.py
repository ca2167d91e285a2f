"""The input rate conversion on the host: rateConverter (host/rate_converter.h, through
tests/cpp/rate_wrap.cpp and as a stand-alone program under the sanitizers) against the reference's
own Airspy handler (tests/golden/rate_kat.npz, written by make_rate_golden.py from
airspy-handler.cpp compiled where it lies), its chunking and block counts, and what the library and
the binding export.  Samples are compared as uint32 bit patterns: there is no tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rate_py as rp
from rate_py import bits

ROOT = rp.ROOT
PKG = os.path.join(ROOT, "sdr-j-dab_amd")


@pytest.fixture(scope="module")
def kat():
    return np.load(rp.KAT)


def test_golden_file_holds_what_the_issue_lists(kat):
    assert kat["rates"].tolist() == [2500000, 3000000]
    for rate in (2500000, 3000000):
        M, k = rate // 1000, "%d_" % rate
        x, y = kat[k + "in"], kat[k + "out"]
        assert x.dtype == np.int16 and x.shape == (3 * M + 1, 2) and y.dtype == np.float32 and y.shape == (3 * 2048, 2)
        assert kat[k + "int"].dtype == np.int16 and kat[k + "int"].shape == (2048,)
        assert kat[k + "float"].dtype == np.float32 and kat[k + "float"].shape == (2048,)
        for v in (-2048, 2047, -32768, 32767):
            assert (x == v).any(), (rate, v)
        inside = (x >= -2048) & (x <= 2047)
        assert inside.mean() > 0.99                       # 12-bit samples but for the int16 extremes
    assert os.path.getsize(rp.KAT) < 200 * 1024


def test_host_converter_equals_reference(kat):
    for rate in (2500000, 3000000):
        k = "%d_" % rate
        c = rp.Converter(rate, rp.IQ_S12)
        base, frac = c.tables()
        assert c.M == rate // 1000
        assert np.array_equal(base, kat[k + "int"]) and np.array_equal(bits(frac), bits(kat[k + "float"]))
        got = c.feed(kat[k + "in"])
        c.close()
        assert got.shape == kat[k + "out"].shape and np.array_equal(bits(got), bits(kat[k + "out"])), rate


def test_tables_follow_the_formula():
    """mapTable_int[2047] + 1 < M at every rate the converter takes, so the carried sample is never
    interpolated from within its block; the fractions are multiples of 1/2048"""
    for rate in (2048000, 2049000, 2500000, 3000000, 10000000):
        c = rp.Converter(rate, rp.IQ_F32)
        base, frac = c.tables()
        c.close()
        M = rate // 1000
        j = np.arange(2048, dtype=np.int64)
        assert np.array_equal(base.astype(np.int64), j * M // 2048)
        assert np.array_equal(frac.astype(np.float64) * 2048, (j * M) % 2048)
        assert base[2047] + 1 < M or M == 2048
        assert base[2047] + 1 <= M


@pytest.mark.parametrize("rate", [2500000, 3000000])
def test_any_chunking_gives_the_same_bytes(kat, rate):
    x = kat["%d_in" % rate]
    want = rp.convert(rate, rp.IQ_S12, x)
    assert np.array_equal(bits(want), bits(kat["%d_out" % rate]))
    for chunk in (1, 2499, 2500, 2501):
        got = rp.convert(rate, rp.IQ_S12, x, chunk)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), chunk


@pytest.mark.parametrize("rate", [2500000, 3000000, 2049000])
def test_block_counts(rate):
    M = rate // 1000
    x = np.random.default_rng(1).integers(-2048, 2048, (2 * M + 1, 2)).astype(np.int16)
    for n, want in zip((0, 1, M, M + 1, 2 * M, 2 * M + 1), (0, 0, 0, 1, 1, 2)):
        assert rp.blocks(n, M) == want
        assert len(rp.convert(rate, rp.IQ_S12, x[:n])) == 2048 * want, n


def test_other_formats_share_the_arithmetic():
    """after the conversion to float the arithmetic is the same: a format's output equals the cf32
    converter's on that format's floats"""
    rng = np.random.default_rng(2)
    M = 2500
    s16 = rng.integers(-32768, 32768, (2 * M + 1, 2)).astype(np.int16)
    u8 = rng.integers(0, 256, (2 * M + 1, 2)).astype(np.uint8)
    for fmt, x, f in ((rp.IQ_S12, s16, s16.astype(np.float32) / np.float32(2048)),
                      (rp.IQ_S16, s16, s16.astype(np.float32) / np.float32(32768)),
                      (rp.IQ_U8, u8, (u8.astype(np.float32) - np.float32(128)) / np.float32(128))):
        assert np.array_equal(bits(rp.convert(2500000, fmt, x)), bits(rp.convert(2500000, rp.IQ_F32, f))), fmt
    assert rp.wrap().rw_new(2500500, rp.IQ_S12) is None and rp.wrap().rw_new(2047000, rp.IQ_S12) is None
    assert rp.wrap().rw_new(10001000, rp.IQ_S12) is None and rp.wrap().rw_new(2500000, 4) is None


def test_host_converter_under_the_sanitizers(tmp_path, kat):
    """the stand-alone program (its own main, -fsanitize=address,undefined) over scripted chunkings,
    every chunk a heap block of exactly its length"""
    subprocess.run(["make", "-s", "-f", rp.MAKEFILE, rp.SANITIZE], check=True)
    rng = np.random.default_rng(5)
    jobs = []
    for rate in (2500000, 3000000):
        x = kat["%d_in" % rate]
        for chunks in ([len(x)], [1], [2499, 2500, 2501], [7, 0, 1000, 4097]):
            jobs.append((rate, rp.IQ_S12, x, chunks))
    jobs.append((2049000, rp.IQ_U8, rng.integers(0, 256, (2 * 2049 + 1, 2)).astype(np.uint8), [2048, 1]))
    jobs.append((10000000, rp.IQ_F32, rng.standard_normal((10001, 2)).astype(np.float32), [3333]))
    jobs.append((2500000, rp.IQ_S16, np.zeros((0, 2), np.int16), [5]))
    jobs.append((2500000, rp.IQ_S16, rng.integers(-32768, 32768, (2500, 2)).astype(np.int16), [0, 0]))
    with open(tmp_path / "in.bin", "wb") as w:
        for rate, fmt, x, chunks in jobs:
            w.write(np.array([rate, fmt, len(x), len(chunks)] + chunks, np.int32).tobytes())
            w.write(np.ascontiguousarray(x).tobytes())
    r = subprocess.run([rp.SANITIZE, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    raw, pos = open(tmp_path / "out.bin", "rb").read(), 0
    for rate, fmt, x, chunks in jobs:
        n = int(np.frombuffer(raw, np.int64, 1, pos)[0])
        pos += 8
        want = rp.convert(rate, fmt, x) if any(chunks) else np.zeros((0, 2), np.float32)
        assert n == len(want), (rate, fmt, chunks)
        assert np.array_equal(np.frombuffer(raw, np.uint32, 2 * n, pos), bits(want).reshape(-1)), (rate, fmt, chunks)
        pos += 8 * n
    assert pos == len(raw)


def test_exports():
    sys.path.insert(0, PKG)
    import dabamd
    l = dabamd.lib()
    assert hasattr(l, "dabgpu_rate_convert") and l.dabgpu_rate_convert.argtypes is not None     # in the binding table
    assert len(l.dabgpu_rate_convert.argtypes) == 11
    assert l.dabgpu_abi_version() == 7
    assert dabamd.IQ_S12 == 3 and (dabamd.IQ_F32, dabamd.IQ_U8, dabamd.IQ_S16) == (0, 1, 2)
    assert callable(dabamd.Context.rate_convert)
    hdr = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    for word in ("#define DABGPU_IQ_S12 3", "#define DABGPU_ABI_VERSION 7",
                 "int dabgpu_rate_convert(dabgpu_ctx *ctx, int in_rate, int format,",
                 "const void *src_d, int64_t src_stride, int n_streams, const int64_t *n_in_h,",
                 "float *iq_d, int64_t iq_stride, int64_t *n_out_h, int64_t *n_used_h);"):
        assert word in hdr, word
    src = open(os.path.join(PKG, "dabamd", "__init__.py")).read()
    assert '"dabgpu_rate_convert": ([vp, i32, i32, vp, i64, i32, vp, vp, i64, vp, vp], i32)' in src
