"""Input rate conversion on the GPU (k_rate.hip): the operator dabgpu_rate_convert, bit-exact
against the reference's own Airspy handler (the golden file tests/golden/rate_kat.npz) and against
the host rateConverter (rate_py, itself pinned to that file by test_rate_cpu).  Samples are
compared as uint32 bit patterns; output buffers are pre-filled with a sentinel bit pattern that
must survive wherever the operator has nothing to write."""
import ctypes as C

import numpy as np
import pytest

import rate_py as rp
from rate_py import bits

pytestmark = pytest.mark.gpu

E_ARG = -1
FILL = 0xA5
SENTINEL = np.uint32(0xA5A5A5A5)
FMTS = [rp.IQ_S12, rp.IQ_S16, rp.IQ_U8, rp.IQ_F32]


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def kat():
    return np.load(rp.KAT)


def samples(fmt, n, seed):
    rng = np.random.default_rng(seed)
    if fmt == rp.IQ_F32:
        return rng.standard_normal((n, 2)).astype(np.float32)
    if fmt == rp.IQ_U8:
        return rng.integers(0, 256, (n, 2)).astype(np.uint8)
    if fmt == rp.IQ_S16:
        return rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    return rng.integers(-2048, 2048, (n, 2)).astype(np.int16)


def gpu_convert(ctx, rate, fmt, streams, src_stride=None, dst_stride=None, lead=0):
    """one call over `streams` (arrays [n, 2] of the format's type): the whole output buffer as
    uint32 [n_streams, dst_stride, 2] (sentinel where nothing was written), n_out, n_used.
    lead: samples in front of stream 0 in the source buffer (the operator is handed the address behind them)"""
    dt = rp.DTYPE[fmt]
    n_in = [len(x) for x in streams]
    src_stride = max(n_in + [1]) if src_stride is None else src_stride
    M = rate // 1000
    dst_stride = 2048 * max([rp.blocks(n, M) for n in n_in] + [1]) if dst_stride is None else dst_stride
    host = np.zeros((lead + len(streams) * src_stride, 2), dt)
    for s, x in enumerate(streams):
        host[lead + s * src_stride: lead + s * src_stride + len(x)] = x
    src, dst = ctx.put(host), ctx.buf(8 * len(streams) * dst_stride)
    try:
        dst.fill(FILL)
        n_out, n_used = ctx.rate_convert(rate, fmt, src, src_stride, n_in, dst, dst_stride, src_off=lead * 2 * np.dtype(dt).itemsize)
        ctx.sync()
        return dst.download(np.uint32, (len(streams), dst_stride, 2)), n_out, n_used
    finally:
        src.free()
        dst.free()


def check_stream(out, n_out, n_used, s, want, M):
    assert n_out[s] == len(want) and n_used[s] == M * (len(want) // 2048), (s, n_out[s], n_used[s], len(want))
    assert np.array_equal(out[s, :len(want)], bits(want)), s
    assert (out[s, len(want):] == SENTINEL).all(), s


@pytest.mark.parametrize("rate", [2500000, 3000000])
def test_operator_equals_reference(ctx, kat, rate):
    x, want = kat["%d_in" % rate], kat["%d_out" % rate]
    out, n_out, n_used = gpu_convert(ctx, rate, rp.IQ_S12, [x], dst_stride=3 * 2048 + 7)
    check_stream(out, n_out, n_used, 0, want, rate // 1000)
    ctx.check()


@pytest.mark.parametrize("rate", [2500000, 3000000])
def test_mixed_counts_in_one_call(ctx, rate):
    """six streams with 0, 1, M, M + 1, 2 M and 2 M + 1 samples, strides that are no multiple of
    2048 or of M: 0, 0, 0, 1, 1 and 2 blocks, the sentinel everywhere else"""
    M = rate // 1000
    counts = [0, 1, M, M + 1, 2 * M, 2 * M + 1]
    streams = [samples(rp.IQ_S12, n, 10 + i) for i, n in enumerate(counts)]
    src_stride, dst_stride = 2 * M + 4, 2 * 2048 + 5
    assert src_stride % M and src_stride % 2048 and dst_stride % 2048 and dst_stride % M
    out, n_out, n_used = gpu_convert(ctx, rate, rp.IQ_S12, streams, src_stride, dst_stride)
    assert n_out.dtype == np.int64 and n_used.dtype == np.int64
    assert list(n_out // 2048) == [0, 0, 0, 1, 1, 2]
    for s, x in enumerate(streams):
        check_stream(out, n_out, n_used, s, rp.convert(rate, rp.IQ_S12, x), M)
    ctx.check()


def test_continuation_from_n_used(ctx):
    """5 M + 1 samples in one call equal two calls: two blocks, then from sample n_used on"""
    rate, M = 2500000, 2500
    x = samples(rp.IQ_S12, 5 * M + 1, 3)
    whole, n_out, n_used = gpu_convert(ctx, rate, rp.IQ_S12, [x])
    assert n_out[0] == 5 * 2048 and n_used[0] == 5 * M
    a, na, ua = gpu_convert(ctx, rate, rp.IQ_S12, [x[:2 * M + 1 + 17]])      # (17 samples short of a third block)
    assert na[0] == 2 * 2048 and ua[0] == 2 * M
    b, nb, ub = gpu_convert(ctx, rate, rp.IQ_S12, [x[ua[0]:]])
    assert nb[0] == 3 * 2048 and ub[0] == 3 * M
    assert np.array_equal(np.concatenate([a[0, :na[0]], b[0, :nb[0]]]), whole[0])
    assert np.array_equal(whole[0], bits(rp.convert(rate, rp.IQ_S12, x)))
    ctx.check()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("rate", [2049000, 10000000])
def test_odd_and_largest_blocks(ctx, rate, fmt):
    """M = 2049: the second block and the second stream start on an odd sample, so on a 4-byte
    boundary for int16 pairs and a 2-byte one for u8, and one sample of lead shifts the first;
    M = 10000: the largest block, done in pieces.  Two blocks each, two streams, against rateConverter"""
    M = rate // 1000
    streams = [samples(fmt, 2 * M + 1, 20), samples(fmt, M + 1, 21)]
    out, n_out, n_used = gpu_convert(ctx, rate, fmt, streams, src_stride=2 * M + 1, dst_stride=2 * 2048 + 1, lead=1)
    for s, x in enumerate(streams):
        check_stream(out, n_out, n_used, s, rp.convert(rate, fmt, x), M)
    ctx.check()


def test_identity_at_the_output_rate(ctx):
    """at 2,048,000 Hz every fraction is 0: cf32 output j of a block is its input sample j, exactly"""
    x = samples(rp.IQ_F32, 2 * 2048 + 1, 30)
    assert np.isfinite(x).all() and (x != 0).all()
    out, n_out, n_used = gpu_convert(ctx, 2048000, rp.IQ_F32, [x, x[:2049]])
    assert list(n_out) == [4096, 2048] and list(n_used) == [4096, 2048]
    assert np.array_equal(out[0], bits(x[:4096])) and np.array_equal(out[1, :2048], bits(x[:2048]))
    assert (out[1, 2048:] == SENTINEL).all()
    ctx.check()


@pytest.mark.parametrize("fmt", [rp.IQ_U8, rp.IQ_S16, rp.IQ_F32])
def test_other_formats(ctx, fmt):
    rate, M = 2500000, 2500
    x = samples(fmt, 2 * M + 1, 40 + fmt)
    if fmt == rp.IQ_S16:
        x[:4, 0] = [-32768, 32767, 0, -1]
    if fmt == rp.IQ_U8:
        x[:4, 0] = [0, 255, 128, 127]
    out, n_out, n_used = gpu_convert(ctx, rate, fmt, [x], dst_stride=2 * 2048 + 3)
    check_stream(out, n_out, n_used, 0, rp.convert(rate, fmt, x), M)
    ctx.check()


def test_more_streams_than_one_launch_takes(ctx):
    """the block counts travel as kernel arguments, 64 streams a launch: 70 streams of 0, 1 or 2 blocks"""
    rate, M = 2500000, 2500
    streams = [samples(rp.IQ_S12, (s % 3) * M + 1, 100 + s) for s in range(70)]
    out, n_out, n_used = gpu_convert(ctx, rate, rp.IQ_S12, streams, src_stride=2 * M + 3, dst_stride=2 * 2048 + 9)
    for s, x in enumerate(streams):
        check_stream(out, n_out, n_used, s, rp.convert(rate, rp.IQ_S12, x), M)
    ctx.check()


def test_refusals_leave_the_output_untouched(ctx):
    import dabamd
    L = dabamd.lib()
    M = 2500
    x = samples(rp.IQ_S12, 2 * M + 1, 50)
    src, dst = ctx.put(np.concatenate([x, x])), ctx.buf(8 * 2 * 4096 + 16)
    n_out, n_used = np.full(2, -5, np.int64), np.full(2, -5, np.int64)

    def call(rate=2500000, fmt=rp.IQ_S12, src_off=0, src_stride=2 * M + 1, n=(2 * M + 1, 2 * M + 1), dst_off=0, dst_stride=4096, n_streams=2):
        n_in = np.array(n, np.int64)
        return L.dabgpu_rate_convert(ctx.h, rate, fmt, C.c_void_p(src.ptr.value + src_off), src_stride, n_streams, n_in.ctypes.data,
                                     C.c_void_p(dst.ptr.value + dst_off), dst_stride, n_out.ctypes.data, n_used.ctypes.data)
    try:
        dst.fill(FILL)
        for rate in (2500500, 2047000, 2048001, 10001000, 0, -2500000):
            assert call(rate=rate) == E_ARG, rate
        for fmt in (4, -1, 59):
            assert call(fmt=fmt) == E_ARG, fmt
        assert call(n_streams=0) == E_ARG and call(n_streams=-1) == E_ARG
        assert call(n=(2 * M + 1, -1)) == E_ARG
        assert call(dst_stride=4095) == E_ARG                       # iq_stride < 2048 B
        assert call(src_stride=2 * M) == E_ARG                      # src_stride < n_in
        assert call(src_off=2) == E_ARG and call(fmt=rp.IQ_U8, src_off=1) == E_ARG and call(fmt=rp.IQ_F32, src_off=4) == E_ARG
        assert call(dst_off=4) == E_ARG
        ctx.sync()
        assert (dst.download(np.uint32, (2 * 4096 * 2 + 4,)) == SENTINEL).all()
        assert (n_out == -5).all() and (n_used == -5).all()
        assert call() == 0                                          # and the same call with nothing wrong runs
        ctx.sync()
        got = dst.download(np.uint32, (2, 4096, 2))
        want = bits(rp.convert(2500000, rp.IQ_S12, x))
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
        assert list(n_out) == [4096, 4096] and list(n_used) == [2 * M, 2 * M]
        # the pipeline's own format entries keep refusing the new format
        assert L.dabgpu_iq_convert(ctx.h, rp.IQ_S12, src.ptr, 16, dst.ptr) == E_ARG
        pipe = dabamd.Pipeline(ctx, 1, 1, [])
        try:
            assert L.dabgpu_pipe_set_iq_format(pipe.h, rp.IQ_S12) == E_ARG
        finally:
            pipe.close()
        ctx.check()
    finally:
        src.free()
        dst.free()
