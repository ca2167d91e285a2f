"""Rate conversion in front of the pipeline, end to end: two synthetic ensembles resampled to the
Airspy's native rates (2.5 and 3 MHz, by zero-padding the spectrum of the whole stream), quantised
to 12-bit int16, converted back to 2.048 MHz with dabgpu_rate_convert and decoded by a 2-stream
pipeline; the FIC bits and CRC flags must equal the oracle's on the host rateConverter's output of
the same int16 data, with every FIB CRC good.  And ensembleDecoder::load_rate against
rateConverter followed by load (tests/cpp/test_rate_dropin.cpp): the same on_fib sequences."""
import os
import subprocess

import numpy as np
import pytest

import oracle_py as orc
import rate_py as rp

pytestmark = pytest.mark.gpu

RATES = [2500000, 3000000]
NFR = 4


def resample(iq, rate):
    """cf32 at 2.048 MHz -> complex at `rate`: the spectrum of the whole stream (cut to a multiple of
    2048 samples) zero-padded"""
    x = iq.reshape(-1, 2).astype(np.float64)
    z = (x[:, 0] + 1j * x[:, 1])[:len(x) // 2048 * 2048]
    n, m = len(z), len(z) // 2048 * (rate // 1000)
    Z = np.fft.fft(z)
    P = np.zeros(m, np.complex128)
    P[:n // 2] = Z[:n // 2]
    P[m - n // 2:] = Z[n // 2:]
    return np.fft.ifft(P) * (m / n)


@pytest.fixture(scope="module")
def native():
    """per stream the int16 I/Q pairs [n, 2] at its native rate, peak 1800"""
    from dabamd.synth import Ensemble
    out = []
    for s, rate in enumerate(RATES):
        iq = Ensemble(NFR + 1, snr_db=20.0, cfo_hz=0.0).generate(61 + s, truth=False)["iq"]
        y = resample(iq, rate)
        y = np.stack([y.real, y.imag], axis=1)
        out.append(np.round(y * (1800.0 / np.abs(y).max())).astype(np.int16))
    return out


def test_pipeline_on_converted_streams_equals_oracle(native):
    import dabamd
    ctx = dabamd.Context(0)
    bufs = []
    try:
        host = [rp.convert(rate, rp.IQ_S12, x) for rate, x in zip(RATES, native)]
        stride = max(len(h) for h in host)
        diq = ctx.buf(8 * 2 * stride)
        bufs.append(diq)
        diq.zero()
        lens = []
        for s, (rate, x) in enumerate(zip(RATES, native)):          # one call per rate
            src = ctx.put(x)
            bufs.append(src)
            n_out, n_used = ctx.rate_convert(rate, dabamd.IQ_S12, src, len(x), [len(x)], diq, stride, dst_off=8 * stride * s)
            assert n_out[0] == len(host[s]) and n_used[0] == (rate // 1000) * (len(host[s]) // 2048)
            lens.append(int(n_out[0]))
        ctx.sync()
        got = diq.download(np.float32, (2, stride, 2))
        for s in range(2):
            assert np.array_equal(rp.bits(got[s, :lens[s]]), rp.bits(host[s])), s
        pipe = dabamd.Pipeline(ctx, 2, NFR, [])
        try:
            pipe.control(dabamd.CTL_ACQ_SYNC)
            fic, crc, _, _ = pipe.run(diq, stride, lens)
            for s in range(2):
                assert pipe.state(s).frames_run == NFR, s
        finally:
            pipe.close()
        for s in range(2):
            ref = orc.decode_stream(np.ascontiguousarray(host[s]).reshape(-1), NFR, [])
            print("stream", s, "oracle frames", ref["n"], "good CRCs", int(ref["crc"].sum()), "gpu good CRCs", int(crc[s].sum()))
            assert ref["n"] == NFR
            assert np.array_equal(fic[s], ref["fic"]) and np.array_equal(crc[s], ref["crc"]), s
            assert crc[s].shape == (NFR, 12) and crc[s].all(), s          # all 48 FIB CRCs good
        ctx.check()
    finally:
        for b in bufs:
            b.free()
        ctx.close()


def test_dropin_load_rate_equals_host_converter_and_load(native, tmp_path):
    subprocess.run(["make", "-s", "-f", rp.MAKEFILE, rp.DROPIN], check=True)
    args = []
    for s, (rate, x) in enumerate(zip(RATES, native)):
        x.tofile(tmp_path / f"iq{s}.s16")
        args += [str(rate), str(tmp_path / f"iq{s}.s16")]
    r = subprocess.run([rp.DROPIN, str(NFR), "1"] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "RATE DROPIN OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    print("drop-in:", r.stdout.splitlines()[-1])
    fibs = [tuple(int(v) for v in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("FIB ")]
    for s in range(2):
        mine = [f for f in fibs if f[0] == s]
        assert [(f[1], f[2]) for f in mine] == [(fr, b) for fr in range(NFR) for b in range(4) for _ in range(3)], s
        assert all(f[3] == 1 for f in mine), s
