"""Generate tests/golden/rate_kat.npz from the REFERENCE's own Airspy handler.

The reference's src/input/airspy/airspy-handler.cpp is compiled where it lies (never copied), with
g++ -O2 -std=gnu++11 (no -ffast-math) against the stub headers in tests/cpp/rate_stubs (QObject,
QSettings, QFrame, ui_airspy-widget.h, virtual-input.h, libairspy/airspy.h) and that directory's
driver, into a temporary directory outside the repository.  The driver defines dlopen / dlsym and
hands out stub airspy_* functions: the single sample rate is the one asked for, and the samples
go through the handler's own callback in transfers of 7, 1000, 65536 and 4097 samples, with
getSamples drained after each.  The handler holds back up to one 64 KiB buffer, so far more
samples are fed than are kept: the file keeps the first three blocks of the output and the
3 M + 1 input samples they cover, for 2,500,000 and 3,000,000 Hz, and the two tables, recomputed
here from the formula and asserted equal to what the handler's output implies (every output block
restated in float32 numpy from them, and a ramp from which the output gives both tables back).
Only the .npz is committed.

Run from the repo root:  python tests/golden/make_rate_golden.py   (REF=/path/to/reference)
"""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = os.environ.get("REF", "/root/reference")
SIZES = ["7", "1000", "65536", "4097"]
BLOCKS = 3


def tables(rate):
    """mapTable_int, mapTable_float (airspy-handler.cpp:142-146): float(rate / 1000) / 2048.0 and the
    product in double, the difference rounded once to float"""
    j = np.arange(2048, dtype=np.float64)
    pos = j * (np.float64(np.float32(rate // 1000)) / 2048.0)
    base = np.floor(pos).astype(np.int64)
    return base.astype(np.int16), (pos - base).astype(np.float32)


def restate(x, rate, base, frac):
    """the handler's arithmetic in float32 numpy: x int16 [n, 2] -> cf32 [2048 B, 2]"""
    M = rate // 1000
    B = (len(x) - 1) // M if len(x) else 0
    c = x.astype(np.float32) / np.float32(2048)
    out = np.zeros((B, 2048, 2), np.float32)
    for b in range(B):
        k = M * b + base.astype(np.int64)
        r = frac[:, None]
        out[b] = c[k + 1] * r + c[k] * (np.float32(1) - r)
    return out.reshape(-1, 2)


def run(exe, tmp, rate, x):
    x = np.ascontiguousarray(x, np.int16)
    x.tofile(os.path.join(tmp, "in.s16"))
    subprocess.run([exe, str(rate), os.path.join(tmp, "in.s16"), os.path.join(tmp, "out.cf32")] + SIZES, check=True,
                   stderr=subprocess.DEVNULL)
    return np.fromfile(os.path.join(tmp, "out.cf32"), np.float32).reshape(-1, 2)


def main():
    stubs = os.path.join(TESTS, "cpp", "rate_stubs")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "rate_golden")
        subprocess.run(["g++", "-O2", "-std=gnu++11", "-w", "-I" + stubs, "-I" + REF + "/includes", "-I" + REF + "/includes/various",
                        "-I" + REF + "/src/input/airspy", "-o", exe, os.path.join(stubs, "rate_golden_driver.cpp"),
                        REF + "/src/input/airspy/airspy-handler.cpp", "-lm"], check=True)
        for rate in (2500000, 3000000):
            M = rate // 1000
            base, frac = tables(rate)
            # a ramp on I (k - 2048 at sample k of the first block): output j is (base[j] + frac[j] - 2048) / 2048
            # within 3 * 2^-25, and that number is a multiple of 2^-22
            ramp = np.zeros((70640, 2), np.int16)
            ramp[:M + 1, 0] = np.arange(M + 1) - 2048
            got = run(exe, tmp, rate, ramp)
            v = np.round(got[:2048, 0].astype(np.float64) * 2.0 ** 22).astype(np.int64) + 2048 * 2048
            assert np.array_equal(v // 2048, base.astype(np.int64)), rate
            assert np.array_equal(((v % 2048) / 2048.0).astype(np.float32), frac), rate
            rng = np.random.default_rng(rate)
            x = rng.integers(-2048, 2048, (70640, 2)).astype(np.int16)
            for b in range(BLOCKS):         # the extremes of 12 bits and of int16, in every block and on both channels
                at = M * b + rng.choice(M, 8, replace=False)
                x[at[:4], 0] = x[at[4:], 1] = [-2048, 2047, -32768, 32767]
            got = run(exe, tmp, rate, x)
            n_blocks = len(got) // 2048
            assert len(got) == 2048 * n_blocks and n_blocks >= BLOCKS, (rate, len(got))
            want = restate(x[:M * n_blocks + 1], rate, base, frac)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), rate
            k = "%d_" % rate
            out[k + "in"] = x[:M * BLOCKS + 1].copy()
            out[k + "out"] = got[:2048 * BLOCKS].copy()
            out[k + "int"] = base
            out[k + "float"] = frac
            print("%d Hz: %d samples fed, %d blocks out, %d kept" % (rate, len(x), n_blocks, BLOCKS))
    out["rates"] = np.array([2500000, 3000000], np.int32)
    path = os.path.join(HERE, "rate_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
