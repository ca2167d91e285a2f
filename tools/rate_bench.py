"""rate_bench.py -- the input rate conversion (dabgpu_rate_convert, k_rate.hip) on one device.

One conversion of the C3 input: --streams streams of --frames frames' worth of samples at --rate Hz
(96 ms a frame: 5,760,000 samples a stream at 2.5 MHz for 24 frames), DABGPU_IQ_S12, every stream
the same random 12-bit samples.  Timed by the context's events, the first call (table upload, first
launch) left out; in the same process and interleaved with it a dabgpu_memcpy_d2d that moves as
many bytes as the kernel reads and writes (half of them read, half written).  Prints one JSON line.
Usage: python tools/rate_bench.py [--streams 64] [--frames 24] [--rate 2500000] [--format 3] [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdr-j-dab_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--rate", type=int, default=2500000)
    ap.add_argument("--format", type=int, default=3, help="DABGPU_IQ_*: 0 cf32, 1 u8, 2 s16, 3 s12")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import dabamd
    S, M = args.streams, args.rate // 1000
    n_in = 96 * M * args.frames                        # a frame is 96 ms
    bps = {0: 8, 1: 2, 2: 4, 3: 4}[args.format]
    rng = np.random.default_rng(1)
    if args.format == 0:
        x = rng.standard_normal((n_in, 2)).astype(np.float32)
    elif args.format == 1:
        x = rng.integers(0, 256, (n_in, 2)).astype(np.uint8)
    else:
        x = rng.integers(-2048, 2048, (n_in, 2)).astype(np.int16)
    blocks = (n_in - 1) // M
    ctx = dabamd.Context(0)
    src, dst = ctx.buf(S * n_in * bps), ctx.buf(S * blocks * 2048 * 8)
    for s in range(S):
        src.upload_at(x, s * n_in * bps)
    moved = S * blocks * (M * bps + 2048 * 8)          # what the kernel reads and writes (the carried samples once)
    half = (moved // 2 + 15) & ~15
    csrc, cdst = ctx.buf(half).zero(), ctx.buf(half)
    l = dabamd.lib()
    t = C.c_float()
    ev, cp = [], []
    for _ in range(1 + args.reps):
        l.dabgpu_event_record(ctx.h, 0)
        n_out, n_used = ctx.rate_convert(args.rate, args.format, src, n_in, [n_in] * S, dst, blocks * 2048)
        l.dabgpu_event_record(ctx.h, 1)
        ctx.sync()
        l.dabgpu_event_elapsed(ctx.h, 0, 1, C.byref(t))
        ev.append(t.value)
        l.dabgpu_event_record(ctx.h, 0)
        dabamd._chk(l.dabgpu_memcpy_d2d(ctx.h, cdst.ptr, csrc.ptr, half), "dabgpu_memcpy_d2d")
        l.dabgpu_event_record(ctx.h, 1)
        ctx.sync()
        l.dabgpu_event_elapsed(ctx.h, 0, 1, C.byref(t))
        cp.append(t.value)
    ctx.check()
    assert (n_out == blocks * 2048).all() and (n_used == blocks * M).all()
    k, c = sorted(ev[1:])[len(ev[1:]) // 2], sorted(cp[1:])[len(cp[1:]) // 2]
    print(json.dumps(dict(shape=f"{S} streams x {n_in} samples at {args.rate} Hz, format {args.format}", blocks_per_stream=blocks,
                          bytes_moved=moved, kernel_ms_events=ev, copy_ms_events=cp, kernel_ms_median=k, copy_ms_median=c,
                          kernel_GBps=moved / (k * 1e-3) / 1e9, copy_GBps=2 * half / (c * 1e-3) / 1e9, kernel_over_copy=k / c)))
    for b in (src, dst, csrc, cdst):
        b.free()
    ctx.close()


if __name__ == "__main__":
    main()
