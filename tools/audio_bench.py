"""audio_bench.py -- the audio output layer (dabgpu_pipe_audio, k_audio.hip) on one device.

A pipeline of --streams x --frames whose table holds --entries UEP-3 128 kbit/s subchannels
carrying the synthetic transmitter's layer II frames (48 kHz), all flagged DABGPU_SUBCH_MP2, the
first --flagged of them also DABGPU_SUBCH_AUDIO.  Every stream is the same ensemble (one is
generated and uploaded --streams times).  Prints one JSON line:
  - the layer alone: wall ms per dabgpu_pipe_audio call to dabgpu_pipe_sync with the device
    otherwise idle (both kernels, launch and synchronise included);
  - a step (dabgpu_pipe_run + dabgpu_pipe_mp2) with the layer called every run against the same
    build without the call, interleaved;
  - the kernels alone through dabgpu_audio_out on the last run's PCM, one call of 1152 pairs at
    48000 per (stream, entry, CIF), by HIP events, beside a dabgpu_memcpy_d2d that moves the same
    number of bytes (half of them read, half written), in the same session.
Usage: python tools/audio_bench.py [--streams 64] [--frames 24] [--entries 9] [--flagged 9] [--reps 3] [--block 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdr-j-dab_amd"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--entries", type=int, default=9)
    ap.add_argument("--flagged", type=int, default=9)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--block", type=int, default=3, help="steps queued back to back per timing")
    args = ap.parse_args()
    import dabamd
    from dabamd.synth import Ensemble, MP2
    from bench import to_raw, AMPLITUDE
    E, F, N, NA = args.streams, args.frames, args.entries, args.flagged
    steps = 3 + 2 * args.reps * args.block + args.reps
    sub = [(96 * i, 96, 128, 3, 1, 0, MP2) for i in range(N)]
    ens = Ensemble(F * steps + 1, subch=sub, snr_db=30.0, amplitude=AMPLITUDE)
    raw = to_raw(ens.generate(7000, truth=False)["iq"], "s16")
    stride = ens.length
    ctx = dabamd.Context(0)
    diq = ctx.buf(E * stride * 4)
    for e in range(E):
        diq.upload_at(raw, e * stride * 4)
    subs = [dabamd.Subch(s[0], s[1], s[2], s[3], 0, dabamd.SUBCH_MP2 | (dabamd.SUBCH_AUDIO if i < NA else 0))
            for i, s in enumerate(sub)]
    pipe = dabamd.Pipeline(ctx, E, F, subs)
    pipe.set_iq_format(dabamd.IQ_S16)
    pipe.set_packed(True)
    pipe.control(dabamd.CTL_ACQ_SYNC)
    na = [stride] * E

    def step(layer):
        pipe.sync()
        t0 = time.perf_counter()
        for _ in range(args.block):
            pipe.run(diq, stride, na, download=False)
            pipe.mp2(download=False)
            if layer:
                pipe.audio(download=False)
        pipe.sync()
        return (time.perf_counter() - t0) * 1e3 / args.block

    def layer_alone():
        pipe.run(diq, stride, na, download=False)
        pipe.mp2(download=False)
        pipe.sync()
        t0 = time.perf_counter()
        pipe.audio(download=False)
        pipe.sync()
        return (time.perf_counter() - t0) * 1e3

    alone = [layer_alone() for _ in range(1 + args.reps)]          # the first holds the first launches and the warm-up
    with_, without = [], []
    for _ in range(args.reps):
        without.append(step(False))
        with_.append(step(True))
    pipe.run(diq, stride, na, download=False)
    pipe.mp2(download=False)
    _, n_out = pipe.audio()
    frames = int(np.count_nonzero(n_out))
    out = dict(shape=f"{E} streams x {F} frames, {N} MP2 entries of 128 kbit/s, {NA} flagged AUDIO", frames_per_call=frames,
               layer_ms=alone, step_ms_without=without, step_ms_with=with_)
    # the kernels alone: one sink and one 48000 call of 1152 pairs per row of the last run's PCM, the rows as they lie
    l = dabamd.lib()
    rows = E * 4 * F * N
    rates, amounts = np.full(rows, 48000, np.int32), np.full(rows, 1152, np.int32)
    dst, dout, dn = ctx.buf(rows * dabamd.AUDIO_STATE_BYTES).zero(), ctx.buf(rows * 3 * 1152 * 8), ctx.buf(rows * 4)
    moved = rows * 1152 * (4 + 8)
    dsrc, dcpy = ctx.buf(moved // 2), ctx.buf(moved // 2)
    ev, cp = [], []
    t = C.c_float()
    for _ in range(1 + args.reps):
        l.dabgpu_event_record(ctx.h, 0)
        dabamd._chk(l.dabgpu_audio_out(ctx.h, pipe.pcm_d.ptr, 1152, rows, 1, 1152, dabamd._p(rates), dabamd._p(amounts), dst.ptr,
                                       dout.ptr, dn.ptr), "dabgpu_audio_out")
        l.dabgpu_event_record(ctx.h, 1)
        ctx.sync()
        l.dabgpu_event_elapsed(ctx.h, 0, 1, C.byref(t))
        ev.append(t.value)
        l.dabgpu_event_record(ctx.h, 0)
        dabamd._chk(l.dabgpu_memcpy_d2d(ctx.h, dcpy.ptr, dsrc.ptr, moved // 2), "dabgpu_memcpy_d2d")
        l.dabgpu_event_record(ctx.h, 1)
        ctx.sync()
        l.dabgpu_event_elapsed(ctx.h, 0, 1, C.byref(t))
        cp.append(t.value)
    out.update(kernel_rows=rows, bytes_moved=moved, kernel_ms_events=ev, copy_ms_events=cp,
               kernel_GBps=moved / (min(ev[1:]) * 1e-3) / 1e9, copy_GBps=moved / (min(cp[1:]) * 1e-3) / 1e9,
               kernel_over_copy=min(cp[1:]) / min(ev[1:]))
    print(json.dumps(out))
    pipe.close()
    ctx.close()


if __name__ == "__main__":
    main()
