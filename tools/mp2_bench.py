"""mp2_bench.py -- the MPEG layer II layer (dabgpu_pipe_mp2) on the C3 shape.

64 streams x 24 frames per run, 9 UEP-3 128 kbit/s subchannels carrying the synthetic
transmitter's layer II frames (valid header, random payload), all flagged DABGPU_SUBCH_MP2.
Every stream is the same ensemble (one is generated and uploaded 64 times: the work per
stream does not depend on which frames it carries).  Prints:
  - the layer alone: wall ms per dabgpu_pipe_mp2 call with the device otherwise idle
    (both kernels; the layer runs on a back-end stream, where the context's events do not
    reach), frames/s, the share of the 32-bit VALU peak its multiply-adds amount to, and
    its PCM bytes against the HBM peak;
  - the decoder kernel alone through dabgpu_mp2_decode on the same frames, by HIP events;
  - the C3 step with the layer called every run against the same build without the call,
    interleaved.
Usage: python tools/mp2_bench.py [--reps 2] [--block 3]
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

MACS_PER_FRAME = 36 * 2 * (64 * 32 + 512)            # matrixing + window
VALU_PEAK = 256 * 4 * 32 * 2.4e9                     # int32 lane-ops/s (bench.py's VALU_PEAK_TOPS)
HBM_PEAK = 8000e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--block", type=int, default=3, help="steps queued back to back per timing")
    ap.add_argument("--ensembles", type=int, default=64)
    ap.add_argument("--frames", type=int, default=24)
    args = ap.parse_args()
    import dabamd
    from dabamd.synth import Ensemble, MP2
    from bench import to_raw, AMPLITUDE
    E, F = args.ensembles, args.frames
    steps = 2 + 2 * args.reps * args.block
    sub = [(96 * i, 96, 128, 3, 1, 0, MP2) for i in range(9)]
    ens = Ensemble(F * steps + 1, subch=sub, snr_db=30.0, amplitude=AMPLITUDE)
    raw = to_raw(ens.generate(7000, truth=False)["iq"], "s16")
    stride = ens.length
    ctx = dabamd.Context(0)
    diq = ctx.buf(E * stride * 4)
    for e in range(E):
        diq.upload_at(raw, e * stride * 4)
    subs = [dabamd.Subch(s[0], s[1], s[2], s[3], 0, dabamd.SUBCH_MP2) for s in sub]
    pipe = dabamd.Pipeline(ctx, E, F, subs)
    pipe.set_iq_format(dabamd.IQ_S16)
    pipe.set_packed(True)
    pipe.control(dabamd.CTL_ACQ_SYNC)
    na = [stride] * E

    def step(layer):
        """ms per step over a block of steps queued back to back, as bench.py times them (a
        run's back end, the layer with it, overlaps the next run's front end)"""
        pipe.sync()
        t0 = time.perf_counter()
        for _ in range(args.block):
            pipe.run(diq, stride, na, download=False)
            if layer:
                pipe.mp2(download=False)
        pipe.sync()
        return (time.perf_counter() - t0) * 1e3 / args.block

    def layer_alone():
        pipe.run(diq, stride, na, download=False)
        pipe.sync()
        t0 = time.perf_counter()
        pipe.mp2(download=False)
        pipe.sync()
        return (time.perf_counter() - t0) * 1e3

    warm = layer_alone()                                  # 16 of its 96 CIFs are warm-up
    alone = layer_alone()
    with_, without = [], []
    for _ in range(args.reps):
        without.append(step(False))
        with_.append(step(True))
    nframes = E * 4 * F * 9
    out = dict(shape=f"{E} streams x {F} frames x 9 MP2 entries of 128 kbit/s", frames_per_call=nframes,
               layer_ms_first_call=warm, layer_ms=alone, frames_per_s=nframes / (alone * 1e-3),
               valu_share=nframes * MACS_PER_FRAME / (alone * 1e-3) / VALU_PEAK,
               pcm_bytes=nframes * 4608, pcm_share_of_hbm=nframes * 4608 / (alone * 1e-3) / HBM_PEAK,
               step_ms_without=without, step_ms_with=with_)
    # the decoder kernel alone: the last run's rows are the frames (packed MSC, one per CIF)
    ms = pipe.msc_stride_packed
    rows = pipe.msc_d.download(np.uint8, (E, 4 * F, 9, ms))
    frames = np.ascontiguousarray(rows.transpose(0, 2, 1, 3)[..., :384]).reshape(-1, 384)
    l = dabamd.lib()
    din, dst = ctx.put(frames), ctx.buf(E * 9 * dabamd.MP2_STATE_BYTES).zero()
    dpcm, dret = ctx.buf(len(frames) * 4608), ctx.buf(len(frames) * 4)
    ev = []
    for _ in range(3):
        l.dabgpu_event_record(ctx.h, 0)
        dabamd._chk(l.dabgpu_mp2_decode(ctx.h, din.ptr, 384, E * 9, 4 * F, dst.ptr, dpcm.ptr, dret.ptr), "dabgpu_mp2_decode")
        l.dabgpu_event_record(ctx.h, 1)
        ctx.sync()
        t = C.c_float()
        l.dabgpu_event_elapsed(ctx.h, 0, 1, C.byref(t))
        ev.append(t.value)
    out["decode_kernel_ms_events"] = ev
    out["decoded"] = int(np.count_nonzero(dret.download(np.int32, len(frames))))
    print(json.dumps(out))
    pipe.close()
    ctx.close()


if __name__ == "__main__":
    main()
