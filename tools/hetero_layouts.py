"""Cost of heterogeneous subchannel tables (not part of the product): one step of 64 streams
whose tables differ against config C3's uniform table, on the same IQ, same box, same
process, configurations interleaved over several repetitions.

  uniform  C3: every stream the 9 UEP-3 128 kbit/s entries (shared-table kernels path)
  hetero   24 streams with 3, 24 with 9 and 16 with 18 such entries, max_subch 18: C3's 576
           codewords per CIF (equal thirds of 3 / 9 / 18 would average 10 entries, not 9),
           decoded through the per-stream descriptor tables and the active-pair enumeration
           of the ACS and the traceback (the output keeps 64 x 18 rows per CIF, half unused)
  padded   the uniform table in a pipeline of max_subch 18: the per-stream path and its
           padded output with nothing else changed

Per configuration: wall ms per step over synchronised steps after warm-up, and the MSC
ACS / traceback kernel ms per launch from the pipeline's stage events (set_profiling(2)).

  python tools/hetero_layouts.py [--reps 3 --steps 8 --warmup 3 --frames 24]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sdr-j-dab_amd"))
import numpy as np  # noqa: E402
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--cfo", type=float, default=1300.0)
    a = ap.parse_args()
    import dabamd
    from dabamd.synth import Ensemble
    SUBCH, E, _ = bench.WORKLOADS["c3"]
    F = a.frames
    ens = Ensemble(F * (a.warmup + a.steps) + 2, subch=SUBCH, snr_db=30.0, cfo_hz=a.cfo)
    ctx = dabamd.Context(0)
    stride = ens.length
    diq = ctx.buf(E * 2 * stride * 4)
    for g0 in range(0, E, 8):
        n = min(8, E - g0)
        diq.upload_at(ens.generate_many(n, seed0=1000 + g0, threads=16), g0 * 2 * stride * 4)

    def sub(start):
        return dabamd.Subch(start, 96, 128, 3, 0, 0)

    c3 = [sub(s[0]) for s in SUBCH]
    t3 = [sub(288 * i) for i in range(3)]
    t18 = [sub(48 * i) for i in range(17)] + [sub(768)]
    tables = [t3] * 24 + [c3] * 24 + [t18] * 16
    assert sum(len(t) for t in tables) == E * len(c3)

    def make(name):
        if name == "uniform":
            return dabamd.Pipeline(ctx, E, F, c3)
        pipe = dabamd.Pipeline(ctx, E, F, c3, max_subch=18)
        if name == "hetero":
            for s, t in enumerate(tables):
                pipe.set_subch(s, t)
        return pipe

    names = ["uniform", "hetero", "padded"]
    res = {n: dict(ms=[], acs=[], tb=[]) for n in names}
    for rep in range(a.reps):
        for name in names:
            pipe = make(name)
            pipe.set_packed(True)
            pipe.acquire(diq, stride, [0] * E, [stride] * E)
            for _ in range(a.warmup):
                pipe.run(diq, stride, [stride] * E, download=False)
            pipe.sync()
            pipe.set_profiling(2)
            t = time.perf_counter()
            for _ in range(a.steps):
                pipe.run(diq, stride, [stride] * E, download=False)
            pipe.sync()
            ms = (time.perf_counter() - t) / a.steps * 1e3
            tm = pipe.timing()
            acs = tm["msc_acs"][0] / max(1, tm["msc_acs"][1])
            tb = tm["msc_traceback"][0] / max(1, tm["msc_traceback"][1])
            res[name]["ms"].append(ms)
            res[name]["acs"].append(acs)
            res[name]["tb"].append(tb)
            print(f"rep {rep} {name}: {ms:.3f} ms/step  acs {acs:.3f}  traceback {tb:.3f} ms/launch", flush=True)
            pipe.close()
    ctx.check()
    med = {n: {k: float(np.median(v)) for k, v in r.items()} for n, r in res.items()}
    out = {"frames_per_step": F, "streams": E, "steps": a.steps, "reps": a.reps, "median": med, "all": res,
           "hetero_over_uniform": {k: med["hetero"][k] / med["uniform"][k] for k in ("ms", "acs", "tb")},
           "padded_over_uniform": {k: med["padded"][k] / med["uniform"][k] for k in ("ms", "acs", "tb")}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
