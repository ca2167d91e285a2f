"""fic_bench.py -- the FIC operator (dabgpu_fib_parse) on the bench shape.

64 databases (the bench's ensembles) x 288 FIBs per call (a 24-frame run), the FIBs the
synthesiser's FIC with FIGs (figs=1) of an ensemble with four subchannels, every slot at another
phase of it.  Prints one JSON line:
  - the operator alone: wall ms from dabgpu_fib_parse to dabgpu_sync with the inputs resident and
    the device otherwise idle, first call (new databases) and steady, with what the calls parsed;
  - the host path over the same FIBs on one core: ensembleDecoder::step()'s own loop
    (deliver_fibs, host/ensemble_decoder.cpp) -- each FIB expanded to one bit per byte, then fib_processor::process_FIB -- through tests/cpp's
    libficwrap.so (fw_fib is exactly that) for one slot's FIBs, times the slots, best of three,
    without the PCIe copy of the FIC the host path also needs.
Under rocprofv3 --kernel-trace --stats the kernel's own time comes from its table.
Usage: python tools/fic_bench.py [--calls 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sdr-j-dab_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--fibs", type=int, default=288)
    args = ap.parse_args()
    import dabamd
    from dabamd.synth import Ensemble
    N, NF = args.slots, args.fibs
    tx = [(0, 96, 128, 3, 1, 0, 0), (96, 48, 64, 0o103, 0, 1, 0), (144, 24, 32, 0o104, 0, 1, 0), (168, 84, 96, 2, 1, 0, 0)]
    frames = (NF * args.calls + N + 11) // 12 + 1
    fic = Ensemble(frames, subch=tx, figs=True).generate(3)["fic"]
    prog = np.packbits(fic.reshape(-1, 256), axis=-1)                               # [12 * frames, 32]
    ctx = dabamd.Context(0)
    l = dabamd.lib()
    db = ctx.buf(N * dabamd.FIC_DB_DTYPE.itemsize).zero()
    ev = ctx.buf(N * dabamd.FIC_EVENT_SLOTS * dabamd.FIC_EVENT_DTYPE.itemsize)
    tab, run = ctx.buf(N * dabamd.FIC_TABLE_DTYPE.itemsize), ctx.buf(N * dabamd.FIC_RUN_DTYPE.itemsize)
    ok = ctx.put(np.ones((N, NF), np.uint8))
    times, recs = [], []
    for call in range(args.calls):
        idx = np.arange(N)[:, None] + call * NF + np.arange(NF)[None, :]             # slot s starts s FIBs into the programme
        df = ctx.put(prog[idx])
        ctx.sync()
        t0 = time.perf_counter()
        rc = l.dabgpu_fib_parse(ctx.h, db.ptr, N, df.ptr, 32 * NF, ok.ptr, NF, 60, ev.ptr, dabamd.FIC_EVENT_SLOTS, tab.ptr, run.ptr)
        assert rc == 0, rc
        ctx.sync()
        times.append((time.perf_counter() - t0) * 1e3)
        r = np.frombuffer(run.download(np.uint8, N * dabamd.FIC_RUN_DTYPE.itemsize).tobytes(), dabamd.FIC_RUN_DTYPE)
        recs.append(dict(parsed=int(r["parsed"].sum()), figs=r["figs"].sum(0).tolist(), events=int(r["n_events"].sum()),
                         overrun=int(r["overrun"].sum()), table_changed=int(r["table_changed"].sum())))
        df.free()
    out = dict(shape=f"{N} databases x {NF} FIBs per call", operator_ms=times, calls=recs)
    try:
        import fib_py
        w = fib_py.host_lib()
        fed = [np.ascontiguousarray(prog[i]) for i in range(NF * args.calls)]        # slot 0's FIBs over all calls
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            h = w.fw_new()
            for i, f in enumerate(fed):
                w.fw_fib(h, f.ctypes.data, i)
            w.fw_free(h)
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
        # the host figure holds a ctypes call per FIB; the operator figure is one host-clock sample per call, launch
        # and sync included -- the kernel's own time comes from rocprofv3 --kernel-trace
        out["host_one_core"] = dict(fibs_per_slot=len(fed), ms_per_slot_all_calls=best * 1e3, ms_all_slots_all_calls=best * 1e3 * N,
                                    ms_per_call_all_slots=best * 1e3 * N / args.calls, us_per_fib=best * 1e6 / len(fed))
    except Exception as e:                                                          # (no host library built)
        out["host_one_core"] = str(e)
    print(json.dumps(out))
    for b in (db, ev, tab, run, ok):
        b.free()
    ctx.close()


if __name__ == "__main__":
    main()
