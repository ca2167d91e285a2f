"""pad_bench.py -- the PAD operator (dabgpu_pad_aus) on the C5 shape.

256 padHandlers (the C5 workload's DAB+ subchannels per GPU) x 120 AUs per call (a 24-frame run
gives a 32 kbit/s subchannel about 115), every AU opening with a data stream element whose PAD
carries a seeded programme built with tests/pad_py's writers: a label carousel (both PAD forms,
segments continued over several AUs) and a MOT slide sent as X-PAD data groups, 48-byte
sub-fields, up to four a PAD.  Every handler gets the programme at a different phase.  Prints
one JSON line:
  - the operator alone: wall ms from dabgpu_pad_aus to dabgpu_sync with the inputs resident
    and the device otherwise idle, first call and steady, with what the calls delivered;
  - the host path over the same AUs on one core: dabgpu::padAssembler (tests/cpp's
    libpadwrap.so) for one handler's AUs, times the handlers, without the PCIe copy of the AUs
    the host path also needs.
Under rocprofv3 --kernel-trace --stats the kernel's own time comes from its table.
Usage: python tools/pad_bench.py [--calls 3]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--aus", type=int, default=120)
    args = ap.parse_args()
    import dabamd
    import pad_py as P
    N, NA, STRIDE = args.slots, args.aus, 256
    rng = np.random.default_rng(11)
    groups, _ = P.slide(nbytes=6000, seg=1000, seed=3)
    prog = []
    while len(prog) < NA * args.calls + N:
        prog += P.label_pads(b"Now playing: a title of some length - an artist", charset=15, sizes=(16, 8, 24))
        prog.append(P.short_pad(2, P.seg_prefix(3, 1, 1) + b"a"))
        prog.append(P.short_pad(3, b"bc."))
        for g in groups:
            prog += P.group_pads(g, 48, 48, per_pad=4)
    rows = np.zeros((len(prog), STRIDE), np.uint8)
    lens = np.zeros(len(prog), np.int32)
    for i, p in enumerate(prog):
        a, n = P.au_of(p, tail=bytes(rng.integers(0, 256, 40, dtype=np.uint8)))
        rows[i, :n], lens[i] = np.frombuffer(a, np.uint8), n
    ctx = dabamd.Context(0)
    l = dabamd.lib()
    sb = dabamd.pad_state_bytes()
    ls = gs = 4 * NA
    ar = max(dabamd.pad_arena_bytes(0), (8192 + 192 * NA + 15) // 16 * 16)
    state = ctx.buf(N * sb).zero()
    dlab, dgr = ctx.buf(N * ls * dabamd.PAD_LABEL_DTYPE.itemsize), ctx.buf(N * gs * dabamd.DATAGROUP_DTYPE.itemsize)
    dby, drun = ctx.buf(N * ar), ctx.buf(N * dabamd.PAD_RUN_DTYPE.itemsize)
    times, recs = [], []
    for call in range(args.calls):
        idx = (np.arange(N)[:, None] + call * NA + np.arange(NA)[None, :])           # slot s starts s AUs into the programme
        da, dl = ctx.put(rows[idx]), ctx.put(lens[idx])
        ctx.sync()
        t0 = time.perf_counter()
        rc = l.dabgpu_pad_aus(ctx.h, state.ptr, N, da.ptr, STRIDE, dl.ptr, NA, None, dlab.ptr, ls, dgr.ptr, gs, dby.ptr, ar, drun.ptr)
        assert rc == 0, rc
        ctx.sync()
        times.append((time.perf_counter() - t0) * 1e3)
        run = np.frombuffer(drun.download(np.uint8, N * dabamd.PAD_RUN_DTYPE.itemsize).tobytes(), dabamd.PAD_RUN_DTYPE)
        recs.append(dict(aus=int(run["aus"].sum()), pads=int(run["pads"].sum()), labels=int(run["n_labels"].sum()),
                         groups=int(run["n_groups"].sum()), group_bytes=int(run["n_bytes"].sum()),
                         crc_failed=int(run["crc_failed"].sum()), undefined=run["undefined"].sum(0).tolist()))
        da.free()
        dl.free()
    out = dict(shape=f"{N} handlers x {NA} AUs per call", operator_ms=times, calls=recs)
    so = os.path.join(ROOT, "tests", "cpp", "build", "libpadwrap.so")
    if os.path.exists(so):
        w = C.CDLL(so)
        w.pw_new.restype = C.c_void_p
        w.pw_free.argtypes = [C.c_void_p]
        w.pw_au.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
        w.pw_labels.argtypes = [C.c_void_p]
        w.pw_groups.argtypes = [C.c_void_p]
        fed = [(rows[i].tobytes(), int(lens[i])) for i in range(NA * args.calls)]      # handler 0's AUs over all calls
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            h = w.pw_new()
            for a, n in fed:
                w.pw_au(h, a, len(a), n)
            nl, ng = w.pw_labels(h), w.pw_groups(h)
            w.pw_free(h)
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
        # the host figure holds a ctypes call per AU; the operator figure is one host-clock sample per call,
        # launch and sync included -- the kernel's own time comes from rocprofv3 --kernel-trace
        out["host_one_core"] = dict(aus_per_handler=len(fed), labels_per_handler=nl, groups_per_handler=ng,
                                    ms_per_handler_all_calls=best * 1e3, ms_all_handlers_all_calls=best * 1e3 * N,
                                    ms_per_call_all_handlers=best * 1e3 * N / args.calls)
    print(json.dumps(out))
    for b in (state, dlab, dgr, dby, drun):
        b.free()
    ctx.close()


if __name__ == "__main__":
    main()
