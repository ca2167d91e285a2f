"""mot_bench.py -- the MOT layer (dabgpu_pipe_mot) on the C3 shape.

64 streams x 24 frames per run, 4 EEP 3-A subchannels of 64 kbit/s flagged
DABGPU_SUBCH_PACKET | DABGPU_SUBCH_MOT (the entry mix of tools/packet_bench.py).  As there, the
entries' MSC rows are overwritten on the device after each run, here with packet streams that
carry a MOT slide carousel (tests/mot_py's writers: three slides of 6 to 12 KB in 1 KB
segments per entry, header groups repeated, cut into packets of all four lengths; every
stream carries the same four carousels).  Prints one JSON line:
  - the layer alone: wall ms from dabgpu_pipe_mot to dabgpu_pipe_sync with the device
    otherwise idle (the packet layer has run and finished before), first call and steady,
    with the groups fed and the objects and bytes delivered per call;
  - the host path over the same groups on one core: dabgpu::motAssembler (tests/cpp's
    libmotwrap.so: CRC, header parse and the motHandler walk per group, as the one-stream
    drop-in does it) for one stream's entries, times the streams, without the PCIe copy of
    the groups the host path also needs.
Under rocprofv3 --kernel-trace --stats the two kernels' shares come from its table.
Usage: python tools/mot_bench.py [--calls 3]
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
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--ensembles", type=int, default=64)
    ap.add_argument("--frames", type=int, default=24)
    args = ap.parse_args()
    import dabamd
    import mot_py as mp
    import packet_py as pp
    from dabamd.synth import Ensemble
    from bench import to_raw, AMPLITUDE
    E, F, NK, BR = args.ensembles, args.frames, 4, 64
    sub = [(48 * i, 48, BR, 0o103, 0, 0, 0) for i in range(NK)]
    ens = Ensemble(F * args.calls + 1, subch=sub, snr_db=30.0, amplitude=AMPLITUDE)
    raw = to_raw(ens.generate(7100, truth=False)["iq"], "s16")
    stride = ens.length
    ctx = dabamd.Context(0)
    diq = ctx.buf(E * stride * 4)
    for e in range(E):
        diq.upload_at(raw, e * stride * 4)
    subs = [dabamd.Subch(s[0], s[1], s[2], s[3], 1, dabamd.SUBCH_PACKET | dabamd.SUBCH_MOT) for s in sub]
    pipe = dabamd.Pipeline(ctx, E, F, subs)
    pipe.set_iq_format(dabamd.IQ_S16)
    pipe.set_packed(True)
    pipe.control(dabamd.CTL_ACQ_SYNC)
    # the entries' carousels as packet streams
    rng = np.random.default_rng(5)
    need = 4 * F * args.calls
    streams = []
    for k in range(NK):
        objs = []
        for o in range(3):
            tid, body = 0x2000 + 16 * k + o, bytes(rng.integers(0, 256, int(rng.integers(6000, 12000)), dtype=np.uint8))
            hdr = mp.header_group(tid, len(body), mp.name_param(b"slide_%d_%d.jpg" % (k, o)))
            objs.append([hdr, hdr] + mp.body_groups(tid, body, 1024))
        pk, i = [], 0
        while sum(len(p) for p in pk) < need * 3 * BR:
            for g in objs[i % 3]:
                pk += pp.packetize(g, 0x100 + k, [int(x) for x in rng.integers(0, 4, 5)])
            i += 1
        streams.append(pp.rows(pk, BR)[:need])
    ms = pipe.msc_stride_packed
    times, recs, fed = [], [], [[] for _ in range(NK)]
    for call in range(args.calls):
        pipe.run(diq, stride, [stride] * E, download=False)
        pipe.sync()
        host = np.zeros((E, 4 * F, NK, ms), np.uint8)
        for k in range(NK):
            host[:, :, k, :3 * BR] = streams[k][call * 4 * F:(call + 1) * 4 * F][None]
        pipe.msc_d.upload_at(host, 0)
        byts, groups, run, _ = pipe.packet()
        ctx.sync()
        t0 = time.perf_counter()
        pipe.mot(download=False)
        pipe.sync()
        times.append((time.perf_counter() - t0) * 1e3)
        mr = np.frombuffer(pipe.motr_d.download(np.uint8, E * NK * dabamd.MOT_RUN_DTYPE.itemsize).tobytes(), dabamd.MOT_RUN_DTYPE)
        recs.append(dict(groups=int(run["n_groups"].sum()), group_bytes=int(run["n_bytes"].sum()),
                         objects=int(mr["n_objects"].sum()), object_bytes=int(mr["n_bytes"].sum()),
                         malformed=int(mr["malformed"].sum()), entries=int(mr["entries"].sum())))
        for k in range(NK):
            for g in groups[0, k, :run[0, k]["n_groups"]]:
                fed[k].append(bytes(byts[0, k, g["offset"]:g["offset"] + g["nbytes"]]))
    out = dict(shape=f"{E} streams x {F} frames x {NK} packet entries of {BR} kbit/s carrying MOT", layer_ms=times, calls=recs)
    so = os.path.join(ROOT, "tests", "cpp", "build", "libmotwrap.so")
    if os.path.exists(so):
        l = C.CDLL(so)
        l.mw_new.restype = C.c_void_p
        l.mw_new.argtypes = [C.c_int]
        l.mw_group.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        l.mw_count.argtypes = [C.c_void_p]
        l.mw_free.argtypes = [C.c_void_p]
        # not like for like with layer_ms: the host figure also holds the bit expansion, the group CRC and
        # the header parse of add_mscDatagroup (on the GPU that is k_pkt_groups, in the packet layer, not in
        # layer_ms) and a ctypes call per group; and layer_ms is one host-clock sample per call, launch and
        # sync included -- the kernels' own times come from rocprofv3 --kernel-trace (profiles/mot_layer.txt)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            n = 0
            for k in range(NK):
                h = l.mw_new(dabamd.MOT_BODY_BYTES)
                for g in fed[k]:
                    l.mw_group(h, g, len(g))
                n += l.mw_count(h)
                l.mw_free(h)
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
        out["host_one_core"] = dict(groups_per_stream=sum(len(f) for f in fed), objects_per_stream=n,
                                    ms_per_stream_all_calls=best * 1e3, ms_all_streams_all_calls=best * 1e3 * E,
                                    ms_per_call_all_streams=best * 1e3 * E / args.calls)
    print(json.dumps(out))
    pipe.close()
    ctx.close()


if __name__ == "__main__":
    main()
