"""ip_bench.py -- the IP layer (dabgpu_pipe_ip) alone and inside a step.

A pipeline of --streams streams x --frames frames per run whose table holds one packet entry of
--bitrate kbit/s flagged DABGPU_SUBCH_PACKET | DABGPU_SUBCH_IP (the synthesiser's DABSYNTH_IP
content: IPv4/UDP datagrams of 8..199 data bytes, one a data group) beside a DAB+ entry of 64
kbit/s; every stream carries the same signal.  The calls alternate:
  - even calls: run, dabplus and packet, a sync, then dabgpu_pipe_ip to dabgpu_pipe_sync with the
    device otherwise idle: the layer alone (wall ms, launch and sync included) and the step
    without it;
  - odd calls: run, dabplus, packet and ip, then one sync: the step with the layer inside.
Prints one JSON line with the times and, per call, the groups fed and the datagrams and bytes
delivered.  Under rocprofv3 --kernel-trace --stats the two kernels' own times come from its table.
Usage: python tools/ip_bench.py [--streams 2 --frames 6 --bitrate 16 --calls 6]
"""
import argparse
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
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--bitrate", type=int, default=16)
    ap.add_argument("--calls", type=int, default=6)
    args = ap.parse_args()
    import dabamd
    from dabamd.synth import Ensemble, IP
    from bench import to_raw, AMPLITUDE
    E, F, BR = args.streams, args.frames, args.bitrate
    cus = 12 * BR // 16                                   # EEP 3-A
    sub = [(0, cus, BR, 0o103, 0, 0, IP), (96, 48, 64, 0o103, 0, 1, 0)]
    ens = Ensemble(F * args.calls + 1, subch=sub, snr_db=30.0, amplitude=AMPLITUDE)
    raw = to_raw(ens.generate(5900, truth=False)["iq"], "s16")
    stride = ens.length
    ctx = dabamd.Context(0)
    diq = ctx.buf(E * stride * 4)
    for e in range(E):
        diq.upload_at(raw, e * stride * 4)
    subs = [dabamd.Subch(0, cus, BR, 0o103, 1, dabamd.SUBCH_PACKET | dabamd.SUBCH_IP),
            dabamd.Subch(96, 48, 64, 0o103, 1, dabamd.SUBCH_DABPLUS)]
    pipe = dabamd.Pipeline(ctx, E, F, subs)
    pipe.set_iq_format(dabamd.IQ_S16)
    pipe.set_packed(True)
    pipe.control(dabamd.CTL_ACQ_SYNC)
    alone, without, inside, recs = [], [], [], []
    for call in range(args.calls):
        ctx.sync()
        t0 = time.perf_counter()
        pipe.run(diq, stride, [stride] * E, download=False)
        pipe.dabplus(download=False)
        pipe.packet(download=False)
        if call & 1:
            pipe.ip(download=False)
            pipe.sync()
            inside.append((time.perf_counter() - t0) * 1e3)
        else:
            pipe.sync()
            t1 = time.perf_counter()
            pipe.ip(download=False)
            pipe.sync()
            t2 = time.perf_counter()
            without.append((t1 - t0) * 1e3)
            alone.append((t2 - t1) * 1e3)
        pr = np.frombuffer(pipe.pkr_d.download(np.uint8, E * dabamd.PACKET_RUN_DTYPE.itemsize).tobytes(), dabamd.PACKET_RUN_DTYPE)
        ir = np.frombuffer(pipe.ipr_d.download(np.uint8, E * dabamd.IP_RUN_DTYPE.itemsize).tobytes(), dabamd.IP_RUN_DTYPE)
        recs.append(dict(groups=int(pr["n_groups"].sum()), group_bytes=int(pr["n_bytes"].sum()),
                         datagrams=int(ir["n_datagrams"].sum()), payload_bytes=int(ir["n_bytes"].sum()),
                         by_status=ir["counts"].sum(axis=0).tolist()))
    print(json.dumps(dict(shape=f"{E} streams x {F} frames, one IP entry of {BR} kbit/s beside a DAB+ entry",
                          layer_alone_ms=alone, step_without_ms=without, step_with_layer_ms=inside, calls=recs)))
    pipe.close()
    ctx.close()


if __name__ == "__main__":
    main()
