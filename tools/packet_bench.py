"""packet_bench.py -- the packet-mode data layer (dabgpu_pipe_packet) on the C3 shape.

64 streams x 24 frames per run, 4 EEP 3-A subchannels of 64 kbit/s flagged
DABGPU_SUBCH_PACKET.  The layer is a function of msc_bits_d, so nothing is synthesised for
it: after each run the entries' rows are overwritten on the device with host-generated
packet streams (tests/packet_py's writers: CRC-flagged data groups of 20..1500 bytes cut
into packets of all four lengths, one packet in 40 corrupted; every stream carries the same
four streams).  Prints one JSON line:
  - the layer alone: wall ms from dabgpu_pipe_packet to dabgpu_pipe_sync with the device
    otherwise idle, first call (16 of its 96 CIFs are warm-up) and steady, packets, groups
    and bytes per call;
  - the host path over the same bits on one core: dabgpu::packetAssembler (tests/cpp's
    libconsumers.so, one bit per byte, bit-serial packet CRC) for every stream and entry,
    plus a CRC over every delivered group (binascii's table-driven CRC-CCITT, so a lower
    bound on check_CRC_bits), without the PCIe copy the host path also needs.
Under rocprofv3 --kernel-trace --stats the four kernels' shares come from its table.
Usage: python tools/packet_bench.py [--calls 3]
"""
import argparse
import binascii
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
    subs = [dabamd.Subch(s[0], s[1], s[2], s[3], 1, dabamd.SUBCH_PACKET) for s in sub]
    pipe = dabamd.Pipeline(ctx, E, F, subs)
    pipe.set_iq_format(dabamd.IQ_S16)
    pipe.set_packed(True)
    pipe.control(dabamd.CTL_ACQ_SYNC)
    # the entries' packet streams
    rng = np.random.default_rng(5)
    need = 4 * F * args.calls
    streams = []
    for k in range(NK):
        pk = []
        while sum(len(p) for p in pk) < need * 3 * BR:
            g = pp.group(bytes(rng.integers(0, 256, int(rng.integers(20, 1500)), dtype=np.uint8)), crcf=1, seg=1, segno=k)
            pk += pp.packetize(g, 0x100 + k, [int(x) for x in rng.integers(0, 4, 5)])
        pk = [p if rng.integers(0, 40) else bytes([p[0], p[1], p[2], p[3] ^ 1]) + p[4:] for p in pk]
        streams.append(pp.rows(pk, BR)[:need])
    ms = pipe.msc_stride_packed
    times, recs = [], []
    fed_rows = [[] for _ in range(NK)]
    for call in range(args.calls):
        pipe.run(diq, stride, [stride] * E, download=False)
        pipe.sync()
        ev = pipe.msc_entry_valid()
        host = np.zeros((E, 4 * F, NK, ms), np.uint8)
        for k in range(NK):
            host[:, :, k, :3 * BR] = streams[k][call * 4 * F:(call + 1) * 4 * F][None]
            fed_rows[k] += [streams[k][call * 4 * F + q] for q in range(4 * F) if ev[0, q, k]]
        pipe.msc_d.upload_at(host, 0)
        ctx.sync()
        t0 = time.perf_counter()
        pipe.packet(download=False)
        pipe.sync()
        times.append((time.perf_counter() - t0) * 1e3)
        run = np.frombuffer(pipe.pkr_d.download(np.uint8, E * NK * 16).tobytes(), dabamd.PACKET_RUN_DTYPE)
        info = np.frombuffer(pipe.pki_d.download(np.uint8, E * 4 * F * NK * 12).tobytes(), dabamd.PACKET_INFO_DTYPE)
        recs.append(dict(packets=int(info["packets"].sum()), crc_errors=int(info["crc_errors"].sum()),
                         groups=int(run["n_groups"].sum()), bytes=int(run["n_bytes"].sum()),
                         fed_cifs=int(np.count_nonzero(info["status"] == 0))))
    out = dict(shape=f"{E} streams x {F} frames x {NK} packet entries of {BR} kbit/s", layer_ms=times, calls=recs)
    # the host path on one core over what one stream's entries were fed, times the streams
    so = os.path.join(ROOT, "tests", "cpp", "build", "libconsumers.so")
    if os.path.exists(so):
        l = C.CDLL(so)
        l.cw_pa_new.restype = C.c_void_p
        l.cw_pa_new.argtypes = [C.c_int, C.c_int]
        l.cw_pa_add.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        l.cw_item.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        bits = [np.ascontiguousarray(np.unpackbits(np.array(r), axis=1)) for r in fed_rows]
        t0 = time.perf_counter()
        handles = []
        for k in range(NK):
            h = l.cw_pa_new(60, 0)
            for row in bits[k]:
                l.cw_pa_add(h, row.ctypes.data, len(row))
            handles.append(h)
        t_asm = time.perf_counter() - t0
        buf = np.zeros(8 * 16384, np.uint8)
        groups = []
        for h in handles:
            i = 0
            while True:
                n = l.cw_item(h, i, buf.ctypes.data, len(buf), None)
                if n < 0:
                    break
                groups.append(np.packbits(buf[:n]).tobytes())
                i += 1
        t0 = time.perf_counter()
        good = sum(1 for g in groups if len(g) >= 2 and binascii.crc_hqx(g[:-2], 0xFFFF) ^ 0xFFFF == g[-2] << 8 | g[-1])
        t_crc = time.perf_counter() - t0
        cifs = sum(len(b) for b in bits)
        out["host_one_core"] = dict(cifs_per_stream=cifs, groups_per_stream=len(groups), good_group_crcs=good,
                                    assembler_ms_per_stream=t_asm * 1e3, group_crc_ms_per_stream=t_crc * 1e3,
                                    ms_all_streams_all_calls=(t_asm + t_crc) * 1e3 * E,
                                    ms_per_call_all_streams=(t_asm + t_crc) * 1e3 * E / args.calls)
    print(json.dumps(out))
    pipe.close()
    ctx.close()


if __name__ == "__main__":
    main()
