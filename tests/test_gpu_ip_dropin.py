"""ensembleDecoder::on_datagram and on_ip_quality (host/dabgpu_dropin.h) on the synthesised signal:
a C++ program over the drop-in library, auto_layout on the transmitter's FIGs, 10 steps of 6
frames.  The program itself holds every datagram and show_ipErrors value the GPU's IP layer
delivers to the host ipAssembler fed the groups on_datagroup delivered (tests/cpp/
test_ip_dropin.cpp: bytes, order, the group's CIF, step by step); here: the table the decoder
parsed flags the DSCTy 59 component for IP, and the synthesiser's datagrams arrive in order."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 6
PACKET, IPF = 8, 64


@pytest.mark.parametrize("fic", ["host", "gpu"])
def test_dropin_on_datagram(tmp_path, fic):
    """fic: the table comes from the host's fib_processor or from the GPU's FIC layer"""
    from dabamd.synth import Ensemble, MP2, PACKET as SP, IP, ip_carousel
    tx = [(0, 48, 64, 0o103, 0, 0, IP), (48, 24, 32, 0o103, 0, 0, SP), (144, 96, 128, 3, 1, 0, MP2)]
    seed = 591
    e = Ensemble(10 * F + 1, subch=tx, figs=True)
    e.generate(seed, truth=False)["iq"].tofile(tmp_path / "iq.f32")
    subprocess.run(["make", "-s", "-f", os.path.join(ROOT, "tests", "cpp", "Makefile.ip")], check=True)
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "build", "test_ip_dropin"), str(tmp_path / "iq.f32"), str(F), "10"] +
                       (["gpu"] if fic == "gpu" else []), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "IP DROPIN OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    table, got, quality = None, [], []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "TABLE":
            step, table = int(w[1]), [tuple(int(x) for x in t.split(":")) for t in w[3:]]
        elif w[0] == "DGRAM":
            got.append((int(w[1]), int(w[2]), bytes.fromhex(w[4]) if len(w) > 4 else b""))
            assert len(got[-1][2]) == int(w[3])
        elif w[0] == "QUALITY":
            quality.append((int(w[1]), int(w[2])))
    # the DSCTy 59 component is flagged for IP, the DSCTy 60 one is a plain packet entry (no
    # on_mot_object); without on_pcm the layer II entry stays unflagged
    assert table is not None and step <= 2
    assert table == [(a, n, br, pl, 0 if uep else 1, {IP: PACKET | IPF, SP: PACKET, MP2: 0}[c]) for a, n, br, pl, uep, _, c in tx]
    assert {k for k, _, _ in got} == {0} and {k for k, _ in quality} == {0}
    # the carousel's deliverable datagrams, round and round from wherever the entry came in
    car = ip_carousel(seed, 0)
    want = [g[2 + 4 * (g[2] & 15) + 8:len(g) - (2 if g[0] & 0x40 else 0)] for k, g in enumerate(car) if k % 7 != 6 and k % 11 != 10]
    # 174 CIFs at least after the table is applied (step <= 2) carry about 0.9 groups each (192 bytes a CIF, one packet in
    # eight padding, 5 of 24..96 packet bytes overhead, half a packet lost per group of 137 bytes on average): two rounds
    assert len(want) == 34 and len(got) >= 68
    first = want.index(got[0][2])
    assert [d for _, _, d in got] == [want[(first + i) % len(want)] for i in range(len(got))]
    assert [c for _, c, _ in got] == sorted(c for _, c, _ in got)          # in group order
    print("drop-in:", len(got), "datagrams, show_ipErrors", quality, "table applied after step", step)
    assert quality and all(84 <= q <= 89 for _, q in quality)              # six bad checksums a round of 44


def test_fic_layer_flags_ip_components():
    """dabgpu_fib_parse's table with the DABGPU_SUBCH_IP bit of want_flags, on the transmitter's FIBs:
    what fib_processor::subchannels gives with its ip argument (tests/cpp/test_fib_ip.cpp holds the
    same table on the host class): the DSCTy 59 entry is flagged 8 | 64 with the bit, with or without
    the packet bit, the DSCTy 60 entry never gets 64, and without the bit nothing changes"""
    import dabamd
    from dabamd.synth import Ensemble, MP2, MOT, IP
    tx = [(0, 96, 128, 3, 1, 0, MP2), (96, 48, 64, 0o103, 0, 0, IP), (144, 24, 32, 0o103, 0, 0, MOT), (200, 48, 64, 0o103, 0, 1, 0)]
    fic = Ensemble(8, subch=tx, figs=True).generate(7)["fic"]
    fibs = np.packbits(fic.reshape(-1, 256), axis=1)[None]
    ctx = dabamd.Context(0)
    try:
        # want bit 8: packet data, 16: MOT, 64: IP -> the flags of the four entries
        for want, flags in ((0, [0, 0, 0, 1]), (8, [0, 8, 8, 1]), (16, [0, 0, 24, 1]), (24, [0, 8, 24, 1]), (64, [0, 72, 0, 1]),
                            (72, [0, 72, 8, 1]), (80, [0, 72, 24, 1]), (88, [0, 72, 24, 1])):
            _, _, table, run = dabamd.fib_parse(ctx, fibs, np.ones(fibs.shape[:2], np.uint8), None, want)
            assert int(table[0]["n"]) == 4 and table[0]["sub"][:4]["flags"].tolist() == flags, (want, table[0]["sub"][:4])
            assert table[0]["sub"][:4]["startAddr"].tolist() == [t[0] for t in tx]
    finally:
        ctx.close()
