"""ensembleDecoder::on_mot_object (host/dabgpu_dropin.h) on the synthesised signal: a C++ program
over the drop-in library, auto_layout on the transmitter's FIGs, 10 steps of 6 frames.  The
program itself holds every object the GPU's MOT layer delivers to the host motAssembler fed the
groups on_datagroup delivered (tests/cpp/test_mot_dropin.cpp: record fields, names, bodies, the
completing group's CIF, step by step); here: the table the decoder parsed flags the DSCTy 60
components for MOT, and every slide of the carousel arrives, more than once."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 6
PACKET, MOTF = 8, 16


def test_dropin_on_mot_object(tmp_path):
    from dabamd.synth import Ensemble, MP2, PACKET as SP, MOT
    # the layout of test_gpu_mot's pipeline test, 61 frames: the table is applied after two steps
    # that parsed it alike and delivers 16 CIFs later, which leaves more than two rounds of the
    # carousel (19 frames carry one, as test_gpu_mot's fixture asserts)
    tx = [(0, 48, 64, 0o103, 0, 0, MOT), (48, 24, 32, 0o103, 0, 0, SP), (144, 96, 128, 3, 1, 0, MP2)]
    e = Ensemble(10 * F + 1, subch=tx, figs=True)
    e.generate(511, truth=False)["iq"].tofile(tmp_path / "iq.f32")
    subprocess.run(["make", "-s", "-f", os.path.join(ROOT, "tests", "cpp", "Makefile.mot")], check=True)
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "build", "test_mot_dropin"), str(tmp_path / "iq.f32"), str(F), "10"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MOT DROPIN OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    table, objs = None, []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "TABLE":
            step, table = int(w[1]), [tuple(int(x) for x in t.split(":")) for t in w[3:]]
        elif w[0] == "OBJ":
            objs.append((int(w[1]), int(w[2]), int(w[3]), int(w[4]), int(w[5]), bytes.fromhex(w[6]) if len(w) > 6 else b""))
    # both packet-mode components are announced as DSCTy 60, so both are flagged for MOT (the
    # plain one's random groups are hostile input, equal to the host's all the same); without
    # on_pcm the layer II entry stays unflagged
    assert table is not None and step <= 2
    assert table == [(a, n, br, pl, 0 if uep else 1, {MOT: PACKET | MOTF, SP: PACKET | MOTF, MP2: 0}[c])
                     for a, n, br, pl, uep, _, c in tx]
    slides = [o for o in objs if o[0] == 0]
    print("drop-in:", len(objs), "objects,", len(slides), "on the carousel's entry, table applied after step", step)
    assert len(slides) >= 8 and {o[2] for o in slides} == {0x1000, 0x1001, 0x1002, 0x1003}
    assert all(kind == 1 and name == b"s0_%d.jpg" % (tid & 15) and nbytes > 0 for _, _, tid, kind, nbytes, name in slides)
    assert [o[1] for o in slides] == sorted(o[1] for o in slides)          # in completion order
