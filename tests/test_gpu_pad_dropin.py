"""ensembleDecoder::on_dynamic_label / on_pad_datagroup / on_pad_object (host/dabgpu_dropin.h) on
the synthesised signal: a C++ program over the drop-in library, auto_layout on the transmitter's
FIGs, 6 steps of 6 frames.  The program itself holds every label, X-PAD data group and slide the
GPU delivers to the host padAssembler + motAssembler fed the AUs on_superframe delivered
(tests/cpp/test_pad_dropin.cpp: records, text and pieces, group bytes, names, bodies, CIFs, step
by step); here: the table the decoder parsed flags the DAB+ components for PAD, and the
programme's labels and its slide arrive; and the one-stream mp4Processor drop-in's optional PAD
hook, behind which a padAssembler shows the same labels."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 6
DABPLUS, PADF = 1, 32


def test_dropin_pad_callbacks(tmp_path):
    from dabamd.synth import Ensemble, PAD
    # the table is applied after two steps that parsed it alike and delivers 16 CIFs later: the
    # rest holds the 29-PAD programme (one PAD an AU, four AUs a superframe) about twice
    tx = [(0, 24, 32, 0o103, 0, 1, PAD), (24, 24, 32, 0o103, 0, 1, 0)]
    e = Ensemble(6 * F + 1, subch=tx, figs=True)
    e.generate(611, truth=False)["iq"].tofile(tmp_path / "iq.f32")
    subprocess.run(["make", "-s", "-f", os.path.join(ROOT, "tests", "cpp", "Makefile.pad")], check=True)
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "build", "test_pad_dropin"), str(tmp_path / "iq.f32"), str(F), "6"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PAD DROPIN OK" in r.stdout and "HOOK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    table, labels, objs = None, [], []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "TABLE":
            step, table = int(w[1]), [tuple(int(x) for x in t.split(":")) for t in w[3:]]
        elif w[0] == "LABEL":
            labels.append((int(w[1]), int(w[2]), int(w[3]), bytes.fromhex(w[4]) if len(w) > 4 else b""))
        elif w[0] == "OBJ":
            objs.append((int(w[1]), int(w[2]), int(w[3]), int(w[4]), int(w[5]), bytes.fromhex(w[6]) if len(w) > 6 else b""))
    # with a PAD callback set, auto_layout flags the DAB+ audio components DABPLUS | PAD
    assert table is not None and step <= 2
    assert table == [(a, n, br, pl, 0 if uep else 1, DABPLUS | PADF) for a, n, br, pl, uep, _, _ in tx]
    texts = [t for k, _, _, t in labels if k == 0]
    print("drop-in:", len(labels), "labels,", len(objs), "objects, table applied after step", step, r.stdout.splitlines()[-1])
    assert b"ABC" in texts and b"sub 0 charset 0" in texts and any(t.startswith(b"DABSYNTH s0 - now playing: track") for t in texts)
    assert {cs for k, _, cs, _ in labels if k == 0} == {0, 15}
    slides = [o for o in objs if o[0] == 0]
    assert slides and all(tid == 0x1000 and kind == 1 and nbytes == 230 and name == b"s0_0.jpg" for _, _, tid, kind, nbytes, name in slides)
    assert [l[1] for l in labels if l[0] == 0] == sorted(l[1] for l in labels if l[0] == 0)
