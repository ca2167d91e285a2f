"""ensembleDecoder (host/dabgpu_dropin.h) with two streams of different layouts and every callback
set: the element index stream * slots + slot of the packet, MOT, IP, PAD, layer II and audio
layers at stream index 1, which the one-stream drop-in tests never reach.  A C++ program over the
drop-in library (tests/cpp/test_streams_dropin.cpp) decodes signal A (MOT, IP, layer II) and
signal B (DAB+ with PAD, DAB+, layer II) alone, as the pair (A, B) and as the pair (B, A), 10 steps
of 6 frames, auto_layout on the transmitter's FIGs.  The program itself holds each stream's log of
a pair (every callback: name, CIF or frame, entry, record fields, hash of the bytes) to the log of
that signal decoded alone, line for line, and the order of the callbacks within a step that the
header documents; here: it said so, and every kind of callback occurred on the signal that
carries it."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 6
STEPS = 10
KINDS_A = {"fib", "msc", "ensemble_name", "service_name", "pcm", "audio", "datagroup", "packet_quality", "mot_object", "datagram",
           "ip_quality"}
KINDS_B = {"fib", "msc", "superframe", "ensemble_name", "service_name", "pcm", "audio", "dynamic_label", "pad_datagroup", "pad_object"}


@pytest.fixture(scope="module")
def signals(tmp_path_factory):
    from dabamd.synth import Ensemble, MP2, MOT, IP, PAD
    d = tmp_path_factory.mktemp("streams")
    a = [(0, 48, 64, 0o103, 0, 0, MOT), (48, 48, 64, 0o103, 0, 0, IP), (144, 96, 128, 3, 1, 0, MP2)]
    b = [(0, 24, 32, 0o103, 0, 1, PAD), (24, 24, 32, 0o103, 0, 1, 0), (144, 96, 128, 3, 1, 0, MP2)]
    for name, tx, seed in (("a", a, 511), ("b", b, 611)):
        Ensemble(STEPS * F + 1, subch=tx, figs=True).generate(seed, truth=False)["iq"].tofile(d / (name + ".f32"))
    subprocess.run(["make", "-s", "-f", os.path.join(ROOT, "tests", "cpp", "Makefile.streams")], check=True)
    return str(d / "a.f32"), str(d / "b.f32")


@pytest.mark.parametrize("fic", ["host", "gpu"])
def test_dropin_two_streams_every_callback(signals, fic):
    """fic: the tables come from the host's fib_processors or from the GPU's FIC layer"""
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "build", "test_streams_dropin"), signals[0], signals[1], str(F), str(STEPS)] +
                       (["gpu"] if fic == "gpu" else []), capture_output=True, text=True, timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "STREAMS DROPIN OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    count = {(w[1], w[2]): int(w[3]) for w in (l.split() for l in r.stdout.splitlines()) if w and w[0] == "COUNT"}
    assert {k for s, k in count if s == "A"} == KINDS_A and {k for s, k in count if s == "B"} == KINDS_B
    assert all(n > 0 for n in count.values()), count
