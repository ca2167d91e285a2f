"""ensembleDecoder with config::fic_on_gpu (host/dabgpu_dropin.h) on the synthesised signal: a C++
program over the drop-in library runs two decoders on two streams with different layouts,
auto_layout on the transmitter's FIGs, 5 steps of 3 frames: one parses the FIBs with the host's
fib_processors, the other on the GPU (dabgpu_pipe_fic).  The program itself holds them equal step
by step (tests/cpp/test_fic_dropin.cpp: the applied tables -- so the same set_subch calls at the
same steps --, the names and their frames, the MSC deliveries, and at the end database(stream)'s
labels and lookups); here: the tables are the transmitter's, the names are the transmitter's, the
lookups find the sub-channels."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, STEPS = 3, 5
TX = [[(0, 24, 32, 0o103, 0, 1, 0), (24, 48, 64, 0o103, 0, 1, 0)],
      [(10, 84, 96, 2, 1, 0, 0), (100, 24, 32, 0o103, 0, 1, 0), (130, 24, 32, 0o103, 0, 1, 0)]]


def test_dropin_fic_on_gpu_equals_host_parse(tmp_path):
    from dabamd.synth import Ensemble
    for s, tx in enumerate(TX):
        Ensemble(F * STEPS + 1, subch=tx, figs=True).generate(700 + s, truth=False)["iq"].tofile(tmp_path / f"iq{s}.f32")
    subprocess.run(["make", "-s", "-f", os.path.join(ROOT, "tests", "cpp", "Makefile.fic")], check=True)
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "build", "test_fic_dropin"), str(tmp_path / "iq0.f32"),
                        str(tmp_path / "iq1.f32"), str(F), str(STEPS)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FIC DROPIN OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    tables, names, lookups = {}, [], []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "TABLE":
            tables.setdefault(int(w[2]), []).append((int(w[1]), [tuple(int(x) for x in t.split(":")) for t in w[3:]]))
        elif w[0] == "NAME":
            names.append((int(w[1]), int(w[2]), w[3], int(w[4]), bytes.fromhex(w[5]).decode()))
        elif w[0] == "LOOKUP":
            lookups.append((int(w[1]), bytes.fromhex(w[2]).decode(), int(w[3]), int(w[4]), int(w[5])))
    print("drop-in:", r.stdout.splitlines()[-1])
    for s, tx in enumerate(TX):
        step, table = tables[s][-1]
        assert step <= 2 and len(tables[s]) == 1
        assert table == [(a, n, br, pl, 0 if uep else 1, 1 if dp else 0) for a, n, br, pl, uep, dp, _ in tx]
        got = [(k, eid, t) for st, _, k, eid, t in names if st == s]
        assert ("E", 0xE1C3, "SYNTH ENSEMBLE  ") in got and len([g for g in got if g[0] == "E"]) == 1
        assert sorted(t for k, _, t in got if k == "S") == ["SERVICE %02d      " % i for i in range(len(tx))]
        for i in range(len(tx)):
            assert (s, "SERVICE %02d      " % i, 0o101, i, -1) in lookups
        assert (s, "nothing", 0o100, -1, -1) in lookups
