"""The pipeline layers' slot logic (sdr-j-dab_amd/csrc/layer_slots.h: which table entry owns which
slot of a layer, which slot's state goes on across a table change) against the per-layer loops it
replaced, restated in tests/cpp/test_layer_slots.cpp: host code with its own main, built here from
the header alone (no GPU library) -- under AddressSanitizer and UBSan where they link."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_layer_slots")


def test_slot_maps_and_carry_plans_equal_the_per_layer_loops():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall",
           "-I" + os.path.join(ROOT, "sdr-j-dab_amd", "csrc"), "-o", EXE,
           os.path.join(ROOT, "tests", "cpp", "test_layer_slots.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        print("sanitizers do not link here: plain build")
        subprocess.run(cmd, check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "LAYER SLOTS OK" in r.stdout, r.stdout + r.stderr
