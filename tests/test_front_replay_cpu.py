"""The pipeline's front-end replay (sdr-j-dab_amd/csrc/front_replay.h: predict a batch of
frames per stream, replay ofdmProcessor::run's per-frame logic on the measured values, commit
the correctly predicted prefix) against the reference's loop taken one frame at a time, on a
synthetic channel: tests/cpp/test_front_replay.cpp, host code with its own main, built here
from the header alone (no GPU library) -- under AddressSanitizer and UBSan where they link."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_front_replay")


def test_batch_replay_equals_one_frame_at_a_time():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall",
           "-I" + os.path.join(ROOT, "sdr-j-dab_amd", "csrc"), "-o", EXE,
           os.path.join(ROOT, "tests", "cpp", "test_front_replay.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        print("sanitizers do not link here: plain build")
        subprocess.run(cmd, check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "FRONT REPLAY OK" in r.stdout, r.stdout + r.stderr
