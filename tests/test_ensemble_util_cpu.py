"""The pure pieces of ensembleDecoder (sdr-j-dab_amd/host/ensemble_util.h: the slot rule
entries_flagged / count_flagged, unpack_bits, the flags auto_layout asks the FIC for, the .sdr
header walk) against the loops and spellings they replaced, restated in
tests/cpp/test_ensemble_util.cpp, and on RIFF/WAVE files that program writes: host code with its own
main, built here from the header alone (no GPU library) -- under AddressSanitizer and UBSan where
they link."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_ensemble_util")


def test_ensemble_util_equals_the_loops_it_replaced(tmp_path):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "sdr-j-dab_amd", "host"), "-o", EXE,
           os.path.join(ROOT, "tests", "cpp", "test_ensemble_util.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        print("sanitizers do not link here: plain build")
        subprocess.run(cmd, check=True)
    r = subprocess.run([EXE, str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ENSEMBLE UTIL OK" in r.stdout, r.stdout + r.stderr
