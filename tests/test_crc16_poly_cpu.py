"""The kernels' CRC-16-CCITT arithmetic (sdr-j-dab_amd/csrc/crc16_poly.h: the multiply, the powers
of x^8, the byte step, the preset's share) against a bit-at-a-time CRC written from check_CRC_bits'
definition, in tests/cpp/test_crc16_poly.cpp: host code with its own main, built here from the
header alone (no GPU library) -- under AddressSanitizer and UBSan where they link."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_crc16_poly")


def test_crc_header_equals_the_bitwise_crc_and_its_slices_join():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall",
           "-I" + os.path.join(ROOT, "sdr-j-dab_amd", "csrc"), "-o", EXE,
           os.path.join(ROOT, "tests", "cpp", "test_crc16_poly.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        print("sanitizers do not link here: plain build")
        subprocess.run(cmd, check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "CRC16 POLY OK" in r.stdout, r.stdout + r.stderr
