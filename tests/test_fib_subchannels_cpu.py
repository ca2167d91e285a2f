"""fib_processor::subchannels() (sdr-j-dab_amd/host/fib_processor.*): the FIG 0/1
sub-channel organisation of a synthetic ensemble's FIBs (dabsynth, figs = 1) as the table
dabgpu_pipe_set_subch takes -- UEP short form, EEP long form (A and B), the DAB+ flag from
FIG 0/2, ordered by SubChId and stable from the second FIG cycle.  Checked by
tests/cpp/test_fib_subchannels.cpp, built here from fib_processor.cpp alone (host code, no
GPU library) with test_fib's compile line."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sdr-j-dab_amd")
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_fib_subchannels")


def test_fib_subchannels_match_transmitted_table():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(PKG, "host"),
                    "-I" + os.path.join(PKG, "synth"), "-o", EXE,
                    os.path.join(ROOT, "tests", "cpp", "test_fib_subchannels.cpp"),
                    os.path.join(PKG, "host", "fib_processor.cpp"), "-L" + os.path.join(PKG, "lib"), "-ldabsynth",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "FIB SUBCHANNELS OK" in r.stdout, r.stdout + r.stderr
