"""ensembleDecoder with per-stream tables (sdr-j-dab_amd/host/dabgpu_dropin.h: config's
caps, set_subch, auto_layout) on the GPU: tests/cpp/test_layouts.cpp decodes two synthetic
ensembles that announce different sub-channel sets (one with a DAB+ sub-channel) from an
empty table; each stream's table must become its transmitter's and every MSC callback past
since_cif + 16 must carry the transmitter's bits.  Built here with test_dropin's compile
line."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sdr-j-dab_amd")
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_layouts")


def _build():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib, orc = os.path.join(PKG, "lib"), os.path.join(ROOT, "oracle")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(PKG, "host"), "-I" + os.path.join(PKG, "synth"), "-I" + orc, "-o", EXE,
                    os.path.join(ROOT, "tests", "cpp", "test_layouts.cpp"), "-L" + lib, "-ldabgpu_dropin", "-ldabgpu",
                    "-ldabsynth", "-L" + orc, "-loracle", "-Wl,-rpath," + lib, "-Wl,-rpath," + orc], check=True)


@pytest.mark.gpu
def test_ensemble_decoder_follows_each_streams_fic():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "LAYOUTS OK" in r.stdout, r.stdout + r.stderr


def test_layouts_program_builds():
    """the program links on a host without a GPU"""
    _build()
    assert os.path.exists(EXE)
