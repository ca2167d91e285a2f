"""TEST INFRASTRUCTURE: the host rateConverter (host/rate_converter.h) from Python, through
tests/cpp/rate_wrap.cpp, for the rate conversion tests on both sides: the golden file is compared
with it on the CPU, dabgpu_rate_convert with it on the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
WRAP = os.path.join(BUILD, "librratewrap.so")
SANITIZE = os.path.join(BUILD, "rate_sanitize")
DROPIN = os.path.join(BUILD, "test_rate_dropin")
MAKEFILE = os.path.join(ROOT, "tests", "cpp", "Makefile.rate")
KAT = os.path.join(ROOT, "tests", "golden", "rate_kat.npz")

IQ_F32, IQ_U8, IQ_S16, IQ_S12 = 0, 1, 2, 3
DTYPE = {IQ_F32: np.float32, IQ_U8: np.uint8, IQ_S16: np.int16, IQ_S12: np.int16}

_lib = None


def wrap():
    """the wrapper library, built here when build()'s copy is not there"""
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-f", MAKEFILE, WRAP], check=True)
        l = C.CDLL(WRAP)
        l.rw_new.restype = C.c_void_p
        l.rw_new.argtypes = [C.c_int, C.c_int]
        l.rw_free.argtypes = [C.c_void_p]
        l.rw_block.argtypes = [C.c_void_p]
        l.rw_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        l.rw_convert.restype = C.c_longlong
        l.rw_convert.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong]
        _lib = l
    return _lib


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def blocks(n_in, M):
    return 0 if n_in < 1 else (n_in - 1) // M


class Converter:
    """one rateConverter: feed(x) returns the cf32 samples [n, 2] the chunk completed"""

    def __init__(self, rate, fmt):
        self.l, self.fmt = wrap(), fmt
        self.h = self.l.rw_new(rate, fmt)
        assert self.h, (rate, fmt)
        self.M = self.l.rw_block(self.h)

    def tables(self):
        base, frac = np.zeros(2048, np.int16), np.zeros(2048, np.float32)
        self.l.rw_tables(self.h, base.ctypes.data, frac.ctypes.data)
        return base, frac

    def feed(self, x):
        x = np.ascontiguousarray(x, DTYPE[self.fmt]).reshape(-1, 2)
        out = np.zeros((2048 * (len(x) // self.M + 2), 2), np.float32)
        n = self.l.rw_convert(self.h, x.ctypes.data, len(x), out.ctypes.data, len(out))
        assert 0 <= n <= len(out)
        return out[:n]

    def close(self):
        if self.h:
            self.l.rw_free(self.h)
            self.h = None


def convert(rate, fmt, x, chunk=None):
    """the whole of x through a new converter, in chunks of `chunk` samples (None: at once)"""
    c = Converter(rate, fmt)
    x = np.ascontiguousarray(x, DTYPE[fmt]).reshape(-1, 2)
    step = len(x) if chunk is None else chunk
    got = [c.feed(x[i:i + step]) for i in range(0, len(x), max(step, 1))] or [np.zeros((0, 2), np.float32)]
    c.close()
    return np.concatenate(got)
