"""audioSink::audioOut (audiosink.cpp:235-360) over LowPassFIR::Pass (fir-filters.cpp:78-92) in
numpy float32: the expectation of the audio output tests where no golden file exists, itself
pinned against tests/golden/sink_kat.npz (tests/test_sink_cpu.py).

Every product, sum and difference is one float32 array operation, so each is rounded to float32
on its own, in the reference's order: out[n] = sum_{i=0..4} s[n-i] * k[i] from (0, 0), each term
the complex product with (k[i], 0) spelled out (re = s.re*k - s.im*0, im = s.re*0 + s.im*k).
"""
import math

import numpy as np

RATES = (16000, 24000, 32000)            # the filters, in DABGPU_TABLE_AUDIO_FIR's order
F32 = np.float32


def coefs() -> np.ndarray:
    """float32 [3, 5]: LowPassFIR (5, 16000, 48000), (5, 24000, 48000), (5, 32000, 96000)
    (fir-filters.cpp:35-69): f, temp and sum float, the rest double"""
    out = np.zeros((3, 5), F32)
    for r, (fc, fs) in enumerate(((16000, 48000), (24000, 48000), (32000, 96000))):
        f = F32(fc) / F32(fs)
        temp = np.zeros(5, F32)
        total = F32(0.0)
        for i in range(5):
            d = i - 2
            t = F32(2 * math.pi * float(f)) if d == 0 else F32(math.sin(2 * math.pi * float(f) * d) / d)
            t = F32(float(t) * (0.42 - 0.5 * math.cos(2 * math.pi * float(i) / 5) + 0.08 * math.cos(4 * math.pi * float(i) / 5)))
            temp[i] = t
            total = F32(total + t)
        out[r] = temp / total
    return out


def scale(pcm: np.ndarray) -> np.ndarray:
    """float (V) / 32767.0: a double division rounded to float"""
    return (np.asarray(pcm, np.int16).astype(F32).astype(np.float64) / 32767.0).astype(F32)


def n_out(amount: int, rate: int) -> int:
    return {16000: 3 * amount, 24000: 2 * amount, 32000: 3 * amount // 2}.get(rate, amount)


class Sink:
    """one audioSink: three filters that live as long as it does"""

    def __init__(self, k: np.ndarray = None):
        self.k = coefs() if k is None else np.asarray(k, F32)
        self.hist = np.zeros((3, 4, 2), F32)         # per filter: the last four stuffed samples it saw

    def audio_out(self, pcm: np.ndarray, rate: int) -> np.ndarray:
        """pcm int16 [amount, 2] -> float32 [n_out, 2]; rate 0 is no call"""
        pcm = np.asarray(pcm, np.int16).reshape(-1, 2)
        if rate == 0 or len(pcm) == 0:
            return np.zeros((0, 2), F32)
        x = scale(pcm)
        if rate not in RATES:
            return x
        r = RATES.index(rate)
        if r == 2 and len(pcm) & 1:
            raise ValueError("odd amount at 32000")
        up = 2 if r == 1 else 3
        n = up * len(x)
        s = np.zeros((4 + n, 2), F32)
        s[:4] = self.hist[r]
        s[4::up] = x
        zero = F32(0.0)
        acc = np.zeros((n, 2), F32)
        for i in range(5):
            seg = s[4 - i:4 - i + n]
            k = self.k[r, i]
            acc[:, 0] = acc[:, 0] + (seg[:, 0] * k - seg[:, 1] * zero)
            acc[:, 1] = acc[:, 1] + (seg[:, 0] * zero + seg[:, 1] * k)
        self.hist[r] = s[-4:]
        return acc[::2].copy() if r == 2 else acc


# ---- the scripted sequences of tests/golden/sink_kat.npz ------------------------------------------
def _pcm(rng, n):
    """n seeded pairs holding the extremes, 0, +-1 and an isolated full-scale pair after three
    zero pairs (and before three more), as far as n goes"""
    v = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    marks = np.array([[0, 0], [0, 0], [0, 0], [32767, -32768], [0, 0], [0, 0], [0, 0], [-32768, 32767], [1, -1], [-1, 1], [0, 0]],
                     np.int16)
    if n >= 8:
        m = marks[:min(len(marks), n)]
        at = (n - len(m)) // 2
        v[at:at + len(m)] = m
    return v


def sequences():
    """[(name, [(rate, pcm int16 [amount, 2]), ...])]: each sequence is one sink's calls in order"""
    rng = np.random.default_rng(20261021)
    script = [("a", [(24000, a) for a in (1, 1, 2, 3, 96, 1152)]),
              ("b", [(48000, 96), (24000, 96), (48000, 96), (24000, 96)]),
              ("c", [(16000, a) for a in (1, 2, 96)]),
              ("d", [(32000, 2), (32000, 4), (32000, 96), (16000, 3)]),
              ("e", [(44100, 8)])]
    seqs = [(name, [(rate, _pcm(rng, a)) for rate, a in calls]) for name, calls in script]
    seqs.append(("f", [(rate, np.zeros((8, 2), np.int16)) for rate in (48000, 24000, 16000, 32000, 24000)]))
    return seqs
