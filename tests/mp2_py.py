"""MPEG-1/2 layer II in numpy, for the tests of the GPU layer II layer (k_mp2.hip).

Three pieces:
  * the tables of mp2Processor (mp2processor.cpp:48-213) in this project's own form:
    the synthesis window as its upper half (the lower half follows by the window's
    symmetry, the table's rounding by a rule), the quantiser classes as functions of the
    bit rate per channel, the subband layouts as runs, the allocation rows as sets;
  * write_frame(): the inverse of the parser -- header fields, allocation, scfsi, scale
    factors and sample codes to a well-formed frame; parse_frame() reads them back;
  * Decoder: mp2Processor::mp2decodeFrame (mp2processor.cpp:365-568) restated in int64
    with the three rules the reference leaves to the compiler or to memory contents:
      - V is int16: a wider value wraps modulo 2^16;
      - bits past the end of the frame read as 0;
      - products and sums are int32, two's complement (wrap).
    Decoder(check=True) asserts instead that no intermediate leaves int32.

tests/golden/mp2_kat.npz (make_mp2_golden.py) pins all of it to the reference's own
decoder: fixtures() below builds the streams that file holds.
"""
import math

import numpy as np

# ---- tables ------------------------------------------------------------------------
# W[256 + k], k = 0..255: the synthesis window of ISO 11172-3 (table 3-B.3, with the
# alternating block signs of the polyphase form folded in) times 65536.
HALF_WINDOW = [
    75038, 74992, 74856, 74630, 74313, 73908, 73415, 72835, 72169, 71420, 70590, 69679,
    68692, 67629, 66494, 65290, 64019, 62684, 61289, 59838, 58333, 56778, 55178, 53534,
    51853, 50137, 48390, 46617, 44821, 43006, 41176, 39336, 37489, 35640, 33791, 31947,
    30112, 28289, 26482, 24694, 22929, 21189, 19478, 17799, 16155, 14548, 12980, 11455,
    9975, 8540, 7154, 5818, 4533, 3300, 2122, 998, -70, -1082, -2037, -2935,
    -3776, -4561, -5288, -5959, 6574, 7134, 7640, 8092, 8492, 8840, 9139, 9389,
    9592, 9750, 9863, 9935, 9966, 9959, 9916, 9838, 9727, 9585, 9416, 9219,
    8998, 8755, 8491, 8209, 7910, 7597, 7271, 6935, 6589, 6237, 5879, 5517,
    5153, 4788, 4425, 4063, 3705, 3351, 3004, 2663, 2330, 2006, 1692, 1388,
    1095, 814, 545, 288, 45, -185, -402, -605, -794, -970, -1131, -1280,
    -1414, -1535, -1644, -1739, -1822, -1893, -1952, -2000, 2037, 2063, 2080, 2087,
    2085, 2075, 2057, 2032, 2001, 1962, 1919, 1870, 1817, 1759, 1698, 1634,
    1567, 1498, 1428, 1356, 1283, 1210, 1137, 1064, 991, 919, 848, 779,
    711, 645, 581, 519, 459, 401, 347, 294, 244, 197, 153, 111,
    72, 36, 2, -29, -57, -83, -106, -127, -146, -163, -177, -189,
    -200, -208, -215, -221, -224, -227, -228, -228, -227, -225, -222, -218,
    213, 208, 202, 196, 190, 183, 176, 169, 161, 154, 147, 139,
    132, 125, 117, 111, 104, 97, 91, 85, 79, 73, 68, 63,
    58, 53, 49, 45, 41, 38, 35, 31, 29, 26, 24, 21,
    19, 17, 16, 14, 13, 11, 10, 9, 8, 7, 7, 6,
    5, 5, 4, 4, 3, 3, 2, 2, 2, 2, 1, 1,
    1, 1, 1, 1,
]


def window():
    """D[512]: W[256 - k] = -W[256 + k] (equal where 256 + k is a multiple of 64), W[0] = 0;
    the table holds trunc(W + 0.5), so a negative W is one closer to zero"""
    w = np.zeros(512, np.int64)
    for k, h in enumerate(HALF_WINDOW):
        w[256 + k] = h
        if k:
            w[256 - k] = h if (256 + k) % 64 == 0 else -h
    return np.where(w < 0, w + 1, w)


def matrix():
    """N[64][32] = (int16)(256 cos((16 + i)(2j + 1) pi / 64)), truncated towards zero, with
    the reference's constant for pi / 64 (mp2processor.cpp:229-233)"""
    n = np.zeros((64, 32), np.int64)
    for i in range(64):
        for j in range(32):
            n[i, j] = int(256.0 * math.cos(((16 + i) * ((j << 1) + 1)) * 0.0490873852123405))
    return n


BITRATES = {0: [32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384],     # MPEG-1
            1: [8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160]}          # MPEG-2 (LSF)
SAMPLE_RATES = {0: [44100, 48000, 32000], 1: [22050, 24000, 16000]}
STEREO, JOINT, DUAL, MONO = 0, 1, 2, 3
SCF_BASE = [0x02000000, 0x01965FEA, 0x01428A30]      # 2^25 * 2^(-k/3)

# subband layouts: runs of (subbands, allocation bits, allocation row)
LAYOUT = {0: [(2, 4, 4), (10, 3, 4)],                                  # low rate (3-B.2c/d)
          1: [(3, 4, 3), (8, 4, 2), (12, 3, 1), (7, 2, 0)],            # high rate (3-B.2a/b)
          2: [(4, 4, 5), (7, 3, 4), (19, 2, 4)]}                       # MPEG-2 LSF (13818-3 B.1)
# allocation rows: the quantisers (1..17) a row offers, in order, after "none"
ROWS = [[1, 2, 17], [1, 2, 3, 4, 5, 6, 17], list(range(1, 15)) + [17],
        [1, 3] + list(range(5, 18)), [1, 2] + list(range(4, 16)) + [17], list(range(1, 16))]


def table_of(lsf, mode, kbps, fs):
    """(layout, sblimit) of a frame: by the bit rate per channel for MPEG-1"""
    if lsf:
        return 2, 30
    per = kbps // (1 if mode == MONO else 2)
    if per <= 48:
        return 0, (12 if fs == 2 else 8)
    if per <= 80:
        return 1, 27
    return 1, (27 if fs == 1 else 30)


def band_of(layout, sb):
    """(allocation bits, row) of subband sb"""
    for n, nbal, row in LAYOUT[layout]:
        if sb < n:
            return nbal, row
        sb -= n
    raise IndexError(sb)


def quantiser(q):
    """(levels, grouped, code-word bits) of quantiser q = 1..17"""
    if q in (1, 2, 4):
        return {1: (3, 1, 5), 2: (5, 1, 7), 4: (9, 1, 10)}[q]
    bits = 3 if q == 3 else q - 1
    return (1 << bits) - 1, 0, bits


def alloc_to_q(row, a):
    return 0 if a == 0 else ROWS[row][a - 1]


# ---- bits ----------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, v, n):
        assert 0 <= v < (1 << n), (v, n)
        self.bits += [(v >> (n - 1 - i)) & 1 for i in range(n)]


class BitReader:
    """msb first from byte 2; bits past the end read as 0 (rule 2)"""

    PAD = 8192        # zero bytes after the frame: more than any frame's fields can run over

    def __init__(self, frame, pos=16):
        self.v = int.from_bytes(bytes(frame) + bytes(self.PAD), "big")
        self.total = 8 * (len(frame) + self.PAD)
        self.pos = pos

    def get(self, n):
        assert self.pos + n <= self.total
        v = (self.v >> (self.total - self.pos - n)) & ((1 << n) - 1)
        self.pos += n
        return v


def frame_geometry(lsf, br_index, fs, mode, mode_ext):
    kbps = BITRATES[lsf][br_index - 1]
    layout, sblimit = table_of(lsf, mode, kbps, fs)
    bound = ((mode_ext + 1) << 2) if mode == JOINT else (0 if mode == MONO else 32)
    return kbps, layout, sblimit, min(bound, sblimit)


def write_frame(spec, nbytes):
    """spec: dict(lsf, br_index 0..15, fs, padding, private, mode, mode_ext, crc (bool: the
    16-bit word present), tail (the header's last 4 bits), alloc[2][32], scfsi[2][32],
    scf[2][32][3], codes[12][2][32][3]) -> nbytes bytes; asserts the fields fit.  A spec
    whose header the decoder rejects (br_index 0 / 15, fs 3) is the header and zeros."""
    w = BitWriter()
    w.put(0xFFF, 12)
    w.put(0 if spec["lsf"] else 1, 1)
    w.put(2, 2)                                   # layer II
    w.put(0 if spec["crc"] else 1, 1)
    w.put(spec["br_index"], 4)
    w.put(spec["fs"], 2)
    w.put(spec.get("padding", 0), 1)
    w.put(spec.get("private", 0), 1)
    w.put(spec["mode"], 2)
    w.put(spec["mode_ext"], 2)
    w.put(spec.get("tail", 0), 4)
    if spec["crc"]:
        w.put(spec.get("crc_word", 0), 16)
    if spec["br_index"] in (0, 15) or spec["fs"] == 3:
        body = spec.get("body")
        if body is not None:
            w.bits += list(body)
    else:
        mode = spec["mode"]
        _, layout, sblimit, bound = frame_geometry(spec["lsf"], spec["br_index"], spec["fs"], mode, spec["mode_ext"])
        nch = 1 if mode == MONO else 2
        alloc, scfsi, scf, codes = spec["alloc"], spec["scfsi"], spec["scf"], spec["codes"]
        for sb in range(sblimit):
            nbal, _ = band_of(layout, sb)
            for ch in range(2 if sb < bound else 1):
                w.put(int(alloc[ch][sb]), nbal)
        for sb in range(sblimit):
            for ch in range(nch):
                if alloc[ch if sb < bound else 0][sb]:
                    w.put(int(scfsi[ch][sb]), 2)
        for sb in range(sblimit):
            for ch in range(nch):
                if alloc[ch if sb < bound else 0][sb]:
                    s = scf[ch][sb]
                    for part in {0: (0, 1, 2), 1: (0, 2), 2: (0,), 3: (0, 2)}[int(scfsi[ch][sb])]:
                        w.put(int(s[part]), 6)
        for g in range(12):
            for sb in range(sblimit):
                _, row = band_of(layout, sb)
                for ch in range(2 if sb < bound else 1):
                    q = alloc_to_q(row, int(alloc[ch][sb]))
                    if not q:
                        continue
                    lev, grouped, bits = quantiser(q)
                    c = [int(x) for x in codes[g][ch][sb]]
                    if grouped:
                        w.put(c[0] + lev * (c[1] + lev * c[2]), bits)
                    else:
                        for x in c:
                            w.put(x, bits)
    assert len(w.bits) <= 8 * nbytes, (len(w.bits), 8 * nbytes)
    bits = np.array(w.bits + [0] * (8 * nbytes - len(w.bits)), np.uint8)
    return bytes(np.packbits(bits))


def _w32(x):
    return ((np.asarray(x, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


class Overflow(AssertionError):
    pass


class Decoder:
    """one mp2Processor's decoder state: the last 15 V vectors per channel, oldest first
    ([2][15][64] int16; zeros for a new processor)"""
    N = matrix()
    D = window()

    def __init__(self, check=False, state=None):
        self.check = check
        self.wrapped = 0                 # V values that did not fit int16 so far
        self.hist = np.zeros((2, 15, 64), np.int64) if state is None else np.array(state, np.int64).reshape(2, 15, 64)

    def state(self):
        return self.hist.astype(np.int16)

    def _i32(self, x):
        x = np.asarray(x, np.int64)
        if self.check:
            if x.size and (x.min() < -(1 << 31) or x.max() >= (1 << 31)):
                raise Overflow("an intermediate leaves int32")
            return x
        return _w32(x)

    def parse(self, frame):
        """the header and side information as mp2decodeFrame reads them: None for a rejected
        header, else a dict with frame_size, the write_frame() fields and `used` bits"""
        f = bytes(frame)
        g = lambda i: f[i] if i < len(f) else 0
        if g(0) != 0xFF or (g(1) & 0xF6) != 0xF4 or (g(2) - 0x10) >= 0xE0:
            return None
        r = BitReader(f)
        bri = r.get(4)
        if bri - 1 < 0 or bri - 1 > 13:
            return None
        fs = r.get(2)
        if fs == 3:
            return None
        lsf = 0 if g(1) & 0x08 else 1
        padding, private, mode = r.get(1), r.get(1), r.get(2)
        mode_ext = r.get(2)
        tail = r.get(4)
        crc = (g(1) & 1) == 0
        crc_word = r.get(16) if crc else 0
        kbps, layout, sblimit, bound = frame_geometry(lsf, bri, fs, mode, mode_ext)
        nch = 1 if mode == MONO else 2
        alloc = np.zeros((2, 32), np.int64)
        q = np.zeros((2, 32), np.int64)
        for sb in range(sblimit):
            nbal, row = band_of(layout, sb)
            for ch in range(2 if sb < bound else 1):
                alloc[ch, sb] = r.get(nbal)
                q[ch, sb] = alloc_to_q(row, alloc[ch, sb])
            if sb >= bound:
                alloc[1, sb], q[1, sb] = alloc[0, sb], q[0, sb]
        scfsi = np.zeros((2, 32), np.int64)
        for sb in range(sblimit):
            for ch in range(nch):
                if q[ch, sb]:
                    scfsi[ch, sb] = r.get(2)
            if mode == MONO:
                scfsi[1, sb] = scfsi[0, sb]
        scf = np.zeros((2, 32, 3), np.int64)
        for sb in range(sblimit):
            for ch in range(nch):
                if q[ch, sb]:
                    k = scfsi[ch, sb]
                    a = r.get(6)
                    if k == 0:
                        scf[ch, sb] = (a, r.get(6), r.get(6))
                    elif k == 1:
                        scf[ch, sb] = (a, a, r.get(6))
                    elif k == 2:
                        scf[ch, sb] = (a, a, a)
                    else:
                        b = r.get(6)
                        scf[ch, sb] = (a, b, b)
            if mode == MONO:
                scf[1, sb] = scf[0, sb]
        codes = np.zeros((12, 2, 32, 3), np.int64)
        for gi in range(12):
            for sb in range(sblimit):
                for ch in range(2 if sb < bound else 1):
                    if not q[ch, sb]:
                        continue
                    lev, grouped, bits = quantiser(int(q[ch, sb]))
                    if grouped:
                        v = r.get(bits)
                        codes[gi, ch, sb] = (v % lev, (v // lev) % lev, v // lev // lev)
                    else:
                        codes[gi, ch, sb] = (r.get(bits), r.get(bits), r.get(bits))
                if sb >= bound:
                    codes[gi, 1, sb] = codes[gi, 0, sb]
        frame_size = 144000 * kbps // SAMPLE_RATES[lsf][fs] + padding
        return dict(lsf=lsf, br_index=bri, fs=fs, padding=padding, private=private, mode=mode, mode_ext=mode_ext,
                    tail=tail, crc=crc, crc_word=crc_word, alloc=alloc, q=q, scfsi=scfsi, scf=scf, codes=codes,
                    frame_size=frame_size, sblimit=sblimit, bound=bound, used=r.pos,
                    sample_rate=SAMPLE_RATES[lsf][fs])

    def samples(self, h):
        """read_samples for the whole frame: [36][2][32] (step = 3 * group + idx)"""
        out = np.zeros((36, 2, 32), np.int64)
        for ch in range(2):
            for sb in range(h["sblimit"]):
                qq = int(h["q"][ch, sb])
                if not qq:
                    continue
                lev = quantiser(qq)[0]
                scale = 65536 // (lev + 1)
                adj = ((lev + 1) >> 1) - 1
                for part in range(3):
                    s = int(h["scf"][ch, sb, part])
                    sf = 0 if s == 63 else (SCF_BASE[s % 3] + ((1 << (s // 3)) >> 1)) >> (s // 3)
                    c = h["codes"][4 * part:4 * part + 4, ch, sb, :]               # [4 groups][3]
                    val = self._i32((adj - c) * scale)
                    hi = self._i32(val * (sf >> 12))
                    lo = self._i32(self._i32(val * (sf & 4095)) + 2048) >> 12
                    out[12 * part:12 * part + 12, ch, sb] = (self._i32(hi + lo) >> 12).reshape(12)
        # above the joint-stereo bound the second channel is a copy of the first one's
        # samples, scale factor included (mp2processor.cpp:508-514)
        out[:, 1, h["bound"]:] = out[:, 0, h["bound"]:]
        return out

    def decode(self, frame):
        """(return value, pcm [1152][2] int16 or None)"""
        h = self.parse(frame)
        if h is None:
            return 0, None
        smp = self.samples(h)
        pcm = np.zeros((1152, 2), np.int16)
        for ch in range(2):
            prod = self.N[None, :, :] * smp[:, ch, None, :]            # [36][64][32]
            if self.check:
                self._i32(np.cumsum(prod, axis=2))
            v = (self._i32(self._i32(prod.sum(axis=2)) + 8192) >> 14)
            self.wrapped += int(np.count_nonzero((v < -32768) | (v > 32767)))
            v = ((v + 32768) & 0xFFFF) - 32768                         # rule 1: V is int16
            vec = np.concatenate([self.hist[ch], v])                   # [15 + 36][64]
            acc = np.zeros((36, 32), np.int64)
            for i in range(16):
                u = vec[15 - i:51 - i, (i & 1) * 32:(i & 1) * 32 + 32]   # step t reads vector t - i
                u = self._i32(self._i32(u * self.D[32 * i:32 * i + 32][None, :]) + 32) >> 6
                acc = self._i32(acc - u)
            acc = self._i32(acc + 8) >> 4
            pcm[:, ch] = np.clip(acc, -32768, 32767).reshape(1152).astype(np.int16)
            self.hist[ch] = vec[36:]
        return h["frame_size"], pcm


def decode_chain(frames, check=False, state=None):
    """frames of one decoder in order -> (ret [n], pcm [n][1152][2] (zeros where ret is 0), state)"""
    d = Decoder(check=check, state=state)
    ret = np.zeros(len(frames), np.int32)
    pcm = np.zeros((len(frames), 1152, 2), np.int16)
    for k, f in enumerate(frames):
        r, p = d.decode(f)
        ret[k] = r
        if p is not None:
            pcm[k] = p
    return ret, pcm, d.state()


# ---- fixtures -------------------------------------------------------------------------
def _cost(layout, sb, a, readers, sfreads=3):
    """bits an allocation a of subband sb adds: 12 groups of code words, and scfsi and
    (at most) three scale factors for each of `readers` channels"""
    if a == 0:
        return 0
    lev, grouped, bits = quantiser(alloc_to_q(band_of(layout, sb)[1], a))
    return 12 * (bits if grouped else 3 * bits) + readers * (2 + 6 * sfreads)


def make_spec(rng, lsf, br_index, fs, mode, mode_ext, crc, nbytes, want, sf_range=(3, 62), counter=None):
    """a well-formed frame of nbytes: allocations taken from `want` (row -> set of allocation
    values not yet seen) while they fit, scfsi cycling through 0..3, now and then a scale
    factor 63"""
    counter = counter if counter is not None else [0]
    kbps, layout, sblimit, bound = frame_geometry(lsf, br_index, fs, mode, mode_ext)
    nch = 1 if mode == MONO else 2
    budget = 8 * nbytes - 32 - (16 if crc else 0)
    slots = []
    for sb in range(sblimit):
        nbal, row = band_of(layout, sb)
        budget -= nbal * (2 if sb < bound else 1)
        for ch in range(2 if sb < bound else 1):
            slots.append((sb, ch))
    alloc = np.zeros((2, 32), np.int64)
    # in random order, the subbands with the longest allocation rows first
    order = sorted(rng.permutation(len(slots)), key=lambda k: -band_of(layout, slots[k][0])[0])
    for k in order:
        sb, ch = slots[k]
        nbal, row = band_of(layout, sb)
        readers = 1 if sb < bound else nch
        pick = 0
        cands = sorted(a for a in want[row] if 0 < a < (1 << nbal))
        cands = [a for a in cands if _cost(layout, sb, a, readers) <= budget]
        if cands:
            pick = cands[int(rng.integers(len(cands)))]
        elif rng.integers(2) and _cost(layout, sb, 1, readers) <= budget:
            pick = 1
        want[row].discard(pick)
        budget -= _cost(layout, sb, pick, readers)
        alloc[ch, sb] = pick
        if sb >= bound:
            alloc[1, sb] = pick
    scfsi = np.zeros((2, 32), np.int64)
    scf = np.zeros((2, 32, 3), np.int64)
    codes = np.zeros((12, 2, 32, 3), np.int64)
    for sb in range(sblimit):
        _, row = band_of(layout, sb)
        for ch in range(2):
            if not alloc[ch, sb]:
                continue
            if ch < nch:
                counter[0] += 1
                k = counter[0] % 4
                s = rng.integers(sf_range[0], sf_range[1] + 1, 3)
                if counter[0] % 7 == 0:
                    s[int(rng.integers(3))] = 63
                if k == 1:
                    s[1] = s[0]
                elif k == 2:
                    s[1] = s[2] = s[0]
                elif k == 3:
                    s[2] = s[1]
                scfsi[ch, sb], scf[ch, sb] = k, s
            else:
                scfsi[ch, sb], scf[ch, sb] = scfsi[0, sb], scf[0, sb]
            lev, grouped, bits = quantiser(alloc_to_q(row, int(alloc[ch, sb])))
            if ch == 0 or sb < bound:
                codes[:, ch, sb, :] = rng.integers(0, lev if grouped else (1 << bits), (12, 3))
            else:
                codes[:, 1, sb, :] = codes[:, 0, sb, :]
    return dict(lsf=lsf, br_index=br_index, fs=fs, padding=0, private=int(rng.integers(2)), mode=mode,
                mode_ext=mode_ext, tail=int(rng.integers(16)), crc=crc, crc_word=int(rng.integers(1 << 16)) if crc else 0,
                alloc=alloc, scfsi=scfsi, scf=scf, codes=codes)


def _br_index(lsf, kbps):
    return BITRATES[lsf].index(kbps) + 1


def fixtures(seed=2024):
    """The streams of tests/golden/mp2_kat.npz: a list of dict(name, bitrate (the
    subchannel's), bits (uint8, one per element), specs (per frame)).  Every frame fills
    its lf bits exactly and starts with twelve 1 bits, so a synchroniser that starts on a
    frame boundary stays on it.  The 24 kHz stream starts 40 bits late: a frame that starts
    at bit 0 of a CIF while the processor still assumes 48 kHz is cut at half its length by
    the reference (lf is taken once per addtoFrame call), which reads stale memory."""
    rng = np.random.default_rng(seed)
    want = {r: set(range(16)) for r in range(6)}
    want[0] = set(range(4))
    want[1] = set(range(8))
    counter = [0]
    out = []

    def stream(name, bitrate, plan, lsf=0, lead=0, sf_range=(3, 62), loud_seed=None):
        r = rng if loud_seed is None else np.random.default_rng(loud_seed)
        nbytes = 3 * bitrate * (2 if lsf else 1)
        specs, bits = [], [0] * lead
        for item in plan:
            if item[0] == "bad":
                _, bri, fs = item
                spec = dict(lsf=lsf, br_index=bri, fs=fs, mode=STEREO, mode_ext=0, crc=False,
                            body=[int(x) for x in r.integers(0, 2, 8 * nbytes - 32)])
            else:
                mode, mode_ext, crc = item
                w = want if loud_seed is None else {k: set(range(1, 16)) for k in range(6)}
                spec = make_spec(r, lsf, _br_index(lsf, bitrate), 1, mode, mode_ext, crc, nbytes, w,
                                 sf_range=sf_range, counter=counter)
            specs.append(spec)
            bits += list(np.unpackbits(np.frombuffer(write_frame(spec, nbytes), np.uint8)))
        pad = (-len(bits)) % (24 * bitrate)
        out.append(dict(name=name, bitrate=bitrate, lsf=lsf, lead=lead, specs=specs,
                        bits=np.array(bits + [0] * pad, np.uint8)))

    S, J, DU, M = STEREO, JOINT, DUAL, MONO
    stream("stereo128", 128, [(S, 0, False), (J, 0, False), (J, 1, False), ("bad", 0, 1), (J, 2, False),
                              (J, 3, False), ("bad", 15, 1), (DU, 0, False), (S, 0, True), ("bad", 8, 3),
                              (S, 2, False), (S, 0, False)])
    stream("stereo192", 192, [(S, 0, False)] * 4)
    stream("mono64", 64, [(M, 0, False)] * 3)
    stream("mono32", 32, [(M, 0, False)] * 5)
    stream("mono48", 48, [(M, 0, False)] * 6)
    stream("lsf64", 64, [(S, 0, False), (J, 1, False), (M, 0, False), (S, 0, True)], lsf=1, lead=40)
    missing = {r: sorted(v) for r, v in want.items() if v}
    assert not missing, "allocation values never used: %r" % missing
    # one loud stream (scale factor indices 0..2 included: factors up to 2.0) at a seed for
    # which no intermediate of the reference leaves int32
    for loud_seed in range(100, 200):
        n = len(out)
        stream("loud128", 128, [(S, 0, False)] * 3, sf_range=(0, 62), loud_seed=loud_seed)
        fr = [write_frame(s, 384) for s in out[n]["specs"]]
        try:
            decode_chain(fr, check=True)
            break
        except Overflow:
            out.pop()
    else:
        raise AssertionError("no loud seed without int32 overflow")
    # Rule 1.  With legal code words |sample| <= 2^16 and at most 30 subbands carry any, so
    # |V| <= 30 * 2^16 * 256 / 2^14 = 30720: a well-formed stream, however loud, never wraps
    # V.  The all-ones code word of the 9-level quantiser is not legal (it is 12 * 81 + ...,
    # past 9^3), and the reference dequantises its third sample to -8/5 of full scale: 20
    # subbands of those and 4 of the 65535-level quantiser's all-ones word, at scale factor
    # 2.0, drive row 48 of the matrixing (N = -256 throughout) to 36861.  384 kbit/s frames
    # hold them; every other group carries random legal code words.
    wspecs = []
    for _ in range(3):
        alloc = np.zeros((2, 32), np.int64)
        alloc[:, 3:23] = 4                       # rows 2 and 1: the 9-level quantiser
        alloc[:, 23:27] = 3                      # row 0: the 65535-level quantiser
        codes = np.zeros((12, 2, 32, 3), np.int64)
        for g in range(12):
            if g % 2 == 0:
                codes[g, :, 3:23] = (6, 5, 12)   # 6 + 9 * (5 + 9 * 12) = 1023
                codes[g, :, 23:27] = 65535
            else:
                codes[g, :, 3:23] = rng.integers(0, 9, (2, 20, 3))
                codes[g, :, 23:27] = rng.integers(0, 65535, (2, 4, 3))
            codes[g, 1, 4:] = codes[g, 0, 4:]    # joint stereo above subband 4
        wspecs.append(dict(lsf=0, br_index=14, fs=1, padding=0, private=0, mode=JOINT, mode_ext=0, tail=0, crc=False,
                           crc_word=0, alloc=alloc, scfsi=np.full((2, 32), 2) * (alloc > 0),
                           scf=np.zeros((2, 32, 3), np.int64), codes=codes))
    bits = []
    for spec in wspecs:
        bits += list(np.unpackbits(np.frombuffer(write_frame(spec, 1152), np.uint8)))
    out.append(dict(name="wrap384", bitrate=384, lsf=0, lead=0, specs=wspecs, bits=np.array(bits, np.uint8)))
    d = Decoder(check=True)
    for spec in wspecs:
        d.decode(write_frame(spec, 1152))
    assert d.wrapped > 0
    return out
