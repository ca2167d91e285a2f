"""The Viterbi operators at the edges of their small integer periods, bit for bit against the
CPU oracle (orc.viterbi, orc.msc_deconvolve, orc.fic_process, orc.prbs).

k_viterbi.hip's control flow is made of periods -- 30 steps per decision word, 60 per
branch-metric tile, a 3-deep chunk ring and 8 chunks (240 bits) per output flush in the
traceback, 64 codewords per traceback wave, 2 per ACS wave, 16-byte stores when the output
is aligned and bit-by-bit stores otherwise -- and of one table, the energy-dispersal
sequence.  The tests here run dabgpu_viterbi, dabgpu_msc_deconvolve, dabgpu_fic_decode and
dabgpu_fic_decode_frames at step counts and codeword counts on both sides of every one of
those boundaries, into output buffers with guard bytes around and between the rows, and at
the EEP subchannels longer than 32768 bits (up to 1824 kbit/s, the longest a CIF holds).
No tolerance anywhere: every comparison is np.array_equal."""
import numpy as np
import pytest

import oracle_py as orc

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
FRAME_SOFT = 75 * 3072


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


def _enc(bits):
    from dabamd.synth import conv_encode
    return conv_encode(bits).astype(np.int16)


def _noisy(rng, coded, sigma, clip=127):
    soft = (2 * coded.astype(np.int32) - 1) * 127
    return np.clip(soft + rng.normal(0, sigma, soft.shape), -clip, clip).astype(np.int16)


def _row(kind, nbits, seed):
    """one mother-code row of 4*(nbits+6) soft values: kind 0 an encoded random message under
    Gaussian noise of sigma 260 (survivors change state), 1 uniform values without code
    structure, 2 all zeros (every step ties: the strict > decides each one)"""
    rng = np.random.default_rng(seed)
    if kind == 0:
        return _noisy(rng, _enc(rng.integers(0, 2, nbits).astype(np.uint8)), sigma=260)
    if kind == 1:
        return rng.integers(-127, 128, 4 * (nbits + 6)).astype(np.int16)
    return np.zeros(4 * (nbits + 6), np.int16)


def _rows(nbits, n, seed0=0):
    """n rows cycling through the three kinds, seeded by row; and the oracle's decode of each"""
    soft = np.stack([_row(i % 3, nbits, 1000 * nbits + 7 * i + seed0) for i in range(n)])
    want = np.stack([orc.viterbi(soft[i], nbits) for i in range(n)])
    return soft, want


def _first_diff(got, want):
    d = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return None if d.size == 0 else int(d[0])


# ------------------------------------------------------- 1. step counts at the period edges
# steps = nbits + 6:  < 30 one partial word | 30 one word | 31 a one-step second word |
# 60, 61 the tile edge | 90, 91, 120: 3, 4, 4 chunks around the ring depth | 239, 240: 8 chunks |
# 241..245: 9 chunks whose second output group holds tail steps only | 246 one whole group |
# 247, 262 one bit / 16 bits into the second group | 480 two groups of steps | 486, 487 two whole
# output groups, and one bit more | 720: 24 chunks | 32774 the operator's maximum
STEP_NBITS = [1, 2, 23, 24, 25, 54, 55, 84, 85, 114, 233, 234, 235, 239, 240, 241, 256, 474, 480, 481, 714, 32768]


@pytest.mark.parametrize("nbits", STEP_NBITS)
def test_viterbi_step_counts(ctx, nbits):
    """three codewords (the last ACS pair half empty) of nbits bits: noisy code, structureless
    values, all ties"""
    soft, want = _rows(nbits, 3)
    got = ctx.viterbi(soft, nbits)
    for i in range(3):
        assert np.array_equal(got[i], want[i]), (nbits, i, _first_diff(got[i], want[i]))


# ------------------------------------------------- 2. codeword counts at the block boundaries
@pytest.mark.parametrize("nbits", [55, 241])
@pytest.mark.parametrize("n_cw", [1, 2, 63, 64, 65, 129])
def test_viterbi_codeword_counts(ctx, n_cw, nbits):
    """1 and 2 codewords (one ACS wave, fewer than 8 waves in xcd_order), 63 / 64 / 65 around a
    traceback wave and a 64-row decision block, 129: a third block with one row"""
    soft, want = _rows(nbits, n_cw, seed0=n_cw)
    got = ctx.viterbi(soft, nbits)
    bad = [i for i in range(n_cw) if not np.array_equal(got[i], want[i])]
    assert not bad, (n_cw, nbits, bad[:8], _first_diff(got[bad[0]], want[bad[0]]))


def test_viterbi_no_codewords_writes_nothing(ctx):
    buf = ctx.buf(1024).fill(FILL)
    try:
        got = ctx.viterbi(np.zeros((0, 4 * (241 + 6)), np.int16), 241, out=buf, out_offset=GUARD)
        assert got.shape == (0, 241)
        assert (buf.download(np.uint8, 1024) == FILL).all()
    finally:
        buf.free()


# ----------------------------------------------------- 3. nothing outside the result is written
@pytest.mark.parametrize("out_offset", [64, 65, 80])
@pytest.mark.parametrize("nbits", [240, 241, 480])
def test_viterbi_writes_only_its_rows(ctx, nbits, out_offset):
    """the rows at an aligned, an odd and a 16-but-not-64-aligned address (240 and 480: a row
    stride that is a multiple of 16, so offsets 64 and 80 take the 16-byte stores), guard bytes
    in front and behind"""
    soft, want = _rows(nbits, 3)
    total = out_offset + 3 * nbits + GUARD
    buf = ctx.buf(total).fill(FILL)
    try:
        got = ctx.viterbi(soft, nbits, out=buf, out_offset=out_offset)
        whole = buf.download(np.uint8, total)
    finally:
        buf.free()
    assert (whole[:out_offset] == FILL).all(), np.flatnonzero(whole[:out_offset] != FILL)[:8]
    back = whole[out_offset + 3 * nbits:]
    assert (back == FILL).all(), np.flatnonzero(back != FILL)[:8]
    assert np.array_equal(got, want)
    assert np.array_equal(whole[out_offset:out_offset + 3 * nbits].reshape(3, nbits), want)


# EEP 2-A 8 kbit/s (192 bits), UEP 384 level 1 (9216), EEP 3-A 128, EEP 2-A 8 again, UEP 64 level 4:
# the short codeword is the first of ACS pair 0 and the second of pair 1; pair 2 is half empty
GUARD_CASES = [(1, 8, 0o102), (0, 384, 1), (1, 128, 0o103), (1, 8, 0o102), (0, 64, 4)]


@pytest.fixture(scope="module")
def guard_batch():
    rng = np.random.default_rng(31)
    frags = rng.integers(-127, 128, (len(GUARD_CASES), 27000)).astype(np.int16)
    want = [orc.msc_deconvolve(1 if uf == 0 else 0, br, pl, frags[i]) for i, (uf, br, pl) in enumerate(GUARD_CASES)]
    return frags, want


@pytest.mark.parametrize("out_stride", [9216, 9217, 9232, 9280])
def test_msc_deconvolve_writes_only_its_bits(ctx, guard_batch, out_stride):
    """dabgpu_msc_deconvolve's contract (include/dabgpu.h): of a row only the codeword's own
    24*bitRate bytes are written -- not the gap up to out_stride, not the rest of a short
    codeword's row, nothing in front of the first row or behind the last"""
    import dabamd
    frags, want = guard_batch
    n = len(GUARD_CASES)
    subs = [dabamd.Subch(0, 0, br, pl, uf, 0) for uf, br, pl in GUARD_CASES]
    total = GUARD + n * out_stride + GUARD
    buf = ctx.buf(total).fill(FILL)
    try:
        outs = ctx.msc_deconvolve(frags, subs, out=buf, out_offset=GUARD, out_stride=out_stride)
        whole = buf.download(np.uint8, total)
    finally:
        buf.free()
    assert (whole[:GUARD] == FILL).all() and (whole[GUARD + n * out_stride:] == FILL).all()
    for i, (uf, br, pl) in enumerate(GUARD_CASES):
        row = whole[GUARD + i * out_stride:GUARD + (i + 1) * out_stride]
        nb = 24 * br
        assert np.array_equal(row[:nb], want[i]), (out_stride, i, _first_diff(row[:nb], want[i]))
        assert np.array_equal(outs[i], want[i])
        assert (row[nb:] == FILL).all(), (out_stride, i, nb + np.flatnonzero(row[nb:] != FILL)[:8])


def test_operators_refuse_bad_shapes(ctx):
    """refused on the host, before any launch"""
    import dabamd
    for nbits in (0, 32769):
        with pytest.raises(dabamd.DabError):
            ctx.viterbi(np.zeros((1, 4 * (nbits + 6)), np.int16), nbits)
    frags = np.zeros((2, 27000), np.int16)
    subs = [dabamd.Subch(0, 0, 128, 0o103, 1, 0), dabamd.Subch(0, 0, 384, 1, 0, 0)]
    with pytest.raises(dabamd.DabError):                       # out_stride below the longest codeword
        ctx.msc_deconvolve(frags, subs, out_stride=24 * 384 - 1)
    frag = dabamd.subch_profile(subs[1])[1]                    # UEP 384 level 1 consumes 26616 soft bits
    with pytest.raises(dabamd.DabError):                       # frag_stride below it
        ctx.msc_deconvolve(frags[:, :frag - 1], subs)
    assert len(ctx.msc_deconvolve(frags[:, :frag], subs, out_stride=24 * 384)) == 2     # both at their limits: accepted


# ------------------------------------------- 4. dabgpu_fic_decode_frames against orc.fic_process
@pytest.fixture(scope="module")
def fic_slots():
    """three frame slots of FRAME_SOFT int16; only the first 9216 values of a slot belong to
    the FIC, the rest holds a value that would change the decode if it were read.  Slot 0:
    structureless values; slot 1: the valid FIC blocks of a noiseless synthetic frame; slot 2:
    the int16 extremes.  With the oracle's result per block."""
    from dabamd.synth import Ensemble
    rng = np.random.default_rng(41)
    soft = np.full((3, FRAME_SOFT), 99, np.int16)
    soft[0, :9216] = rng.integers(-127, 128, 9216)
    g = Ensemble(1, snr_db=300.0).generate(11)
    n, info, s = orc.ofdm_run(g["iq"], 1)
    assert n == 1
    soft[1, :9216] = s[0, 0:3].reshape(-1)[:9216]
    soft[2, :9216] = np.resize(np.array([32767, -32768, 300, -300], np.int16), 9216)
    bits = np.zeros((3, 4, 768), np.uint8)
    ok = np.zeros((3, 12), np.uint8)
    for sl in range(3):
        for b in range(4):
            bits[sl, b], ok[sl, 3 * b:3 * b + 3] = orc.fic_process(soft[sl, 2304 * b:2304 * (b + 1)])
    assert ok[1].all()
    return soft, bits, ok


@pytest.mark.parametrize("slots", [[2, 0, 2, 1], [0], [i % 3 for i in range(17)]], ids=["repeated", "one", "17-frames"])
def test_fic_decode_frames_matches_oracle(ctx, fic_slots, slots):
    """the input-major ACS loader on int16 soft values (the pipeline runs it on RING8 bytes):
    slots out of order and repeated, one frame, and 68 codewords (a second traceback wave)"""
    soft, wbits, wok = fic_slots
    d = ctx.put(soft)
    try:
        bits, ok = ctx.fic_decode_frames(d, slots)
    finally:
        d.free()
    for i, sl in enumerate(slots):
        assert np.array_equal(bits[i], wbits[sl]), (i, sl, _first_diff(bits[i], wbits[sl]))
        assert np.array_equal(ok[i], wok[sl]), (i, sl, ok[i], wok[sl])
        if sl == 1:
            assert ok[i].all()
    # dabgpu_fic_decode on the gathered blocks: the same bytes
    blocks = np.concatenate([soft[sl, :9216].reshape(4, 2304) for sl in slots])
    b2, ok2 = ctx.fic_process(blocks)
    assert np.array_equal(b2.reshape(-1, 4, 768), bits)
    assert np.array_equal(ok2.reshape(-1, 12), ok)


# ----------------------------------------------------------- 5. the FIB CRC by single-bit flips
def _crc16(bits):
    """the 16 CRC bits of a FIB's 240 payload bits (CRC-CCITT x^16 + x^12 + x^5 + 1 from all
    ones, complemented; EN 300 401 5.2.1), msb first"""
    reg = 0xFFFF
    for b in bits:
        top = ((reg >> 15) & 1) ^ int(b)
        reg = (reg << 1) & 0xFFFF
        if top:
            reg ^= 0x1021
    reg ^= 0xFFFF
    return np.array([(reg >> (15 - k)) & 1 for k in range(16)], np.uint8)


def _fic_keep():
    """the mother-code positions fic_profile keeps (PI_16 x 21 blocks, PI_15 x 3, the PI_X
    tail): where the oracle's depuncturing puts its inputs"""
    ones = np.ones(2304, np.int16)
    out = np.zeros(3072 + 24, np.int16)
    orc.oracle().orc_fic_depuncture(orc.P(ones), orc.P(out))
    keep = np.flatnonzero(out)
    assert len(keep) == 2304
    return keep


def _fic_block_soft(block_bits, keep):
    """768 FIC bits -> 2304 noiseless soft values: dispersal, mother code, puncturing, +-127"""
    coded = _enc(block_bits ^ orc.prbs(768))
    return ((2 * coded[keep].astype(np.int32) - 1) * 127).astype(np.int16)


def test_fib_crc_single_bit_flips(ctx):
    """k_fic_post takes the CRC from a 257-entry linearity table, one nibble per lane.  One
    FIC block whose three FIBs are valid, then FIB 0 with each of its 256 bits flipped in
    turn: the check must fail for every one of them (a wrong table entry for bit i would pass
    variant i or fail the original) and hold for FIBs 1 and 2.  A last variant has a payload bit
    flipped and the CRC made good again.  That takes the CRC bits of the flipped bit's
    syndrome, never one bit alone: x has order 32767 modulo the generator, so no two of a
    FIB's 256 bit positions have syndromes that cancel.  Across the three payloads every
    payload position is 1 in one FIB and 0 in another, so every table entry takes part in a
    passing check."""
    rng = np.random.default_rng(51)
    p0 = rng.integers(0, 2, 240).astype(np.uint8)
    pay = [p0, p0 ^ 1, rng.integers(0, 2, 240).astype(np.uint8)]
    st = np.stack(pay)
    assert (st.max(axis=0) == 1).all() and (st.min(axis=0) == 0).all()
    block = np.concatenate([np.concatenate([p, _crc16(p)]) for p in pay])
    keep = _fic_keep()
    variants = [block]
    for i in range(256):
        v = block.copy()
        v[i] ^= 1
        variants.append(v)
    v = block.copy()
    v[100] ^= 1
    v[240:256] = _crc16(v[:240])
    assert (v[240:256] != block[240:256]).sum() > 1
    variants.append(v)
    soft = np.stack([_fic_block_soft(b, keep) for b in variants])
    assert soft.shape == (258, 2304)
    bits, ok = ctx.fic_process(soft)
    want_ok0 = np.zeros(258, np.uint8)
    want_ok0[[0, 257]] = 1
    for i in range(258):
        ob, ook = orc.fic_process(soft[i])
        inv = variants[i].copy()                  # the noiseless block comes back, each CRC field inverted
        for q in range(3):
            inv[256 * q + 240:256 * q + 256] ^= 1
        assert np.array_equal(ob, inv), i
        assert np.array_equal(bits[i], ob), (i, _first_diff(bits[i], ob))
        assert np.array_equal(ok[i], ook), (i, ok[i], ook)
    assert np.array_equal(ok[:, 0], want_ok0), np.flatnonzero(ok[:, 0] != want_ok0)
    assert ok[:, 1:].all()


# ------------------------------------------------- 6. EEP subchannels longer than 32768 bits
# (uepFlag, bitRate, protLevel): 32640 bits, the last EEP 4-A length inside 32768; 32832, the
# first beyond; 41472 (864 CU, the whole CIF); EEP 4-B at 43776 bits (855 CU), the longest
LONG_CASES = {"1360": [(1, 1360, 0o104)], "1368": [(1, 1368, 0o104)], "1728": [(1, 1728, 0o104)],
              "1824": [(1, 1824, 0o204)], "1728+1824": [(1, 1728, 0o104), (1, 1824, 0o204)]}
TEXT = b"The quick brown fox jumps over the lazy dog. "


def _msc_keep(br, pl):
    """mother-code positions an EEP profile keeps, and its fragment size"""
    nb = 24 * br
    ones = np.ones(4 * nb + 24, np.int16)
    out = np.zeros(4 * nb + 24, np.int16)
    used = orc.oracle().orc_msc_depuncture(0, br, pl, orc.P(ones), orc.P(out))
    keep = np.flatnonzero(out)
    assert used == len(keep) and used % 64 == 0
    return keep, used


def _orc_raw(br, pl, frag):
    """eep_deconvolve::deconvolve alone: the oracle's depuncturing, then orc.viterbi"""
    nb = 24 * br
    vb = np.zeros(4 * nb + 24, np.int16)
    assert orc.oracle().orc_msc_depuncture(0, br, pl, orc.P(np.ascontiguousarray(frag, np.int16)), orc.P(vb)) >= 0
    return orc.viterbi(vb, nb)


@pytest.fixture(scope="module")
def long_frags():
    """per (bitRate, protLevel): a structureless fragment and a noiseless encoded text, with the
    oracle's decode of both without dispersal, and the text's bits"""
    out = {}
    rng = np.random.default_rng(61)
    for _, br, pl in {c for cs in LONG_CASES.values() for c in cs}:
        nb = 24 * br
        keep, frag = _msc_keep(br, pl)
        rnd = rng.integers(-127, 128, frag).astype(np.int16)
        msg = np.unpackbits(np.frombuffer((TEXT * (nb // (8 * len(TEXT)) + 1))[:nb // 8], np.uint8))
        coded = _enc(msg ^ orc.prbs(nb))
        txt = ((2 * coded[keep].astype(np.int32) - 1) * 127).astype(np.int16)
        out[(br, pl)] = dict(frag=frag, rnd=rnd, txt=txt, msg=msg, raw_rnd=_orc_raw(br, pl, rnd),
                             raw_txt=_orc_raw(br, pl, txt))
    return out


@pytest.mark.parametrize("raw", [0, 1], ids=["dispersed", "raw"])
@pytest.mark.parametrize("case", list(LONG_CASES))
def test_msc_deconvolve_long_eep(ctx, long_frags, case, raw):
    """legal EEP subchannels up to 1824 kbit/s: the energy-dispersal sequence runs on past bit
    32768 (dab-concurrent.cpp:183-190 builds it for 24*bitRate bits); DABGPU_SUBCH_RAW equals
    the bare Viterbi.  On a mismatch the assertion names the first differing bit."""
    import dabamd
    cs = LONG_CASES[case]
    subs = [dabamd.Subch(0, 0, br, pl, uf, dabamd.SUBCH_RAW if raw else 0) for uf, br, pl in cs]
    stride = max(long_frags[(br, pl)]["frag"] for _, br, pl in cs)
    for kind in ("rnd", "txt"):
        frags = np.zeros((len(cs), stride), np.int16)
        for i, (_, br, pl) in enumerate(cs):
            frags[i, :long_frags[(br, pl)]["frag"]] = long_frags[(br, pl)][kind]
        outs = ctx.msc_deconvolve(frags, subs)
        for i, (_, br, pl) in enumerate(cs):
            L = long_frags[(br, pl)]
            want = L["raw_" + kind] if raw else L["raw_" + kind] ^ orc.prbs(24 * br)
            if not raw:
                assert np.array_equal(want, orc.msc_deconvolve(0, br, pl, frags[i]))
            print(f"{case} {'raw' if raw else 'dispersed'} {kind} codeword {i} ({24 * br} bits): "
                  f"first differing bit {_first_diff(outs[i], want)}")
            assert np.array_equal(outs[i], want), (case, raw, kind, i, "first differing bit", _first_diff(outs[i], want))
            if kind == "txt" and not raw:
                assert np.array_equal(outs[i], L["msg"])
                assert np.packbits(outs[i]).tobytes().startswith(TEXT)


@pytest.mark.parametrize("flags", [0, 2], ids=["dispersed", "raw"])
@pytest.mark.parametrize("br", [1832, 1856, 32767])
def test_msc_deconvolve_refuses_bitrates_beyond_its_table(ctx, br, flags):
    """above 1824 kbit/s (more than a CIF holds, and more than the dispersal table covers):
    DABGPU_E_UNSUP on the host, first in a call or behind a good codeword"""
    import dabamd
    assert flags in (0, dabamd.SUBCH_RAW)
    good, bad = dabamd.Subch(0, 0, 8, 0o102, 1, flags), dabamd.Subch(0, 0, br, 0o204, 1, flags)
    for subs in ([bad], [good, bad]):
        with pytest.raises(dabamd.DabError) as e:
            ctx.msc_deconvolve(np.zeros((len(subs), 512), np.int16), subs)
        assert e.value.code == -5, e.value
