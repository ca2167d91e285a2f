"""TEST INFRASTRUCTURE: a DAB+ superframe builder (plain Python and numpy) and the crafted
cases of the superframe layer's edge tests (test_dabplus_cpu.py pins them to the reference,
test_gpu_dabplus_edges.py runs them through k_dp_layer).

superframe() makes what mp4Processor::addtoFrame / processSuperframe (mp4processor.cpp:
107-292) take apart: header and AU start table (:185-230), each AU's inverted CRC-CCITT
(:40-61), the fire code of bytes 2-10 in bytes 0-1 (firecode-checker.cpp), RS(120,110)
parity per interleaved column (column j = bytes j + k * RS), cut into 5 CIF rows of
3 * bitRate bytes.  The RS encoder is the oracle's (orc_rs_enc); everything else is here.

A case is a Case(name, sf, expect, past_end): the 120 * RS bytes of one superframe, the fields
of the record the case is named for (checked against orc.MP4 on the CPU so that a case cannot
silently test something else), and whether an AU of its table reaches past the superframe
(there the reference reads uninitialised memory; the kernel and the oracle read zeros)."""
import functools
from collections import namedtuple

import numpy as np

import oracle_py as orc

WIDTHS = (1, 2, 3, 5, 7, 11, 21, 32, 33, 48)          # RSDims of the edge table: 8 .. 384 kbit/s
LAYOUTS = {(0, 0): (4, 8), (0, 1): (2, 5), (1, 0): (6, 11), (1, 1): (3, 6)}   # (dacRate, SBR): (AUs, first start)
EDGE_LENS = (0, 1, 63, 64, 65)                        # around the 64 slices of the kernel's AU CRC

Case = namedtuple("Case", "name sf expect past_end")


# ---- the three checksums -----------------------------------------------------------
def fire_code(b9):
    """the 16 check bits of bytes 2..10: remainder by x^16+x^14+x^13+x^12+x^11+x^5+x^3+x^2+x+1, zero preset"""
    r = 0
    for b in b9:
        for k in range(7, -1, -1):
            top = ((r >> 15) & 1) ^ ((int(b) >> k) & 1)
            r = (r << 1) & 0xFFFF
            if top:
                r ^= 0x782F
    return r


def fire_fix(buf, at=0):
    """write bytes at, at+1 of buf as the fire code of bytes at+2 .. at+10"""
    r = fire_code(buf[at + 2:at + 11])
    buf[at], buf[at + 1] = r >> 8, r & 0xFF


def au_crc(data):
    """CRC-CCITT (0x1021, preset 0xFFFF) as the AU carries it: inverted"""
    acc = 0xFFFF
    for b in data:
        acc ^= int(b) << 8
        for _ in range(8):
            acc = ((acc << 1) ^ 0x1021) & 0xFFFF if acc & 0x8000 else (acc << 1) & 0xFFFF
    return ~acc & 0xFFFF


def rs_encode(data110):
    cw = np.zeros(120, np.uint8)
    orc.oracle().orc_rs_enc(orc.P(np.ascontiguousarray(data110, np.uint8)), orc.P(cw))
    return cw


# ---- one superframe ------------------------------------------------------------------
def starts_of(br, dac, sbr, lens):
    """the start table [a0 .. a_n] of AUs of these lengths (each followed by its 2 CRC bytes)"""
    n, a0 = LAYOUTS[(dac, sbr)]
    a = [a0]
    for ln in lens[:n]:
        a.append(a[-1] + ln + 2)
    return a


def fit_m(br, dac, sbr, first=()):
    """(n AU lengths that fill the superframe exactly, each below 960, beginning with as many
    of `first` as leave that possible; how many of `first` that is).  The AUs after them take
    the rest, the largest that fits first.  (None, 0) where the layout cannot fill this width."""
    n, a0 = LAYOUTS[(dac, sbr)]
    room = 110 * (br // 8) - a0 - 2 * n
    for m in range(min(len(first), n - 1), -1, -1):
        lens = list(first[:m])
        left = room - sum(lens)
        if left < 0 or left > 959 * (n - m):
            continue
        free = []
        for _ in range(n - m):
            free.append(min(959, left))
            left -= free[-1]
        for tail in (free, free[::-1]):                       # the table holds 12-bit starts: a long last AU
            if starts_of(br, dac, sbr, lens + tail)[n - 1] <= 4095:
                return lens + tail, m
    return None, 0


def fit(br, dac, sbr, first=()):
    return fit_m(br, dac, sbr, first)[0]


def reads_past(a, end):
    """the AU loop of processSuperframe reads past the superframe before it stops"""
    for i in range(len(a) - 1):
        ln = a[i + 1] - a[i] - 2
        if a[i + 1] < a[i] or ln >= 960 or ln < 0:
            return False
        if a[i] + ln + 2 > end:
            return True
    return False


def superframe(br, dac, sbr, lens=None, payload=None, starts=None, bad_crc=(), fire_rows=False):
    """120 * RS bytes.  lens: the AU lengths (fit() fills the width); starts: the raw table
    a[1..n-1] instead, for tables the layer must reject (AUs that then lie wholly inside in
    ascending order still get a CRC).  payload: 110 * RS bytes, the AU contents and the free
    header bits.  bad_crc: AUs whose CRC is stored wrong.  fire_rows: rows 1..4 open with 11
    bytes that pass the fire code too (a candidate at every CIF)."""
    RS = br // 8
    end = 110 * RS
    n, a0 = LAYOUTS[(dac, sbr)]
    d = np.array(payload, np.uint8).copy()
    assert d.shape == (end,)
    if starts is None:
        a = starts_of(br, dac, sbr, lens)
        assert len(a) == n + 1 and a[n] == end, (a, end)
    else:
        a = [a0] + list(starts) + [end]
        assert len(a) == n + 1
    d[2] = (int(d[2]) & 0x9F) | (dac << 6) | (sbr << 5)
    t = a[1:n] + [0] * 5
    assert max(t) <= 4095
    hdr = [t[0] >> 4, ((t[0] & 0xF) << 4) | (t[1] >> 8), t[1] & 0xFF, t[2] >> 4, ((t[2] & 0xF) << 4) | (t[3] >> 8),
           t[3] & 0xFF, t[4] >> 4, (t[4] & 0xF) << 4]
    nb = {2: 2, 3: 3, 4: 5, 6: 8}[n]                  # bytes 3.. that the layout's table takes
    for i in range(nb):
        keep = 0x0F if (i == nb - 1 and n in (2, 4, 6)) else 0       # a table of odd count ends in a half byte
        d[3 + i] = hdr[i] | (int(d[3 + i]) & keep)
    if fire_rows:
        for r in range(1, 5):
            fire_fix(d, r * 24 * RS)
    top = a0
    for i in range(n):
        ln = a[i + 1] - a[i] - 2
        if a[i] < top or ln < 0 or a[i + 1] > end:
            continue
        c = au_crc(d[a[i]:a[i] + ln]) ^ (0x0100 if i in bad_crc else 0)
        d[a[i] + ln], d[a[i] + ln + 1] = c >> 8, c & 0xFF
        top = a[i + 1]
    fire_fix(d)
    if fire_rows:
        for r in range(1, 5):
            assert fire_code(d[r * 24 * RS + 2:r * 24 * RS + 11]) == (int(d[r * 24 * RS]) << 8 | int(d[r * 24 * RS + 1]))
    sf = np.zeros(120 * RS, np.uint8)
    sf[:end] = d
    for j in range(RS):
        sf[j + 110 * RS::RS] = rs_encode(d[j::RS])[110:]
    return sf


def inject(sf, br, col, rows, rng):
    """symbol errors (non-zero values) in column col at these rows (0..109 data, 110..119 parity)"""
    RS = br // 8
    for r in rows:
        sf[col + int(r) * RS] ^= int(rng.integers(1, 256))


def apply_pattern(sf, br, col, pat):
    RS = br // 8
    for r, v in pat:
        sf[col + r * RS] ^= v


def column(sf, br, col):
    return np.ascontiguousarray(sf[col::br // 8])


def rows_of(sf, br):
    """the 5 CIF rows of 3 * br bytes"""
    return [sf[r * 3 * br:(r + 1) * 3 * br].copy() for r in range(5)]


def emit(row, packed):
    """a CIF row as the MSC output holds it: packed bytes, or one bit per byte (msb first)"""
    return np.asarray(row, np.uint8) if packed else np.unpackbits(np.asarray(row, np.uint8))


@functools.lru_cache(maxsize=None)
def filler(br, seed=0):
    """a row whose fire code fails (what follows a script's end)"""
    row = np.random.default_rng(1000 + seed).integers(0, 256, 3 * br).astype(np.uint8)
    fire_fix(row)
    row[0] ^= 0x80
    return row


def _payload(br, rng):
    return rng.integers(0, 256, 110 * (br // 8)).astype(np.uint8)


def fillable(br):
    """a start table exists that the layer accepts.  Above 360 kbit/s none does: 6 AUs below
    960 bytes behind 12-bit starts end by byte 5056, and 110 * RS is larger (5280 at 384)."""
    return any(fit(br, d, s) is not None for d, s in LAYOUTS)


BEST_STARTS = [972, 1933, 2894, 3855, 4095]           # 6 AUs, the last start as late as the table can say


def clean(br, rng, layout=(0, 0), fire_rows=False, bad_crc=()):
    """a well-formed superframe in the layout asked for, or else one that fills this width.
    Where none does (fillable): 5 good AUs and a last one too long, which the layer rejects
    after the RS decode and the first 5 CRCs (status 2, mask 0x1F)."""
    for lay in (layout, (1, 0), (0, 0)):
        lens = fit(br, lay[0], lay[1])
        if lens is not None:
            return superframe(br, lay[0], lay[1], lens, _payload(br, rng), fire_rows=fire_rows, bad_crc=bad_crc)
    return superframe(br, 1, 0, payload=_payload(br, rng), starts=BEST_STARTS, fire_rows=fire_rows, bad_crc=bad_crc)


def clean_expect(br, n_corrected):
    if fillable(br):
        return dict(status=3, n_corrected=n_corrected, all_crc=True)
    return dict(status=2, n_corrected=n_corrected, num_aus=6, mask=0x1F)


def pick_rows(br, col, k, rng, data=True, parity=False):
    """k rows of column col for symbol errors, none in the superframe's first 11 bytes (the
    fire code is checked before the RS decode: an error there ends the candidate as status 1)"""
    RS = br // 8
    rows = [r for r in range(110) if col + r * RS >= 11] if data else []
    rows += list(range(110, 120)) if parity else []
    return rng.choice(rows, k, replace=False)


# ---- case 1: every width, clean and at the correction limit -------------------------
def rs_cases(br, rng):
    RS = br // 8
    out = [Case("clean", clean(br, rng), clean_expect(br, 0), False)]
    sf = clean(br, rng)
    for j in range(RS):
        inject(sf, br, j, pick_rows(br, j, 5, rng), rng)              # data rows: a parity row is not counted
    out.append(Case("five_errors_every_column", sf, clean_expect(br, 5 * RS), False))
    sf = clean(br, rng)
    for j in range(RS):
        inject(sf, br, j, pick_rows(br, j, 1 + j % 5, rng, data=False, parity=True), rng)
    out.append(Case("parity_rows_only", sf, clean_expect(br, 0), False))
    sf = clean(br, rng)
    for j in range(RS):
        inject(sf, br, j, list(pick_rows(br, j, 2, rng)) + [110 + int(rng.integers(10))], rng)
    out.append(Case("two_data_one_parity", sf, clean_expect(br, 2 * RS), False))
    return out


# ---- case 2: the first failing column stops the count -------------------------------
def _failing(sf, br, col, rng):
    """6 errors in column col that the decoder gives up on (about 1 pattern in 170 miscorrects instead)"""
    while True:
        t = sf.copy()
        inject(t, br, col, pick_rows(br, col, 6, rng, parity=True), rng)
        if orc.rs_dec(column(t, br, col))[1] < 0:
            sf[:] = t
            return


def fail_cases(br, rng):
    RS = br // 8
    sf = clean(br, rng)
    _failing(sf, br, 0, rng)
    out = [Case("six_in_column_0", sf, dict(status=2, n_corrected=0, num_aus=0), False)]
    sf = clean(br, rng)
    for j in range(RS - 1):
        inject(sf, br, j, pick_rows(br, j, 5, rng), rng)
    _failing(sf, br, RS - 1, rng)
    out.append(Case("six_in_last_column", sf, dict(status=2, n_corrected=5 * (RS - 1), num_aus=0), False))
    sf = clean(br, rng)
    mid, before = RS // 2, 0
    for j in range(RS):
        if j != mid:
            ne = 1 + j % 5
            inject(sf, br, j, pick_rows(br, j, ne, rng), rng)             # data rows: each one counts
            before += ne if j < mid else 0
    _failing(sf, br, mid, rng)
    out.append(Case("six_in_middle_column", sf, dict(status=2, n_corrected=before, num_aus=0), False))
    return out


# ---- case 3: columns the decoder miscorrects ----------------------------------------
@functools.lru_cache(maxsize=None)
def miscorrecting(seed=5, tries=3000):
    """{6, 7, 8 errors: [error pattern ((row, value) ...)] that orc_rs_dec answers with a count
    instead of -1}, from `tries` random patterns each.  The decoder's verdict and corrections
    depend on the syndromes alone, so a pattern does the same on top of any codeword."""
    rng = np.random.default_rng(seed)
    found = {}
    for ne in (6, 7, 8):
        found[ne] = []
        for _ in range(tries):
            rows = 11 + rng.choice(109, ne, replace=False)        # (row 0..10 would break the fire code at width 1)
            vals = rng.integers(1, 256, ne)
            cw = np.zeros(120, np.uint8)
            cw[rows] = vals
            if orc.rs_dec(cw)[1] >= 0:
                found[ne].append(tuple((int(r), int(v)) for r, v in zip(rows, vals)))
    return found


def misc_cases(br, rng, reverse=False, limit=4):
    """superframes whose columns carry the miscorrecting patterns in turn (at most `limit`)"""
    RS = br // 8
    pats = [p for ne in (6, 7, 8) for p in miscorrecting()[ne]]
    if reverse:
        pats = pats[::-1]
    out = []
    for m in range(min(limit, -(-len(pats) // RS))):
        sf = clean(br, rng)
        for j in range(RS):
            apply_pattern(sf, br, j, pats[(m * RS + j) % len(pats)])
        out.append(Case("miscorrecting_%d" % m, sf, dict(min_status=2), False))
    return out


# ---- case 4: AU table and CRC edges --------------------------------------------------
def au_cases(br, dac, sbr, rng):
    RS = br // 8
    end = 110 * RS
    n, a0 = LAYOUTS[(dac, sbr)]
    full = (1 << n) - 1
    out = []

    def add(name, expect, **kw):
        a = [a0] + list(kw["starts"]) + [end] if "starts" in kw else starts_of(br, dac, sbr, kw["lens"])
        out.append(Case(name, superframe(br, dac, sbr, payload=_payload(br, rng), **kw), expect, reads_past(a, end)))

    base = fit(br, dac, sbr)
    if base is not None:
        # lengths 0, 1, 63, 64, 65 in the leading AUs until each has had its turn, the other AUs
        # the largest that fits
        k, seen = 0, set()
        while k < 5:
            lens, m = fit_m(br, dac, sbr, [EDGE_LENS[(k + i) % 5] for i in range(n - 1)])
            if tuple(lens) not in seen:
                add("edge_lens_%d" % k, dict(status=3, mask=full, lens=lens), lens=lens)
            seen.add(tuple(lens))
            k += max(1, m)
        lens, m = fit_m(br, dac, sbr, [959])
        if m == 1 and tuple(lens) not in seen:
            add("len_959", dict(status=3, mask=full, lens=lens), lens=lens)
        # a wrong CRC in every position: the even AUs, then the odd ones
        for par in (0, 1):
            bad = [i for i in range(n) if i % 2 == par]
            add("wrong_crc_%s" % ("even" if par == 0 else "odd"),
                dict(status=3, mask=full & ~sum(1 << i for i in bad)), lens=base, bad_crc=bad)
        a = starts_of(br, dac, sbr, base)
        # the second AU impossible (negative length), the first one good: the mask keeps its bit
        s = a[1:n]
        if n >= 3:
            s[1] = s[0] + 1
        else:
            s[0] = end - 1
        if s[0] - a0 - 2 < 960:
            add("second_negative", dict(status=2, mask=1, num_aus=n), starts=s)
        if n >= 3:
            # a descending table after the good AUs before it
            s = a[1:n]
            s[-1] = s[-2] - 1
            add("descending", dict(status=2, mask=(1 << (n - 2)) - 1, num_aus=n), starts=s)
    if base is None and n == 6 and end > 4095 + 2:
        # no table fills this width: 5 good AUs, then wrong CRCs among them, before the last one is rejected
        out.append(Case("last_too_long", clean(br, rng), dict(status=2, mask=0x1F, num_aus=6), False))
        for par in (0, 1):
            bad = [i for i in range(5) if i % 2 == par]
            out.append(Case("last_too_long_wrong_crc_%d" % par, clean(br, rng, bad_crc=bad),
                            dict(status=2, mask=0x1F & ~sum(1 << i for i in bad), num_aus=6), False))
    # length 960 in AU 0: rejected at once
    add("len_960_first", dict(status=2, mask=0, num_aus=n), starts=[a0 + 962 + 10 * i for i in range(n - 1)])
    # length 960 in the last AU but one, short good AUs before it
    s = [a0 + 12 * (i + 1) for i in range(n - 2)]
    s.append((s[-1] if s else a0) + 962)
    if n >= 3 and s[-1] <= end:
        add("len_960_later", dict(status=2, mask=(1 << (n - 2)) - 1, num_aus=n), starts=s)
    # a start of 4095 in the last table entry
    s = (starts_of(br, dac, sbr, base)[1:n - 1] if base is not None else [a0 + 2 + 4 * i for i in range(n - 2)]) + [4095]
    add("start_4095", dict(status=2, num_aus=n, has_start=4095), starts=s)
    # AU 0 starts inside and ends past the superframe; the AUs behind it lie wholly past it with
    # length 0 (their CRC over nothing holds: zeros are the inverted preset) up to a descending end
    if end + 8 - a0 < 960:
        add("ends_past", dict(status=2, num_aus=n, mask_has=((1 << (n - 1)) - 1) & ~1, past=True),
            starts=[end + 10 + 2 * i for i in range(n - 1)])
    else:
        # a wider superframe: good AUs of equal length up to the last but one, which starts inside
        # and ends 10 bytes past the end (the zero reads at a large start); the last start is then
        # behind the end, a descending table.  The starts must fit 12 bits (not above 371 kbit/s)
        # and the n - 1 AUs must span the superframe (6 AUs at RSDims 33; 4 AUs cannot).
        step = -(-(end + 10 - a0) // (n - 1))
        s = [a0 + step * (i + 1) for i in range(n - 2)] + [end + 10]
        if step - 2 < 960 and end + 10 <= 4095 and n >= 3 and s[-2] < end:
            add("ends_past", dict(status=2, num_aus=n, mask_has=(1 << (n - 2)) - 1, past=True), starts=s)
    return out


# ---- case 5: the walk under dense candidates -----------------------------------------
def walk_script(br, variant, rng, n_sf=8):
    """rows of one (stream, subchannel): variant 0 all-zero rows (a muted subchannel: the fire
    code and the RS decode pass at every CIF, the AU table rejects); 1 aligned superframes
    whose every row passes the fire code, the first row of the third one dropped; 2 the same
    drop among plain superframes (the fire code fails on the misaligned windows)"""
    if variant == 0:
        return [np.zeros(3 * br, np.uint8) for _ in range(5 * n_sf)]
    RS, rows = br // 8, []
    # AUs that end on the CIF rows' boundaries: no CRC then lies in a row's first 11 bytes
    if RS <= 25:
        lay, a = (0, 0), [8, 24 * RS, 48 * RS, 72 * RS, 110 * RS]
    else:
        lay, a = (1, 0), [11, 24 * RS, 48 * RS, 72 * RS, 96 * RS, 96 * RS + 20, 110 * RS]
    for m in range(n_sf):
        if fillable(br):
            sf = superframe(br, lay[0], lay[1], [y - x - 2 for x, y in zip(a, a[1:])], _payload(br, rng),
                            fire_rows=variant == 1)
        else:
            sf = clean(br, rng, fire_rows=variant == 1)
        r = rows_of(sf, br)
        rows += r[1:] if m == 2 else r
    return rows


# ---- a record (orc.MP4's dict, or a GPU record in that shape) against a case's expectation ----
def mask_of(o):
    return sum(int(o["au_crc"][i]) << i for i in range(o["num_aus"]))


def check_expect(w, c, o):
    e, tag = c.expect, (w, c.name)
    if "status" in e:
        assert o["status"] == e["status"], tag
    if "min_status" in e:
        assert o["status"] >= e["min_status"], tag
    for k in ("n_corrected", "num_aus"):
        if k in e:
            assert o[k] == e[k], (tag, k, o[k], e[k])
    if e.get("all_crc"):
        assert o["num_aus"] > 0 and mask_of(o) == (1 << o["num_aus"]) - 1, tag
    if "mask" in e:
        assert mask_of(o) == e["mask"], (tag, bin(mask_of(o)))
    if "mask_has" in e:
        assert mask_of(o) & e["mask_has"] == e["mask_has"], (tag, bin(mask_of(o)))
    if "has_start" in e:
        assert e["has_start"] in list(o["au_start"][:o["num_aus"]]), tag
    if e.get("lens") is not None:
        a = list(o["au_start"][:o["num_aus"] + 1])
        assert [y - x - 2 for x, y in zip(a, a[1:])] == e["lens"], tag
    if "past" in e:
        assert c.past_end == e["past"], tag


# ---- the cases both test files use: the same seeds, so what the CPU test pins to the
# reference is byte for byte what the GPU test runs --------------------------------------
FAIL_WIDTHS = (1, 7, 33, 48)
AU_WIDTHS = (2, 33)
FORMAT_WIDTHS = (3, 48)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


@functools.lru_cache(maxsize=None)
def cases_rs(w, stream):
    return rs_cases(8 * w, _rng(1, w, stream))


@functools.lru_cache(maxsize=None)
def cases_fail(w, stream):
    return fail_cases(8 * w, _rng(2, w, stream))


@functools.lru_cache(maxsize=None)
def cases_misc(w, stream):
    return misc_cases(8 * w, _rng(3, w, stream), reverse=bool(stream))


@functools.lru_cache(maxsize=None)
def cases_au(w, layout, stream):
    return au_cases(8 * w, layout[0], layout[1], _rng(4, w, layout[0], layout[1], stream))


def walk_variant(w, stream):
    return (WIDTHS.index(w) + stream) % 3


@functools.lru_cache(maxsize=None)
def script_walk(w, stream):
    return walk_script(8 * w, walk_variant(w, stream), _rng(5, w, stream))


def walk_statuses(w, variant, n_rows):
    """what addtoFrame answers to walk_script's rows, from its rules alone: 0 while fewer than
    5 blocks are in; a decoded superframe (3) empties the count; every other verdict (1 the
    fire code fails, 2 rejected) keeps 4 blocks, so that the next CIF is looked at again"""
    if variant == 0:
        return [0] * 4 + [2] * (n_rows - 4)
    miss = 2 if variant == 1 else 1                    # a misaligned window: fire-passing rows fail in RS
    aligned, i = set(), 4
    for m in range(8):                                 # the rows at which a whole superframe ends
        if m == 2:
            i += 4
            continue
        aligned.add(i)
        i += 5
    out, blocks = [], 0
    for c in range(n_rows):
        blocks += 1
        if blocks < 5:
            out.append(0)
        elif c in aligned:
            out.append(3 if fillable(8 * w) else 2)
            blocks = 0 if fillable(8 * w) else 4
        else:
            out.append(miss)
            blocks = 4
    return out


def to_script(cases, br):
    """the cases' superframes end to end as CIF rows"""
    return [r for c in cases for r in rows_of(c.sf, br)]


# what each GPU test plays: {width: cases} of stream s (their superframes end to end; 12 frames
# hold 48 rows, so at most 8 superframes, and where a list is longer the streams share it)
def _share(cases, s):
    """up to 8 cases run on both streams (each with its own bytes); of a longer list stream 0
    takes the even ones and stream 1 the odd ones"""
    return cases if len(cases) <= 8 else cases[s::2]


def plan_limit(s):
    return {w: cases_rs(w, s) for w in WIDTHS}


def plan_fail(s):
    return {w: cases_fail(w, s) + cases_rs(w, s)[:1] for w in FAIL_WIDTHS}


def plan_misc(s):
    return {w: cases_misc(w, s) for w in WIDTHS}


def plan_au(layout, s):
    return {w: _share(cases_au(w, layout, s), s) for w in AU_WIDTHS}


def plan_step(s):
    return {w: cases_rs(w, s) + (cases_fail(w, s) if w in FAIL_WIDTHS else cases_misc(w, s)[:3]) + cases_rs(w, s)[:1]
            for w in WIDTHS}


def plan_formats(layout, s):
    return {w: _share(cases_rs(w, s) + cases_au(w, layout, s), s) for w in FORMAT_WIDTHS}


def every_plan():
    for s in (0, 1):
        for f in (plan_limit, plan_fail, plan_misc, plan_step):
            yield f(s)
        for lay in LAYOUTS:
            yield plan_au(lay, s)
            yield plan_formats(lay, s)
