"""k_dp_layer (csrc/k_dabplus.hip) on crafted superframes: every RS width the pipeline accepts,
the rejection branches, the AU CRC slicing and the block walk under controlled inputs, record
by record against orc.MP4 (mp4Processor::addtoFrame restated; tests/test_dabplus_cpu.py pins it
to the reference's own classes on these very bytes).

The seam is the one test_gpu_mp2.py, test_gpu_packet.py and test_gpu_audio_pipeline.py use: after
a run the valid rows of its MSC output are overwritten (Pipeline.msc_d) and Pipeline.dabplus()
reads exactly that buffer.  The transmitted subchannels are random bits; the pipeline's table
flags them DAB+.  One table holds RSDims 1, 2, 3, 5, 7, 11, 21, 32, 33 and 48 (8 to 384 kbit/s,
EEP 4-A, 652 CUs); rows are crafted from the entry's CIF 16 on, each (stream, width) plays its own
script of CIF rows, and the two streams carry different bytes.

What the reference leaves open, and the rule compared here: an AU that a crafted table places
past the superframe's 110 * RSDims bytes reads zeros (the reference reads uninitialised stack).
At RSDims 48 no start table can be accepted (dabplus_py.fillable), so its `clean` superframes
end as status 2 with 5 good AU CRCs; their RS counts, tables and masks are compared all the same.

No tolerance anywhere: every comparison is equality."""
import numpy as np
import pytest

import dabplus_py as dp
import oracle_py as orc

pytestmark = pytest.mark.gpu

N_FRAMES = 16                      # 4 of de-interleaver warm-up, 12 (48 CIFs) of crafted rows
TF = 196608


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def table():
    """[(startAddr, CUs, kbit/s, EEP 4-A, ...)] of dp.WIDTHS, the sizes from dabgpu_subch_profile"""
    import dabamd
    out, sa = [], 0
    for w in dp.WIDTHS:
        _, frag, _, _ = dabamd.subch_profile(dabamd.Subch(0, 864, 8 * w, 0o104, 1, dabamd.SUBCH_DABPLUS))
        assert frag % 64 == 0 and frag // 64 == 4 * w
        out.append((sa, frag // 64, 8 * w, 0o104, 0, 0))
        sa += frag // 64
    assert sa == 652
    return out


@pytest.fixture(scope="module")
def iq(ctx, table):
    """(device IQ of 2 streams, stride, lengths): random-bit subchannels at 300 dB SNR"""
    from dabamd.synth import Ensemble
    e = Ensemble(N_FRAMES, subch=table)
    iqs = [e.generate(s, truth=False)["iq"] for s in (401, 402)]
    lens = [len(x) // 2 for x in iqs]
    buf = np.zeros((2, 2 * max(lens)), np.float32)
    for s, x in enumerate(iqs):
        buf[s, :len(x)] = x
    d = ctx.put(buf)
    yield d, max(lens), lens
    d.free()


def gpu_record(rec):
    na = int(rec["num_aus"])
    return dict(status=int(rec["status"]), n_corrected=int(rec["n_corrected"]), num_aus=na,
                au_start=[int(x) for x in rec["au_start"]], au_crc=[(int(rec["au_crc_ok"]) >> i) & 1 for i in range(8)])


def same_record(rec, sfb, o, br):
    """every field of a record against orc.MP4's; the bytes of a decoded superframe"""
    if rec["status"] != o["status"]:
        return False
    if o["status"] < 2:
        return rec["num_aus"] == 0 and rec["n_corrected"] == 0 and rec["au_crc_ok"] == 0 and not rec["au_start"].any()
    na = o["num_aus"]
    ok = (rec["n_corrected"] == o["n_corrected"] and rec["num_aus"] == na and
          np.array_equal(rec["au_start"][:na + 1], o["au_start"][:na + 1]) and not rec["au_start"][na + 1:].any() and
          rec["au_crc_ok"] == dp.mask_of(o))
    if ok and o["status"] == 3:
        ok = sfb is not None and np.array_equal(sfb[:110 * (br // 8)], o["out"])
    return bool(ok)


class Rig:
    """one two-stream pipeline over the fixture's IQ, run by run: the valid rows of every entry are
    overwritten with the next rows of its script (dp.filler, which fails the fire code, once the
    script has ended), the same rows go to one orc.MP4 per (stream, entry), and every record of
    the DAB+ layer is compared with the oracle's.  fmt: "bits" one bit per byte; "words" packed
    rows of a 4-byte-multiple stride (window_to_lds's word path); "bytes" packed rows of an odd
    stride (its byte path).  recs[s][k] / want[s][k]: the GPU's and the oracle's records of the
    delivered CIFs in order; sfs[s][k]: the bytes of the status-3 ones."""

    def __init__(self, ctx, iq, table, F, fmt="bits", compact=False):
        import dabamd
        self.diq, self.stride, self.lens = iq
        self.F, self.fmt, self.compact, self.tab = F, fmt, compact, table
        subs = [dabamd.Subch(t[0], t[1], t[2], t[3], 1, dabamd.SUBCH_DABPLUS) for t in table]
        self.pipe = p = dabamd.Pipeline(ctx, 2, F, subs, max_bitrate=384)
        assert (p.max_subch, p.max_dabplus) == (len(table), len(table))
        if fmt != "bits":
            p.set_packed(dabamd.PACK_MSC)
            p.msc_stride_packed += 1 if fmt == "bytes" else 0
            assert (p.msc_stride_packed % 4 == 0) == (fmt == "words")
        if compact:
            p.set_dabplus_compact(True)
        p.control(dabamd.CTL_ACQ_SYNC)
        n = len(table)
        self.mp4 = [[orc.MP4(t[2]) for t in table] for _ in range(2)]
        self.recs = [[[] for _ in range(n)] for _ in range(2)]
        self.want = [[[] for _ in range(n)] for _ in range(2)]
        self.sfs = [[[] for _ in range(n)] for _ in range(2)]
        self.frames = [[], []]
        self.bad = []

    def close(self):
        self.pipe.close()

    def play(self, scripts, short=None):
        """scripts[s][k]: list of CIF rows (3 * bitRate bytes each).  short: {run: samples stream 1
        gets beyond its next window in that run} -- it then delivers fewer CIFs than stream 0"""
        p, F, NS = self.pipe, self.F, len(self.tab)
        ms = p.msc_stride_packed if p.packed else p.msc_stride
        pos = [[0] * NS for _ in range(2)]
        for r in range(-(-N_FRAMES // F) + 2 * len(short or {}) + 1):
            na = list(self.lens)
            if short and r in short:
                na[1] = min(self.lens[1], p.state(1).next_pos + short[r])
            p.run(self.diq, self.stride, na, download=False, partial=True)
            p.sync()
            st = [p.state(s) for s in range(2)]
            if not any(x.frames_run for x in st) and not (short and r in short):
                break
            ev = p.msc_entry_valid()
            host = np.zeros((2, 4 * F, NS, ms), np.uint8)
            fed = []
            for s in range(2):
                nf = st[s].frames_run
                self.frames[s].append(nf)
                cif0 = st[s].cif_count - 4 * nf
                for c in range(4 * F):
                    valid = c < 4 * nf and cif0 + c >= 16
                    assert (ev[s, c] == valid).all(), (r, s, c)
                    if not valid:
                        continue
                    for k, t in enumerate(self.tab):
                        sc = scripts[s][k]
                        row = sc[pos[s][k]] if pos[s][k] < len(sc) else dp.filler(t[2], s)
                        pos[s][k] += 1
                        e = dp.emit(row, p.packed)
                        host[s, c, k, :len(e)] = e
                        fed.append((s, c, k, self.mp4[s][k].add(np.unpackbits(row))))
            p.msc_d.upload_at(host, 0)
            info, sf = p.dabplus()
            seen = np.zeros((2, 4 * F, NS), bool)
            for s, c, k, o in fed:
                rec, br = info[s, c, k], self.tab[k][2]
                seen[s, c, k] = True
                if self.compact:
                    sfb = sf[s, k, rec["reserved"]] if rec["reserved"] != 0xFF else None
                else:
                    sfb = sf[s, c, k]
                if not same_record(rec, sfb, o, br):
                    self.bad.append((r, s, c, br // 8, gpu_record(rec), {x: o[x] for x in o if x != "out"}))
                self.recs[s][k].append(rec.copy())
                self.want[s][k].append(o)
                if rec["status"] == 3:
                    self.sfs[s][k].append(sfb[:110 * (br // 8)].copy())
            assert (info["status"][~seen] == -1).all(), r          # warm-up, or a CIF the stream did not deliver
            if self.compact:
                for s in range(2):
                    for k in range(NS):
                        dec = info["status"][s, :, k] == 3
                        assert list(info["reserved"][s, dec, k]) == list(range(int(dec.sum()))), (r, s, k)
                        assert (info["reserved"][s, ~dec, k] == 0xFF).all(), (r, s, k)
            else:
                assert not info["reserved"].any()
        self.consumed = pos
        assert not self.bad, (len(self.bad), self.bad[:3])
        return self

    def check_cases(self, cases, s, k):
        """the record at the 5th row of each case of a script made by dp.to_script is the one the
        case is named for"""
        w = self.tab[k][2] // 8
        assert self.consumed[s][k] >= 5 * len(cases), (s, w, self.consumed[s][k], len(cases))
        for m, c in enumerate(cases):
            dp.check_expect(w, c, gpu_record(self.recs[s][k][5 * m + 4]))


def run_cases(ctx, iq, table, F, case_lists, fmt="bits", compact=False, short=None):
    """case_lists[s][w]: the cases of stream s at width w (the other widths get filler rows)"""
    rig = Rig(ctx, iq, table, F, fmt, compact)
    try:
        scripts = [[dp.to_script(case_lists[s].get(t[2] // 8, []), t[2]) for t in table] for s in range(2)]
        assert max(len(x) for sc in scripts for x in sc) <= 44          # 12 frames hold 48 rows
        rig.play(scripts, short)
        for s in range(2):
            for k, t in enumerate(table):
                rig.check_cases(case_lists[s].get(t[2] // 8, []), s, k)
    finally:
        rig.close()
    return rig


# ---- 1 --------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2])
def test_every_width_clean_and_at_the_correction_limit(ctx, iq, table, F):
    """clean; exactly 5 errors in every column (n_corrected 5 * RS, 240 at width 48); errors in the
    parity rows only (syndromes non-zero, nothing counted or changed); 2 data + 1 parity errors
    per column (counted as 2) -- at every width, whose syndrome phase maps lanes to (column
    lane % RS, row slice lane / RS): widths that do not divide 64 leave lanes idle and slices
    uneven, width 1 puts 64 lanes on one column, above 32 each column has one lane, at 48 the
    LDS stage, the syndrome array and the carry are full.  F = 1: every 5-CIF window crosses a
    run boundary and reads the carry"""
    rig = run_cases(ctx, iq, table, F, [dp.plan_limit(s) for s in range(2)])
    k48 = len(dp.WIDTHS) - 1
    assert [int(r["n_corrected"]) for r in rig.recs[0][k48][4:20:5]] == [0, 240, 0, 96]
    assert rig.frames[0][:N_FRAMES // F] == [F] * (N_FRAMES // F) == rig.frames[1][:N_FRAMES // F]
    assert not np.array_equal(rig.sfs[0][0][0], rig.sfs[1][0][0])         # the streams' own bytes


# ---- 2 --------------------------------------------------------------------------------
def test_first_failing_column_stops_the_count(ctx, iq, table):
    """6 errors in column 0 (status 2, nothing counted), in the last column behind columns of 5
    (5 * (RS - 1) counted), in a middle column with errors behind it (only the columns before
    it counted); then a clean superframe, found again through blocks = 4"""
    rig = run_cases(ctx, iq, table, 2, [dp.plan_fail(s) for s in range(2)])
    for s in range(2):
        for w in dp.FAIL_WIDTHS:
            got = [int(r["status"]) for r in rig.recs[s][dp.WIDTHS.index(w)][:20]]
            assert got[:15] == [0, 0, 0, 0, 2] + [1, 1, 1, 1, 2] * 2 and got[15:19] == [1] * 4


# ---- 3 --------------------------------------------------------------------------------
def test_miscorrecting_columns(request):
    """columns of 6, 7 and 8 errors that the decoder answers with a count instead of -1 (about
    0.6 % of random patterns; found on the CPU from a fixed seed): the wrongly corrected
    superframe's status, count, AU table and bytes equal the oracle's, and k_rs gives the same
    words the same verdicts"""
    found = dp.miscorrecting()
    assert all(len(found[k]) >= 8 for k in (6, 7, 8)), {k: len(v) for k, v in found.items()}
    ctx, iq, table = (request.getfixturevalue(x) for x in ("ctx", "iq", "table"))     # the GPU only after that
    plans = [dp.plan_misc(s) for s in range(2)]
    rig = run_cases(ctx, iq, table, 2, plans)
    got = [int(r["status"]) for s in range(2) for k, w in enumerate(dp.WIDTHS)
           for r in rig.recs[s][k][4:5 * len(plans[s][w]):5]]
    assert got.count(3) > 0 and set(got) <= {2, 3}
    rng = np.random.default_rng(12)
    cws = []
    for k in (6, 7, 8):
        for pat in found[k]:
            cw = dp.rs_encode(rng.integers(0, 256, 110).astype(np.uint8))
            for r, v in pat:
                cw[r] ^= v
            cws.append(cw)
    out, ret = ctx.rs_decode(np.stack(cws))
    for i, cw in enumerate(cws):
        o, r = orc.rs_dec(cw)
        assert r >= 0 and ret[i] == r and np.array_equal(out[i], o), i


# ---- 4 --------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(dp.LAYOUTS), ids=lambda x: "dac%d_sbr%d" % x)
def test_au_table_and_crc_edges(ctx, iq, table, layout):
    """AU lengths 0, 1, 63, 64, 65 (around the 64 slices of the CRC) and the largest that fits,
    959, 960 (rejected), a descending table, a start of 4095, a wrong CRC in every position, a
    table whose second or later AU is impossible (status 2, the mask keeps the earlier AUs'
    bits), an AU that starts inside and ends past the superframe -- at widths 2 and 33.  What a
    width cannot hold does not occur there: at 33 the 2- and 3-AU layouts cannot fill the
    superframe (only their rejections exist), the 4-AU layout holds only 959, 959, 959, 737, and
    an AU that ends past the end needs the 6-AU layout (AU 4 from 2915 to 3640); at 2 nothing
    is 959 or 960 long.  profiles/dabplus_edges.txt lists the cases per width and layout"""
    run_cases(ctx, iq, table, 2, [dp.plan_au(layout, s) for s in range(2)])


# ---- 5 --------------------------------------------------------------------------------
def test_walk_under_dense_candidates(ctx, iq, table):
    """all-zero rows (a muted subchannel: every CIF passes the fire code and the RS decode, the AU
    table rejects: status 2 from the 5th CIF on); superframes whose every row passes the fire
    code (status 3 every 5th CIF, 0 between, no stray 2: the walk discards the candidates the
    reference never looks at); a dropped CIF behind a decoded superframe (found again through
    status 2, or 1 among plain rows).  F = 3: 12 CIFs a run.  Sparse and compact output: the
    compact slots and `reserved` give the sparse run's status-3 records in CIF order"""
    rigs = []
    for compact in (False, True):
        rig = Rig(ctx, iq, table, 3, compact=compact)
        try:
            rig.play([[dp.script_walk(t[2] // 8, s) for t in table] for s in range(2)])
        finally:
            rig.close()
        rigs.append(rig)
    a, b = rigs
    n3 = 0
    for s in range(2):
        for k, t in enumerate(table):
            w = t[2] // 8
            got = [int(r["status"]) for r in a.recs[s][k]]
            assert a.consumed[s][k] >= 39 and got[:39] == dp.walk_statuses(w, dp.walk_variant(w, s), 39), (s, w, got)
            assert got == [int(r["status"]) for r in b.recs[s][k]]
            assert len(a.sfs[s][k]) == len(b.sfs[s][k]) == got.count(3)
            assert all(np.array_equal(x, y) for x, y in zip(a.sfs[s][k], b.sfs[s][k]))
            n3 += got.count(3)
    assert n3 >= 6 * 2 * 6                               # 7 superframes of 2 variants at the fillable widths


# ---- 6 --------------------------------------------------------------------------------
def test_streams_out_of_step(ctx, iq, table):
    """F = 2.  Stream 1 gets samples for no frame in run 3 and for one frame (4 CIFs) in run 5, and
    all of them in the runs between and after: its 5-CIF windows across the gaps (the carry kept
    through a run without CIFs, and advanced by 4 of 8 slots) equal the oracle fed only the
    delivered CIFs; stream 0 is unaffected"""
    rig = run_cases(ctx, iq, table, 2, [dp.plan_step(s) for s in range(2)], short={3: 1000, 5: TF + 60000})
    assert rig.frames[0][:8] == [2] * 8
    assert rig.frames[1][:7] == [2, 2, 2, 0, 2, 1, 2] and sum(rig.frames[1]) == sum(rig.frames[0]) == N_FRAMES


# ---- 7 --------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(dp.LAYOUTS), ids=lambda x: "dac%d_sbr%d" % x)
@pytest.mark.parametrize("fmt", ["bits", "words", "bytes"])
def test_row_formats(ctx, iq, table, fmt, layout):
    """cases 1 and 4 at widths 3 and 48 with the MSC rows one bit per byte, packed with a stride
    that is a multiple of 4 (window_to_lds reads words) and packed with an odd stride (bytes)"""
    run_cases(ctx, iq, table, 2, [dp.plan_formats(layout, s) for s in range(2)], fmt=fmt)


# ---- k_rs on its own ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_rs_operator_block_edges(ctx, n):
    """dabgpu_rs_decode at codeword counts around its 64-lane blocks: the all-zero word, a word
    of all 0xFF, the reference's golden words (tests/golden/rs_kat.npz) repeated across the
    block boundary, words at and past the correction limit"""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rs_kat.npz"))
    rng = np.random.default_rng(n)
    cws = [np.zeros(120, np.uint8), np.full(120, 0xFF, np.uint8)]
    while len(cws) < n + 2:
        i = len(cws)
        if i % 3:
            cws.append(g["cw"][i % len(g["cw"])].copy())
        else:
            cw = dp.rs_encode(rng.integers(0, 256, 110).astype(np.uint8))
            cw[rng.choice(120, i % 8, replace=False)] ^= rng.integers(1, 256, i % 8).astype(np.uint8)
            cws.append(cw)
    cws = np.stack(cws)[:n]
    out, ret = ctx.rs_decode(cws)
    assert out.shape == (n, 110) and ret.shape == (n,)
    for i in range(n):
        o, r = orc.rs_dec(cws[i])
        assert ret[i] == r and np.array_equal(out[i], o), (n, i)
    if n >= 63:
        kat = [i for i in range(2, n) if i % 3]
        assert np.array_equal(ret[kat], g["ret"][[i % len(g["cw"]) for i in kat]])
