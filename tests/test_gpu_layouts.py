"""Per-stream subchannel tables (dabgpu_pipe_create_caps / dabgpu_pipe_set_subch) against
the reference CPU path.

The criterion is the project's own: zero mismatching decoded bits against the oracle run
per stream with that stream's own table (oracle_py: ofdmProcessor::run's soft bits through
dabConcurrent per entry -- orc_msc_stream), FIC and frame placement through
pipeline_check.compare.  An entry set while the stream stands at CIF `since` is a
dabConcurrent started there: the oracle is fed the stream's soft CIFs from `since` on and
its output j is CIF since + j, delivered from j = 16 (dab-concurrent.cpp:162-175).

All tests share three 13-frame synthetic streams (25 dB, cf32, one transmitted layout that
holds the MIXED subchannels of test_gpu_pipeline_oracle and two DAB+ ones) and their oracle
front end, computed once; any CU range decodes deterministically in both paths, so a
stream's table need not be what its transmitter sent.  F = 3 frames per run,
DABGPU_CTL_ACQ_SYNC."""
import numpy as np
import pytest

import oracle_py as orc
import pipeline_check as pc
from test_gpu_pipeline_oracle import MIXED

pytestmark = pytest.mark.gpu

F = 3
NFR = 13
SENT = 0xA5                      # fill of the MSC output before a run: untouched rows keep it
E_ARG, E_UNSUP = -1, -5

# (startAddr, CUs, bitRate, protLevel, uep, dabplus)
A, B, Cc, D, E5 = [sc + (0,) for sc in MIXED]
D64 = (96, 48, 64, 0o103, 0, 1)          # B's CUs as the DAB+ subchannel the transmitter sends there
D32 = (252, 24, 32, 0o103, 0, 1)
EEPB = (300, 18, 32, 0o203, 0, 0)        # EEP-3B over CUs the transmitter leaves empty
TX = [A, D64, Cc, D, D32, E5]


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


class Streams:
    """the shared streams, their oracle front end, and the oracle's dabConcurrent per
    (stream, entry, since) -- each computed once"""

    def __init__(self):
        from dabamd.synth import Ensemble
        e = Ensemble(NFR, subch=TX, snr_db=25.0)
        self.iqs = [e.generate(s, truth=False)["iq"] for s in (71, 72, 73)]
        self.refs = orc.decode_streams(self.iqs, NFR - 1, [])
        self._msc = {}

    def entry(self, s, sc, since):
        """[ncif - since][24 * bitRate]: row j is CIF since + j of a decoder started at since"""
        key = (s, tuple(sc[:5]), since)
        if key not in self._msc:
            soft = self.refs[s]["soft"]
            cifs = soft[:, 3:75].reshape(4 * len(soft), -1)[since:]
            sa, ln, br, pl, uep = sc[:5]
            frag = np.ascontiguousarray(cifs[:, sa * 64:(sa + ln) * 64])
            out = np.zeros((len(cifs), 24 * br), np.uint8)
            assert orc.oracle().orc_msc_stream(uep, br, pl, ln * 64, len(cifs), orc.P(frag), orc.P(out)) == 0
            self._msc[key] = out
        return self._msc[key]


@pytest.fixture(scope="module")
def streams():
    return Streams()


def _subs(table):
    import dabamd
    return [dabamd.Subch(sc[0], sc[1], sc[2], sc[3], 0 if sc[4] else 1, dabamd.SUBCH_DABPLUS if sc[5] else 0)
            for sc in table]


def _tuples(subs):
    return [(s.startAddr, s.length, s.bitRate, s.protLevel, 0 if s.uepFlag else 1, s.flags & 1) for s in subs]


class Rig:
    """a caps pipeline over streams[which], the expected tables (entry, since) kept beside
    it by the rule of dabgpu_pipe_set_subch, and every run checked as it is made"""

    def __init__(self, ctx, streams, which, init, caps, packed=0, compact=False):
        import dabamd
        self.ctx, self.st, self.which = ctx, streams, list(which)
        self.S = len(self.which)
        self.iqs = [streams.iqs[w] for w in self.which]
        self.lens = [len(x) // 2 for x in self.iqs]
        self.stride = max(self.lens)
        buf = np.zeros((self.S, 2 * self.stride), np.float32)
        for s, x in enumerate(self.iqs):
            buf[s, :len(x)] = x
        self.diq = ctx.put(buf)
        self.pipe = dabamd.Pipeline(ctx, self.S, F, _subs(init), max_subch=caps[0], max_bitrate=caps[1],
                                    max_dabplus=caps[2])
        self.NS, self.NDP = caps[0], caps[2]
        self.pipe.control(dabamd.CTL_ACQ_SYNC)
        self.packed = packed
        if packed:
            self.pipe.set_packed(packed)
        self.compact = compact
        if compact:
            self.pipe.set_dabplus_compact(True)
        self.tab = [[(tuple(sc), 0) for sc in init] for _ in range(self.S)]
        self.gpu = [dict(info=[], fic=[], crc=[], msc={}, soft={}) for _ in range(self.S)]
        self.lives = {}                  # (s, k, entry, since) -> [(cif, record, bytes or None)]
        self.msc_cw = self.msc_bad = 0
        self.valid_cifs = {}             # (s, k, entry, since) -> CIFs delivered

    def close(self):
        self.pipe.close()
        self.diq.free()

    def cif_count(self, s):
        return self.pipe.state(s).cif_count

    def set(self, s, table):
        """set_subch and the expected table: same index and fields keeps since"""
        self.pipe.set_subch(s, _subs(table))
        for t in (range(self.S) if s < 0 else [s]):
            now = self.cif_count(t)
            old = self.tab[t]
            self.tab[t] = [(tuple(sc), old[k][1] if k < len(old) and old[k][0] == tuple(sc) else now)
                           for k, sc in enumerate(table)]
            subs, since = self.pipe.get_subch(t)
            assert _tuples(subs) == [e[0] for e in self.tab[t]] and since == [e[1] for e in self.tab[t]], (t, since)

    def run(self, na=None):
        import dabamd
        pipe = self.pipe
        pipe.sync()
        out = pipe._outs[pipe._run & 1][2]
        dabamd._chk(dabamd.lib().dabgpu_memset_d(self.ctx.h, out.ptr, SENT, out.nbytes), "memset")
        fic, crc, raw, valid = pipe.run(self.diq, self.stride, na if na is not None else self.lens, partial=True)
        ev = pipe.msc_entry_valid()
        dp = pipe.dabplus() if self.NDP else None
        msc = np.unpackbits(raw, axis=-1) if self.packed & dabamd.PACK_MSC else raw
        if self.packed & dabamd.PACK_FIC:
            fic = np.unpackbits(fic, axis=-1)
        fi = pipe.frame_info()
        for s in range(self.S):
            st = pipe.state(s)
            nf = st.frames_run
            cif0 = st.cif_count - 4 * nf
            for f in range(nf):
                self.gpu[s]["info"].append(fi[s][f])
                self.gpu[s]["fic"].append(fic[s, f].copy())
                self.gpu[s]["crc"].append(crc[s, f].copy())
            for c in range(4 * F):
                assert valid[s, c] == (c < 4 * nf and cif0 + c >= 16), (s, c)
                for k in range(self.NS):
                    ent = self.tab[s][k] if k < len(self.tab[s]) else None
                    want = ent is not None and c < 4 * nf and cif0 + c >= ent[1] + 16
                    assert ev[s, c, k] == want, (s, c, k, cif0, ent)
                    if not want:                  # absent, not delivered or warming up: untouched
                        assert (raw[s, c, k] == SENT).all(), (s, c, k, cif0, ent)
                        continue
                    sc, since = ent
                    ref = self.st.entry(self.which[s], sc, since)[cif0 + c - since]
                    self.msc_cw += 1
                    self.msc_bad += int(not np.array_equal(msc[s, c, k, :24 * sc[2]], ref))
                    self.valid_cifs.setdefault((s, k, sc, since), []).append(cif0 + c)
            if dp is None:
                continue
            info, sfb = dp
            slots = [k for k, e in enumerate(self.tab[s]) if e[0][5]]
            for j in range(self.NDP):
                if j >= len(slots):               # absent slot: status -1 records
                    assert (info[s, :, j]["status"] == -1).all(), (s, j)
                    continue
                k = slots[j]
                life = self.lives.setdefault((s, k) + self.tab[s][k], [])
                for c in range(4 * nf):
                    rec = info[s, c, j]
                    if self.compact:
                        assert (rec["reserved"] != 0xFF) == (rec["status"] == 3), (s, c, j, rec)
                        by = sfb[s, j, rec["reserved"]].copy() if rec["status"] == 3 else None
                    else:
                        by = sfb[s, c, j].copy()
                    life.append((cif0 + c, rec.copy(), by))
                assert (info[s, 4 * nf:, j]["status"] == -1).all()

    def check_fic(self):
        """FIC bits, CRC flags and frame placement of every stream against the oracle"""
        for s in range(self.S):
            g = dict(self.gpu[s], fic=np.array(self.gpu[s]["fic"]).reshape(-1, 4, 768),
                     crc=np.array(self.gpu[s]["crc"]).reshape(-1, 12))
            r = pc.compare(g, self.st.refs[self.which[s]], [], check_soft=False)
            assert r["frames"] > 0 and r["placement"] == 0 and r["fic_bad"] == 0 and r["crc_bad"] == 0, (s, r)

    def check_dabplus(self):
        """every DAB+ entry's records against a fresh mp4Processor fed the oracle's bits of
        that entry from its since_cif on.  Returns superframes decoded per life."""
        done = {}
        for key, recs in self.lives.items():
            s, k, sc, since = key
            ref = self.st.entry(self.which[s], sc, since)
            mp4 = orc.MP4(sc[2])
            ok3 = 0
            for cif, rec, by in recs:
                if cif < since + 16:
                    assert rec["status"] == -1, (key, cif, rec)
                    continue
                o = mp4.add(ref[cif - since])
                same = rec["status"] == o["status"]
                if same and o["status"] >= 2:
                    same = rec["n_corrected"] == o["n_corrected"] and rec["num_aus"] == o["num_aus"]
                if same and o["status"] == 3:
                    na, nb = o["num_aus"], 110 * (sc[2] // 8)
                    same = (np.array_equal(rec["au_start"][:na + 1], o["au_start"][:na + 1]) and
                            rec["au_crc_ok"] == sum(int(o["au_crc"][a]) << a for a in range(na)) and
                            np.array_equal(by[:nb], o["out"][:nb]))
                    ok3 += 1
                assert same, (key, cif, rec, o["status"])
            done[key] = ok3
        return done


def _layouts(ctx, streams, packed):
    import dabamd
    rig = Rig(ctx, streams, [0, 1, 2], [A, B, Cc, D, E5], (6, 128, 0), packed=packed)
    try:
        t1 = [Cc, B, EEPB]
        rig.set(1, t1)
        rig.set(2, [])
        for _ in range(4):
            rig.run()
        rig.check_fic()
        print("layouts: codewords", rig.msc_cw, "mismatching", rig.msc_bad)
        assert rig.msc_bad == 0
        assert rig.msc_cw == (5 + 3) * (4 * F * 4 - 16)     # every entry, every CIF >= 16
        rig.pipe.sync()
        ctx.check()
    finally:
        rig.close()


def test_streams_with_different_layouts(ctx, streams):
    """three streams: the five MIXED entries; two of them in swapped order plus an EEP-B
    entry; an empty table -- max_subch 6, so every stream has padding rows.  4 runs: every
    entry's bits of every CIF >= 16 equal the oracle, msc_entry_valid is 0 and the rows keep
    the fill for absent entries, FIC and placement match for all three, no kernel refused
    work"""
    _layouts(ctx, streams, 0)


def test_different_layouts_packed_outputs(ctx, streams):
    """the same with DABGPU_PACK_MSC | DABGPU_PACK_FIC"""
    import dabamd
    _layouts(ctx, streams, dabamd.PACK_MSC | dabamd.PACK_FIC)


def test_pipeline_created_empty_then_tables_set(ctx, streams):
    """create_caps with n_subch = 0, one FIC-only run (12 CIFs), set_subch per stream, 3 runs:
    the entries deliver from since + 16 = 28 and equal orc_msc_stream fed the oracle's soft
    CIFs from CIF 12 on"""
    rig = Rig(ctx, streams, [0, 1], [], (5, 128, 0))
    try:
        rig.run()
        assert rig.msc_cw == 0
        rig.set(0, [A, B, Cc, D, E5])
        rig.set(1, [Cc, B, A])
        assert [e[1] for e in rig.tab[0]] == [12] * 5 and [e[1] for e in rig.tab[1]] == [12] * 3
        for _ in range(3):
            rig.run()
        rig.check_fic()
        assert rig.msc_bad == 0
        assert rig.msc_cw == (5 + 3) * (48 - 28)
        for key, cifs in rig.valid_cifs.items():
            assert cifs == list(range(28, 48)), key
        rig.pipe.sync()
        ctx.check()
    finally:
        rig.close()


def test_table_changed_mid_stream(ctx, streams):
    """two streams, 2 runs, stream 1 switches from {A, B} to {A, C, D}, 2 more runs: A is
    bit-equal to the uninterrupted oracle decode at every CIF (no gap, since_cif still 0);
    C and D are valid from since + 16 and equal the oracle restarted at since; stream 0 is
    untouched; get_subch returns what was set (Rig.set asserts it)"""
    rig = Rig(ctx, streams, [0, 1], [A, B], (5, 128, 0))
    try:
        rig.set(0, [A, B, Cc, D, E5])
        rig.run()
        rig.run()
        rig.set(1, [A, Cc, D])
        assert [e[1] for e in rig.tab[1]] == [0, 24, 24] and [e[1] for e in rig.tab[0]] == [0] * 5
        rig.run()
        rig.run()
        rig.check_fic()
        assert rig.msc_bad == 0
        assert rig.valid_cifs[(1, 0, A, 0)] == list(range(16, 48))
        assert rig.valid_cifs[(1, 1, B, 0)] == list(range(16, 24))
        assert rig.valid_cifs[(1, 1, Cc, 24)] == rig.valid_cifs[(1, 2, D, 24)] == list(range(40, 48))
        for k, sc in enumerate([A, B, Cc, D, E5]):
            assert rig.valid_cifs[(0, k, sc, 0)] == list(range(16, 48))
        rig.pipe.sync()
        ctx.check()
    finally:
        rig.close()


def test_streams_out_of_lockstep_with_own_tables(ctx, streams):
    """as test_pipeline_streams_out_of_lockstep: stream 1 gets samples up to the end of its
    2nd frame in run 1.  The streams have different tables and stream 1's is replaced after
    run 1: since_cif follows that stream's own cif_count (8, not stream 0's 12)"""
    rig = Rig(ctx, streams, [0, 1], [A, B, Cc], (4, 128, 0))
    try:
        rig.set(1, [D, A])
        n = rig.lens
        fi = streams.refs[1]["info"][1]
        short = fi.window_start + fi.start_index + 2048 + 75 * 2552 + 10
        rig.run([n[0], short])
        assert rig.pipe.state(0).frames_run == F and rig.pipe.state(1).frames_run == 2
        rig.set(1, [D, B, Cc])
        assert [e[1] for e in rig.tab[1]] == [0, 8, 8]
        for _ in range(3):
            rig.run()
        rig.check_fic()
        assert rig.msc_bad == 0
        assert rig.cif_count(0) == 48 and rig.cif_count(1) == 44
        assert rig.valid_cifs[(1, 0, D, 0)] == list(range(16, 44))
        assert rig.valid_cifs[(1, 1, B, 8)] == rig.valid_cifs[(1, 2, Cc, 8)] == list(range(24, 44))
        assert rig.valid_cifs[(0, 0, A, 0)] == list(range(16, 48))
        rig.pipe.sync()
        ctx.check()
    finally:
        rig.close()


@pytest.mark.parametrize("compact", [False, True], ids=["sparse", "compact"])
def test_dabplus_slots_per_stream(ctx, streams, compact):
    """stream 0: two DAB+ entries (64 and 32 kbit/s, EEP-3A) around a non-DAB+ one; stream 1:
    one DAB+ entry, its last entry (slot 0 of 2, the other absent).  Records and bytes per
    stream against the oracle's mp4Processor, sparse and compact.  After run 1 stream 0's
    64 kbit/s entry is replaced by a 32 kbit/s one and the other DAB+ entry kept: the kept
    one's superframe sequence continues, the replaced slot starts like a fresh orc.MP4 at
    CIF 12 + 16; after run 3 the replaced one goes and the kept entry moves from slot 1 to
    slot 0, still continuing"""
    rig = Rig(ctx, streams, [0, 1], [D64, A, D32], (3, 128, 2), compact=compact)
    try:
        rig.set(1, [A, Cc, D64])
        rig.run()
        rig.set(0, [D32, A, D32])
        assert [e[1] for e in rig.tab[0]] == [12, 0, 0]
        rig.run()
        rig.run()
        rig.set(0, [A, A, D32])
        assert [e[1] for e in rig.tab[0]] == [36, 0, 0]
        rig.run()
        rig.check_fic()
        assert rig.msc_bad == 0
        done = rig.check_dabplus()
        print("superframes decoded per DAB+ entry:", done)
        # (counts of the oracle's own decoded superframes: 32 CIFs past the warm-up hold at
        # least 6 whole superframes of 5 CIFs, the 8 CIFs 28..35 at least one)
        assert done[(0, 2, D32, 0)] >= 6                 # through both changes
        assert done[(1, 2, D64, 0)] >= 6
        assert done[(0, 0, D32, 12)] >= 1
        assert done[(0, 0, D64, 0)] == 0                 # CIFs 0..11: warm-up only
        rig.pipe.sync()
        ctx.check()
    finally:
        rig.close()


def test_set_subch_errors_leave_the_table(ctx, streams):
    """each refused table returns its code, leaves get_subch unchanged, and the next run
    still matches the oracle"""
    import dabamd
    rig = Rig(ctx, streams, [0], [A, D64, Cc], (5, 128, 2))
    try:
        rig.run()
        rig.run()
        before = rig.pipe.get_subch(0)
        bad = [([A, B, Cc, D, E5, EEPB], E_ARG),                         # n > max_subch
               ([A, (0, 144, 192, 0o103, 0, 0)], E_ARG),                 # bitRate above the cap
               ([D64, D32, (300, 48, 64, 0o103, 0, 1)], E_ARG),          # a third DAB+ entry, max_dabplus = 2
               ([A, (800, 96, 128, 3, 1, 0)], E_ARG),                    # startAddr + length > 864
               ([A, (96, 96, 128, 0o105, 0, 0)], E_UNSUP)]               # EEP-A level 5: undefined
        for table, code in bad:
            with pytest.raises(dabamd.DabError) as ei:
                rig.pipe.set_subch(0, _subs(table))
            assert ei.value.code == code, (table, ei.value)
            after = rig.pipe.get_subch(0)
            assert _tuples(after[0]) == _tuples(before[0]) and after[1] == before[1]
            with pytest.raises(dabamd.DabError) as ei:
                rig.pipe.set_subch(-1, _subs(table))
            assert ei.value.code == code
        rig.run()
        rig.check_fic()
        assert rig.msc_bad == 0 and rig.msc_cw == 3 * (36 - 16)
        rig.check_dabplus()
    finally:
        rig.close()


def test_plain_pipeline_equals_caps_pipeline(ctx, streams):
    """Pipeline as before against create_caps with the same table and equal caps, on the
    same IQ: every output byte equal (of the MSC the rows of valid CIFs, of the superframe
    bytes those a record says decoded: the rest of those buffers is never written)"""
    import dabamd
    table = _subs([A, D64, Cc])
    iq = streams.iqs[0]
    n = len(iq) // 2
    diq = ctx.put(iq)
    pa = dabamd.Pipeline(ctx, 1, F, table)
    pb = dabamd.Pipeline(ctx, 1, F, table, max_subch=3, max_bitrate=128, max_dabplus=1)
    try:
        for r in range(3):
            oa = pa.run(diq, n, [n])
            ob = pb.run(diq, n, [n])
            for i, (x, y) in enumerate(zip(oa, ob)):
                assert x.shape == y.shape, (r, i)
                if i == 2:                        # MSC: the rows of warm-up CIFs and a row's bytes
                    for k, sc in enumerate(table):    # past 24 * bitRate are never written
                        nb = 24 * sc.bitRate
                        assert np.array_equal(x[oa[3] != 0][:, k, :nb], y[ob[3] != 0][:, k, :nb]), (r, k)
                    continue
                assert np.array_equal(x, y), (r, i)
            ia, sa = pa.dabplus()
            ib, sb = pb.dabplus()
            assert ia.tobytes() == ib.tobytes()
            dec = ia["status"] == 3
            w = 110 * 8
            assert np.array_equal(sa[..., :w][dec], sb[..., :w][dec])
        assert (pb.msc_entry_valid()[0, :, :] == oa[3][0, :, None]).all()
    finally:
        pa.close()
        pb.close()
        diq.free()
