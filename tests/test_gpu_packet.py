"""Packet-mode data on the GPU (k_packet.hip): the pipeline layer dabgpu_pipe_packet against
its byte-level restatement packet_py.Assembler (itself held to oracle_py.Datagroups and to
the reference's own code through tests/golden/packet_kat.npz by test_packet_cpu).

As in test_gpu_mp2 the expected records come from the MSC rows the pipeline itself delivered
for the entry: the layer is checked as the function of its input that mscDatagroup is."""
import os
import subprocess

import numpy as np
import pytest

import packet_py as pp
from test_packet_cpu import kat  # noqa: F401  (the golden file as a fixture)

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUP, E_STATE = -1, -5, -6
F = 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 8 kbit/s (one 24-byte cell per CIF), 32 kbit/s (all four packet lengths fit) and 128 kbit/s
# packet-mode entries, EEP 3-A, beside a layer II and a DAB+ entry
TX = [(0, 6, 8, 0o103, 0, 8), (6, 24, 32, 0o103, 0, 8), (48, 96, 128, 0o103, 0, 8), (144, 96, 128, 3, 1, 4),
      (240, 24, 32, 0o103, 0, 1)]
PK = [(0, 8), (1, 32), (2, 128)]


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


def _subs(table):
    import dabamd
    return [dabamd.Subch(a, n, br, pl, 0 if uep else 1, fl) for a, n, br, pl, uep, fl in table]


@pytest.fixture(scope="module")
def tx_iq():
    """two streams of one ensemble layout, 19 frames, every subchannel with its own content"""
    from dabamd.synth import Ensemble, MP2, PACKET
    e = Ensemble(3 * F + 1, subch=[(0, 6, 8, 0o103, 0, 0, PACKET), (6, 24, 32, 0o103, 0, 0, PACKET),
                                   (48, 96, 128, 0o103, 0, 0, PACKET), (144, 96, 128, 3, 1, 0, MP2),
                                   (240, 24, 32, 0o103, 0, 1, 0)], figs=True)
    return [e.generate(s, truth=False)["iq"] for s in (411, 412)]


@pytest.fixture(scope="module")
def long_iq():
    """one stream of the same layout, 61 frames: long enough for the 8 kbit/s entry's 20 groups
    and for several 500-packet windows on the 128 kbit/s entry"""
    from dabamd.synth import Ensemble, MP2, PACKET
    e = Ensemble(10 * F + 1, subch=[(0, 6, 8, 0o103, 0, 0, PACKET), (6, 24, 32, 0o103, 0, 0, PACKET),
                                    (48, 96, 128, 0o103, 0, 0, PACKET), (144, 96, 128, 3, 1, 0, MP2),
                                    (240, 24, 32, 0o103, 0, 1, 0)], figs=True)
    return [e.generate(413, truth=False)["iq"]]


class Layer:
    """a pipeline with packet-mode entries, run by run: everything the layer writes against
    an Assembler per (stream, slot) fed with the entry's own delivered rows"""

    def __init__(self, ctx, iqs, subs, packed=False, first=True, frames=F, audio=True, **caps):
        import dabamd
        self.ctx, self.S, self.F, self.audio = ctx, len(iqs), frames, audio
        self.lens = [len(x) // 2 for x in iqs]
        self.stride = max(self.lens)
        buf = np.zeros((self.S, 2 * self.stride), np.float32)
        for s, x in enumerate(iqs):
            buf[s, :len(x)] = x
        self.diq = ctx.put(buf)
        self.pipe = dabamd.Pipeline(ctx, self.S, frames, subs, **caps)
        self.pipe.control(dabamd.CTL_ACQ_SYNC)
        self.packed, self.first = packed, first
        if packed:
            self.pipe.set_packed(True)
        self.asm = {}
        self.table(subs)
        self.out, self.other, self.rows, self.fed = [], [], [], {}

    def table(self, subs, keep=()):
        """the packet slots of `subs`; the table entries in `keep` go on with their assemblers"""
        import dabamd
        slots = [(k, s.bitRate) for k, s in enumerate(subs) if s.flags & dabamd.SUBCH_PACKET]
        old = {(s, self.slots[j][0]): a for (s, j), a in self.asm.items()} if self.asm else {}
        self.slots = slots
        self.asm = {(s, j): old[(s, k)] for s in range(self.S) for j, (k, _) in enumerate(slots) if k in keep and (s, k) in old}

    def run(self, craft=None):
        pipe, F = self.pipe, self.F
        fic, crc, msc, valid = pipe.run(self.diq, self.stride, self.lens, partial=True)
        ev = pipe.msc_entry_valid()
        if craft is not None:
            msc = craft(self, msc, ev)

        def others():
            o = []
            if pipe.max_mp2 and self.audio:
                o.append(pipe.mp2())
            if pipe.max_dabplus and self.audio:
                o.append(pipe.dabplus())
            return o
        if not self.first:
            self.other.append(others())
        byts, groups, run, info = pipe.packet()
        if self.first:
            self.other.append(others())
        # the layer only reads the run's MSC bits
        assert np.array_equal(pipe.msc_d.download(np.uint8, msc.shape), msc)
        self.out.append((byts, groups, run, info))
        for s in range(self.S):
            for j in range(pipe.max_packet):
                if j >= len(self.slots):
                    assert (info[s, :, j]["status"] == -1).all() and run[s, j]["n_groups"] == 0
                    continue
                k, br = self.slots[j]
                a = self.asm.setdefault((s, j), pp.Assembler(br, pipe.max_group_bytes))
                a.begin_run()
                want = np.zeros(4 * F, pp.INFO_DTYPE)
                for q in range(4 * F):
                    if ev[s, q, k]:
                        row = msc[s, q, k, :3 * br] if self.packed else np.packbits(msc[s, q, k, :24 * br])
                        want[q] = a.cif(q, row)
                        self.rows.append(((s, j), bytes(row)))
                        self.fed[(s, j)] = self.fed.get((s, j), 0) + 1
                    else:
                        want[q] = a.skip()
                assert np.array_equal(info[s, :, j], want), (s, j, info[s, :, j][info[s, :, j] != want], want[info[s, :, j] != want])
                assert run[s, j].tolist() == a.run_record(), (s, j, run[s, j], a.run_record())
                n = len(a.groups)
                got, exp = groups[s, j, :n], a.group_records()
                assert np.array_equal(got, exp), (s, j, got[got != exp][:3], exp[got != exp][:3])
                assert bytes(byts[s, j, :len(a.arena)]) == bytes(a.arena), (s, j)
        return msc, ev

    def close(self):
        self.pipe.close()
        self.diq.free()


def test_pipeline_transmitter_content(ctx, tx_iq):
    """3 runs of 6 frames, one bit per byte, the layer called before the audio layers: info,
    run and group records and the arena equal the restatement.  Again with DABGPU_PACK_MSC and
    the layer called last: the same output, and the same layer II and DAB+ output beside it.
    Every group has good packet CRCs (the transmitter's), several span a run boundary.  The
    transmitter's groups are 20..319 bytes: >= 20 of them fit the 56 fed CIFs of the 32 and
    128 kbit/s entries; the 8 kbit/s entry carries 19 bytes per CIF, 1064 in all, which holds
    3 groups of the largest size and not 20 of any, so >= 3 is asked of it here and its 20
    groups in test_pipeline_long_transmitter_signal, on a signal long enough to carry them."""
    res = []
    for packed, first in ((False, True), (True, False)):
        L = Layer(ctx, tx_iq, _subs(TX), packed=packed, first=first)
        try:
            for _ in range(3):
                L.run()
            res.append((L.out, L.other, L.asm))
        finally:
            L.close()
    (oa, xa, asm), (ob, xb, _) = res
    for r in range(3):
        ia, ib = oa[r][3], ob[r][3]
        assert np.array_equal(ia, ib) and np.array_equal(oa[r][2], ob[r][2])
        assert not ia["crc_errors"].any() and (ia["quality"] == -1).all()
        for s in range(2):
            for j in range(3):
                n, nb = oa[r][2][s, j]["n_groups"], oa[r][2][s, j]["n_bytes"]
                assert np.array_equal(oa[r][1][s, j, :n], ob[r][1][s, j, :n])
                assert np.array_equal(oa[r][0][s, j, :nb], ob[r][0][s, j, :nb])
        (pa, ma), (pb, mb) = xa[r][0], xb[r][0]
        assert np.array_equal(ma, mb) and np.array_equal(pa[ma["status"] == 2], pb[mb["status"] == 2])
        (da, sa), (db, sb) = xa[r][1], xb[r][1]
        ok = da["status"] == 3
        assert np.array_equal(da, db) and np.array_equal(sa[ok], sb[ok])
    assert (xa[2][0][1]["status"] == 2).any() and (xa[2][1][0]["status"] == 3).any()
    spans = 0
    print("groups per (stream, slot):", {key: len(a.delivered) for key, a in asm.items()})
    for (s, j), a in asm.items():
        assert len(a.delivered) >= (3 if j == 0 else 20), (s, j, len(a.delivered))
        assert all(g["flags"] & pp.TRUNCATED == 0 for g in a.groups)
    for r in range(2):
        spans += int(np.count_nonzero(oa[r][2]["pending_bytes"] > 0))
    print("series in flight at a run's end:", spans)
    assert spans >= 3


def test_pipeline_long_transmitter_signal(ctx, long_iq):
    """10 runs of 6 frames of one stream, 224 fed CIFs per entry: records, bytes and info equal
    the restatement run by run (Layer.run); every entry, the 8 kbit/s one included, completes
    >= 20 groups, and the 128 kbit/s entry's 500-packet window emits at least twice"""
    L = Layer(ctx, long_iq, _subs(TX), audio=False)
    try:
        for _ in range(10):
            L.run()
        n = {j: len(L.asm[(0, j)].delivered) for j in range(3)}
        q = [len(L.asm[(0, j)].qualities) for j in range(3)]
        print("long signal: groups per entry", n, "quality emissions per entry", q)
        assert min(n.values()) >= 20 and q[2] >= 2
        info = np.concatenate([o[3] for o in L.out], axis=1)[0, :, 2]
        assert info["quality"][info["quality"] >= 0].tolist() == L.asm[(0, 2)].qualities
    finally:
        L.close()


def _feeder(plan):
    """craft(): overwrite the valid rows of the planned (stream, table entry) with the plan's
    rows, CIF by CIF across the runs (zeros when the plan is exhausted)"""
    pos = {key: 0 for key in plan}

    def craft(L, msc, ev):
        for (s, k), (br, rows) in plan.items():
            for q in range(4 * L.F):
                if not ev[s, q, k]:
                    continue
                row = rows[pos[(s, k)]] if pos[(s, k)] < len(rows) else np.zeros(3 * br, np.uint8)
                pos[(s, k)] += 1
                piece = np.ascontiguousarray(row if L.packed else np.unpackbits(row))
                msc[s, q, k, :len(piece)] = piece
                L.pipe.msc_d.upload_at(piece, (((s * 4 * L.F + q) * L.pipe.max_subch) + k) * msc.shape[-1])   # (the row stride of the format)
        return msc
    return craft, pos


SEP = pp.rows([pp.packet(0, 1, 77, b"")], 128)[0]       # ends a series in flight: the next fixture starts in state 0


def _chain(fxs, br):
    """fixtures of one bit rate in a row, a separator CIF behind each -> rows, [(name, first, n)]"""
    out, marks = [], []
    for f in fxs:
        assert f["bitrate"] == br
        marks.append((f["name"], len(out), len(f["rows"])))
        out += list(f["rows"]) + [SEP[:3 * br]]
    return out, marks


def test_pipeline_crafted_rows(ctx, tx_iq, kat):  # noqa: F811
    """the golden fixtures and the cases the reference cannot run, written over the entries'
    valid rows CIF by CIF across three runs: everything equals the restatement (Layer.run), the
    delivered groups equal the golden file's fixture by fixture, the 128 kbit/s entry of
    stream 0 sees >= 500 packets and emits a quality value, msc_bits_d is left as written"""
    fx = {f["name"]: f for f in pp.fixtures() + pp.extra_fixtures()}
    gold = {f["name"]: f for f in kat}
    plan, marks = {}, {}
    for key, br, names in (((0, 0), 8, ["lengths8"]), ((0, 1), 32, ["sequence", "overrun", "lengths32", "clip", "short"]),
                           ((0, 2), 128, ["window"]), ((1, 2), 128, ["headers", "useful", "big"])):
        rows, marks[key] = _chain([fx[n] for n in names], br)
        plan[key] = (br, rows)
    craft, pos = _feeder(plan)
    L = Layer(ctx, tx_iq, _subs(TX))
    try:
        for _ in range(3):
            L.run(craft)
        for key, (br, rows) in plan.items():
            assert pos[key] >= min(len(rows), 56) and (key == (0, 2) or pos[key] >= len(rows)), (key, pos[key], len(rows))
        info = np.concatenate([o[3] for o in L.out], axis=1)
        w = info[0, :, 2]
        print("128 kbit/s entry:", int(w["packets"].sum()), "packets,", int(w["crc_errors"].sum()), "CRC errors, quality",
              w["quality"][w["quality"] >= 0].tolist(), "; groups per entry", {k: len(a.delivered) for k, a in L.asm.items()})
        assert w["packets"].sum() >= 500 and (w["quality"] >= 0).any()
        assert w["quality"][w["quality"] >= 0][0] == gold["window"]["qualities"][0]
        # fixture by fixture: the groups delivered while its rows were fed are the golden file's
        for key, ms in marks.items():
            a = pp.Assembler(plan[key][0])
            fed = [r for k2, r in L.rows if k2 == key]
            for name, first, n in ms:
                if name not in gold or first + n > len(fed):
                    continue
                n0 = len(a.delivered)
                for q in range(first, first + n + 1):
                    if q < len(fed):
                        a.cif(0, np.frombuffer(fed[q], np.uint8))
                got = a.delivered[n0:]
                want = gold[name]["groups"]
                assert got[:len(want)] == want and len(got) - len(want) <= 1, (key, name, len(got), len(want))
        rec = np.concatenate([o[1][1, 2, :o[2][1, 2]["n_groups"]] for o in L.out])
        assert ((rec["nbytes"] > 4095) & ((rec["flags"] & pp.ACCEPTED) != 0)).any()       # rule 2: no int16 wrap
    finally:
        L.close()


SMALL = [(0, 6, 8, 0o103, 0, 8), (6, 12, 16, 0o103, 0, 8)]


def test_pipeline_smallest_rows_both_formats(ctx):
    """the smallest rows the shared row reader and delivery rule see: one stream, runs of one frame,
    a packet-mode entry at 8 kbit/s (one 24-byte cell per CIF) and one at 16 kbit/s, crafted rows
    (the golden lengths8 fixture; groups with a CRC cut into 24- and 48-byte packets, one of them
    with a bad group CRC), six runs: the four of the 16-CIF warm-up, where nothing is fed, and two
    behind it.  Once one bit per byte and once packed: info, run and group records and the bytes
    are equal between the formats and equal the restatement's (Layer.run)."""
    from dabamd.synth import Ensemble, PACKET
    e = Ensemble(7, subch=[(0, 6, 8, 0o103, 0, 0, PACKET), (6, 12, 16, 0o103, 0, 0, PACKET)], figs=True)
    iq = [e.generate(414, truth=False)["iq"]]
    rows8 = [f for f in pp.fixtures() if f["name"] == "lengths8"][0]["rows"]
    rng = np.random.default_rng(16)
    pk = []
    for n, good in ((40, True), (30, False), (21, True)):
        pk += pp.packetize(pp.group(pp._bytes(rng, n), crcf=1, seg=1, segno=n, good=good), 77, [0, 1])
    rows16 = pp.rows(pk, 16)
    assert len(rows16) <= 8 <= len(rows8)
    res = []
    for packed in (False, True):
        craft, pos = _feeder({(0, 0): (8, list(rows8)), (0, 1): (16, list(rows16))})
        L = Layer(ctx, iq, _subs(SMALL), packed=packed, frames=1, audio=False)
        try:
            for _ in range(6):
                L.run(craft)
            assert pos == {(0, 0): 8, (0, 1): 8} and L.fed == {(0, 0): 8, (0, 1): 8}
            res.append((L.out, L.asm))
        finally:
            L.close()
    (oa, asm), (ob, _) = res
    for r in range(6):
        assert np.array_equal(oa[r][3], ob[r][3]) and np.array_equal(oa[r][2], ob[r][2])
        assert (oa[r][3][0, :, :2]["status"] == (-1 if r < 4 else 0)).all(), (r, oa[r][3][0, :, :2]["status"])
        for j in range(2):
            n, nb = oa[r][2][0, j]["n_groups"], oa[r][2][0, j]["n_bytes"]
            assert np.array_equal(oa[r][1][0, j, :n], ob[r][1][0, j, :n])
            assert np.array_equal(oa[r][0][0, j, :nb], ob[r][0][0, j, :nb])
    rec = {j: np.concatenate([o[1][0, j, :o[2][0, j]["n_groups"]] for o in oa]) for j in range(2)}
    print("smallest rows: groups per entry", {j: len(rec[j]) for j in rec})
    assert len(rec[0]) == 2                                 # lengths8's packets 0 and 4: the 24-byte ones
    assert ((rec[1]["flags"] & pp.ACCEPTED) != 0).tolist() == [True, False, True]     # by the group CRC


def test_pipeline_cap(ctx, tx_iq):
    """groups above a 256-byte cap set through packet_caps: truncated, reported in full, not
    accepted; the groups around them whole; a series in flight across runs under the cap"""
    f = [x for x in pp.extra_fixtures() if x["name"] == "cap"][0]
    craft, pos = _feeder({(0, 2): (128, list(f["rows"]) * 12)})
    L = Layer(ctx, tx_iq[:1], _subs(TX), max_group_bytes=256)
    try:
        assert L.pipe.max_group_bytes == 256
        for _ in range(3):
            L.run(craft)
        rec = np.concatenate([o[1][0, 2, :o[2][0, 2]["n_groups"]] for o in L.out])
        assert np.count_nonzero(rec["flags"] & pp.TRUNCATED) >= 5 and np.count_nonzero(rec["flags"] & pp.ACCEPTED) >= 10
        assert (rec["nbytes"][(rec["flags"] & pp.TRUNCATED) != 0] > 256).all()
    finally:
        L.close()


def test_pipeline_tables_and_caps(ctx, tx_iq):
    """set_subch with the packet entries unchanged: no gap and the series in flight completes;
    with an entry's bitRate changed: -1 until since + 16, then a new mscDatagroup (address -1
    again); the refusals; packet_caps raising the capacity keeps the assemblers"""
    import dabamd
    L = Layer(ctx, tx_iq[:1], _subs(TX), max_subch=5, max_bitrate=128, max_dabplus=1, max_mp2=1, max_packet=3)
    try:
        L.run()
        assert (L.out[-1][2][0]["state"] == 1).any() and (L.out[-1][2][0]["pending_bytes"] > 0).any()
        L.pipe.set_subch(0, _subs(TX[:4]))                     # the DAB+ entry goes, the packet entries stay
        L.table(_subs(TX[:4]), keep=(0, 1, 2))
        _, ev = L.run()
        assert ev[0, :, :3].all() and (L.out[-1][3][0]["status"] == 0).all()     # no gap
        assert (L.out[-1][3][0, -1]["address"] >= 0).all()
        L.pipe.packet_caps(4)                                  # more slots: the assemblers go on
        since = L.pipe.state(0).cif_count
        changed = [TX[0], (6, 36, 48, 0o103, 0, 8)] + TX[2:4]
        L.pipe.set_subch(0, _subs(changed))
        L.table(_subs(changed), keep=(0, 2))
        _, ev = L.run()
        i1 = L.out[-1][3][0, :, 1]
        assert (i1["status"][:16] == -1).all() and (i1["status"][16:] == 0).all() and L.pipe.get_subch(0)[1][1] == since
        assert (i1["address"][:16] == -1).all()
        assert (L.out[-1][3][0, :, 0]["status"] == 0).all() and (L.out[-1][3][0, :, 3]["status"] == -1).all()
        for bad, code in (([TX[0], TX[1], TX[2], (144, 6, 8, 0o103, 0, 8), (150, 6, 8, 0o103, 0, 8)], E_ARG),   # five flagged, four slots
                          ([(0, 6, 8, 0o103, 0, 12)], E_ARG),                  # packet mode and layer II
                          ([(0, 6, 8, 0o103, 0, 9)], E_ARG),                   # packet mode and DAB+
                          ([(0, 96, 12, 0o103, 0, 8)], E_UNSUP),               # no multiple of 8
                          ([(0, 192, 256, 0o103, 0, 8)], E_UNSUP)):            # above max_bitrate
            with pytest.raises(dabamd.DabError) as e:
                L.pipe.set_subch(0, _subs(bad))
            assert e.value.code == code, bad
        for args in ((-1, 0), (2, -1), (6, 0), (2, 0)):        # negative, above max_subch, below the table's three
            with pytest.raises(dabamd.DabError) as e:
                L.pipe.packet_caps(*args)
            assert e.value.code == E_ARG, args
        with pytest.raises(dabamd.DabError) as e:
            L.pipe.packet()                                     # the run was consumed
        assert e.value.code == E_STATE
    finally:
        L.close()
    with pytest.raises(dabamd.DabError) as e:
        dabamd.Pipeline(ctx, 1, F, _subs([(0, 6, 8, 0o103, 0, 12)]))
    assert e.value.code == E_ARG
    p = dabamd.Pipeline(ctx, 1, F, _subs([TX[4]]))              # no packet entry: no layer
    try:
        with pytest.raises(dabamd.DabError) as e:
            p.packet()
        assert e.value.code == E_STATE
    finally:
        p.close()


def test_pipeline_kept_entries_change_slot(ctx, tx_iq):
    """set_subch that takes the first packet entry's flags away and leaves the other two as they
    are: those keep their assemblers though their slots move from 1 and 2 down to 0 and 1 -- the
    series in flight completes (Layer.run's comparison against the carried Assemblers) and no
    CIF of the next run is missing (status 0 throughout); the slot left over is empty"""
    L = Layer(ctx, tx_iq[:1], _subs(TX))
    try:
        L.run()
        run = L.out[-1][2][0]
        print("before the change: state", run["state"].tolist(), "pending_bytes", run["pending_bytes"].tolist())
        assert (run["state"][1:3] == 1).any() and (run["pending_bytes"][1:3] > 0).any()   # a kept entry has a series in flight
        moved = [TX[0][:5] + (0,)] + TX[1:4]
        L.pipe.set_subch(0, _subs(moved))
        L.table(_subs(moved), keep=(1, 2))
        assert [k for k, _ in L.slots] == [1, 2] and sorted(L.asm) == [(0, 0), (0, 1)]
        _, ev = L.run()
        info = L.out[-1][3][0]
        assert ev[0, :, 1:3].all() and (info[:, :2]["status"] == 0).all()     # no gap
        assert (info[:, 2]["status"] == -1).all()
    finally:
        L.close()


def test_dropin_on_datagroup(ctx, long_iq, tmp_path):
    """ensembleDecoder::on_datagroup / on_packet_quality (a C++ program over the drop-in
    library, auto_layout on the transmitter's FIGs, 10 steps of 6 frames): the table it parses
    flags the three packet-mode entries, and from the step it applies it on its calls equal
    the Python layer's records, bytes and quality fields under the same schedule.  The signal
    is long enough for the 128 kbit/s entry to cross 500 handled packets after the table is
    applied, so on_packet_quality is called"""
    subprocess.run(["make", "-s", "-f", os.path.join(ROOT, "tests", "cpp", "Makefile.packet")], check=True)
    long_iq[0].tofile(tmp_path / "iq.f32")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "build", "test_packet_dropin"), str(tmp_path / "iq.f32"),
                        str(tmp_path / "dg.bin"), str(F), "10"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PACKET DROPIN OK" in r.stdout, r.stdout + r.stderr
    raw = (tmp_path / "dg.bin").read_bytes()
    hdr = np.dtype([("kind", "<i4"), ("subch", "<i4"), ("cif", "<i8"), ("value", "<i4"), ("nbytes", "<i4")])
    got, quality, applied, p = [], [], None, 0
    while p < len(raw):
        h = np.frombuffer(raw, hdr, 1, p)[0]
        p += hdr.itemsize
        if h["kind"] == 0:                                      # a group: its record, then its bytes
            rec = np.frombuffer(raw, pp.GROUP_DTYPE, 1, p)[0]
            p += pp.GROUP_DTYPE.itemsize
            got.append((int(h["cif"]), int(h["subch"]), rec, raw[p:p + int(h["nbytes"])]))
            p += int(h["nbytes"])
        elif h["kind"] == 1:
            quality.append((int(h["cif"]), int(h["subch"]), int(h["value"])))
        else:                                                   # the table was applied at the end of step `value`:
            applied = int(h["value"])                           # n entries follow, 6 int16 each
            table = np.frombuffer(raw, "<i2", 6 * int(h["nbytes"]), p).reshape(-1, 6)
            p += 12 * int(h["nbytes"])
    assert applied is not None and applied <= 2
    want_table = [(a, n, br, pl, 0 if uep else 1, fl if fl != 4 else 0) for a, n, br, pl, uep, fl in TX]   # no on_pcm: layer II unflagged
    assert table.tolist() == [list(t) for t in want_table]
    import dabamd
    subs = [dabamd.Subch(*t) for t in want_table]
    L = Layer(ctx, long_iq, [], audio=False, max_subch=5, max_bitrate=128, max_dabplus=1, max_packet=3)
    try:
        want, wq = [], []
        for step in range(10):
            L.run()
            for j, (k, br) in enumerate(L.slots):
                want += [(4 * F * step + g["cif"], k, g) for g in L.asm[(0, j)].groups]
                wq += [(4 * F * step + q, k, int(v)) for q, v in enumerate(L.out[-1][3][0, :, j]["quality"]) if v >= 0]
            if step == applied:
                L.pipe.set_subch(0, subs)
                L.table(subs)
        print("drop-in:", len(got), "groups,", len(quality), "quality values, table applied after step", applied)
        assert len(want) == len(got) >= 30 and wq == quality and len(quality) >= 1
        for (c, k, g), (gc, gk, rec, byts) in zip(want, got):
            assert (c, k) == (gc, gk) and byts == g["stored"], (c, k, gc, gk)
            assert all(rec[f] == g[f] for f in pp.GROUP_DTYPE.names if f not in ("reserved", "cif", "offset")), (c, k)
    finally:
        L.close()
