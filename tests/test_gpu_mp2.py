"""MPEG layer II on the GPU (k_mp2.hip): the batched operator dabgpu_mp2_decode and the
pipeline layer dabgpu_pipe_mp2, bit-exact against the reference's own decoder (the golden
file tests/golden/mp2_kat.npz) and against its numpy restatement (mp2_py, itself pinned to
that file by test_mp2_cpu) with the frame synchroniser restatement oracle_py.MP2.

The pipeline tests take the expected PCM from the MSC bits the pipeline itself delivered for
the entry (at 300 dB SNR those are the transmitter's; the MSC decoding has its own tests):
the layer is checked as the function of its input that mp2Processor is."""
import numpy as np
import pytest

import mp2_py
import oracle_py as orc
from test_mp2_cpu import kat, sync_frames  # noqa: F401  (kat: the golden file as a fixture)

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -6
STRIDE = 1152                # the longest golden frame (384 kbit/s); shorter ones zero-padded


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


def _rows(chains, stride):
    """chains of frames (bytes) -> [n_chains * chain_len][stride], short chains padded with
    all-zero frames (rejected: ret 0), short frames with zeros"""
    n = max(len(c) for c in chains)
    out = np.zeros((len(chains), n, stride), np.uint8)
    for i, c in enumerate(chains):
        for j, f in enumerate(c):
            out[i, j, :min(len(f), stride)] = np.frombuffer(f, np.uint8)[:stride]
    return out.reshape(-1, stride), n


def test_operator_equals_reference(ctx, kat):  # noqa: F811
    """every golden stream as a chain: PCM equals what the reference's sink received, ret is
    the frame size (0 for the rejected headers); cut in two calls with the state carried the
    PCM is the same, with a zero state after the cut it is not"""
    chains = [[f for f, _ in sync_frames(s["bits"], s["bitrate"])] for s in kat]
    rows, n = _rows(chains, STRIDE)
    pcm, ret, _ = ctx.mp2_decode(rows, n)
    for i, s in enumerate(kat):
        want_ret = mp2_py.decode_chain(chains[i])[0]
        assert np.array_equal(ret[i, :len(chains[i])], want_ret) and not ret[i, len(chains[i]):].any(), s["name"]
        dec = np.flatnonzero(ret[i])
        assert len(dec) == len(s["pcm"]), s["name"]
        assert np.array_equal(pcm[i, dec], s["pcm"]), s["name"]
        assert not pcm[i, ret[i] == 0].any()                       # rows of rejected frames untouched
    cut = 5
    r3 = rows.reshape(len(chains), n, STRIDE)
    a, ra, st = ctx.mp2_decode(r3[:, :cut].reshape(-1, STRIDE), cut)
    b, rb, _ = ctx.mp2_decode(r3[:, cut:].reshape(-1, STRIDE), n - cut, state=st)
    assert np.array_equal(np.concatenate([a, b], axis=1), pcm) and np.array_equal(np.concatenate([ra, rb], axis=1), ret)
    z, _, _ = ctx.mp2_decode(r3[:, cut:].reshape(-1, STRIDE), n - cut)
    for i, s in enumerate(kat):
        if ret[i, :cut].any() and ret[i, cut:].any():
            assert not np.array_equal(z[i], b[i]), s["name"]       # the state is used
    assert any(ret[i, :cut].any() and ret[i, cut:].any() for i in range(len(kat)))


@pytest.fixture(scope="module")
def random_chains():
    """16 chains x 3 seeded random well-formed frames over modes, bit rates and both
    MPEG versions, all scale factors allowed"""
    rng = np.random.default_rng(77)
    S, J, D, M = mp2_py.STEREO, mp2_py.JOINT, mp2_py.DUAL, mp2_py.MONO
    kinds = [(0, 128, S, 0), (0, 192, J, 1), (0, 64, M, 0), (0, 32, M, 0), (0, 48, M, 0), (0, 160, D, 0),
             (0, 384, S, 0), (0, 96, J, 3), (1, 64, S, 0), (1, 160, J, 0), (1, 8, M, 0), (1, 32, D, 0),
             (0, 56, M, 0), (0, 112, J, 2), (0, 256, S, 0), (0, 80, M, 0)]
    chains = []
    for lsf, kbps, mode, ext in kinds:
        nbytes = 144000 * kbps // (24000 if lsf else 48000)
        want = {r: set(range(16)) for r in range(6)}
        chains.append([mp2_py.write_frame(mp2_py.make_spec(rng, lsf, mp2_py.BITRATES[lsf].index(kbps) + 1, 1, mode, ext,
                                                           bool(rng.integers(2)), nbytes, want, sf_range=(0, 62)), nbytes)
                       for _ in range(3)])
    return chains


def _against_restatement(ctx, chains, stride):
    rows, n = _rows(chains, stride)
    pcm, ret, state = ctx.mp2_decode(rows, n)
    r3 = rows.reshape(len(chains), n, stride)
    for i in range(len(chains)):
        wr, wp, ws = mp2_py.decode_chain([r3[i, j].tobytes() for j in range(n)])
        assert np.array_equal(ret[i], wr), i
        assert np.array_equal(pcm[i], wp), i
        assert np.array_equal(state[i].view(np.int16), ws.reshape(-1)), i
    return ret


def test_operator_equals_restatement(ctx, random_chains):
    """random well-formed frames; the same frames cut short so their fields run past
    frame_stride (rule 2: zeros); the synthetic transmitter's layer II frames (a valid
    header, random payload: the fields it implies run far past the frame); a header for
    every bit rate and sampling frequency of both MPEG versions in one chain of 128 frames
    (ret, the frame size, for all of them).  Rule 1 is the golden stream wrap384's."""
    ret = _against_restatement(ctx, random_chains, 1152)
    assert ret.all()
    _against_restatement(ctx, random_chains, 100)
    from dabamd.synth import Ensemble, MP2
    msc = Ensemble(2, subch=[(0, 96, 128, 3, 1, 0, MP2), (96, 48, 64, 0o103, 0, 0, MP2)]).generate(5)["msc"]
    tx = [[np.packbits(msc[c, k, :24 * br]).tobytes() for c in range(6)] for k, br in ((0, 128), (1, 64))]
    assert _against_restatement(ctx, tx, 384).all()
    hdr = []
    for lsf in (0, 1):
        for bri in range(16):
            for fs in range(4):
                hdr.append(bytes([0xFF, 0xF5 if lsf else 0xFD, bri << 4 | fs << 2 | (bri & 2), 0xC0 if bri % 3 == 0 else 0x40]))
    ret = _against_restatement(ctx, [hdr], 8)
    assert np.count_nonzero(ret) == 2 * 14 * 3


# ---- the pipeline layer ----------------------------------------------------------------
F = 6


def _expected(msc, ev, s, k, br, packed, proc=None):
    """mp2Processor over the rows of entry k of stream s that are valid, in order ->
    {CIF slot: (frame, rate)}; proc (an oracle_py.MP2) carries over from earlier runs"""
    proc = proc or orc.MP2(br)
    out = {}
    for q in range(msc.shape[1]):
        if not ev[s, q, k]:
            continue
        row = msc[s, q, k]
        bits = np.unpackbits(row)[:24 * br] if packed else row[:24 * br]
        n0 = len(proc.frames)
        proc.add([int(x) for x in bits])
        assert len(proc.frames) - n0 <= 1
        if len(proc.frames) > n0:
            out[q] = proc.frames[-1]
    return out, proc


class Layer:
    """a pipeline with layer II entries, run by run: the layer's records and PCM against the
    synchroniser + decoder restatements fed with the entry's own delivered rows"""

    def __init__(self, ctx, iqs, subs, packed=False, mp2_first=True, check=True, **caps):
        import dabamd
        self.ctx, self.S = ctx, len(iqs)
        self.lens = [len(x) // 2 for x in iqs]
        self.stride = max(self.lens)
        buf = np.zeros((self.S, 2 * self.stride), np.float32)
        for s, x in enumerate(iqs):
            buf[s, :len(x)] = x
        self.diq = ctx.put(buf)
        self.pipe = dabamd.Pipeline(ctx, self.S, F, subs, **caps)
        self.pipe.control(dabamd.CTL_ACQ_SYNC)
        self.packed, self.mp2_first, self.check = packed, mp2_first, check
        if packed:
            self.pipe.set_packed(True)
        self.table(subs)
        self.dp, self.pcm, self.info, self.n2 = [], [], [], 0

    def table(self, subs, keep=()):
        """the MP2 slots of `subs`; slots in `keep` go on with their processors"""
        import dabamd
        old = getattr(self, "procs", {})
        self.slots = [(k, s.bitRate) for k, s in enumerate(subs) if s.flags & dabamd.SUBCH_MP2]
        self.procs = {key: v for key, v in old.items() if key[1] in keep}

    def run(self, craft=None):
        pipe = self.pipe
        fic, crc, msc, valid = pipe.run(self.diq, self.stride, self.lens, partial=True)
        ev = pipe.msc_entry_valid()
        if craft is not None:
            msc = craft(self, msc, ev)
        if not self.mp2_first and pipe.max_dabplus:
            self.dp.append(pipe.dabplus())
        pcm, info = pipe.mp2()
        if self.mp2_first and pipe.max_dabplus:
            self.dp.append(pipe.dabplus())
        self.pcm.append(pcm)
        self.info.append(info)
        self.msc = getattr(self, "msc", []) + [np.unpackbits(msc, axis=-1) if self.packed else msc]
        for s in range(self.S if self.check else 0):
            for j in range(pipe.max_mp2):
                if j >= len(self.slots):
                    assert (info[s, :, j]["status"] == -1).all()
                    continue
                k, br = self.slots[j]
                assert np.array_equal(info[s, :, j]["status"] == -1, ev[s, :, k] == 0), (s, j)
                proc, dec = self.procs.get((s, j), (None, None))
                exp, proc = _expected(msc, ev, s, k, br, self.packed, proc)
                dec = dec or mp2_py.Decoder()
                self.procs[(s, j)] = (proc, dec)
                for q in range(4 * F):
                    rec = info[s, q, j]
                    if not ev[s, q, k]:
                        continue
                    if q not in exp:
                        assert rec["status"] == 0, (s, q, j, rec)
                        continue
                    frame, rate = exp[q]
                    ret, want = dec.decode(frame)
                    assert rec["status"] == (2 if ret else 1) and rec["sample_rate"] == rate, (s, q, j, rec, ret, rate)
                    if ret:
                        assert rec["frame_bytes"] == ret
                        assert np.array_equal(pcm[s, q, j], want), (s, q, j)
                        self.n2 += 1
        return msc, ev

    def close(self):
        self.pipe.close()
        self.diq.free()


def _subs(table):
    import dabamd
    return [dabamd.Subch(a, n, br, pl, 0 if uep else 1, fl) for a, n, br, pl, uep, fl in table]


@pytest.fixture(scope="module")
def tx_iq():
    """two streams of one ensemble layout, 19 frames: a 128 kbit/s UEP-3 and a 64 kbit/s
    EEP-3A subchannel carrying layer II frames, and a DAB+ one"""
    from dabamd.synth import Ensemble, MP2
    e = Ensemble(3 * F + 1, subch=[(0, 96, 128, 3, 1, 0, MP2), (96, 48, 64, 0o103, 0, 0, MP2), (144, 24, 32, 0o103, 0, 1, 0)])
    return [e.generate(s, truth=False)["iq"] for s in (301, 302)]


TX = [(0, 96, 128, 3, 1, 4), (96, 48, 64, 0o103, 0, 4), (144, 24, 32, 0o103, 0, 1)]


def test_pipeline_transmitter_content(ctx, tx_iq):
    """3 runs of 6 frames with one bit per byte and the layer called before the DAB+ layer:
    records and PCM equal the restatements.  Again with DABGPU_PACK_MSC and the DAB+ layer
    called first: the same MSC bits, so the same records and PCM must come out, and the
    DAB+ layer gives the same superframes in either order"""
    res = []
    for packed, first in ((False, True), (True, False)):
        L = Layer(ctx, tx_iq, _subs(TX), packed=packed, mp2_first=first, check=not packed)
        try:
            for _ in range(3):
                L.run()
            if L.check:
                assert L.n2 >= 2 * 2 * 50                              # 56 valid CIFs per entry, a frame in nearly each
            res.append((np.concatenate(L.pcm, axis=1), np.concatenate(L.info, axis=1),
                        [np.concatenate([d[i] for d in L.dp], axis=1) for i in (0, 1)], np.concatenate(L.msc, axis=1)))
        finally:
            L.close()
    (pa, ia, da, ma), (pb, ib, db, mb) = res
    for k, br in ((0, 128), (1, 64)):
        ok = ia["status"][:, :, k] >= 0
        assert np.array_equal(ma[:, :, k, :24 * br][ok], mb[:, :, k, :24 * br][ok])
    assert np.array_equal(ia, ib)
    assert np.array_equal(pa[ia["status"] == 2], pb[ib["status"] == 2])
    ok = da[0]["status"] == 3
    assert np.array_equal(da[0], db[0]) and ok.any() and np.array_equal(da[1][ok], db[1][ok])


def _sync_stream():
    """the stream of test_consumers_cpu.test_mp2_frame_sync_matches_reference: garbage before
    sync, 48 kHz frames with two 24 kHz ones (twice the length) among them, a 3-bit slip"""
    rng = np.random.default_rng(3)
    br = 64
    stream = list(rng.integers(0, 2, 500))
    for k in range(12):
        mpeg2 = k in (5, 6)
        hdr = bytes([0xFF, 0xF4 if mpeg2 else 0xFC, (0x8 << 4) | (1 << 2)])
        n = 24 * br * (2 if mpeg2 else 1)
        body = hdr + bytes(rng.integers(0, 256, n // 8 - 3, dtype=np.uint8))
        stream += list(np.unpackbits(np.frombuffer(body, np.uint8)))
        if k == 8:
            stream += [0, 1, 0]
    return np.array(stream, np.uint8)


def test_pipeline_synchroniser_cases(ctx, tx_iq):
    """the layer reads the run's msc_bits_d: the 64 kbit/s entry's valid rows are overwritten
    with the crafted stream, CIF by CIF over two runs, so a frame in progress and the search
    state cross the run boundary"""
    bits = _sync_stream()
    pos = [0]

    def craft(L, msc, ev):
        k, br = 1, 64
        for q in range(4 * F):
            if not ev[0, q, k]:
                continue
            piece = np.zeros(24 * br, np.uint8)
            take = bits[pos[0]:pos[0] + 24 * br]
            piece[:len(take)] = take
            pos[0] += 24 * br
            msc[0, q, k, :24 * br] = piece
            off = ((q * L.pipe.max_subch) + k) * L.pipe.msc_stride
            L.pipe.msc_d.upload_at(piece, off)
        return msc

    L = Layer(ctx, tx_iq[:1], _subs(TX))
    try:
        L.run(craft)
        n1 = L.n2
        L.run(craft)
        assert pos[0] >= len(bits)
        info = np.concatenate(L.info, axis=1)[0, :, 1]
        assert np.count_nonzero(info["status"] >= 1) >= 8 and (info["sample_rate"] == 24000).any()
        assert n1 > 0 and L.n2 > n1
    finally:
        L.close()


def test_pipeline_tables(ctx, tx_iq):
    """set_subch with the layer II entry unchanged: no gap; with its bitRate changed: -1
    until since + 16, then a new mp2Processor; caps and flags the table check refuses"""
    import dabamd
    L = Layer(ctx, tx_iq[:1], _subs(TX), max_subch=3, max_bitrate=128, max_dabplus=1, max_mp2=2)
    try:
        L.run()
        L.pipe.set_subch(0, _subs(TX[:2]))                     # the DAB+ entry goes, both layer II entries stay
        L.table(_subs(TX[:2]), keep=(0, 1))
        _, ev = L.run()
        assert ev[0, :, 0].all() and (L.info[-1][0, :, 0]["status"] == 2).all()      # no gap
        since = L.pipe.state(0).cif_count
        changed = [TX[0], (96, 48, 48, 0o103, 0, 4)]
        L.pipe.set_subch(0, _subs(changed))
        L.table(_subs(changed), keep=(0,))
        _, ev = L.run()
        st = L.info[-1][0, :, 1]["status"]
        assert (st[:16] == -1).all() and (st[16:] >= 0).all() and L.pipe.get_subch(0)[1][1] == since
        assert (L.info[-1][0, :, 0]["status"] == 2).all()
        for bad in ([TX[0], TX[1], (144, 24, 32, 0o103, 0, 4)],              # three layer II entries, two slots
                    [(0, 96, 128, 3, 1, 5)]):                              # layer II and DAB+ on one entry
            with pytest.raises(dabamd.DabError) as e:
                L.pipe.set_subch(0, _subs(bad))
            assert e.value.code == E_ARG
    finally:
        L.close()
    with pytest.raises(dabamd.DabError) as e:
        dabamd.Pipeline(ctx, 1, F, _subs([(0, 96, 128, 3, 1, 5)]))
    assert e.value.code == E_ARG
    p = dabamd.Pipeline(ctx, 1, F, _subs([TX[2]]))                         # no layer II entry: max_mp2 = 0
    try:
        with pytest.raises(dabamd.DabError) as e:
            p.mp2()
        assert e.value.code == E_STATE
    finally:
        p.close()


def test_dropin_on_pcm(ctx, tx_iq, tmp_path):
    """ensembleDecoder::on_pcm (a C++ program over the drop-in library) hands over, for one
    stream of the transmitter content test, exactly the frames and samples the pipeline
    layer gives through the Python binding: same CIFs, entries, rates and PCM"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-s", "-f", os.path.join(root, "tests", "cpp", "Makefile.mp2")], check=True)
    L = Layer(ctx, tx_iq[:1], _subs(TX), check=False)
    try:
        for _ in range(3):
            L.run()
    finally:
        L.close()
    pcm, info = np.concatenate(L.pcm, axis=1)[0], np.concatenate(L.info, axis=1)[0]
    want = {(q, j): (int(info[q, j]["sample_rate"]), pcm[q, j]) for q in range(info.shape[0]) for j in range(2)
            if info[q, j]["status"] == 2}
    tx_iq[0].tofile(tmp_path / "iq.f32")
    args = [str(v) for a, n, br, pl, uep, fl in TX for v in (a, n, br, pl, 0 if uep else 1, fl)]
    r = subprocess.run([os.path.join(root, "tests", "cpp", "build", "test_mp2_dropin"), str(tmp_path / "iq.f32"),
                        str(tmp_path / "pcm.bin"), str(F), "3"] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MP2 DROPIN OK" in r.stdout, r.stdout + r.stderr
    rec = np.fromfile(tmp_path / "pcm.bin", np.dtype([("cif", "<i8"), ("subch", "<i4"), ("rate", "<i4"), ("n", "<i4"),
                                                      ("pcm", "<i2", (1152, 2))]))
    assert len(rec) == len(want) >= 100
    for x in rec:
        rate, p = want[(int(x["cif"]), int(x["subch"]))]
        assert x["n"] == 1152 and x["rate"] == rate and np.array_equal(x["pcm"], p), (x["cif"], x["subch"])
