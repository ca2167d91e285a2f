"""The audio output layer in the pipeline (dabgpu_pipe_audio) and the drop-in (ensembleDecoder::
on_audio): what the layer delivers equals sink_py (tests/sink_py.py, pinned to the reference by
test_sink_cpu) applied per slot to the PCM and rates the same runs' layer II layer delivered, bit
for bit, with the sinks carried from run to run and across table changes.

The content is the layer II transmitter content of test_gpu_mp2 (48 kHz frames); the second entry's
delivered rows are overwritten with half-rate (LSF, 24 kHz) frames, which span two CIFs each, as
test_gpu_mp2's synchroniser test overwrites them."""
import os
import subprocess

import numpy as np
import pytest

import mp2_py
import sink_py as sp
from test_sink_cpu import bits
from test_gpu_mp2 import F, _subs

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP2, AUDIO = 4, 128
# (startAddr, length, bitRate, protLevel, uep, flags): a 128 and a 64 kbit/s entry that feed the
# audio output layer and a 32 kbit/s layer II entry that does not
A = [(0, 96, 128, 3, 1, MP2 | AUDIO), (96, 48, 64, 0o103, 0, MP2 | AUDIO), (144, 24, 32, 0o103, 0, MP2)]
# the first entry as it was, the other two swapped: both are new entries (new mp2Processors, a new sink)
B = [A[0], A[2], A[1]]
# the 64 kbit/s entry as it was (its sink, the one whose filter runs, goes on, in audio slot 0 where it had slot 1);
# the other two with other flags, so both are new entries: the first leaves the layer, the third enters it
C = [A[0][:5] + (MP2,), A[1], A[2][:5] + (MP2 | AUDIO,)]


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tx_iq():
    """two streams of one ensemble layout, 19 frames: three subchannels carrying layer II frames"""
    from dabamd.synth import Ensemble, MP2 as CONTENT
    e = Ensemble(3 * F + 1, subch=[(a, n, br, pl, uep, 0, CONTENT) for a, n, br, pl, uep, _ in A])
    return [e.generate(s, truth=False)["iq"] for s in (311, 312)]


def lsf_bits(seed, n_frames):
    """one all-zero CIF (the synchroniser finds nothing in it), then 64 kbit/s LSF frames back to
    back, two CIFs each: every frame straddles a CIF edge, and with an odd number of CIFs before a
    run's end one straddles the run edge"""
    rng = np.random.default_rng(seed)
    out = [np.zeros(24 * 64, np.uint8)]
    for _ in range(n_frames):
        want = {r: set(range(16)) for r in range(6)}
        spec = mp2_py.make_spec(rng, 1, mp2_py.BITRATES[1].index(64) + 1, 1, mp2_py.STEREO, 0, False, 384, want, sf_range=(0, 62))
        out.append(np.unpackbits(np.frombuffer(mp2_py.write_frame(spec, 384), np.uint8)))
    return np.concatenate(out)


class Runs:
    """a two-stream pipeline run by run: the 64 kbit/s entry's rows crafted, mp2() then audio(), and
    the layer's output against one sink_py.Sink per (stream, audio slot)"""

    def __init__(self, ctx, iqs, table):
        import dabamd
        self.S = len(iqs)
        self.lens = [len(x) // 2 for x in iqs]
        self.stride = max(self.lens)
        buf = np.zeros((self.S, 2 * self.stride), np.float32)
        for s, x in enumerate(iqs):
            buf[s, :len(x)] = x
        self.diq = ctx.put(buf)
        self.pipe = dabamd.Pipeline(ctx, self.S, F, _subs(table), max_subch=3, max_bitrate=128, max_dabplus=0, max_mp2=3)
        self.pipe.control(dabamd.CTL_ACQ_SYNC)
        self.sinks, self.records = {}, []
        self.table(table)

    def table(self, table, keep=(), restart=True):
        """the audio slots of `table`; the sinks of the entries in `keep` (index in the table) go on;
        restart: the 64 kbit/s entry is a new one, so its crafted stream begins again"""
        self.tab = table
        self.mp2_slot = {k: j for j, k in enumerate(k for k, e in enumerate(table) if e[5] & MP2)}
        self.audio_entries = [k for k, e in enumerate(table) if e[5] & AUDIO]
        self.sinks = {(s, k): v for (s, k), v in self.sinks.items() if k in keep}
        if restart:
            self.lsf = [lsf_bits(100 * len(self.records) + s, 40) for s in range(self.S)]    # restarts at a frame edge
            self.pos = [0] * self.S

    def craft(self):
        """overwrite the valid rows of the 64 kbit/s entry with the LSF stream"""
        pipe = self.pipe
        ev = pipe.msc_entry_valid()
        k = [i for i, e in enumerate(self.tab) if e[2] == 64][0]
        for s in range(self.S):
            for q in range(4 * F):
                if not ev[s, q, k]:
                    continue
                piece = self.lsf[s][self.pos[s]:self.pos[s] + 24 * 64]
                self.pos[s] += 24 * 64
                assert len(piece) == 24 * 64
                pipe.msc_d.upload_at(piece, (((s * 4 * F + q) * pipe.max_subch) + k) * pipe.msc_stride)

    def run(self, audio=True):
        pipe = self.pipe
        pipe.run(self.diq, self.stride, self.lens, partial=True)
        self.craft()
        pcm, info = pipe.mp2()
        if not audio:
            return None
        samples, n_out = pipe.audio()
        assert samples.shape == (self.S, 4 * F, pipe.max_audio, 2304, 2) and n_out.shape == samples.shape[:3]
        rec = []
        for s in range(self.S):
            for j in range(pipe.max_audio):
                if j >= len(self.audio_entries):
                    assert not n_out[s, :, j].any()
                    continue
                k = self.audio_entries[j]
                m = self.mp2_slot[k]
                sink = self.sinks.setdefault((s, k), sp.Sink())
                for q in range(4 * F):
                    if info[s, q, m]["status"] != 2:
                        assert n_out[s, q, j] == 0, (s, q, j)
                        continue
                    want = sink.audio_out(pcm[s, q, m], int(info[s, q, m]["sample_rate"]))
                    assert n_out[s, q, j] == len(want), (s, q, j)
                    assert np.array_equal(bits(samples[s, q, j, :len(want)]), bits(want)), (s, q, j)
                    rec.append((s, q, k, int(info[s, q, m]["sample_rate"]), samples[s, q, j, :len(want)].copy()))
        self.records.append(rec)
        return pcm, info, samples, n_out

    def close(self):
        self.pipe.close()
        self.diq.free()


def test_pipeline_equals_restatement(ctx, tx_iq):
    """three consecutive runs with the sinks carried, a half-rate frame straddling a run edge; then a
    table that keeps the first entry (its sink continues) and moves the second (a new sink: its
    first outputs equal a fresh restatement's); the layer II entry that is not flagged gives nothing"""
    import dabamd
    R = Runs(ctx, tx_iq, A)
    try:
        assert R.pipe.max_audio == 2 and R.pipe.max_mp2 == 3
        for r in range(3):
            pcm, info, samples, n_out = R.run()
            # the unflagged entry decodes (the layer II layer delivers it) and reaches no audio slot
            assert (info[:, :, 2]["status"] == 2).any() and n_out.shape[2] == 2
            if r:
                # an LSF frame that began in the run before completes in this run's first CIF
                assert (n_out[:, 0, 1] == 2304).all() and (n_out[:, 0, 0] == 1152).all()
        rates = {(k, rate) for rec in R.records for _, _, k, rate, _ in rec}
        assert rates == {(0, 48000), (1, 24000)}
        assert sum(len(rec) for rec in R.records) >= 2 * (50 + 20)
        # a second call for the run, and a call without an mp2 call for the run
        with pytest.raises(dabamd.DabError) as e:
            R.pipe.audio()
        assert e.value.code == E_STATE
        R.pipe.set_subch(-1, _subs(B))
        R.table(B, keep=(0,))
        R.pipe.run(R.diq, R.stride, R.lens, partial=True)
        with pytest.raises(dabamd.DabError) as e:
            R.pipe.audio()
        assert e.value.code == E_STATE
    finally:
        R.close()


def test_table_change_renews_the_sink_of_a_moved_entry(ctx, tx_iq):
    """the 24 kHz entry moves to another index: a new mp2Processor and a new sink, whose first outputs
    equal a fresh restatement's (Runs.run) and differ from what the old history would give"""
    R = Runs(ctx, tx_iq, A)
    try:
        R.run()
        R.run()
        before = {key: v.hist.copy() for key, v in R.sinks.items()}
        assert all(before[(s, 1)][1].any() for s in range(R.S))            # the 24000 filter has history
        R.pipe.set_subch(-1, _subs(B))
        R.table(B, keep=(0,))
        assert set(R.sinks) == {(0, 0), (1, 0)}
        pcm, info, samples, n_out = R.run()                                # Runs.run gives the moved entry a fresh Sink
        new = [x for x in R.records[-1] if x[2] == 2]
        assert len(new) >= 2 * 2 and all(rate == 24000 for _, _, _, rate, _ in new)
        assert all(q >= 16 for _, q, _, _, _ in new)                       # the moved entry's own warm-up
        assert len([x for x in R.records[-1] if x[2] == 0]) == 2 * 4 * F   # the kept entry: no gap
        # a sink that had gone on with the old history would give other first samples
        for s in range(R.S):
            first = [x for x in new if x[0] == s][0]
            stale = sp.Sink()
            stale.hist = before[(s, 1)]
            m = R.mp2_slot[2]
            assert not np.array_equal(bits(stale.audio_out(pcm[s, first[1], m], 24000)), bits(first[4]))
    finally:
        R.close()


def test_table_change_keeps_the_sink_of_an_unchanged_entry(ctx, tx_iq):
    """the 24 kHz entry stays as it is while both others change and its audio slot moves from 1 to 0:
    its filter goes on with its history, so its first outputs after the change equal the continued
    restatement's (Runs.run, the Sink kept) and differ from a fresh one's; the entry that enters the
    layer gets a new sink in slot 1"""
    R = Runs(ctx, tx_iq, A)
    try:
        R.run()
        R.run()
        assert all(R.sinks[(s, 1)].hist[1].any() for s in range(R.S))      # the 24000 filter has history
        R.pipe.set_subch(-1, _subs(C))
        R.table(C, keep=(1,), restart=False)                               # the crafted stream goes on too, mid-frame
        assert set(R.sinks) == {(0, 1), (1, 1)} and R.audio_entries == [1, 2]
        pcm, info, samples, n_out = R.run()                                # compared with the kept Sinks
        kept = [x for x in R.records[-1] if x[2] == 1]
        assert len(kept) == 2 * 2 * F and all(rate == 24000 for _, _, _, rate, _ in kept)     # a frame every second CIF: no gap
        assert (n_out[:, 0, 0] == 2304).all()                              # the frame that straddles the change, in slot 0 now
        m = R.mp2_slot[1]
        for s in range(R.S):
            first = [x for x in kept if x[0] == s][0]
            assert first[1] == 0
            assert not np.array_equal(bits(sp.Sink().audio_out(pcm[s, 0, m], 24000)), bits(first[4]))
        entered = [x for x in R.records[-1] if x[2] == 2]
        assert len(entered) >= 2 * 4 and all(q >= 16 and rate == 48000 for _, q, _, rate, _ in entered)
        assert not [x for x in R.records[-1] if x[2] == 0]                 # the entry that left the layer
    finally:
        R.close()


def test_caps_and_refusals(ctx, tx_iq):
    import dabamd
    plain = [(a, n, br, pl, uep, MP2) for a, n, br, pl, uep, _ in A]
    p = dabamd.Pipeline(ctx, 1, F, _subs(plain))                           # nothing flagged: no audio output layer
    try:
        assert p.max_audio == 0
        with pytest.raises(dabamd.DabError) as e:
            p.audio()
        assert e.value.code == E_STATE
        with pytest.raises(dabamd.DabError) as e:                          # the table flags more than the layer holds
            p.set_subch(0, _subs(A))
        assert e.value.code == E_ARG
        with pytest.raises(dabamd.DabError) as e:                          # more slots than layer II slots
            p.audio_caps(4)
        assert e.value.code == E_ARG
        p.audio_caps(2)
        p.set_subch(0, _subs(A))
        with pytest.raises(dabamd.DabError) as e:                          # fewer slots than the applied table flags
            p.audio_caps(1)
        assert e.value.code == E_ARG
        with pytest.raises(dabamd.DabError) as e:                          # no run, no mp2 call
            p.audio()
        assert e.value.code == E_STATE
        for bad in ([(0, 96, 128, 3, 1, AUDIO)], [(0, 96, 128, 3, 1, 1 | AUDIO)], [(0, 96, 128, 3, 1, 8 | AUDIO)]):
            with pytest.raises(dabamd.DabError) as e:                      # AUDIO without MP2
                p.set_subch(0, _subs(bad))
            assert e.value.code == E_ARG
    finally:
        p.close()
    with pytest.raises(dabamd.DabError) as e:
        dabamd.Pipeline(ctx, 1, F, _subs([(0, 96, 128, 3, 1, AUDIO)]))
    assert e.value.code == E_ARG


def _dropin(tmp_path, iq, with_audio):
    subprocess.run(["make", "-s", "-f", os.path.join(ROOT, "tests", "cpp", "Makefile.audio"),
                    os.path.join(ROOT, "tests", "cpp", "build", "test_audio_dropin")], check=True)
    iq.tofile(tmp_path / "iq.f32")
    # the transmitter's own frames: the first two entries feed the audio output layer
    args = [str(v) for a, n, br, pl, uep, fl in A for v in (a, n, br, pl, 0 if uep else 1, fl)]
    out = tmp_path / ("audio%d.bin" % with_audio)
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "build", "test_audio_dropin"), str(tmp_path / "iq.f32"), str(out),
                        str(F), "3", str(with_audio)] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "AUDIO DROPIN OK" in r.stdout, r.stdout + r.stderr
    raw, pos, steps, step = open(out, "rb").read(), 0, [], []
    while pos < len(raw):
        kind = int(np.frombuffer(raw, "<i4", 1, pos)[0])
        cif = int(np.frombuffer(raw, "<i8", 1, pos + 4)[0])
        subch, n = (int(v) for v in np.frombuffer(raw, "<i4", 2, pos + 12))
        pos += 20
        if kind == 2:
            steps.append(step)
            step = []
        elif kind == 0:
            rate = int(np.frombuffer(raw, "<i4", 1, pos)[0])
            step.append((0, cif, subch, rate, np.frombuffer(raw, "<i2", 2 * n, pos + 4).reshape(n, 2)))
            pos += 4 + 4 * n
        else:
            step.append((1, cif, subch, 0, np.frombuffer(raw, "<f4", 2 * n, pos).reshape(n, 2)))
            pos += 8 * n
    return steps


def test_dropin_on_audio(ctx, tx_iq, tmp_path):
    """ensembleDecoder::on_audio (a C++ program over the drop-in library): its calls come after the
    step's on_pcm calls, one per accepted frame of a flagged entry, and carry what the restatement
    makes of the on_pcm frames of the same entry; with the callback unset there are none"""
    steps = _dropin(tmp_path, tx_iq[0], 1)
    assert len(steps) == 3
    sinks, n_audio = {}, 0
    for step in steps:
        kinds = [x[0] for x in step]
        assert kinds == sorted(kinds)                                       # every on_pcm before the first on_audio
        pcm = {(cif, subch): (rate, p) for kind, cif, subch, rate, p in step if kind == 0}
        audio = [(cif, subch, p) for kind, cif, subch, _, p in step if kind == 1]
        assert [(c, k) for c, k, _ in audio] == sorted((c, k) for (c, k) in pcm if k in (0, 1))
        assert any(k == 2 for _, k in pcm)                                  # the unflagged entry has PCM and no audio
        for cif, subch, got in audio:
            rate, p = pcm[(cif, subch)]
            want = sinks.setdefault(subch, sp.Sink()).audio_out(p, rate)
            assert np.array_equal(bits(got), bits(want)), (cif, subch)
            n_audio += 1
    assert n_audio >= 100
    steps = _dropin(tmp_path, tx_iq[0], 0)
    assert len(steps) == 3 and all(x[0] == 0 for step in steps for x in step) and sum(len(s) for s in steps) >= 150
