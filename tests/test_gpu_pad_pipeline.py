"""The PAD layer in the pipeline (dabgpu_pipe_pad, dabgpu_pipe_pad_caps, DABGPU_SUBCH_PAD): the
layer is checked as the function of what dabgpu_pipe_dabplus delivered (that layer has its own
tests): the AUs of status-3 superframes, gathered here from its sparse or compact output in CIF
and AU order, go through the restatement pad_py.Handler, and everything the layer wrote is
compared exactly.  The streams carry the transmitter's DABSYNTH_PAD programme (labels and a
slide as X-PAD groups) on one subchannel and its random-AU DAB+ content on the others: there
about one AU in eight opens with a data stream element, and its PAD is random bytes."""
import numpy as np
import pytest

import pad_py as P

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -6
NFR = 17
# (startAddr, CUs, bitRate, protLevel, uep flag of the transmitter, dabplus, content)
TX = [(0, 48, 64, 0o103, 0, 1, 6), (48, 24, 32, 0o103, 0, 1, 0), (96, 24, 32, 0o103, 0, 1, 0)]
TX2 = [(0, 24, 32, 0o103, 0, 1, 6), (24, 24, 32, 0o103, 0, 1, 0)]       # one DABSYNTH_PAD, one random content


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


def _rig(ctx, tx):
    from dabamd.synth import Ensemble
    e = Ensemble(NFR, subch=tx, snr_db=25.0)
    iqs = [e.generate(s, truth=False)["iq"] for s in (81, 82)]
    lens = [len(x) // 2 for x in iqs]
    buf = np.zeros((2, 2 * max(lens)), np.float32)
    for s, x in enumerate(iqs):
        buf[s, :len(x)] = x
    return dict(diq=ctx.put(buf), stride=max(lens), lens=lens, tx=tx)


@pytest.fixture(scope="module")
def rig(ctx):
    r = _rig(ctx, TX)
    yield r
    r["diq"].free()


@pytest.fixture(scope="module")
def rig2(ctx):
    r = _rig(ctx, TX2)
    yield r
    r["diq"].free()


def _subs(flags, tx=TX):
    import dabamd
    return [dabamd.Subch(sc[0], sc[1], sc[2], sc[3], 1, f) for sc, f in zip(tx, flags)]


def _pipe(ctx, F, flags, compact=False, tx=TX, **kw):
    import dabamd
    p = dabamd.Pipeline(ctx, 2, F, _subs(flags, tx), **kw)
    p.control(dabamd.CTL_ACQ_SYNC)
    if compact:
        p.set_dabplus_compact(True)
    return p


def _aus(info, sf, s, d, compact):
    """the AUs mp4Processor hands on, of DAB+ slot d of stream s: (bytes, length, cif, au)"""
    out, rejected = [], 0
    for c in range(info.shape[1]):
        r = info[s, c, d]
        rejected += int(r["status"] == 2)
        if r["status"] != 3:
            continue
        row = sf[s, d, r["reserved"]] if compact else sf[s, c, d]
        for a in range(r["num_aus"]):
            a0, ln = int(r["au_start"][a]), int(r["au_start"][a + 1]) - int(r["au_start"][a]) - 2
            if (r["au_crc_ok"] >> a) & 1:
                out.append((bytes(row[a0:a0 + ln]), ln, c, a))
    return out, rejected


def _step(pipe, rig, handlers, slots, compact):
    """one run, its DAB+ and PAD layers; handlers[(s, m)] fed the same AUs and compared"""
    import dabamd
    pipe.run(rig["diq"], rig["stride"], rig["lens"], partial=True)
    info, sf = pipe.dabplus()
    labels, groups, data, run = pipe.pad_last = pipe.pad()
    assert labels.shape[2] == 4 * dabamd.pad_au_slots(pipe.F) and data.shape[2] == dabamd.pad_arena_bytes(pipe.F)
    for s in range(2):
        for m, d in enumerate(slots[s]):
            h = handlers[(s, m)]
            aus, rejected = _aus(info, sf, s, d, compact)
            h.begin_run(data.shape[2])
            for a in aus:
                h.au(*a)
            h.c["rejected_sf"] = rejected
            what = (s, m, pipe._run)
            assert run[s, m].tobytes() == h.run_record().tobytes(), (what, run[s, m], h.run_record())
            wl, wg = h.label_records(), h.group_records()
            assert np.array_equal(labels[s, m, :len(wl)], wl) and np.array_equal(groups[s, m, :len(wg)], wg), what
            assert bytes(data[s, m, :len(h.arena)]) == bytes(h.arena), what
    return info


@pytest.mark.parametrize("compact", [False, True], ids=["sparse", "compact"])
def test_pipeline_pad_equals_restatement(ctx, rig2, compact):
    """2 streams x 2 DAB+ subchannels at 32 kbit/s, one DABSYNTH_PAD and one random content, 12
    frames in runs of 4 and in one run; the programme's labels and its slide come out"""
    import dabamd
    import mot_py
    import packet_py as pp
    flags = [dabamd.SUBCH_DABPLUS | dabamd.SUBCH_PAD] * 2
    slots = [[0, 1], [0, 1]]
    total = {}
    for F in (4, 12):
        pipe = _pipe(ctx, F, flags, compact, TX2)
        hs = {(s, m): P.Handler() for s in range(2) for m in range(2)}
        try:
            for _ in range(12 // F):
                _step(pipe, rig2, hs, slots, compact)
            if F == 12:                                        # the run's groups into dabgpu_mot_groups as they are
                _, groups, data, run = pipe.pad_last
                prun = np.zeros(4, pp.RUN_DTYPE)
                prun["n_groups"], prun["n_bytes"] = run.reshape(-1)["n_groups"], run.reshape(-1)["n_bytes"]
                objects, out, mot_run, _ = dabamd.mot_groups(ctx, groups.reshape(4, -1), data.reshape(4, -1), prun)
                for s in range(2):
                    o = objects[2 * s, 0]
                    assert mot_run[2 * s]["n_objects"] == 1 and o["kind"] == dabamd.MOT_SLIDE and o["nbytes"] == 230
                    assert o["name"][:o["name_len"]].tobytes() == b"s0_0.jpg" and o["transportId"] == 0x1000
        finally:
            pipe.close()
        total[F] = {k: ([(l["charset"], l["text"]) for l in h.labels], [(g["flags"], g["stored"]) for g in h.groups],
                        len(h.touched), [sorted(t) for t in h.touched]) for k, h in hs.items()}
    assert total[4] == total[12]
    for s in range(2):
        labels, groups, pads, _ = total[12][(s, 0)]
        assert [t for _, t in labels][1:] == [b"ABC", b"sub 0 charset 0"] and labels[0][1].startswith(b"DABSYNTH s0 - now playing")
        assert sum(1 for f, _ in groups if f & pp.ACCEPTED) == 6 and pads == 24
        a = mot_py.Assembler()
        a.feed(*mot_py.pack([g for f, g in groups if f & pp.ACCEPTED]))
        assert len(a.objects) == 1 and len(a.objects[0]["body"]) == 230
        assert 0 < total[12][(s, 1)][2] < 24                   # the random content: some AUs reach processPAD


def test_set_subch_keeps_an_unchanged_handler_and_renews_a_changed_one(ctx, rig):
    import dabamd
    DP, PAD = dabamd.SUBCH_DABPLUS, dabamd.SUBCH_PAD
    pipe = _pipe(ctx, 4, [DP | PAD, DP, DP | PAD])
    hs = {(s, m): P.Handler() for s in range(2) for m in range(2)}
    slots = [[0, 2], [0, 2]]
    try:
        _step(pipe, rig, hs, slots, False)
        _step(pipe, rig, hs, slots, False)
        # stream 1: entry 1 gains the flag (a new handler in slot 1), entry 2, unchanged, moves to slot 2
        # and keeps its handler; entry 0 unchanged.  More flagged entries than the layer holds: refused.
        with pytest.raises(dabamd.DabError) as e:
            pipe.set_subch(1, _subs([DP | PAD, DP | PAD, DP | PAD]))
        assert e.value.code == E_ARG
        pipe.pad_caps(3)
        pipe.set_subch(1, _subs([DP | PAD, DP | PAD, DP | PAD]))
        with pytest.raises(dabamd.DabError) as e:      # the last run was decoded under the old table
            pipe.pad()
        assert e.value.code == E_STATE
        hs[(1, 2)] = hs[(1, 1)]
        hs[(1, 1)] = P.Handler()
        hs[(0, 2)] = P.Handler()                       # stream 0 has no third flagged entry: its slot stays idle
        slots = [[0, 2], [0, 1, 2]]
        seen = sum(len(h.touched) for h in hs.values())
        _step(pipe, rig, hs, slots, False)
        _step(pipe, rig, hs, slots, False)
        assert sum(len(h.touched) for h in hs.values()) > seen
        assert len(hs[(1, 2)].touched) > len(hs[(1, 1)].touched)      # the kept handler has the longer history
    finally:
        pipe.close()


def test_caps_and_call_order(ctx, rig):
    import dabamd
    DP, PAD = dabamd.SUBCH_DABPLUS, dabamd.SUBCH_PAD
    with pytest.raises(dabamd.DabError) as e:          # the flag without DAB+
        dabamd.Pipeline(ctx, 2, 4, _subs([DP | PAD, PAD, DP]))
    assert e.value.code == E_ARG
    pipe = _pipe(ctx, 4, [DP | PAD, DP, DP | PAD])
    try:
        for bad in (-1, 4, 1):                         # negative, above max_dabplus, fewer than the table flags
            with pytest.raises(dabamd.DabError) as e:
                pipe.pad_caps(bad)
            assert e.value.code == E_ARG, bad
        with pytest.raises(dabamd.DabError) as e:      # before any run
            pipe.pad()
        assert e.value.code == E_STATE
        pipe.run(rig["diq"], rig["stride"], rig["lens"], partial=True)
        with pytest.raises(dabamd.DabError) as e:      # no DAB+ call for the run
            pipe.pad()
        assert e.value.code == E_STATE
        pipe.dabplus()
        pipe.pad()
        with pytest.raises(dabamd.DabError) as e:      # a second time for the run
            pipe.pad()
        assert e.value.code == E_STATE
        pipe.run(rig["diq"], rig["stride"], rig["lens"], partial=True)
        pipe.dabplus()
        l = dabamd.lib()                               # other buffers than the DAB+ call's
        rc = l.dabgpu_pipe_pad(pipe.h, pipe.sfi_d.ptr, pipe.sf_stride, pipe.sfi_d.ptr, pipe._pad[0][0].ptr, pipe._pad[0][1].ptr,
                               pipe._pad[0][2].ptr, pipe._pad[0][3].ptr)
        assert rc == E_ARG
        pipe.pad()
    finally:
        pipe.close()


def test_without_a_flagged_entry_nothing_is_there(ctx, rig):
    """no layer: dabgpu_pipe_pad returns E_STATE, and the DAB+ layer's outputs are byte for byte
    those of a pipeline whose entries are flagged"""
    import dabamd
    DP, PAD = dabamd.SUBCH_DABPLUS, dabamd.SUBCH_PAD
    outs = []
    for flags in ([DP, DP, DP], [DP | PAD, DP | PAD, DP | PAD]):
        pipe = _pipe(ctx, 4, flags)
        try:
            rows = []
            for _ in range(3):
                fic, crc, msc, valid = pipe.run(rig["diq"], rig["stride"], rig["lens"], partial=True)
                info, sf = pipe.dabplus()
                if flags[0] & PAD:
                    pipe.pad()
                else:
                    assert pipe.max_pad == 0 and not pipe._pad
                    scratch = ctx.buf(1 << 16)
                    rc = dabamd.lib().dabgpu_pipe_pad(pipe.h, pipe.sf_d.ptr, pipe.sf_stride, pipe.sfi_d.ptr, scratch.ptr,
                                                      scratch.ptr, scratch.ptr, scratch.ptr)
                    scratch.free()
                    assert rc == E_STATE
                dec = info["status"] == 3
                # a run leaves the rows of CIFs inside the warm-up, and a superframe row past its
                # 110 * bitRate / 8 bytes, untouched: what the layers write is compared
                sfs = b"".join(sf[:, :, d][dec[:, :, d]][:, :110 * sc[2] // 8].tobytes() for d, sc in enumerate(TX))
                rows.append((fic.tobytes(), crc.tobytes(), valid.tobytes(), msc[valid.astype(bool)][..., :24 * 32].tobytes(),
                             info.tobytes(), sfs))
            outs.append(rows)
        finally:
            pipe.close()
    assert outs[0] == outs[1]
    assert any(len(r[5]) for r in outs[0])             # superframes were decoded
