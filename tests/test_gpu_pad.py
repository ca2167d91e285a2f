"""DAB+ PAD on the GPU (k_pad.hip): the operator dabgpu_pad_aus against the reference's own
records (tests/golden/pad_kat.npz) and against the byte-level restatement pad_py.Handler (itself
held to that file and to the host padAssembler by test_pad_cpu).  Everything is compared
exactly: label records with their pieces, group records, the groups' bytes, the run counters
and the carried state."""
import numpy as np
import pytest

import pad_py as P
import packet_py as pp

pytestmark = pytest.mark.gpu

E_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def kat():
    return P.load_kat()


def _layout(cases, stride=None):
    """the AUs of several slots as [n, n_aus, stride] bytes and [n, n_aus] lengths; a slot with
    fewer AUs than the longest is filled up with AUs that failed their CRC (length -1)"""
    na = max(1, max(len(c) for c in cases))
    stride = stride or max(8, max((len(a[0]) for c in cases for a in c), default=8))
    aus = np.zeros((len(cases), na, stride), np.uint8)
    lens = np.full((len(cases), na), -1, np.int32)
    for i, c in enumerate(cases):
        for k, a in enumerate(c):
            b = np.frombuffer(bytes(a[0]), np.uint8)[:stride]
            aus[i, k, :len(b)] = b
            lens[i, k] = a[1]
    return aus, lens


def _check(h, labels, groups, data, run, what):
    """one slot's outputs against its Handler (after feed)"""
    assert run.tobytes() == h.run_record().tobytes(), (what, run, h.run_record())
    wl, wg = h.label_records(), h.group_records()
    assert np.array_equal(labels[:len(wl)], wl), (what, labels[:len(wl)], wl)
    assert np.array_equal(groups[:len(wg)], wg), (what, groups[:len(wg)], wg)
    assert bytes(data[:len(h.arena)]) == bytes(h.arena), what
    assert not labels[len(wl):].view(np.uint8).any() and not groups[len(wg):].view(np.uint8).any(), what
    assert not data[len(h.arena):].any(), what


def _run(ctx, cases, states=None, handlers=None, cif=None, **kw):
    import dabamd
    aus, lens = _layout(cases, kw.pop("stride", None))
    labels, groups, data, run, state = dabamd.pad_aus(ctx, aus, lens, states, cif, **kw)
    handlers = handlers or [P.Handler() for _ in cases]
    for i, c in enumerate(cases):
        fed = [(bytes(aus[i, k]), int(lens[i, k]), k if cif is None else int(cif[i, k]), k) for k in range(aus.shape[1])]
        handlers[i].feed(fed, data.shape[1])
        _check(handlers[i], labels[i], groups[i], data[i], run[i], i)
    return state, handlers, (labels, groups, data, run)


def test_operator_equals_reference_on_every_fixture(ctx, kat):
    """three slots at a time, each a fixture of its own (so a slot's neighbours differ): the
    labels and the accepted groups are the reference's own, everything else the restatement's"""
    seen_l = seen_g = 0
    for i in range(0, len(kat), 3):
        batch = kat[i:i + 3]
        _, hs, (labels, groups, data, run) = _run(ctx, [k["aus"] for k in batch])
        for s, k in enumerate(batch):
            got = [(int(l["au"]), int(l["charset"]), l["piece_len"][:l["n_pieces"]].tolist(), l["text"][:l["nbytes"]].tobytes())
                   for l in labels[s, :run[s]["n_labels"]]]
            assert got == [(l["au"], l["charset"], l["pieces"], l["text"]) for l in k["labels"]], k["name"]
            acc = [g for g in groups[s, :run[s]["n_groups"]] if g["flags"] & pp.ACCEPTED]
            got = [(int(g["reserved"][0]), int(g["groupType"]), int(bool(g["flags"] & pp.LAST)), int(g["segmentNumber"]),
                    int(g["transportId"]), int(g["data_offset"]), data[s, g["offset"]:g["offset"] + g["nbytes"]].tobytes()) for g in acc]
            assert got == [(c["au"], c["groupType"], c["last"], c["segmentNumber"], c["transportId"], c["index"], c["bytes"])
                           for c in k["calls"]], k["name"]
            assert run[s]["undefined"].tolist() == [0, 0, 0, 0], k["name"]
            seen_l, seen_g = seen_l + len(k["labels"]), seen_g + len(k["calls"])
    assert seen_l >= 25 and seen_g >= 25


def test_operator_state_is_carried_across_calls(ctx, kat):
    """every fixture split at every AU boundary into two calls: slot c takes the first c AUs in
    the first call and the rest in the second; what the two calls deliver, joined, and the state
    they leave are those of the unsplit fixture"""
    for k in kat:
        aus = k["aus"]
        first = [aus[:c] for c in range(len(aus) + 1)]
        second = [aus[c:] for c in range(len(aus) + 1)]
        state, hs, _ = _run(ctx, first, stride=320)
        mid = [(list(h.run_labels), list(h.run_groups)) for h in hs]
        state, hs, _ = _run(ctx, second, state, hs, stride=320)
        whole = P.Handler().feed(aus)
        for c, h in enumerate(hs):
            assert [(l["charset"], l["text"], l["pieces"]) for l in h.labels] == \
                [(l["charset"], l["text"], l["pieces"]) for l in whole.labels], (k["name"], c)
            assert [(g["flags"], g["stored"], g["data_offset"]) for g in h.groups] == \
                [(g["flags"], g["stored"], g["data_offset"]) for g in whole.groups], (k["name"], c)
            assert len(mid[c][0]) + len(h.run_labels) == len(whole.labels)
        assert all(state[c].tobytes() == state[0].tobytes() for c in range(len(hs))), k["name"]


def test_operator_rules_against_the_restatement(ctx):
    """rules 1-4, one slot per case, and the two truncations"""
    cases = P.rule_cases()
    _, hs, (labels, groups, data, run) = _run(ctx, [c["aus"] for c in cases])
    for s, c in enumerate(cases):
        assert run[s]["undefined"][c["rule"] - 1] >= 1, c["name"]
    by = {c["name"]: s for s, c in enumerate(cases)}
    s = by["rule4_bytes"]
    lab = labels[s, run[s]["n_labels"] - 1]
    assert (lab["nbytes"], lab["n_pieces"], lab["flags"]) == (257, 17, P.LABEL_TRUNCATED)
    assert lab["text"].tobytes() == b"x" * 16 + b"y" * 240
    s = by["rule4_pieces"]
    lab = labels[s, run[s]["n_labels"] - 1]
    assert (lab["nbytes"], lab["n_pieces"], lab["flags"]) == (65, 65, P.LABEL_TRUNCATED)
    assert lab["piece_len"].tolist() == [1] * 64
    assert run[by["rule1"]]["undefined"].tolist() == [2, 0, 0, 0] and run[by["rule2"]]["undefined"][1] == 6


def test_operator_reads_nothing_past_length_or_stride(ctx, kat):
    """bytes past an AU's length, and past au_stride, read 0: a stride that cuts the PADs short
    and lengths that do, against the restatement fed the same rows"""
    k = [x for x in kat if x["name"] == "slide"][0]
    cut = [(a[0], min(a[1], 40)) for a in k["aus"]]
    _run(ctx, [k["aus"], cut, k["aus"]], stride=33)
    cif = np.arange(3 * len(k["aus"]), dtype=np.int32).reshape(3, -1) * 7 + 1000
    _, hs, (labels, groups, _, run) = _run(ctx, [k["aus"], cut, k["aus"]], cif=cif)
    assert labels[0, 0]["cif"] == 1000 and groups[2, 0]["cif"] == cif[2, groups[2, 0]["reserved"][0]]


def test_operator_slots_and_arena(ctx, kat):
    """labels and groups beyond the slots are counted and not recorded; a group the arena cannot
    hold is recorded without bytes, truncated and not accepted; bad sizes are refused"""
    import dabamd
    k = [x for x in kat if x["name"] == "slide"][0]
    four = [x for x in kat if x["name"] == "four_cis"][0]
    aus, lens = _layout([k["aus"], four["aus"]])
    labels, groups, data, run, _ = dabamd.pad_aus(ctx, aus, lens, label_slots=2, group_slots=3)
    assert run["n_labels"].tolist() == [1, 3] and run["n_groups"].tolist() == [8, 0]
    whole = [P.Handler().feed(x["aus"]) for x in (k, four)]
    assert np.array_equal(labels[1], whole[1].label_records()[:2]) and np.array_equal(groups[0], whole[0].group_records()[:3])
    # an arena of the least size the call accepts holds far more than this fixture: fill it first
    big = pp.group(bytes(8000), crcf=1, seg=1, ua=1, gtype=4)
    fill = P.group_pads(big, 48, 48, per_pad=4)
    h = P.Handler()
    n = P.arena_bytes(0)
    run_aus = [P.au_of(p) for p in fill + P.group_pads(pp.group(bytes(2000), crcf=1, seg=1, ua=1, gtype=4), 48, 48, per_pad=4)]
    _, hs, (_, groups, _, run) = _run(ctx, [run_aus], handlers=[h], arena_bytes=n)
    got = groups[0, :run[0]["n_groups"]]
    assert len(got) == 2 and got[0]["flags"] & pp.ACCEPTED and got[1]["flags"] & pp.TRUNCATED and not got[1]["flags"] & pp.ACCEPTED
    assert run[0]["n_bytes"] == len(big)
    for bad in (dict(arena_bytes=n - 16), dict(arena_bytes=0), dict(label_slots=-1), dict(group_slots=-1)):
        with pytest.raises(dabamd.DabError) as e:
            dabamd.pad_aus(ctx, aus, lens, **bad)
        assert e.value.code == E_ARG and "dabgpu_pad_aus" in str(e.value), (bad, e.value)


def test_groups_feed_the_mot_layer(ctx, kat):
    """the PAD layer's groups and bytes go into dabgpu_mot_groups as they are and deliver the
    fixture's slide"""
    import dabamd
    k = [x for x in kat if x["name"] == "slide"][0]
    aus, lens = _layout([k["aus"], k["aus"][:6]])
    _, groups, data, run, _ = dabamd.pad_aus(ctx, aus, lens)
    prun = np.zeros(2, pp.RUN_DTYPE)
    prun["n_groups"], prun["n_bytes"] = run["n_groups"], run["n_bytes"]
    objects, out, mot_run, _ = dabamd.mot_groups(ctx, groups, data, prun)
    _, body = P.slide()
    assert mot_run["n_objects"].tolist() == [1, 0]
    o = objects[0, 0]
    assert o["kind"] == dabamd.MOT_SLIDE
    assert o["transportId"] == 0x4242 and out[0, o["offset"]:o["offset"] + o["nbytes"]].tobytes() == body
    assert o["name"][:o["name_len"]].tobytes() == b"pad.jpg"
