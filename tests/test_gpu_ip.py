"""IP data on the GPU (k_ip.hip): the operator dabgpu_ip_groups against the byte-level restatement
ip_py.Handler (itself held to the reference's own ip-datahandler.cpp through
tests/golden/ip_kat.npz, and to the host ipAssembler, by test_ip_cpu).  Everything is compared
exactly: result records, payload bytes, run counters and the carried counters.  The pipeline
layer has its own file, test_gpu_ip_pipeline."""
import ctypes as C

import numpy as np
import pytest

import ip_py as ip
import packet_py as pp

pytestmark = pytest.mark.gpu

E_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


def _layout(cases, slots=None):
    """the groups of several slots in one [n, slots] / [n, arena] layout"""
    packed = [ip.pack(c) for c in cases]
    gs = max(1, max(len(r) for r, _ in packed)) if slots is None else slots
    ar = max(16, max(len(a) for _, a in packed))
    groups = np.zeros((len(cases), gs), pp.GROUP_DTYPE)
    data = np.zeros((len(cases), ar), np.uint8)
    run = np.zeros(len(cases), pp.RUN_DTYPE)
    for i, (r, a) in enumerate(packed):
        groups[i, :len(r)] = r
        data[i, :len(a)] = a
        run[i]["n_groups"], run[i]["n_bytes"] = len(r), len(a)
    return groups, data, run


def _check(h, groups, data, n, results, out, ip_run, state, what):
    """one slot's outputs and carried counters against its Handler (fed here)"""
    want, wout, wrun = h.feed(groups[:n], data, out.shape[0])
    assert np.array_equal(results[:n], want), (what, results[:n][results[:n] != want][:4], want[results[:n] != want][:4])
    assert not results[n:].view(np.uint8).any(), what               # the records past the run's groups are not written
    assert ip_run.tobytes() == wrun.tobytes(), (what, ip_run, wrun)
    assert state.tobytes() == h.state().tobytes(), (what, state, h.state())
    assert np.array_equal(out, wout), what                          # payloads, and zeros (as uploaded) everywhere else
    # payloads at multiples of 16, in group order, disjoint
    d = want[want["status"] == ip.DELIVERED]
    assert (d["offset"] % 16 == 0).all() and (d["offset"][1:] >= d["offset"][:-1] + d["nbytes"][:-1]).all(), what
    return want


def _run(ctx, cases, states=None, handlers=None, out_arena=None, slots=None):
    import dabamd
    groups, data, run = _layout(cases, slots)
    results, out, ip_run, state = dabamd.ip_groups(ctx, groups, data, run, states, out_arena)
    handlers = handlers or [ip.Handler(*(states[i].tolist() if states is not None else ())) for i in range(len(cases))]
    want = [_check(handlers[i], groups[i], data[i], len(c), results[i], out[i], ip_run[i], state[i], i) for i, c in enumerate(cases)]
    return state, handlers, want


def test_operator_on_every_fixture_and_rule_case(ctx):
    """1 and 3 slots at a time, each slot a fixture of its own, so the group counts of a call
    differ; an empty slot among them"""
    cases = [c["groups"] for c in ip.fixtures() + ip.rule_cases()]
    seen = np.zeros(7, int)
    for i, c in enumerate(cases):
        batch = [c] if i % 2 == 0 else [c, [], cases[(i + 5) % len(cases)]]
        _, _, want = _run(ctx, batch)
        seen += np.bincount(want[0]["status"], minlength=7)
    assert (seen > 0).all() and seen[ip.DELIVERED] > 240, seen      # the golden file's datagrams, every status met
    _, hs, _ = _run(ctx, [ip.fixtures()[-1]["groups"]])
    assert hs[0].qualities == [97, 97] and (hs[0].handled, hs[0].crc_errors) == (30, 1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_operator_batch_edges(ctx, n):
    """group counts around the 64-group batch, three seeded slots of every kind of group each,
    handlers that start anywhere in their window"""
    cases = [ip.random_groups(1000 + 7 * n + k, n) for k in range(3)]
    states = np.array([(0, 0), (97, 3), (40, 11)], ip.STATE_DTYPE)
    _, hs, want = _run(ctx, cases, states)
    if n >= 63:
        assert all((w["status"] == ip.DELIVERED).sum() * 4 >= n for w in want)
        assert hs[1].qualities and hs[1].qualities[0] <= 97          # a window closed inside the first batch


def test_operator_state_is_carried_across_calls(ctx):
    """99 handled before the call, then one group: show_ipErrors inside group 0; and the window
    fixture split into two calls at several group boundaries, slot c taking the first c groups first"""
    g = [pp.group(ip.datagram(b"carried"))]
    state, hs, want = _run(ctx, [g, g], np.array([(99, 4), (98, 4)], ip.STATE_DTYPE))
    assert want[0]["quality"].tolist() == [96] and want[1]["quality"].tolist() == [-1]
    assert state.tolist() == [(0, 0), (99, 4)]
    w = ip.fixtures()[-1]["groups"]
    cuts = [0, 1, 64, 107, 108, 109, 128, 216, len(w)]
    state, hs, _ = _run(ctx, [w[:c] for c in cuts], slots=len(w))
    _run(ctx, [w[c:] for c in cuts], state, hs, slots=len(w))
    for h in hs:
        assert h.qualities == [97, 97] and (h.handled, h.crc_errors) == (30, 1) and len(h.datagrams) == 223


def test_operator_refuses_records_that_point_outside(ctx):
    """hostile records (rule 5): offsets and lengths outside the arena are NOT_ACCEPTED and nothing
    is read or written through them; a group count above the slots is clamped; an arena that is too
    small leaves its datagrams malformed (rule 6)"""
    import dabamd
    g = ip.fixtures()[0]["groups"]
    groups, data, run = _layout([g, g, g])
    groups[0, 1]["offset"] = data.shape[1] - 4
    groups[0, 2]["data_offset"] = -1
    groups[1, 1]["offset"] = -8
    groups[1, 3]["data_offset"] = 0x7FFFFFFE
    groups[2, 1]["nbytes"] = 1 << 30
    groups[2, 2]["nbytes"] = -5
    run[2]["n_groups"] = 1 << 20
    for oa in (None, 160, 0):
        results, out, ip_run, state = dabamd.ip_groups(ctx, groups, data, run, None, oa)
        for i in range(3):
            want = _check(ip.Handler(), groups[i], data[i], len(g), results[i], out[i], ip_run[i], state[i], (oa, i))
            assert (want["status"] == ip.NOT_ACCEPTED).sum() == (2, 1, 2)[i]
            if oa is not None:
                assert (want["status"] == ip.MALFORMED).any()


def test_operator_arguments_and_guards(ctx):
    """DABGPU_E_ARG for bad sizes and null pointers, before anything is read or written; and a
    good call between guard bytes leaves every guard as it was"""
    import dabamd
    lib = dabamd.lib()
    cases = [c["groups"] for c in ip.fixtures()[:3]]
    groups, data, run = _layout(cases)
    n, gs, ar = groups.shape[0], groups.shape[1], data.shape[1]
    oa = ip.arena_bytes(gs, ar) + 4                                  # no multiple of 16: the slots' arenas are unaligned
    G = 64
    sizes = [n * ip.STATE_DTYPE.itemsize, n * gs * ip.RESULT_DTYPE.itemsize, n * oa, n * ip.RUN_DTYPE.itemsize]
    host = [np.full(sz + 2 * G, 0xA5, np.uint8) for sz in sizes]
    for h, sz in zip(host, sizes):
        h[G:G + sz] = 0
    bufs = [ctx.put(h) for h in host]
    dg, db, dr = ctx.put(groups.view(np.uint8)), ctx.put(data), ctx.put(run.view(np.uint8))
    at = lambda b: C.c_void_p(b.ptr.value + G)
    try:
        def call(state=at(bufs[0]), n_slots=n, grp=dg.ptr, slots=gs, byts=db.ptr, arena=ar, rn=dr.ptr, res=at(bufs[1]),
                 out=at(bufs[2]), out_arena=oa, iprun=at(bufs[3])):
            return lib.dabgpu_ip_groups(ctx.h, state, n_slots, grp, slots, byts, arena, rn, res, out, out_arena, iprun)
        for bad in (dict(n_slots=-1), dict(slots=-1), dict(arena=-1), dict(arena=1 << 31), dict(out_arena=-16),
                    dict(out_arena=1 << 31), dict(state=None), dict(grp=None), dict(byts=None), dict(rn=None), dict(res=None),
                    dict(out=None), dict(iprun=None)):
            assert call(**bad) == E_ARG, bad
        assert lib.dabgpu_ip_groups(None, at(bufs[0]), n, dg.ptr, gs, db.ptr, ar, dr.ptr, at(bufs[1]), at(bufs[2]), oa, at(bufs[3])) == E_ARG
        ctx.sync()
        for b, h in zip(bufs, host):                                 # the refused calls wrote nothing
            assert np.array_equal(b.download(np.uint8, h.size), h)
        assert call(n_slots=0) == 0 and call() == 0
        ctx.sync()
        back = [b.download(np.uint8, h.size) for b, h in zip(bufs, host)]
        for b, sz in zip(back, sizes):
            assert (b[:G] == 0xA5).all() and (b[G + sz:] == 0xA5).all()
        results = np.frombuffer(back[1][G:G + sizes[1]].tobytes(), ip.RESULT_DTYPE).reshape(n, gs)
        out = back[2][G:G + sizes[2]].reshape(n, oa)
        ip_run = np.frombuffer(back[3][G:G + sizes[3]].tobytes(), ip.RUN_DTYPE)
        state = np.frombuffer(back[0][G:G + sizes[0]].tobytes(), ip.STATE_DTYPE)
        for i, c in enumerate(cases):
            _check(ip.Handler(), groups[i], data[i], len(c), results[i], out[i], ip_run[i], state[i], i)
    finally:
        for b in bufs + [dg, db, dr]:
            b.free()
