"""MOT objects on the GPU (k_mot.hip): the operator dabgpu_mot_groups and the pipeline layer
dabgpu_pipe_mot against the byte-level restatement mot_py.Assembler (itself held to the
reference's own mot-data.cpp through tests/golden/mot_kat.npz, and to the host motAssembler, by
test_mot_cpu).  Everything is compared exactly: object records, names, bodies, run counters
and the carried state.

The pipeline layer is checked as the function of the groups dabgpu_pipe_packet delivered (that
layer has its own tests in test_gpu_packet)."""
import numpy as np
import pytest

import mot_py as mp
import packet_py as pp

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -6
F = 6


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


def _layout(cases):
    """the groups of several slots in one [n, slots] / [n, arena] layout"""
    packed = [mp.pack(c) for c in cases]
    gs = max(1, max(len(r) for r, _ in packed))
    ar = max(16, max(len(a) for _, a in packed))
    groups = np.zeros((len(cases), gs), pp.GROUP_DTYPE)
    data = np.zeros((len(cases), ar), np.uint8)
    run = np.zeros(len(cases), pp.RUN_DTYPE)
    for i, (r, a) in enumerate(packed):
        groups[i, :len(r)] = r
        data[i, :len(a)] = a
        run[i]["n_groups"], run[i]["n_bytes"] = len(r), len(a)
    return groups, data, run


def _check(asm, objects, out, mot_run, state, cap, what):
    """one slot's outputs and carried state against its Assembler (after feed)"""
    n = len(asm.run_objects)
    want = asm.object_records()
    assert mot_run.tobytes() == asm.run_record().tobytes(), (what, mot_run, asm.run_record())
    assert np.array_equal(objects[:n], want), (what, objects[:n][objects[:n] != want], want[objects[:n] != want])
    for o in asm.run_objects:
        assert bytes(out[o["offset"]:o["offset"] + o["nbytes"]]) == o["body"], (what, o["group"])
    h, ent, bodies = mp.parse_state(state, cap)
    wh, went, wbodies = asm.state()
    assert h.tobytes() == wh.tobytes() and np.array_equal(ent, went), (what, h, wh, np.nonzero(ent != went))
    assert bodies == wbodies, what


def _run(ctx, cases, cap, states=None, asms=None, out_arena=None):
    import dabamd
    groups, data, run = _layout(cases)
    objects, out, mot_run, state = dabamd.mot_groups(ctx, groups, data, run, states, cap, out_arena)
    asms = asms or [mp.Assembler(cap or mp.BODY_BYTES) for _ in cases]
    for i, c in enumerate(cases):
        rec, _ = mp.pack(c)
        asms[i].feed(groups[i, :len(rec)], data[i], out.shape[1])
        _check(asms[i], objects[i], out[i], mot_run[i], state[i], cap or mp.BODY_BYTES, i)
    return state, asms, objects, mot_run


def test_operator_on_every_fixture_and_rule_case(ctx):
    """1 to 3 slots at a time, each slot a fixture of its own"""
    cases = mp.fixtures() + [c for c in mp.rule_cases() if c["cap"] == mp.BODY_BYTES]
    seen, i, k = 0, 0, 0
    while i < len(cases):
        n = 1 + k % 3
        batch = cases[i:i + n]
        _, asms, _, _ = _run(ctx, [c["groups"] for c in batch], 0)
        seen += sum(len(a.objects) for a in asms)
        i, k = i + n, k + 1
    assert seen == 36          # the golden file's 29 slides and files, its EPG object, 6 from the rule cases
    small = [c for c in mp.rule_cases() if c["cap"] != mp.BODY_BYTES]
    assert len(small) == 1
    _, asms, _, _ = _run(ctx, [small[0]["groups"], mp.fixtures()[0]["groups"]], small[0]["cap"])
    assert asms[0].handle(0x3334).flags == mp.TOO_LARGE and len(asms[0].objects) == 1


def test_operator_output_arena_overflow(ctx):
    """an object that does not fit the arena is recorded without bytes; the next smaller one fits"""
    c = [x for x in mp.rule_cases() if x["name"] == "rule4"][0]
    _, asms, objects, mot_run = _run(ctx, [c["groups"]], 304, out_arena=mp.arena_bytes(0, 304) + 64)
    assert [(o["flags"], o["nbytes"]) for o in asms[0].run_objects] == [(0, 300), (mp.OVERFLOW, 0)]
    import dabamd
    groups, data, run = _layout([c["groups"]])
    # each refused by dabgpu_mot_groups itself: an arena too small, one that is no multiple of 16,
    # bodies above 1 << 24 (with an arena that is fine and with the binding's own), negative ones
    for bad in (dict(out_arena_bytes=mp.arena_bytes(0, 256) - 16), dict(out_arena_bytes=mp.arena_bytes(0, 256) + 8),
                dict(max_body_bytes=(1 << 24) + 16, out_arena_bytes=mp.arena_bytes(0, (1 << 24) + 16)),
                dict(max_body_bytes=(1 << 24) + 1), dict(max_body_bytes=-1)):
        with pytest.raises(dabamd.DabError) as e:
            dabamd.mot_groups(ctx, groups, data, run, None, **{"max_body_bytes": 256, **bad})
        assert e.value.code == E_ARG and "dabgpu_mot_groups" in str(e.value), (bad, e.value)


def test_operator_state_is_carried_across_calls(ctx):
    """every fixture split at every group boundary into two calls: slot c takes the first c
    groups in the first call and the rest in the second"""
    cap = 4096
    for f in mp.fixtures():
        g = f["groups"]
        first = [g[:c] for c in range(len(g) + 1)]
        second = [g[c:] for c in range(len(g) + 1)]
        state, asms, _, _ = _run(ctx, first, cap)
        _run(ctx, second, cap, state, asms)
        whole = mp.Assembler(cap)
        whole.feed(*mp.pack(g))
        for c, a in enumerate(asms):
            assert [(o["transportId"], o["body"]) for o in a.objects] == \
                [(o["transportId"], o["body"]) for o in whole.objects], (f["name"], c)


def test_operator_refuses_records_that_point_outside(ctx):
    """hostile records: offsets and lengths outside the arena are counted as malformed and
    nothing is read or written through them"""
    g = mp.fixtures()[0]["groups"]
    groups, data, run = _layout([g, g, g])
    groups[0, 1]["offset"] = data.shape[1] - 4
    groups[0, 2]["data_nbytes"] = groups[0, 2]["nbytes"] + 1
    groups[1, 1]["offset"] = -8
    groups[1, 3]["data_offset"] = -1
    groups[2, 1]["nbytes"] = 1 << 30
    run[2]["n_groups"] = 1 << 20                       # more than the slots hold: clamped
    import dabamd
    objects, out, mot_run, state = dabamd.mot_groups(ctx, groups, data, run)
    for i in range(3):
        a = mp.Assembler()
        a.feed(groups[i], data[i], out.shape[1])
        _check(a, objects[i], out[i], mot_run[i], state[i], mp.BODY_BYTES, i)
        assert a.malformed >= 1 and not a.objects


# ---- the pipeline layer -------------------------------------------------------------------
PACKET, MOTF, MP2F = 8, 16, 4
TABLE = [(0, 48, 64, 0o103, 0, PACKET | MOTF), (48, 24, 32, 0o103, 0, PACKET), (144, 96, 128, 3, 1, MP2F)]
SWAPPED = [TABLE[1], TABLE[0], TABLE[2]]


def _subs(table):
    import dabamd
    return [dabamd.Subch(a, n, br, pl, 0 if uep else 1, fl) for a, n, br, pl, uep, fl in table]


@pytest.fixture(scope="module")
def tx():
    """two streams of one layout, 19 frames: a MOT carousel on a 64 kbit/s packet entry beside
    a plain packet entry and a layer II entry; and, from the transmitted bits, that 19 frames
    at this bit rate carry every slide of the carousel at least once"""
    from dabamd.synth import Ensemble, MP2, PACKET as SP, MOT
    e = Ensemble(3 * F + 1, subch=[(0, 48, 64, 0o103, 0, 0, MOT), (48, 24, 32, 0o103, 0, 0, SP),
                                   (144, 96, 128, 3, 1, 0, MP2)], figs=True)
    iqs = []
    for seed in (511, 512):
        g = e.generate(seed)
        a = pp.Assembler(64)
        for q in range(16, g["msc"].shape[0]):
            a.cif(q, np.packbits(g["msc"][q, 0, :24 * 64]))
        m = mp.Assembler()
        m.feed(a.group_records(), np.frombuffer(bytes(a.arena), np.uint8))
        assert {o["transportId"] for o in m.objects} == {0x1000, 0x1001, 0x1002, 0x1003}, seed
        iqs.append(g["iq"])
    return iqs


class MotPipe:
    def __init__(self, ctx, iqs, table, **caps):
        import dabamd
        self.S = len(iqs)
        self.lens = [len(x) // 2 for x in iqs]
        self.stride = max(self.lens)
        buf = np.zeros((self.S, 2 * self.stride), np.float32)
        for s, x in enumerate(iqs):
            buf[s, :len(x)] = x
        self.diq = ctx.put(buf)
        self.pipe = dabamd.Pipeline(ctx, self.S, F, _subs(table), **caps)
        self.pipe.control(dabamd.CTL_ACQ_SYNC)
        self.tables = [list(table) for _ in range(self.S)]
        self.asm = {}

    def mot_slots(self, s):
        """[(table index, packet slot)] of stream s's MOT slots"""
        out, j = [], 0
        for k, e in enumerate(self.tables[s]):
            if e[5] & PACKET:
                if e[5] & MOTF:
                    out.append((k, j))
                j += 1
        return out

    def run_packet(self):
        p = self.pipe
        _, _, msc, _ = p.run(self.diq, self.stride, self.lens, partial=True)
        p.mp2()
        return msc, p.packet()

    def mot(self, pk):
        """dabgpu_pipe_mot, everything it writes checked against an Assembler per (stream, table entry)"""
        p = self.pipe
        byts, groups, run, _ = pk
        out, objects, mot_run = p.mot()
        gs = groups.shape[2]
        for s in range(self.S):
            slots = self.mot_slots(s)
            for m in range(p.max_mot):
                if m >= len(slots):
                    assert mot_run[s, m]["n_objects"] == 0 and mot_run[s, m]["entries"] == 0
                    continue
                k, j = slots[m]
                a = self.asm.setdefault((s, k), mp.Assembler(p.max_body_bytes))
                a.feed(groups[s, j, :min(int(run[s, j]["n_groups"]), gs)], byts[s, j], out.shape[2])
                n = len(a.run_objects)
                want = a.object_records()
                assert mot_run[s, m].tobytes() == a.run_record().tobytes(), (s, m, mot_run[s, m], a.run_record())
                assert np.array_equal(objects[s, m, :n], want), (s, m)
                for o in a.run_objects:
                    assert bytes(out[s, m, o["offset"]:o["offset"] + o["nbytes"]]) == o["body"], (s, m, o["group"])
        return out, objects, mot_run

    def close(self):
        self.pipe.close()
        self.diq.free()


def _code(fn):
    import dabamd
    with pytest.raises(dabamd.DabError) as e:
        fn()
    return e.value.code


def test_pipeline_layer(ctx, tx):
    """2 streams x 6 frames a run over 19 frames: the layer equals the restatement over the
    groups the packet layer delivered, every slide arrives, the layer writes nothing it only
    reads, and the sequence errors are refused"""
    import dabamd
    L = MotPipe(ctx, tx, TABLE, max_mot=2)
    try:
        p = L.pipe
        assert p.max_mot == 2 and p.max_packet == 2
        assert _code(p.mot) == E_STATE                              # no run yet
        for r in range(3):
            msc, pk = L.run_packet() if r else (None, None)
            if r == 0:
                p.run(L.diq, L.stride, L.lens, partial=True)
                assert _code(p.mot) == E_STATE                      # before this run's dabgpu_pipe_packet
                p.mp2()
                msc = p.msc_d.download(np.uint8, (L.S, 4 * F, p.max_subch, p.msc_stride))
                pk = p.packet()
            L.mot(pk)
            assert _code(p.mot) == E_STATE                          # a second call
            # msc_bits_d and the packet outputs are as they were
            assert np.array_equal(p.msc_d.download(np.uint8, msc.shape), msc)
            assert np.array_equal(p.pkb_d.download(np.uint8, pk[0].shape), pk[0])
            assert p.pkg_d.download(np.uint8, pk[1].nbytes).tobytes() == pk[1].tobytes()
            assert p.pkr_d.download(np.uint8, pk[2].nbytes).tobytes() == pk[2].tobytes()
        for s in range(L.S):
            a = L.asm[(s, 0)]
            assert {o["transportId"] for o in a.objects} == {0x1000, 0x1001, 0x1002, 0x1003}, s
            assert all(o["kind"] == mp.SLIDE and o["name"] == b"s0_%d.jpg" % (o["transportId"] & 15) for o in a.objects)
            assert a.malformed == a.bad_segment == a.other_types == 0
    finally:
        L.close()


def test_pipeline_set_subch_keeps_and_replaces_state(ctx, tx):
    """after the first run stream 0 gets the table it has (its motHandler goes on) and stream 1
    the same entries in another order (every entry is new: a new motHandler, and a second one on
    the plain packet entry, whose random groups are hostile input).  Beside the exact check, a
    motHandler that was wrongly replaced or wrongly kept would have delivered other objects."""
    import copy
    L = MotPipe(ctx, tx, TABLE, max_mot=2)
    try:
        p = L.pipe
        _, pk = L.run_packet()
        L.mot(pk)
        assert min(L.asm[(s, 0)].created for s in range(L.S)) >= 1  # there is state to keep or to lose
        n0 = len(L.asm[(0, 0)].objects)
        wrongly_new, wrongly_kept = mp.Assembler(), copy.deepcopy(L.asm[(1, 0)])
        p.set_subch(0, _subs(TABLE))
        swapped = [SWAPPED[0][:5] + (PACKET | MOTF,), SWAPPED[1], SWAPPED[2]]
        p.set_subch(1, _subs(swapped))
        L.tables[1] = swapped
        L.asm = {(0, 0): L.asm[(0, 0)]}                             # stream 1 starts anew, at other table indices
        assert L.mot_slots(1) == [(0, 0), (1, 1)]
        assert _code(p.mot) == E_STATE                              # the packet call of the old table is gone
        for _ in range(2):
            _, pk = L.run_packet()
            L.mot(pk)
            byts, groups, run, _ = pk
            wrongly_new.feed(groups[0, 0, :run[0, 0]["n_groups"]], byts[0, 0])
            wrongly_kept.feed(groups[1, 1, :run[1, 1]["n_groups"]], byts[1, 1])
        ids = lambda objs: [(o["transportId"], o["group"]) for o in objs]
        kept, new = L.asm[(0, 0)], L.asm[(1, 1)]
        assert len(kept.objects) - n0 >= 4 and len(new.objects) >= 4
        assert ids(kept.objects[n0:]) != ids(wrongly_new.objects)
        assert ids(new.objects) != ids(wrongly_kept.objects[len(wrongly_kept.objects) - len(new.objects):]) or \
            len(wrongly_kept.objects) != len(new.objects)
    finally:
        L.close()


def test_pipeline_arguments(ctx, tx):
    import dabamd
    mot_only = [(0, 48, 64, 0o103, 0, MOTF)] + TABLE[1:]
    assert _code(lambda: dabamd.Pipeline(ctx, 1, F, _subs(mot_only))) == E_ARG     # MOT without PACKET
    plain = dabamd.Pipeline(ctx, 1, F, _subs(TABLE[1:]))
    try:
        assert plain.max_mot == 0
        assert _code(plain.mot) == E_STATE                          # no layer
        assert _code(lambda: plain.mot_caps(2)) == E_ARG            # max_mot > max_packet
        assert _code(lambda: plain.mot_caps(-1)) == E_ARG
        assert _code(lambda: plain.mot_caps(1, -5)) == E_ARG
        assert _code(lambda: plain.mot_caps(1, (1 << 24) + 1)) == E_ARG
        assert _code(lambda: plain.set_subch(0, _subs([TABLE[0]] + TABLE[2:]))) == E_ARG     # no MOT slot for it
        plain.mot_caps(1, 4096)
        plain.set_subch(0, _subs([(48, 24, 32, 0o103, 0, PACKET | MOTF), TABLE[2]]))
        assert _code(lambda: plain.mot_caps(0)) == E_ARG            # the table flags one
        assert _code(lambda: plain.packet_caps(0)) == E_ARG         # fewer packet slots than MOT slots
        assert _code(lambda: plain.set_subch(0, _subs(mot_only))) == E_ARG
    finally:
        plain.close()


def test_pipeline_caps_keep_state(ctx, tx):
    """dabgpu_pipe_mot_caps between runs: the motHandlers go on in larger and in smaller bodies"""
    L = MotPipe(ctx, tx[:1], TABLE)
    try:
        p = L.pipe
        assert p.max_mot == 1
        _, pk = L.run_packet()
        L.mot(pk)
        p.mot_caps(2, 1024)                                         # the carousel's bodies are <= 300 bytes
        L.asm[(0, 0)].cap = 1024
        _, pk = L.run_packet()
        L.mot(pk)
        p.mot_caps(1, 0)
        L.asm[(0, 0)].cap = mp.BODY_BYTES
        _, pk = L.run_packet()
        L.mot(pk)
        assert len(L.asm[(0, 0)].objects) >= 4
    finally:
        L.close()
