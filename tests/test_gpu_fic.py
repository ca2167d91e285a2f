"""The FIC layer on the GPU (k_fib.hip): the operator dabgpu_fib_parse against the host class
dabgpu::fib_processor (tests/fib_py.Host, itself held to the restatement by test_fic_cpu).
Everything is compared exactly, as bytes: the database, the event slots, the table and the run
record of every slot after every call."""
import ctypes as C

import numpy as np
import pytest

import fib_py as F

pytestmark = pytest.mark.gpu

E_ARG = -1
NAMES = ("db", "events", "table", "run")


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


def _same(a, b, what):
    assert a.tobytes() == b.tobytes(), (what, [(n, a[n], b[n]) for n in a.dtype.names if a[n].tobytes() != b[n].tobytes()])


def _call(ctx, fibs, ok=None, hosts=None, dbs=None, want=0, event_slots=65, clear=None):
    """one dabgpu_fib_parse call on len(fibs) slots (fibs [n, n_fibs, 32]) and the same call on
    the hosts; returns (dbs, hosts, (db, events, table, run))"""
    import dabamd
    fibs = np.asarray(fibs, np.uint8)
    n, nf = fibs.shape[:2]
    ok = np.ones((n, nf), np.uint8) if ok is None else np.asarray(ok, np.uint8)
    hosts = hosts or [F.Host() for _ in range(n)]
    out = dabamd.fib_parse(ctx, fibs, ok, dbs, want, event_slots, clear)
    for i, h in enumerate(hosts):
        if clear is not None and clear[i]:
            h.clearEnsemble()
        exp = h.feed(fibs[i], ok[i], want, event_slots)
        for got, e, name in zip(out, exp, NAMES):
            _same(got[i], e, (i, name))
    return out[0], hosts, out


def _stream(seed, n, overrun=0.15, noise=0.1):
    rng = np.random.default_rng(seed)
    return F.random_fibs(rng, n, F.pools(rng, seed), overrun=overrun, noise=noise)


@pytest.mark.parametrize("n_fibs", [1, 12, 37])
def test_three_slots_equal_the_host_class_call_after_call(ctx, n_fibs):
    """3 slots, each with a FIB stream of its own (well-formed, overrunning and random-byte
    FIBs), a few CRC-bad FIBs among them, over four consecutive calls on the carried databases"""
    streams = np.stack([_stream(100 * n_fibs + s, 4 * n_fibs) for s in range(3)])
    rng = np.random.default_rng(n_fibs)
    dbs = hosts = None
    for c in range(4):
        ok = (rng.random((3, n_fibs)) > 0.1).astype(np.uint8)
        dbs, hosts, out = _call(ctx, streams[:, c * n_fibs:(c + 1) * n_fibs], ok, hosts, dbs, want=60)
    if n_fibs > 1:
        assert out[3]["parsed"].sum() > 0 and sum(int(h.db()["services"]["inUse"].sum()) for h in hosts) > 6


def test_all_sixteen_want_flags(ctx):
    """the table for every combination of DABGPU_SUBCH_MP2 | PACKET | MOT | PAD, on a database
    with DAB+, layer II, packet and MOT components (and the table_changed flag between them)"""
    b = F._Bits().put(0, 3).put(1, 5)
    for sub in (1, 2, 3, 4):                   # FIG 0/1: four sub-channels, short form
        b.put(sub, 6).put(100 * sub, 10).put(0, 2).put(10 + sub, 6)
    f01 = F._fig(0, b.bytes())
    b = F._Bits().put(0, 3).put(2, 5).put(0x1111, 16).put(0, 4).put(4, 4)
    b.put(0, 2).put(63, 6).put(1, 6).put(0, 2)                    # DAB+ on 1
    b.put(0, 2).put(0, 6).put(2, 6).put(0, 2)                     # layer II on 2
    b.put(3, 2).put(10, 12).put(0, 2).put(3, 2).put(11, 12).put(0, 2)   # packet components SCId 10, 11
    f02 = F._fig(0, b.bytes())
    b = F._Bits().put(0, 3).put(3, 5)
    b.put(10, 12).put(0, 4).put(1, 1).put(0, 1).put(60, 6).put(3, 6).put(5, 10).put(0, 16)   # SCId 10: MOT on 3
    b.put(11, 12).put(0, 4).put(0, 1).put(0, 1).put(5, 6).put(4, 6).put(6, 10).put(0, 16)    # SCId 11: TDC on 4
    f03 = F._fig(0, b.bytes())
    fibs = np.stack([np.frombuffer(F.fib_of([f01, f02]), np.uint8), np.frombuffer(F.fib_of([f03]), np.uint8)])[None]
    fibs = np.concatenate([fibs, _stream(7, 10, overrun=0.0, noise=0.0)[None]], axis=1)
    dbs, hosts, out = _call(ctx, fibs, want=0)
    seen = set()
    for want in range(0, 64, 4):
        dbs, hosts, out = _call(ctx, np.zeros((1, 0, 32), np.uint8), None, hosts, dbs, want=want)
        seen.add(out[2][0]["sub"]["flags"].tobytes())
    assert len(seen) == 16                     # every combination gives a table of its own here


def test_one_call_of_36_equals_three_calls_of_12(ctx):
    fibs = np.stack([_stream(20 + s, 36) for s in range(2)])
    one, _, out1 = _call(ctx, fibs, want=60)
    dbs = hosts = None
    n_ev = np.zeros(2, np.int64)
    for c in range(3):
        dbs, hosts, out = _call(ctx, fibs[:, 12 * c:12 * c + 12], None, hosts, dbs, want=60)
        n_ev += out[3]["n_events"]
    for i in range(2):
        _same(dbs[i], one[i], i)
        _same(out[2][i], out1[2][i], i)
    assert (n_ev == out1[3]["n_events"]).all()


def test_permuting_the_slots_permutes_the_results(ctx):
    fibs = np.stack([_stream(40 + s, 24) for s in range(5)])
    a = _call(ctx, fibs, want=12)[2]
    perm = np.array([3, 0, 4, 1, 2])
    b = _call(ctx, fibs[perm], want=12)[2]
    for x, y in zip(a, b):
        assert x[perm].tobytes() == y.tobytes()


def test_fibs_with_ok_0_leave_no_trace(ctx):
    good = _stream(50, 12)
    noise = _stream(51, 12, noise=0.5)
    mixed = np.zeros((24, 32), np.uint8)
    mixed[0::2], mixed[1::2] = good, noise
    ok = np.zeros(24, np.uint8)
    ok[0::2] = 1
    a = _call(ctx, mixed[None], ok[None], want=60)[2]
    b = _call(ctx, good[None], want=60)[2]
    _same(a[0][0], b[0][0], "db")
    _same(a[2][0], b[2][0], "table")
    assert a[3][0]["skipped"] == 12 and a[3][0]["parsed"] == 12 and a[3][0]["n_events"] == b[3][0]["n_events"]
    assert (a[1][0]["fib"][:a[3][0]["n_events"]] == 2 * b[1][0]["fib"][:b[3][0]["n_events"]]).all()


def _fig0_17(sids, pty=3):
    b = F._Bits().put(0, 3).put(17, 5)
    for s in sids:
        b.put(s, 16).put(0, 8).put(0, 3).put(pty, 5)
    return F._fig(0, b.bytes())


def _fig1_1(sid, label=b"One more        "):
    return F._fig(1, bytes([0x01]) + sid.to_bytes(2, "big") + label + b"\xff\x00")


def test_full_service_table_then_one_more_sid(ctx):
    """64 services, then a FIG 1/1 and a FIG 0/17 for a 65th SId: find_service answers entry 0,
    which takes the name and the programme type"""
    fibs = [F.fib_of([_fig0_17(range(0x100 + 7 * k, 0x100 + 7 * k + 7))]) for k in range(10)]
    fibs += [F.fib_of([_fig1_1(0x9999)]), F.fib_of([_fig0_17([0x9998], pty=17)]), F.fib_of([_fig1_1(0x9997, b"Another         ")])]
    fibs = np.stack([np.frombuffer(f, np.uint8) for f in fibs])
    dbs, hosts, out = _call(ctx, fibs[None])
    s = dbs[0]["services"]
    assert s["inUse"].all() and s["serviceId"][0] == 0x100 and s["serviceId"][63] == 0x100 + 63
    assert bytes(s["label"][0]) == b"One more        " and s["programType"][0] == 17 and s["hasName"].sum() == 1
    assert out[3][0]["n_events"] == 1 and out[1][0]["id"][0] == 0 and out[1][0]["fib"][0] == 10


def _fig0_2(sid, n, asctys=63, subch=1):
    b = F._Bits().put(0, 3).put(2, 5).put(sid, 16).put(0, 4).put(n, 4)
    for i in range(n):
        b.put(0, 2).put(asctys, 6).put((subch + i) & 63, 6).put(0, 2)
    return F._fig(0, b.bytes())


def test_full_component_table(ctx):
    """72 bindings for 64 slots: the last eight write nothing (rule 2), their services exist"""
    fibs = np.stack([np.frombuffer(F.fib_of([_fig0_2(0x200 + k, 12, subch=12 * k)]), np.uint8) for k in range(6)])
    dbs, hosts, out = _call(ctx, fibs[None], want=32)
    c = dbs[0]["components"]
    assert c["inUse"].all() and c["service"][63] == 5 and c["componentNr"][63] == 3
    assert dbs[0]["services"]["inUse"].sum() == 6
    dbs, hosts, out = _call(ctx, fibs[None, ::-1], None, hosts, dbs, want=32)   # again: everything is bound or refused
    _same(dbs[0]["components"], c, "components")


def test_fig0_14_over_all_64_entries(ctx):
    """FIG 0/14 matches the SubChId field: in a new database (all 0) id 0 sets every entry; in a
    database whose entries carry their own ids it sets the ones named"""
    import dabamd
    f14 = lambda pairs: np.frombuffer(F.fib_of([F._fig(0, bytes([14]) + bytes((i << 2) | f for i, f in pairs))]), np.uint8)
    dbs, hosts, out = _call(ctx, f14([(0, 2), (9, 3)])[None, None])
    assert (dbs[0]["sub"]["FEC_scheme"] == 2).all()
    db = np.zeros(1, dabamd.FIC_DB_DTYPE)
    db[0]["sub"]["SubChId"] = np.arange(64)
    h = F.Host()
    h.load(db[0])
    dbs, hosts, out = _call(ctx, f14([(5, 1), (63, 3), (0, 2), (63, 1)])[None, None], None, [h], db)
    fec = dbs[0]["sub"]["FEC_scheme"]
    assert (fec[5], fec[63], fec[0], fec.sum()) == (1, 3, 2, 6)    # (the reference's `used < Length` leaves the last byte out)


def test_overrun_rule_on_the_two_stated_cases(ctx):
    """a FIG at byte 29 with length 31 and a FIG 0/2 with 15 components at the end of the data
    field: reads past bit 255 are zeros, each FIB is counted in overrun"""
    fibs = np.stack([np.frombuffer(f, np.uint8) for f, _ in F.STATED_OVERRUNS])
    dbs, hosts, out = _call(ctx, fibs[:, None, :])
    assert list(out[3]["overrun"]) == [n for _, n in F.STATED_OVERRUNS]
    assert out[2][0]["n"] == 2 and dbs[1]["components"]["inUse"].sum() == 15
    dbs, hosts, out = _call(ctx, fibs[None])                       # both in one slot: counted twice
    assert out[3][0]["overrun"] == 2


def test_two_event_slots_with_five_events(ctx):
    fibs = [F.fib_of([_fig1_1(0x300 + k, b"Service %-8d" % k)]) for k in range(4)]
    fibs.insert(2, F.fib_of([F._fig(1, bytes([0x00, 0xE0, 0x01]) + b"The Ensemble    " + b"\xff\x00")]))
    fibs = np.stack([np.frombuffer(f, np.uint8) for f in fibs])
    dbs, hosts, out = _call(ctx, fibs[None], event_slots=2)
    assert out[3][0]["n_events"] == 5 and out[1].shape == (1, 2) and list(out[1][0]["fib"]) == [0, 1]
    dbs, hosts, out = _call(ctx, fibs[None], event_slots=65)
    assert list(out[1][0]["kind"][:5]) == [2, 2, 1, 2, 2] and out[1][0]["id"][2] == 0xE001
    assert bytes(dbs[0]["label"]) == b"The Ensemble    " and dbs[0]["named"] == 1
    _call(ctx, fibs[None], event_slots=0)


def test_clear_keeps_language_and_programme_type(ctx):
    """dabgpu_fic_clear on the chosen slots only: components, subchannels, names go; language,
    programme type and hasLanguage stay and show in the entry's next service"""
    b = F._Bits().put(0, 3).put(17, 5).put(0x4321, 16).put(0, 2).put(1, 1).put(0, 1).put(0, 4).put(9, 8).put(0, 3).put(21, 5)
    f01 = F._fig(0, F._Bits().put(0, 3).put(1, 5).put(1, 6).put(0, 10).put(0, 2).put(20, 6).bytes())
    two = np.stack([np.frombuffer(F.fib_of([F._fig(0, b.bytes()), _fig1_1(0x4321)]), np.uint8),
                    np.frombuffer(F.fib_of([f01, _fig0_2(0x4321, 2)]), np.uint8)])
    dbs, hosts, out = _call(ctx, np.stack([two, two]), want=32)
    assert list(out[2]["n"]) == [1, 1] and out[2][0]["sub"]["flags"][0] == 33
    empty = np.zeros((2, 0, 32), np.uint8)
    dbs, hosts, out = _call(ctx, empty, None, hosts, dbs, want=32, clear=[1, 0])
    s = dbs["services"][:, 0]
    assert list(s["inUse"]) == [0, 1] and list(s["language"]) == [9, 9] and list(s["programType"]) == [21, 21]
    assert list(s["hasLanguage"]) == [1, 1] and not s["label"][0].any() and s["label"][1].any()
    assert list(dbs["components"]["inUse"].sum(axis=1)) == [0, 2] and list(out[3]["table_changed"]) == [1, 0]
    again = np.frombuffer(F.fib_of([_fig1_1(0x5555, b"New service     ")]), np.uint8)
    dbs, hosts, out = _call(ctx, np.stack([again, again])[:, None, :], None, hosts, dbs, want=32)
    assert dbs["services"][0, 0]["serviceId"] == 0x5555 and dbs["services"][0, 0]["language"] == 9


def test_guard_bytes_round_every_output_and_argument_checks(ctx):
    import dabamd
    L = dabamd.lib()
    n, nf, es, G = 3, 12, 4, 64
    fibs = np.stack([_stream(60 + s, nf, noise=0.3) for s in range(n)])
    sizes = [n * dabamd.FIC_DB_DTYPE.itemsize, n * nf * 32, n * nf, n * es * dabamd.FIC_EVENT_DTYPE.itemsize,
             n * dabamd.FIC_TABLE_DTYPE.itemsize, n * dabamd.FIC_RUN_DTYPE.itemsize]
    off, at = [], G
    for s in sizes:
        off.append(at)
        at += (s + 15) // 16 * 16 + G
    buf = ctx.buf(at).fill(0xA5)
    try:
        buf.upload_at(np.zeros(sizes[0], np.uint8), off[0]).upload_at(fibs, off[1]).upload_at(np.ones(n * nf, np.uint8), off[2])
        p = [C.c_void_p(buf.ptr.value + o) for o in off]
        assert L.dabgpu_fib_parse(ctx.h, p[0], n, p[1], 32 * nf, p[2], nf, 60, p[3], es, p[4], p[5]) == 0
        ctx.sync()
        raw = buf.download(np.uint8, at)
        used = np.zeros(at, bool)
        for o, s in zip(off, sizes):
            used[o:o + s] = True
        assert (raw[~used] == 0xA5).all()
        assert bytes(raw[off[1]:off[1] + sizes[1]]) == fibs.tobytes()          # the inputs are not written
        db = np.frombuffer(raw[off[0]:off[0] + sizes[0]].tobytes(), dabamd.FIC_DB_DTYPE)
        ev = np.frombuffer(raw[off[3]:off[3] + sizes[3]].tobytes(), dabamd.FIC_EVENT_DTYPE).reshape(n, es)
        for i in range(n):
            exp = F.Host().feed(fibs[i], np.ones(nf, np.uint8), 60, es)
            _same(db[i], exp[0], i)
            _same(ev[i], exp[1], i)            # the slots the call did not fill are zeroed, whatever they held
        # refused before anything is launched
        assert L.dabgpu_fib_parse(ctx.h, p[0], n, p[1], 32 * nf - 1, p[2], nf, 0, p[3], es, p[4], p[5]) == E_ARG
        assert L.dabgpu_fib_parse(ctx.h, p[0], -1, p[1], 32 * nf, p[2], nf, 0, p[3], es, p[4], p[5]) == E_ARG
        assert L.dabgpu_fib_parse(ctx.h, p[0], n, p[1], 32 * nf, p[2], -1, 0, p[3], es, p[4], p[5]) == E_ARG
        assert L.dabgpu_fib_parse(ctx.h, p[0], n, p[1], 32 * nf, p[2], nf, 0, p[3], -1, p[4], p[5]) == E_ARG
        assert L.dabgpu_fic_clear(ctx.h, p[0], -1, None) == E_ARG
        ctx.sync()
        assert (buf.download(np.uint8, at) == raw).all()
    finally:
        buf.free()
