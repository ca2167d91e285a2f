"""The FIC layer in the pipeline (dabgpu_pipe_fic, dabgpu_pipe_fic_caps, dabgpu_pipe_fic_db,
dabgpu_pipe_fic_clear): the layer is checked as the function of what dabgpu_pipe_run delivered
(the FIC decoder has its own tests): the run's FIBs and CRC flags, downloaded, go through the
host class dabgpu::fib_processor (tests/fib_py.Host), and everything the layer wrote -- events,
table, run record, the carried database -- is compared exactly.  Two streams of the transmitter
with FIGs and different layouts."""
import ctypes as C

import numpy as np
import pytest

import fib_py as F

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -6
NFR = 9
# (startAddr, CUs, bitRate, protLevel, uep flag of the transmitter, dabplus, content)
TX = [[(0, 24, 32, 0o103, 0, 1, 0), (24, 48, 64, 0o103, 0, 1, 0)],
      [(10, 84, 96, 2, 1, 0, 0), (100, 24, 32, 0o103, 0, 1, 0), (130, 24, 32, 0o103, 0, 1, 0)]]
CAPS = dict(max_subch=3, max_bitrate=96, max_dabplus=3)


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rig(ctx):
    from dabamd.synth import Ensemble
    iqs = [Ensemble(NFR, subch=tx, snr_db=25.0, figs=True).generate(91 + s, truth=False)["iq"] for s, tx in enumerate(TX)]
    lens = [len(x) // 2 for x in iqs]
    buf = np.zeros((2, 2 * max(lens)), np.float32)
    for s, x in enumerate(iqs):
        buf[s, :len(x)] = x
    r = dict(diq=ctx.put(buf), stride=max(lens), lens=lens)
    yield r
    r["diq"].free()


def _hand(s, flags=1):
    import dabamd
    return [dabamd.Subch(a, n, br, pl, 0 if uep else 1, flags if dp else 0) for a, n, br, pl, uep, dp, _ in TX[s]]


def _pipe(ctx, nf, packed=False):
    import dabamd
    p = dabamd.Pipeline(ctx, 2, nf, [], **CAPS)
    p.control(dabamd.CTL_ACQ_SYNC)
    if packed:
        p.set_packed(dabamd.PACK_FIC)
    return p


def _same(a, b, what):
    assert a.tobytes() == b.tobytes(), (what, [(n, a[n], b[n]) for n in a.dtype.names if a[n].tobytes() != b[n].tobytes()])


def _step(pipe, rig, hosts, want, packed):
    """one run and its FIC layer; the hosts fed the downloaded FIBs and CRC flags and compared"""
    fic, crc, msc, valid = pipe.run(rig["diq"], rig["stride"], rig["lens"], partial=True)
    ev, table, run = pipe.fic(want)
    S, nf = pipe.S, pipe.F
    fibs = fic.reshape(S, 12 * nf, 32) if packed else np.packbits(fic.reshape(S, 12 * nf, 256), axis=-1)
    for s, h in enumerate(hosts):
        exp = h.feed(fibs[s], crc[s].reshape(-1), want)
        for got, e, name in zip((pipe.fic_db(s), ev[s], table[s], run[s]), exp, ("db", "events", "table", "run")):
            _same(got, e, (s, pipe._run, name))
    return ev, table, run, crc


@pytest.mark.parametrize("packed", [False, True], ids=["bits", "packed"])
@pytest.mark.parametrize("nf", [2, 4])
def test_pipeline_fic_equals_host_class(ctx, rig, nf, packed):
    """9 frames in runs of 2 or 4, the FIC one bit per byte or DABGPU_PACK_FIC bytes: the databases
    are carried across the runs; the last run, where the streams run out of samples, commits fewer
    FIBs; the tables are the transmitter's, the names arrive once"""
    import dabamd
    pipe = _pipe(ctx, nf, packed)
    hosts = [F.Host(), F.Host()]
    try:
        pipe.fic_caps(True)
        n_events = np.zeros(2, int)
        for r in range((NFR + nf - 1) // nf):
            ev, table, run, crc = _step(pipe, rig, hosts, dabamd.SUBCH_PAD, packed)
            n_events += run["n_events"]
            if r == 0:
                assert (run["parsed"] == 12 * nf).all() and (run["table_changed"] == 1).all() and (run["overrun"] == 0).all()
                assert sorted(ev[0]["kind"][:3]) == [1, 2, 2] and sorted(ev[1]["kind"][:4]) == [1, 2, 2, 2]
                e = ev[0][:3][ev[0]["kind"][:3] == 1][0]
                assert e["id"] == 0xE1C3 and bytes(e["label"]) == b"SYNTH ENSEMBLE  " and 0 <= e["fib"] < 12
                assert sorted(bytes(x) for x in ev[1]["label"][:4]) == [b"SERVICE 00      ", b"SERVICE 01      ", b"SERVICE 02      ",
                                                                        b"SYNTH ENSEMBLE  "]
            else:
                assert (run["table_changed"] == 0).all()
        done = np.array([pipe.state(s).frames_run for s in range(2)])
        assert (done < nf).all() and (run["parsed"] == 12 * done).all() and (run["skipped"] == 12 * nf - run["parsed"]).all()
        assert list(n_events) == [1 + len(TX[0]), 1 + len(TX[1])]
        for s in range(2):
            got = dabamd.table_subch(table[s])
            assert [(e.startAddr, e.length, e.bitRate, e.protLevel, e.uepFlag, e.flags) for e in got] == \
                   [(e.startAddr, e.length, e.bitRate, e.protLevel, e.uepFlag, e.flags) for e in _hand(s, 33)]
            assert list(table[s]["ids"][:len(TX[s])]) == list(range(len(TX[s])))
    finally:
        pipe.close()


def test_state_errors_and_clear(ctx, rig):
    """DABGPU_E_STATE without the layer, without a run, on a second call for the same run and once
    the layer is off again; DABGPU_E_ARG for other buffers than the run's; clearEnsemble for one
    stream, after which its names arrive again"""
    import dabamd
    L = dabamd.lib()
    pipe = _pipe(ctx, 2)
    hosts = [F.Host(), F.Host()]
    ev_d, t_d, r_d = ctx.buf(2 * 65 * 32), ctx.buf(2 * 848), ctx.buf(2 * 64)
    call = lambda fic, crc: L.dabgpu_pipe_fic(pipe.h, fic.ptr, crc.ptr, 0, ev_d.ptr, t_d.ptr, r_d.ptr)
    db = np.zeros(1, dabamd.FIC_DB_DTYPE)
    try:
        with pytest.raises(dabamd.DabError) as ei:
            pipe.fic()
        assert ei.value.code == E_STATE
        pipe.run(rig["diq"], rig["stride"], rig["lens"])
        assert call(pipe.fic_d, pipe.crc_d) == E_STATE                         # no layer
        assert L.dabgpu_pipe_fic_db(pipe.h, 0, db.ctypes.data) == E_STATE and L.dabgpu_pipe_fic_clear(pipe.h, 0) == E_STATE
        pipe.fic_caps(True)
        assert call(pipe.fic_d, pipe.crc_d) == E_STATE                         # no run since the layer is on
        assert L.dabgpu_pipe_fic_db(pipe.h, 2, db.ctypes.data) == E_ARG and L.dabgpu_pipe_fic_clear(pipe.h, 2) == E_ARG
        fic, crc, _, _ = pipe.run(rig["diq"], rig["stride"], rig["lens"])
        assert call(pipe.crc_d, pipe.fic_d) == E_ARG                           # not the run's buffers
        assert call(pipe.fic_d, pipe.crc_d) == 0
        assert call(pipe.fic_d, pipe.crc_d) == E_STATE                         # a second call for the same run
        pipe.sync()
        fibs = np.packbits(fic.reshape(2, 24, 256), axis=-1)
        for s, h in enumerate(hosts):
            h.feed(fibs[s], crc[s].reshape(-1), 0)
            _same(pipe.fic_db(s), h.db(), s)
        pipe.fic_clear(0)
        hosts[0].clearEnsemble()
        for s, h in enumerate(hosts):
            _same(pipe.fic_db(s), h.db(), ("cleared", s))
        assert not pipe.fic_db(0)["services"]["inUse"].any() and pipe.fic_db(1)["services"]["inUse"].any()
        ev, table, run, _ = _step(pipe, rig, hosts, 0, False)
        assert list(run["n_events"]) == [1 + len(TX[0]), 0]
        pipe.fic_caps(False)
        pipe.run(rig["diq"], rig["stride"], rig["lens"], partial=True)
        assert call(pipe.fic_d, pipe.crc_d) == E_STATE
        pipe.fic_caps(True)                                                    # new databases
        assert not pipe.fic_db(1).tobytes().strip(b"\0")
    finally:
        pipe.close()
        for b in (ev_d, t_d, r_d):
            b.free()


def test_set_subch_from_the_device_table(ctx, rig):
    """two pipelines that start without a table: one is given each stream's table by hand after
    the first run, the other the table the FIC layer built from that run's FIBs: the same tables,
    and from then on the same MSC output, entry for entry"""
    import dabamd
    nf = 2
    pa, pb = _pipe(ctx, nf), _pipe(ctx, nf)
    try:
        pb.fic_caps(True)
        for p in (pa, pb):
            p.run(rig["diq"], rig["stride"], rig["lens"])
        ev, table, run = pb.fic(0)
        for s in range(2):
            pa.set_subch(s, _hand(s))
            pb.set_subch(s, dabamd.table_subch(table[s]))
            ta, tb = pa.get_subch(s), pb.get_subch(s)
            assert ta[1] == tb[1] and [bytes(x) for x in ta[0]] == [bytes(x) for x in tb[0]] and len(ta[0]) == len(TX[s])
        rows = 0
        for r in range(1, 4):
            oa = pa.run(rig["diq"], rig["stride"], rig["lens"])
            ob = pb.run(rig["diq"], rig["stride"], rig["lens"])
            pb.fic(0)
            va, vb = pa.msc_entry_valid(), pb.msc_entry_valid()
            assert np.array_equal(va, vb) and np.array_equal(oa[0], ob[0]) and np.array_equal(oa[1], ob[1])
            for s in range(2):
                for k, sc in enumerate(_hand(s)):
                    ok = va[s, :, k] != 0
                    assert np.array_equal(oa[2][s, ok, k, :24 * sc.bitRate], ob[2][s, ok, k, :24 * sc.bitRate]), (r, s, k)
                    rows += int(ok.sum())
        assert rows > 0
    finally:
        pa.close()
        pb.close()
