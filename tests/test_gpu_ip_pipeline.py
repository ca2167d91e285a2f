"""The IP layer in the pipeline (dabgpu_pipe_ip): the function of the groups dabgpu_pipe_packet
delivered (that layer has its own tests in test_gpu_packet), against ip_py.Handler, exactly; the
counters carried across runs and across table changes; the sequence and table errors."""
import numpy as np
import pytest

import ip_py as ip

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -6
F = 6                              # as the packet pipeline tests
DABPLUS, PACKET, MOTF, IPF = 1, 8, 16, 64
TABLE = [(0, 12, 16, 0o103, 0, PACKET | IPF), (48, 48, 64, 0o103, 0, DABPLUS)]
RUNS = 4


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


def _subs(table):
    import dabamd
    return [dabamd.Subch(a, n, br, pl, 0 if uep else 1, fl) for a, n, br, pl, uep, fl in table]


def _code(fn):
    import dabamd
    with pytest.raises(dabamd.DabError) as e:
        fn()
    return e.value.code


@pytest.fixture(scope="module")
def tx():
    """two streams of one layout, 25 frames: an IP entry at 16 kbit/s beside a DAB+ entry"""
    from dabamd.synth import Ensemble, IP
    e = Ensemble(RUNS * F + 1, subch=[(0, 12, 16, 0o103, 0, 0, IP), (48, 48, 64, 0o103, 0, 1, 0)])
    return [e.generate(seed, truth=False)["iq"] for seed in (591, 592)]


def test_pipeline_layer_counters_and_errors(ctx, tx):
    """2 streams x 6 frames a run: three runs of the layer against the restatement over the groups
    the packet layer delivered, the counters carried from run to run; then the table changes"""
    import dabamd
    S = len(tx)
    lens = [len(x) // 2 for x in tx]
    buf = np.zeros((S, 2 * max(lens)), np.float32)
    for s, x in enumerate(tx):
        buf[s, :len(x)] = x
    diq = ctx.put(buf)
    p = dabamd.Pipeline(ctx, S, F, _subs(TABLE), max_packet=2)
    try:
        p.control(dabamd.CTL_ACQ_SYNC)
        hs = [ip.Handler() for _ in range(S)]
        assert _code(p.ip) == E_STATE                                   # no run yet
        for r in range(3):
            p.run(diq, max(lens), lens, partial=True)
            assert _code(p.ip) == E_STATE                               # before this run's dabgpu_pipe_packet
            p.dabplus()
            pk = p.packet()
            byts, groups, run, _ = pk
            out, results, ip_run = p.ip()
            assert _code(p.ip) == E_STATE                               # a second call
            gs = groups.shape[2]
            assert out.shape[2] == ip.arena_bytes(gs, byts.shape[2]) and results.shape == (S, 2, gs)
            for s in range(S):
                n = min(int(run[s, 0]["n_groups"]), gs)
                want, wout, wrun = hs[s].feed(groups[s, 0, :n], byts[s, 0], out.shape[2])
                assert np.array_equal(results[s, 0, :n], want), (r, s, results[s, 0, :n], want)
                assert ip_run[s, 0].tobytes() == wrun.tobytes(), (r, s, ip_run[s, 0], wrun)
                for g in want[want["status"] == ip.DELIVERED]:
                    o, nb = int(g["offset"]), int(g["nbytes"])
                    assert o % 16 == 0 and np.array_equal(out[s, 0, o:o + nb], wout[o:o + nb]), (r, s, o)
                assert not ip_run[s, 1].tobytes().strip(b"\x00")         # a slot without a flagged entry: zeroed, not walked
                st = p.ip_state(s)
                assert st[0].tobytes() == hs[s].state().tobytes() and st[1].tolist() == (0, 0), (r, s, st)
            # the packet outputs are as they were
            assert np.array_equal(p.pkb_d.download(np.uint8, pk[0].shape), pk[0])
            assert p.pkg_d.download(np.uint8, pk[1].nbytes).tobytes() == pk[1].tobytes()
            assert p.pkr_d.download(np.uint8, pk[2].nbytes).tobytes() == pk[2].tobytes()
        for s in range(S):                                              # there was something to carry: datagrams in more than one run
            assert len(hs[s].datagrams) >= 8 and hs[s].handled >= 10 and hs[s].crc_errors >= 1, (s, hs[s].state())
        # the table changes: an unchanged entry keeps its counters, a changed bitRate zeroes them
        p.set_subch(0, _subs(TABLE))
        p.set_subch(1, _subs([(0, 12, 8, 0o103, 0, PACKET | IPF), TABLE[1]]))
        assert p.ip_state(0)[0].tobytes() == hs[0].state().tobytes() and p.ip_state(1)[0].tolist() == (0, 0)
        assert _code(p.ip) == E_STATE                                   # the packet call of the old tables is gone
        # ... and so does dropping the flag; a table with IP and without PACKET, or with MOT, is refused
        assert _code(lambda: p.set_subch(0, _subs([(0, 12, 16, 0o103, 0, IPF), TABLE[1]]))) == E_ARG
        assert _code(lambda: p.set_subch(0, _subs([(0, 12, 16, 0o103, 0, PACKET | MOTF | IPF), TABLE[1]]))) == E_ARG
        assert p.ip_state(0)[0].tobytes() == hs[0].state().tobytes()    # (a refused table changes nothing)
        plain = [(0, 12, 16, 0o103, 0, PACKET), TABLE[1]]
        p.set_subch(-1, _subs(plain))
        assert p.ip_state(0)[0].tolist() == (0, 0) and p.ip_state(1)[0].tolist() == (0, 0)
        p.run(diq, max(lens), lens, partial=True)
        p.packet()
        assert _code(p.ip) == E_STATE                                   # no applied table flags an entry
    finally:
        p.close()
        diq.free()


def test_pipeline_without_a_packet_layer_and_bad_tables(ctx):
    import dabamd
    assert _code(lambda: dabamd.Pipeline(ctx, 1, F, _subs([(0, 12, 16, 0o103, 0, IPF), TABLE[1]]))) == E_ARG
    assert _code(lambda: dabamd.Pipeline(ctx, 1, F, _subs([(0, 12, 16, 0o103, 0, PACKET | MOTF | IPF), TABLE[1]]))) == E_ARG
    p = dabamd.Pipeline(ctx, 1, F, _subs(TABLE[1:]))
    try:
        assert p.max_packet == 0 and _code(p.ip) == E_STATE
        d = ctx.buf(4096)                                               # the library itself refuses, before it writes
        assert dabamd.lib().dabgpu_pipe_ip(p.h, d.ptr, d.ptr, d.ptr) == E_STATE
        st = np.zeros(1, ip.STATE_DTYPE)
        assert dabamd.lib().dabgpu_pipe_ip_state(p.h, 0, st.ctypes.data) == E_STATE
        assert dabamd.lib().dabgpu_pipe_ip(p.h, None, d.ptr, d.ptr) == E_ARG
        d.free()
    finally:
        p.close()
