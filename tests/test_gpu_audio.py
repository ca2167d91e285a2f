"""Audio output on the GPU (k_audio.hip): the batched operator dabgpu_audio_out, bit-exact against
the reference's own audioSink (the golden file tests/golden/sink_kat.npz) and against its numpy
restatement (sink_py, itself pinned to that file by test_sink_cpu).  Samples are compared as uint32
bit patterns, signs of zero included: there is no tolerance."""
import numpy as np
import pytest

import sink_py as sp
from test_sink_cpu import KAT, SWEEP, bits, kat_sequences

pytestmark = pytest.mark.gpu

E_ARG = -1
SENTINEL = np.float32(-7.5)


@pytest.fixture(scope="module")
def ctx():
    import dabamd
    c = dabamd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def kat():
    return np.load(KAT)


def _batch(chains):
    """chains of (rate, pcm) calls -> pcm [n_chains, chain_len, max_amount, 2], rates, amounts; short
    chains end in rate-0 slots"""
    cl = max(len(c) for c in chains)
    ma = max([len(p) for c in chains for _, p in c] + [1])
    pcm = np.zeros((len(chains), cl, ma, 2), np.int16)
    rates, amounts = np.zeros((len(chains), cl), np.int32), np.zeros((len(chains), cl), np.int32)
    for i, c in enumerate(chains):
        for j, (rate, p) in enumerate(c):
            pcm[i, j, :len(p)] = p
            rates[i, j], amounts[i, j] = rate, len(p)
    return pcm, rates, amounts


def _check(samples, n_out, i, calls, wants):
    """chain i of an operator call: the pairs written are `wants`, every other one keeps the sentinel"""
    for j, want in enumerate(wants):
        assert n_out[i, j] == len(want), (i, j, n_out[i, j], len(want))
        assert np.array_equal(bits(samples[i, j, :len(want)]), bits(want)), (i, j)
        assert (samples[i, j, len(want):] == SENTINEL).all(), (i, j)
    assert (n_out[i, len(wants):] == 0).all() and (samples[i, len(wants):] == SENTINEL).all()


def test_operator_equals_reference(ctx, kat):
    """each scripted sequence as one chain of one operator call; then the same sequences split over
    two calls with the state carried between them: the same samples and the same final state"""
    seqs = kat_sequences(kat)
    chains = [[(r, p) for r, p, _ in calls] for _, calls in seqs]
    samples, n_out, state = ctx.audio_out(*_batch(chains), fill=SENTINEL)
    for i, (name, calls) in enumerate(seqs):
        _check(samples, n_out, i, calls, [w for _, _, w in calls])
    cut = [max(1, len(c) // 2) for c in chains]
    s1, n1, st1 = ctx.audio_out(*_batch([c[:k] for c, k in zip(chains, cut)]), fill=SENTINEL)
    s2, n2, st2 = ctx.audio_out(*_batch([c[k:] for c, k in zip(chains, cut)]), state=st1, fill=SENTINEL)
    for i, (name, calls) in enumerate(seqs):
        wants = [w for _, _, w in calls]
        _check(s1, n1, i, calls[:cut[i]], wants[:cut[i]])
        _check(s2, n2, i, calls[cut[i]:], wants[cut[i]:])
    assert np.array_equal(st2, state)
    assert st1.any() and not np.array_equal(st1, st2)


def test_sweep_of_every_int16(ctx, kat):
    """all 65536 values through one rate-48000 call of 32768 pairs"""
    samples, n_out, state = ctx.audio_out(SWEEP[None, None], [[48000]], [[32768]])
    assert n_out[0, 0] == 32768 and np.array_equal(bits(samples[0, 0, :32768]), bits(kat["sweep48"]))
    assert not samples[0, 0, 32768:].any() and not state.any()          # a 48000 call touches no filter


def test_operator_equals_restatement(ctx):
    """8 random chains x 6 calls of mixed rates, rate-0 and amount-0 slots among them, max_amount 96,
    in two operator calls of 3 calls each with the state carried"""
    rng = np.random.default_rng(42)
    rates = rng.choice([16000, 24000, 32000, 48000, 0, 22050], (8, 6)).astype(np.int32)
    rates[0], rates[1, :3] = [24000, 0, 24000, 32000, 0, 32000], [16000, 16000, 0]
    amounts = 2 * rng.integers(0, 49, (8, 6)).astype(np.int32)
    odd = (rates != 32000) & (rng.random((8, 6)) < 0.5)
    amounts[odd] = np.maximum(amounts[odd] - 1, 0)
    amounts[2, 1], amounts[3, 4], amounts[4, 0], amounts[5, 2] = 0, 0, 96, 1
    pcm = rng.integers(-32768, 32768, (8, 6, 96, 2)).astype(np.int16)
    sinks = [sp.Sink() for _ in range(8)]
    state = None
    seen = set()
    for h in (0, 3):
        samples, n_out, state = ctx.audio_out(pcm[:, h:h + 3], rates[:, h:h + 3], amounts[:, h:h + 3], state=state, fill=SENTINEL)
        for i in range(8):
            wants = [sinks[i].audio_out(pcm[i, j, :amounts[i, j]], int(rates[i, j])) for j in range(h, h + 3)]
            _check(samples, n_out, i, None, wants)
            seen |= {(int(rates[i, j]), len(w) > 0) for j, w in zip(range(h, h + 3), wants)}
    assert {(r, True) for r in (16000, 24000, 32000, 48000, 22050)} <= seen and (0, False) in seen


def test_refusals_leave_everything_untouched(ctx):
    import dabamd
    pcm = np.ones((1, 2, 4, 2), np.int16)
    for rates, amounts in (([[32000, 24000]], [[3, 2]]), ([[24000, 24000]], [[5, 2]]), ([[24000, 16000]], [[2, -1]])):
        with pytest.raises(dabamd.DabError) as e:
            ctx.audio_out(pcm, rates, amounts)
        assert e.value.code == E_ARG
    # an odd amount in a rate-0 slot is no call
    samples, n_out, state = ctx.audio_out(pcm, [[0, 32000]], [[3, 2]], fill=SENTINEL)
    assert n_out.tolist() == [[0, 3]] and (samples[0, 0] == SENTINEL).all() and (samples[0, 1, 3:] == SENTINEL).all()
