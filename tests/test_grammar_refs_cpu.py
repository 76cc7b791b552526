"""CPU-only: the numpy restatements of tests/grammar_refs.py against torch on inputs masked with -inf beforehand."""
import numpy as np
import pytest
import torch

import grammar_refs as GR
from omr_a2s_multimodal_transformer_amd.grammar import Grammar

NINF = float("-inf")


def _case(rows, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((rows, V), generator=g) * 6 - 3).numpy()
    allowed = (torch.rand((rows, V), generator=g) < 0.5).numpy()
    allowed[:, 0] |= ~allowed.any(axis=1)                      # every row allows something
    return x, allowed


def _masked(x, allowed):
    return torch.from_numpy(x).masked_fill(~torch.from_numpy(allowed), NINF)


@pytest.mark.parametrize("V", [5, 257, 700])
def test_masked_argmax(V):
    x, allowed = _case(5, V, 3)
    x[1, :] = 0.5                                              # all equal: the first allowed index
    x[2, np.flatnonzero(allowed[2])[-2:]] = 9.0                # a tie between two allowed tokens
    x[3, np.flatnonzero(~allowed[3])[:1]] = np.nan             # NaN / +inf in forbidden columns only
    x[4, np.flatnonzero(~allowed[4])[:1]] = np.inf
    idx, val = GR.masked_argmax(x, allowed)
    want = _masked(x, allowed)
    assert idx.tolist() == torch.argmax(want, dim=1).tolist()
    assert val.tolist() == want.max(dim=1).values.tolist() and np.isfinite(val).all()
    assert allowed[np.arange(5), idx].all()
    assert idx[1] == np.flatnonzero(allowed[1])[0] and idx[2] == np.flatnonzero(allowed[2])[-2]


@pytest.mark.parametrize("V,k", [(5, 1), (30, 3), (700, 8)])
def test_masked_topk_log_softmax(V, k):
    x, allowed = _case(4, V, 7)
    allowed[0, :] = False
    allowed[0, [1, 3]] = True                                  # fewer than k allowed (k = 3, 8): forbidden tokens follow at -inf
    x[1, np.flatnonzero(~allowed[1])[:1]] = np.inf
    idx, val = GR.masked_topk_log_softmax(x, allowed, k)
    lp = torch.log_softmax(_masked(x, allowed), dim=1)
    tv, ti = torch.topk(lp, k, dim=1)
    live = np.isfinite(val)
    assert live.sum(axis=1).tolist() == [min(k, int(a.sum())) for a in allowed]
    assert idx[live].tolist() == ti.numpy()[live].tolist()                       # no ties among the random values
    np.testing.assert_allclose(val[live], tv.numpy()[live], rtol=0, atol=4e-6)      # a few fp32 roundings of values below 16 in size
    assert (val[~live] == NINF).all() and not allowed[0][idx[0][~live[0]]].any()
    # renormalised: the allowed log-probabilities sum to one
    full = GR.log_softmax32(GR.mask_logits(x, allowed))
    np.testing.assert_allclose(np.exp(full.astype(np.float64)).sum(axis=1), 1.0, atol=1e-5)


@pytest.mark.parametrize("alpha", [0.0, 0.3, 1.0])
def test_masked_weighted_mix(alpha):
    la, allowed = _case(4, 61, 11)
    lb, _ = _case(4, 61, 12)
    la[0, np.flatnonzero(~allowed[0])[:1]] = np.nan
    lb[1, np.flatnonzero(~allowed[1])[:1]] = np.inf
    p = GR.masked_weighted_mix(la, lb, allowed, alpha)
    want = alpha * torch.softmax(_masked(la, allowed), dim=1) + (1 - alpha) * torch.softmax(_masked(lb, allowed), dim=1)
    np.testing.assert_allclose(p, want.numpy(), rtol=0, atol=3e-7)                  # probabilities <= 1: a few roundings of 6e-8
    assert (p[~allowed] == 0).all() and np.isfinite(p).all()
    idx, val = GR.masked_weighted_topk(la, lb, allowed, alpha, 3)
    assert idx[:, 0].tolist() == torch.argmax(want, dim=1).tolist()
    np.testing.assert_allclose(val, np.log(np.take_along_axis(want.numpy(), idx, axis=1)), rtol=0, atol=1e-5)


def test_state_walk_and_allowed_mask_follow_the_grammar():
    g = Grammar([0, 1, 2, 2], [[1, -1, -1], [-1, 0, 2], [1, 0, -1]], 0, 1)
    for ids in ([0, 2, 0, 3, 1, 1], [0, 0, 2], [1], []):
        assert GR.state_walk(g.next, g.token_class, g.start, ids) == g.walk(ids)
    for s in range(g.S):
        assert GR.allowed_mask(g.next, g.token_class, s).tolist() == g.allowed(s).tolist()


def test_select_body_liveness_is_decided_by_the_table():
    """Two rows of beam 2; state 0 allows only token 2, so row 0's second candidate (a forbidden token at -inf) is dropped by the
    table although its parent is live, and no forbidden token is ever a survivor."""
    g = Grammar([0, 1, 2, 0], [[-1, -1, 1], [1, 0, 1]], 0, 1)
    idx, val = [[2, 0], [0, 3]], [[0.0, NINF], [-0.5, -1.0]]
    stopped, best, par, tok, sc, st = GR.select_body(idx, val, 2, 1, [0.0, -0.25], (NINF, 0, 0), 0, g.next, g.token_class, [0, 1])
    assert not stopped and par == [0, 1] and tok == [2, 0] and sc == [0.0, -0.75] and st == [1, 1]
    stopped, best, par, tok, sc, st = GR.select_body(idx, val, 2, 1, [0.0, NINF], (NINF, 0, 0), 0, g.next, g.token_class, [0, 1])
    assert not stopped and par == [0, 0] and tok == [2, 2] and sc == [0.0, NINF] and st == [1, 1]      # one survivor, one dead copy
    free = GR.select_body(idx, val, 2, 1, [0.0, NINF], (NINF, 0, 0), 0)
    assert free[3] == [2, 0] and free[4] == [0.0, NINF]          # without the table the -inf candidate survives


def test_host_beam_loop_with_a_permissive_grammar_is_the_plain_loop():
    """A three-token toy model whose logits depend on the last token only: the loop under a permissive grammar finds the
    sequence of the unconstrained search, and under a grammar that forbids the greedy favourite it avoids that token."""
    table = np.array([[0.0, -9.0, 2.0, 1.0], [0.0, 0.0, 0.0, 0.0], [0.0, 1.5, 0.0, 1.0], [0.0, 2.0, 0.5, 0.0]], dtype=np.float32)

    def step(tokens, parents):
        return table[np.asarray(tokens)]

    def topk(masked):
        return GR.masked_topk_log_softmax(masked, np.ones_like(masked, dtype=bool), 2)

    free = Grammar.permissive(4, 1, forbid=(0,))
    seq, score = GR.host_beam_loop(step, topk, 2, 0, 1, 6, free.next, free.token_class, free.start)
    assert seq[-1] == 1 and 0 not in seq and np.isfinite(score)
    strict = Grammar.permissive(4, 1, forbid=(0, 2))
    seq2, score2 = GR.host_beam_loop(step, topk, 2, 0, 1, 6, strict.next, strict.token_class, strict.start)
    assert 2 in seq and 2 not in seq2 and seq2[-1] == 1 and strict.accepts(seq2)
