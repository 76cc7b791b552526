"""The constrained pick and selection kernels (include/omr_hip.h "grammar-constrained decoding").  The criterion is exactness:
a constrained kernel on RAW logits equals the existing unconstrained kernel on logits the host masked with -inf beforehand, bit
for bit -- tokens, values, fp64 scores, parents, history -- and the states it writes equal the host walk.  Where a state allows
fewer tokens than the beam, the unconstrained selection lets forbidden tokens (at -inf) through; there the constrained one is
held to the restatement tests/grammar_refs.py select_body, fed with the unconstrained top-k of the masked rows."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import grammar_refs as GR  # noqa: E402
from test_beam_batch_gpu import NINF, _bits, _SelState  # noqa: E402

from omr_a2s_multimodal_transformer_amd import kernels as K  # noqa: E402
from omr_a2s_multimodal_transformer_amd._lib import cur_stream, lib, ptr  # noqa: E402
from omr_a2s_multimodal_transformer_amd.grammar import Grammar, _GrammarDesc  # noqa: E402

DEV = "cuda:0"
EOS = 1
VS, CS, SS = (5, 256, 257, 700), (2, 7, 256), (1, 3, 40)
PAD_VALUE = 1e9          # the ldv - V entries behind a row are never read: a value that would win every comparison


def _grammar(V, C, S, seed):
    """A random automaton of S states (+ sink) over C classes: <eos> (class C - 1, its own) is allowed in every state, class 0 in
    none (C >= 3), any other with probability 1/2 -- so every state allows a token and accepts, states differ in what they
    allow, and with C = 2 a state allows either everything or <eos> alone."""
    rng = np.random.default_rng(seed)
    tc = rng.integers(0, C - 1, size=V)
    tc[EOS] = C - 1
    nxt = np.where(rng.random((S, C)) < 0.5, rng.integers(0, S, size=(S, C)), -1).astype(np.int32)
    if C >= 3:
        nxt[:, 0] = -1
        tc[0], tc[2] = 0, 1                                   # classes 0 and 1 have a token whatever the draw
    nxt[:, C - 1] = 0
    g = Grammar(tc, nxt, 0, EOS)
    for s in range(g.S):
        assert g.allowed(s).any()                              # the constructor's guarantee: no row with everything forbidden
    return g


def _bind(g, states):
    cls, nxt = g.to(DEV)
    state = torch.tensor(states, dtype=torch.int32, device=DEV)
    d = _GrammarDesc()
    d.cls, d.next, d.state, d.S, d.C = cls.data_ptr(), nxt.data_ptr(), state.data_ptr(), g.S, g.C
    return d, state, (cls, nxt)


def _crafted_rows(g, states, V, seed):
    """One fp32 row per state -> (raw [rows, V], allowed [rows, V], the kinds that could be built).  Row r mod 5: 0 the
    unconstrained winner is forbidden; 1 a tie between two allowed tokens; 2 all allowed logits equal; 3 NaN and +inf in
    forbidden columns; 4 random."""
    rng = np.random.default_rng(seed)
    x = (rng.random((len(states), V)) * 6 - 3).astype(np.float32)
    allowed = np.stack([g.allowed(s) for s in states])
    kinds = set()
    for r in range(len(states)):
        ok, no = np.flatnonzero(allowed[r]), np.flatnonzero(~allowed[r])
        kind = r % 5
        if kind == 0 and no.size:
            x[r, no[-1]] = 50.0
            kinds.add("winner_forbidden")
        elif kind == 1 and ok.size >= 2:
            x[r, ok[-1]] = x[r, ok[ok.size // 2 - 1]] = 9.0
            kinds.add("tie")
        elif kind == 2:
            x[r, ok] = 0.5
            kinds.add("all_equal")
        elif kind == 3 and no.size:
            x[r, no[0]] = np.nan
            x[r, no[-1]] = np.inf
            kinds.add("nan_inf")
    return x, allowed, kinds


def _device_rows(x, ldv):
    """x on the device with row stride ldv, the padding full of PAD_VALUE."""
    out = torch.full((x.shape[0], ldv), PAD_VALUE, dtype=torch.float32)
    out[:, :x.shape[1]] = torch.from_numpy(x)
    return out.to(DEV)


def _i32(t):
    return t.view(torch.int32).cpu().tolist()


# ------------------------------------------------------------------------------------------------------------------ picks
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("V", VS)
def test_grammar_pick_equals_argmax_of_masked_logits(V, B):
    ldv, seen = V + 8, set()
    for C in CS:
        for S in SS:
            g = _grammar(V, C, S, 1000 * C + S)
            states = [(3 * r + 1) % g.S for r in range(5)]      # each row in a different state (as far as S goes)
            x, allowed, kinds = _crafted_rows(g, states, V, V + C + S)
            seen |= kinds if C >= 7 else set()
            raw, masked = _device_rows(x, ldv), _device_rows(GR.mask_logits(x, allowed), ldv)
            for r0 in (range(0, 5) if B == 1 else [0]):         # B = 1: every crafted row alone
                rows = slice(r0, r0 + B)
                d, state, _keep = _bind(g, states[rows])
                idx, val, tok = (torch.empty(B, dtype=dt, device=DEV) for dt in (torch.int64, torch.float32, torch.int64))
                lib().call("omr_grammar_pick", ptr(raw[rows]), ldv, B, V, ctypes.byref(d), ptr(idx), ptr(val), ptr(tok), cur_stream())
                want_idx, want_val = torch.empty_like(idx), torch.empty_like(val)
                lib().call("omr_argmax", ptr(masked[rows]), B, V, ldv, ptr(want_idx), ptr(want_val), cur_stream())
                ctx = (V, B, C, S, r0)
                assert idx.tolist() == want_idx.tolist() == tok.tolist(), ctx
                assert _i32(val) == _i32(want_val) and bool(torch.isfinite(val).all()), ctx
                ref_idx, ref_val = GR.masked_argmax(x[rows], allowed[rows])
                assert idx.tolist() == ref_idx.tolist() and val.cpu().numpy().tolist() == ref_val.tolist(), ctx
                assert allowed[rows][np.arange(B), ref_idx].all(), ctx
                assert state.tolist() == [g.walk([t], s)[0] for t, s in zip(idx.tolist(), states[rows])], ctx
                assert all(0 <= s < g.S for s in state.tolist()), ctx
    assert seen == {"winner_forbidden", "tie", "all_equal", "nan_inf"}


@pytest.mark.parametrize("V", VS)
def test_permissive_grammar_picks_what_the_unconstrained_kernels_pick(V):
    g = Grammar.permissive(V, EOS)
    rng = np.random.default_rng(V)
    ldv, B = V + 8, 5
    a, b = (_device_rows((rng.random((B, V)) * 6 - 3).astype(np.float32), ldv) for _ in range(2))
    a[2, :V] = 0.25                                            # a row of equal logits: index 0 on both sides
    d, state, _keep = _bind(g, [0] * B)
    idx, want_idx, tok = (torch.empty(B, dtype=torch.int64, device=DEV) for _ in range(3))
    val, want_val = (torch.empty(B, dtype=torch.float32, device=DEV) for _ in range(2))
    lib().call("omr_grammar_pick", ptr(a), ldv, B, V, ctypes.byref(d), ptr(idx), ptr(val), None, cur_stream())
    lib().call("omr_argmax", ptr(a), B, V, ldv, ptr(want_idx), ptr(want_val), cur_stream())
    assert idx.tolist() == want_idx.tolist() and _i32(val) == _i32(want_val)
    assert state.tolist() == [g.sink if t == EOS else 0 for t in idx.tolist()]
    state.zero_()
    lib().call("omr_weighted_grammar_pick", ptr(a), ldv, ptr(b), ldv, B, V, 0.3, ctypes.byref(d), ptr(idx), ptr(val), ptr(tok), cur_stream())
    lib().call("omr_weighted_argmax_rows", ptr(a), ldv, ptr(b), ldv, B, V, 0.3, ptr(want_idx), ptr(want_val), None, cur_stream())
    assert idx.tolist() == want_idx.tolist() == tok.tolist() and _i32(val) == _i32(want_val)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("V", VS)
def test_weighted_grammar_pick_equals_weighted_argmax_of_masked_logits(V, B):
    ldv, ldb = V + 8, V + 16
    for C in CS:
        for S in SS:
            g = _grammar(V, C, S, 2000 * C + S)
            states = [(3 * r + 2) % g.S for r in range(5)]
            xa, allowed, _ = _crafted_rows(g, states, V, 3 * V + C + S)
            xb, _, _ = _crafted_rows(g, states, V, 5 * V + C + S)
            raw_a, raw_b = _device_rows(xa, ldv), _device_rows(xb, ldb)
            msk_a, msk_b = _device_rows(GR.mask_logits(xa, allowed), ldv), _device_rows(GR.mask_logits(xb, allowed), ldb)
            for alpha in (0.0, 0.3, 1.0):
                for r0 in (range(0, 5) if B == 1 else [0]):
                    rows = slice(r0, r0 + B)
                    d, state, _keep = _bind(g, states[rows])
                    idx, want_idx, tok = (torch.empty(B, dtype=torch.int64, device=DEV) for _ in range(3))
                    prob, want_prob = (torch.empty(B, dtype=torch.float32, device=DEV) for _ in range(2))
                    lib().call("omr_weighted_grammar_pick", ptr(raw_a[rows]), ldv, ptr(raw_b[rows]), ldb, B, V, alpha, ctypes.byref(d), ptr(idx),
                               ptr(prob), ptr(tok), cur_stream())
                    lib().call("omr_weighted_argmax_rows", ptr(msk_a[rows]), ldv, ptr(msk_b[rows]), ldb, B, V, alpha, ptr(want_idx), ptr(want_prob),
                               None, cur_stream())
                    ctx = (V, B, C, S, alpha, r0)
                    assert idx.tolist() == want_idx.tolist() == tok.tolist(), ctx
                    assert _i32(prob) == _i32(want_prob) and bool(torch.isfinite(prob).all()), ctx
                    assert allowed[rows][np.arange(B), idx.cpu().numpy()].all(), ctx
                    p = GR.masked_weighted_mix(xa[rows], xb[rows], allowed[rows], alpha)
                    assert np.abs(p[np.arange(B), idx.cpu().numpy()] - p.max(axis=1)).max() <= 1e-6, ctx      # the restatement's maximum: p <= 1, a few roundings and two expf of 2 ulp on either side
                    assert state.tolist() == [g.walk([t], s)[0] for t, s in zip(idx.tolist(), states[rows])], ctx


def test_pick_entries_refuse_bad_descriptors():
    g = _grammar(30, 7, 3, 5)
    x = torch.zeros((2, 32), device=DEV)
    idx = torch.empty(2, dtype=torch.int64, device=DEV)
    for field, value in (("cls", None), ("next", None), ("state", None), ("C", 0), ("C", 257), ("S", 0)):
        d, _state, _keep = _bind(g, [0, 1])
        setattr(d, field, value)
        assert lib().query("omr_grammar_pick", ptr(x), 32, 2, 30, ctypes.byref(d), ptr(idx), None, None, cur_stream()) == -1, field
        assert lib().query("omr_weighted_grammar_pick", ptr(x), 32, ptr(x), 32, 2, 30, 0.5, ctypes.byref(d), ptr(idx), None, None, cur_stream()) == -1
    d, _state, _keep = _bind(g, [0, 1])
    assert lib().query("omr_grammar_pick", ptr(x), 32, 2, 30, None, ptr(idx), None, None, cur_stream()) == -1
    assert lib().query("omr_grammar_pick", ptr(x), 16, 2, 30, ctypes.byref(d), ptr(idx), None, None, cur_stream()) == -1      # ld < n
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- selections
def _selection_case(V, beam, weighted, g, seed):
    """N = 3 inputs: input 0 all rows live, input 1 done, input 2 with a dead last row (beam > 1).  -> everything a run needs."""
    N, rows = 3, 3 * beam
    rng = np.random.default_rng(seed)
    states = [int(s) for s in rng.integers(0, g.S - 1, size=rows)]      # never the sink: a live hypothesis has not taken <eos>
    x = [(rng.random((rows, V)) * 6 - 3).astype(np.float32) for _ in range(2 if weighted else 1)]
    allowed = np.stack([g.allowed(s) for s in states])
    for m in x:
        no = np.flatnonzero(~allowed[0])
        if no.size:
            m[0, no[0]], m[0, no[-1]] = np.nan, np.inf             # NaN / +inf in forbidden columns only
        m[beam - 1, EOS] = 4.0                                     # <eos> on top of a live row: a finished record, the search goes on
    scores = np.array([-0.5 * k for k in range(beam)] * 3, dtype=np.float64)
    if beam > 1:
        scores[3 * beam - 1] = NINF
    return N, states, x, allowed, scores, [0, 1, 0]


def _select(entry, logits, lds, V, alpha, st, d, t):
    args = [ptr(logits[0]), lds[0]] + ([ptr(logits[1]), lds[1]] if len(logits) == 2 else []) + [V] + ([alpha] if len(logits) == 2 else [])
    args += [ctypes.byref(st.bd)] + ([ctypes.byref(d)] if d is not None else []) + [t, cur_stream()]
    lib().call(entry, *args)
    torch.cuda.synchronize()
    return st.views(st.dev.cpu().numpy())


def _check_selection(V, beam, weighted, g, seed, t=4, max_len=7):
    N, states, x, allowed, scores, done = _selection_case(V, beam, weighted, g, seed)
    rows, lds = N * beam, [V + 8, V + 16]
    raw = [_device_rows(m, ld) for m, ld in zip(x, lds)]
    masked = [_device_rows(GR.mask_logits(m, allowed), ld) for m, ld in zip(x, lds)]
    tokens0 = list(range(2, 2 + rows))
    mk = lambda: _SelState(N, beam, max_len, EOS, scores, [NINF] * N, [0] * N, [0] * N, done, [1 - v for v in done], tokens0)
    # phase 1 of the yardstick: the unconstrained top-k kernels on the masked rows
    if weighted:
        idx, val = K.weighted_topk_logprob(masked[0][:, :V], masked[1][:, :V], 0.3, beam)
    else:
        idx, val = K.topk_logprob(masked[0][:, :V], beam)
    idx_h, val_h = idx.cpu().tolist(), val.cpu().tolist()
    d, state, _keep = _bind(g, states)
    st = mk()
    got = _select("omr_weighted_beam_select_grammar" if weighted else "omr_beam_select_grammar", raw, lds, V, 0.3, st, d, t)
    got_states = state.tolist()
    init = st.views(st.initial)
    scarce = went_on = False
    for n in range(N):
        r = slice(n * beam, (n + 1) * beam)
        ctx = (V, beam, weighted, g.C, g.S, n)
        if done[n]:
            for f in ("scores", "tokens", "parents"):
                assert got[f][r].tolist() == init[f][r].tolist(), ctx
            assert (got["hist_token"][:, r] == -7).all() and got_states[r] == states[r], ctx      # a done input's states are left alone
            continue
        live = [k for k in range(beam) if scores[n * beam + k] > NINF]
        scarce |= any(int(allowed[n * beam + k].sum()) < beam for k in live)
        stopped, bd, par, tok, sc, ns = GR.select_body(idx_h[r], val_h[r], beam, EOS, [float(s) for s in scores[r]], (NINF, 0, 0), t, g.next,
                                                       g.token_class, states[r])
        assert _bits([got["best_score"][n]]) == _bits([bd[0]]) and (int(got["best_row"][n]), int(got["best_pos"][n])) == (bd[1], bd[2]), ctx
        assert int(got["done"][n]) == int(stopped), ctx
        if stopped:
            assert got["tokens"][r].tolist() == tokens0[r] and got_states[r] == states[r] and (got["hist_token"][:, r] == -7).all(), ctx
            continue
        went_on = True
        assert got["parents"][r].tolist() == par and got["tokens"][r].tolist() == tok and _bits(got["scores"][r]) == _bits(sc), ctx
        assert got["hist_parent"][t, r].tolist() == par and got["hist_token"][t, r].tolist() == tok, ctx
        assert got_states[r] == ns, ctx
        for k in range(beam):                                    # no forbidden token in the history; slots beyond the allowed ones are dead
            assert g.walk([tok[k]], states[n * beam + par[k]])[0] == ns[k] >= 0, ctx
        n_live = sum(1 for s in sc if s > NINF)
        assert n_live <= sum(int(allowed[n * beam + k].sum()) for k in live), ctx
    # the existing kernel on the masked rows: bit for bit the same block, unless a live state allows fewer than `beam` tokens
    st2 = mk()
    want = _select("omr_weighted_beam_select" if weighted else "omr_beam_select", masked, lds, V, 0.3, st2, None, t)
    if not scarce:
        for f in got:
            assert got[f].tobytes() == want[f].tobytes(), (V, beam, weighted, f)
    return scarce, went_on


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("beam", [1, 3, 8])
@pytest.mark.parametrize("V", VS)
def test_constrained_selection_equals_the_unconstrained_one_on_masked_logits(V, beam, weighted):
    if beam > V:
        V = 9                                                   # the selection wants V >= beam: the smallest vocabulary for beam 8
    flags = [_check_selection(V, beam, weighted, _grammar(V, C, S, 3000 * C + S), 7 * V + beam) for C in CS for S in SS]
    if beam > 1:                                                # both regimes were met, and the search went on somewhere
        assert any(sc for sc, _ in flags) and any(go for _, go in flags) and (V < 256 or not all(sc for sc, _ in flags))


@pytest.mark.parametrize("weighted", [False, True])
def test_a_state_that_allows_one_token_leaves_one_live_slot(weighted):
    """Every hypothesis sits in a state that allows <eos> and ONE other token: after the selection exactly one slot per live
    parent can be live, the rest are dead copies of the first survivor, and no forbidden token is in the history."""
    V, beam = 30, 3
    tc = np.zeros(V, dtype=np.int64)
    tc[EOS], tc[7] = 1, 2
    g = Grammar(tc, [[-1, 0, 0]], 0, EOS)                       # state 0: class 2 (token 7) and <eos> only
    rng = np.random.default_rng(1)
    x = [(rng.random((3 * beam, V)) * 6 - 3).astype(np.float32) for _ in range(2 if weighted else 1)]
    for m in x:
        m[:, EOS] = -30.0
    lds = [V + 8, V + 16]
    raw = [_device_rows(m, ld) for m, ld in zip(x, lds)]
    scores = np.array([0.0] + [NINF] * (beam - 1) + [-0.5 * k for k in range(beam)] * 2)
    st = _SelState(3, beam, 6, EOS, scores, [NINF] * 3, [0] * 3, [0] * 3, [0] * 3, [1] * 3, [2] * (3 * beam))
    d, state, _keep = _bind(g, [0] * (3 * beam))
    got = _select("omr_weighted_beam_select_grammar" if weighted else "omr_beam_select_grammar", raw, lds, V, 0.3, st, d, 2)
    assert got["hist_token"][2].tolist() == [7] * (3 * beam) and got["tokens"].tolist() == [7] * (3 * beam)
    live = (got["scores"] > NINF).reshape(3, beam).sum(axis=1).tolist()
    assert live == [1, beam, beam] and state.tolist() == [0] * (3 * beam)
    assert got["parents"].reshape(3, beam)[0].tolist() == [0, 0, 0]


def test_permissive_grammar_selects_what_the_unconstrained_kernels_select():
    V, beam = 257, 3
    g = Grammar.permissive(V, EOS)
    rng = np.random.default_rng(9)
    x = [(rng.random((3 * beam, V)) * 6 - 3).astype(np.float32) for _ in range(2)]
    x[0][beam, EOS] = 20.0
    lds = [V + 8, V + 16]
    raw = [_device_rows(m, ld) for m, ld in zip(x, lds)]
    scores = np.array([-0.25 * k for k in range(beam)] * 3)
    mk = lambda: _SelState(3, beam, 6, EOS, scores, [NINF] * 3, [0] * 3, [0] * 3, [0, 0, 1], [1, 1, 0], [2] * (3 * beam))
    for weighted in (False, True):
        logits = raw if weighted else raw[:1]
        d, state, _keep = _bind(g, [0] * (3 * beam))
        got = _select("omr_weighted_beam_select_grammar" if weighted else "omr_beam_select_grammar", logits, lds, V, 0.3, mk(), d, 1)
        want = _select("omr_weighted_beam_select" if weighted else "omr_beam_select", logits, lds, V, 0.3, mk(), None, 1)
        for f in got:
            assert got[f].tobytes() == want[f].tobytes(), (weighted, f)
        assert state.tolist() == [0] * (3 * beam)
