"""Grammar-constrained decoding through whole models: every decode route under a small alternating automaton against host
loops that decode ONE position per call, read the logits back, mask them and pick on the host side (the unconstrained kernels on
masked logits, or numpy) -- the loop the constrained routes exist to avoid.  Tokens and scores are compared exactly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import grammar_refs as GR  # noqa: E402
from test_beam_batch_gpu import NO_DROP, SIZES, _multimodal, _transformer, rnd  # noqa: E402

from omr_a2s_multimodal_transformer_amd import kernels as K  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402
from omr_a2s_multimodal_transformer_amd.grammar import Grammar  # noqa: E402
from omr_a2s_multimodal_transformer_amd.metrics import compute_metrics  # noqa: E402
from omr_a2s_multimodal_transformer_amd.weighted_fusion import (weighted_beam_search, weighted_beam_search_batch, weighted_evaluate,  # noqa: E402
                                                                weighted_predict, weighted_prediction)

DEV = "cuda:0"
V, MAX_SEQ, EOS, SOS = 30, 20, 1, 2
AUDIO_SIZES = [(32, 600), (48, 720), (32, 96), (32, 520), (48, 880), (64, 400)]      # tests/test_weighted_beam_gpu.py
# <eos> head-bias changes (added, or taken off where every input ends as the model stands) tried until, UNDER the automaton, some input ends by <eos> and another runs out of positions
# (random-weight models answer all inputs much alike: the band in which that happens is narrow, hence the fine steps)
EOS_BIAS_STEPS = [round(0.05 * i, 2) for i in range(61)] + [3.5, 4.0, 5.0, 6.0, 8.0]


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def alternating(V=V):
    """Symbols (odd ids >= 3) and separators (even ids >= 4) alternate, a sequence begins with a symbol, <eos> comes only after a
    symbol, <PAD> / <sos> never appear: level 1 of kern_grammar over the synthetic vocabulary."""
    tc = np.array([3, 2, 3] + [i % 2 for i in range(3, V)])   # classes: 0 separator, 1 symbol, 2 <eos>, 3 forbidden
    return Grammar(tc, [[-1, 1, -1, -1], [0, -1, 0, -1]], 0, EOS)


def _ids(m, words):
    return [m.w2i[w] for w in words]


def _search_eos_bias(models, decode):
    """Move the <eos> head bias of `models` step by step -- up, or down where every input already ends -- until decode() (the
    host loop's constrained id lists) has inputs that end by <eos> before the budget beside inputs that run out of positions
    -> those lists.  Fails, never skips."""
    seen, before, sign = [], 0.0, 1.0
    for step in EOS_BIAS_STEPS:
        add = sign * step
        for m in models:
            m.decoder.out_layer.bias.omr_phys[EOS] += add - before
        before = add
        out = decode()
        ended = sum(ids[-1] == EOS and len(ids) < MAX_SEQ for ids in out)
        seen.append((add, ended))
        if 0 < ended < len(out):
            print(f"<eos> bias {add:+}: {ended} of {len(out)} inputs end by <eos>, lengths {[len(ids) for ids in out]}")
            return out
        if step == 0.0 and ended == len(out):
            sign = -1.0                                        # the count of ended inputs grows with the bias: look below
    raise AssertionError(f"no <eos> bias increment gave inputs that end by <eos> beside inputs that run out (increment, ended): {seen}")


def _host_greedy(m, mem, g):
    """One position per call on a batch-size-1 state: logits back, mask, arg-max (numpy) -> (ids, masked top-1 logits)."""
    st = m.decoder.init_decode(mem)
    tok, state, ids, vals = SOS, g.start, [], []
    for _ in range(m.max_seq_len):
        logits = st.step_logits(torch.tensor([[tok]], dtype=torch.int64, device=DEV)).cpu().numpy()
        idx, val = GR.masked_argmax(logits, g.allowed(state))
        tok = int(idx[0])
        state = g.walk([tok], state)[0]
        ids.append(tok)
        vals.append(float(val[0]))
        if tok == EOS:
            break
    return ids, vals


def _host_beam(models, mems, g, beam, alpha=None):
    """grammar_refs.host_beam_loop over the KV-cached step of one model (or two in lock-step: the weighted fusion), the top-k
    by the UNCONSTRAINED kernels on the masked logits."""
    states = [m.decoder.init_decode(mem) for m, mem in zip(models, mems)]
    for st in states:
        st.share_memory_between(beam)

    def step(tokens, parents):
        if parents is not None:
            for st in states:
                st.reorder_rows(torch.tensor(parents, dtype=torch.int64, device=DEV))
        tok = torch.tensor(tokens, dtype=torch.int64, device=DEV).view(beam, 1)
        out = tuple(st.step_logits(tok).cpu().numpy().reshape(beam, -1) for st in states)
        return out if len(out) == 2 else out[0]

    def topk(*masked):
        dev = [torch.from_numpy(x).to(DEV).contiguous() for x in masked]
        idx, val = K.topk_logprob(dev[0], beam) if len(dev) == 1 else K.weighted_topk_logprob(dev[0], dev[1], alpha, beam)
        return idx.cpu().tolist(), val.cpu().tolist()

    max_len = max(m.max_seq_len for m in models)
    return GR.host_beam_loop(step, topk, beam, SOS, EOS, max_len, g.next, g.token_class, g.start)


@pytest.fixture(scope="module")
def uni():
    """The tiny unimodal model, seven inputs (memories of 24 .. 450 tokens, one size twice), the automaton, and per input the host
    loop's constrained greedy result -- computed once, shared by the tests below."""
    with torch.no_grad():
        m = _transformer(ModelConfig(**NO_DROP), max_seq=MAX_SEQ)
        xs = [rnd((1, 1, h, w), 900 + i).to(DEV) for i, (h, w) in enumerate(SIZES + SIZES[3:4])]
        mems = [m.encode(x) for x in xs]
        g = alternating()
        _search_eos_bias([m], lambda: [_host_greedy(m, mem, g)[0] for mem in mems])
        host = [_host_greedy(m, mem, g) for mem in mems]
        free = m.predict(xs, batch_size=4)
    return m, xs, mems, g, host, free


def test_the_constraint_binds_and_every_output_is_valid(uni):
    m, xs, mems, g, host, free = uni
    assert any(not g.prefix_ok(_ids(m, seq)) for seq in free)          # precondition: unconstrained output breaks the grammar
    got = m.predict(xs, batch_size=4, grammar=g)
    assert got != free
    ended = 0
    for seq in got:
        ids = _ids(m, seq)
        assert g.prefix_ok(ids)
        if ids[-1] == EOS:
            assert g.accepts(ids)
            ended += 1
        else:
            assert len(ids) == MAX_SEQ                                 # the budget ran out before an accepting state: a valid prefix
    assert 0 < ended


def test_greedy_routes_equal_the_host_loop(uni):
    m, xs, mems, g, host, _ = uni
    want = [m._words([ids])[0] for ids, _ in host]
    for mem, w in zip(mems, want):
        assert m.greedy_batch(mem, grammar=g) == [w]                   # dense state, B = 1
    m.decode_grammar = g
    try:
        assert [m._greedy(mem)[0] for mem in mems] == want             # `_greedy` (validation_step's decode) under the attribute
        assert m.predict(xs, batch_size=4) == want
        assert m.predict(xs, batch_size=4, grammar=None) != want       # the keyword overrides the attribute, None included
    finally:
        m.decode_grammar = None
    assert m.greedy_batch(mems, grammar=g) == want                     # one ragged state (the 24-token memory alone)
    assert m.greedy_batch(mems, sync_every=1, grammar=g) == want       # n_steps = 1: the state crosses host calls too
    assert m.predict(xs, batch_size=3, grammar=g) == want              # groups of three rows, 8 positions per call
    assert m.predict(xs, batch_size=2, refill=True, grammar=g) == want     # two slots, seven inputs: refilled slots restart at `start`
    seen = []
    m._refill_state_hook = seen.append
    try:
        assert m.predict(xs, batch_size=2, refill=True, grammar=g) == want
    finally:
        m._refill_state_hook = None
    assert seen and seen[0].admitted > seen[0].B                       # slots were handed on


def test_predict_with_probs_returns_the_top_allowed_logit(uni):
    m, xs, mems, g, host, _ = uni
    words, probs = m.predict_with_probs(xs, batch_size=4, grammar=g)
    assert words == [m._words([ids])[0] for ids, _ in host]
    assert probs == [vals for _, vals in host]
    words2, probs2 = m.predict_with_probs(xs, batch_size=2, refill=True, grammar=g)
    assert (words2, probs2) == (words, probs)


def test_beam_routes_equal_the_host_beam_loop(uni):
    m, xs, mems, g, host, _ = uni
    greedy = [m._words([ids])[0] for ids, _ in host]
    assert [w for w, _ in m.beam_search_batch(mems, 1, grammar=g)] == greedy          # beam 1 is the constrained greedy decode
    want = [_host_beam([m], [mem], g, 4) for mem in mems]
    got = m.beam_search_batch(mems, 4, grammar=g)
    for i, ((ids, score), (words, s2)) in enumerate(zip(want, got)):
        assert words == m._words([ids])[0] and s2 == score, i
        assert g.prefix_ok(ids) and (ids[-1] != EOS or g.accepts(ids)), i
    assert m.predict(xs, batch_size=8, beam=4, grammar=g) == [w for w, _ in got]
    assert [m.beam_search(mem, 4, grammar=g) for mem in mems] == got                  # the host route of the model itself


def test_a_permissive_grammar_changes_nothing(uni):
    m, xs, mems, g, host, free = uni
    p = Grammar.permissive(V, EOS)
    assert m.predict(xs, batch_size=4, grammar=p) == free
    assert m.predict(xs, batch_size=2, refill=True, grammar=p) == free
    assert m.predict_with_probs(xs, batch_size=4, grammar=p) == m.predict_with_probs(xs, batch_size=4)
    assert m.greedy_batch(mems, grammar=p) == m.greedy_batch(mems)
    assert m.beam_search_batch(mems, 4, grammar=p) == m.beam_search_batch(mems, 4)
    assert m.beam_search(mems[0], 3, grammar=p) == m.beam_search(mems[0], 3)
    assert m.predict(xs, batch_size=8, beam=4, grammar=p) == m.predict(xs, batch_size=8, beam=4)


def test_evaluate_under_a_grammar(uni):
    m, xs, mems, g, host, _ = uni
    ys = [torch.tensor([[SOS] + [3 + (i + k) % 27 for k in range(4 + i)] + [EOS]]) for i in range(len(xs))]
    truth = [[m.ytest_i2w[t] for t in y[0][1:].tolist()] for y in ys]
    for kw in (dict(), dict(beam=4), dict(refill=True)):
        want = compute_metrics(y_true=truth, y_pred=m.predict(xs, batch_size=4, grammar=g, **kw))
        assert m.evaluate(list(zip(xs, ys)), batch_size=4, grammar=g, **kw) == want, kw
    with pytest.raises(ValueError, match="vocabulary"):
        m.predict(xs[:1], grammar=Grammar.permissive(V + 1, EOS))
    with pytest.raises(TypeError):
        m.predict(xs[:1], grammar="kern")


def test_multimodal_predict_equals_the_host_loop():
    m = _multimodal("concat", max_seq=MAX_SEQ)
    g = alternating()
    pairs = [(rnd((1, 1, hi, wi), 950 + i).to(DEV), rnd((1, 1, ha, wa), 960 + i).to(DEV))
             for i, ((hi, wi), (ha, wa)) in enumerate(zip(SIZES[:4], AUDIO_SIZES[:4]))]
    mems = [m._encode_input(p) for p in pairs]
    want = m._words(_search_eos_bias([m], lambda: [_host_greedy(m, mem, g)[0] for mem in mems]))
    free = m.predict(pairs, batch_size=4)
    assert any(not g.prefix_ok(_ids(m, seq)) for seq in free)
    assert m.predict(pairs, batch_size=4, grammar=g) == want
    assert m.predict(pairs, batch_size=2, refill=True, grammar=g) == want
    beams = m.predict(pairs, batch_size=8, beam=4, grammar=g)
    assert beams == [m._words([_host_beam([m], [mem], g, 4)[0]])[0] for mem in mems]
    assert all(g.prefix_ok(_ids(m, seq)) for seq in beams)


def test_the_generic_executor_decodes_under_a_grammar():
    """A feed-forward width the row kernel does not take (ff 2304 > 2048): the constrained pick stands where omr_argmax stood, the
    token reaches the next position through `tokens`; refill=True decodes in groups there; the beam runs the same executor."""
    m = _transformer(ModelConfig(ff_dim=2304, **NO_DROP), max_seq=MAX_SEQ)
    assert not m.decoder.takes_slot_state()
    g = alternating()
    xs = [rnd((1, 1, h, w), 990 + i).to(DEV) for i, (h, w) in enumerate(SIZES[:4])]
    mems = [m.encode(x) for x in xs]
    want = m._words(_search_eos_bias([m], lambda: [_host_greedy(m, mem, g)[0] for mem in mems]))
    assert any(not g.prefix_ok(_ids(m, seq)) for seq in m.predict(xs, batch_size=4))
    assert m.predict(xs, batch_size=4, grammar=g) == want
    assert m.predict(xs, batch_size=2, refill=True, grammar=g) == want
    assert m.greedy_batch(mems, sync_every=3, grammar=g) == want
    beams = m.beam_search_batch(mems, 3, grammar=g)
    assert beams == [(m._words([ids])[0], score) for ids, score in (_host_beam([m], [mem], g, 3) for mem in mems)]


# ------------------------------------------------------------------------------------------------ weighted late fusion
def _host_weighted_greedy(mi, ma, mem_i, mem_a, g, alpha):
    """Both models one position per call, both logit rows masked, the pick by the unconstrained mixing kernel."""
    sts = [mi.decoder.init_decode(mem_i), ma.decoder.init_decode(mem_a)]
    tok, state, ids = SOS, g.start, []
    for _ in range(max(mi.max_seq_len, ma.max_seq_len)):
        t = torch.tensor([[tok]], dtype=torch.int64, device=DEV)
        rows = [GR.mask_logits(st.step_logits(t).cpu().numpy(), g.allowed(state)) for st in sts]
        idx, _ = K.weighted_argmax_rows(torch.from_numpy(rows[0]).to(DEV), torch.from_numpy(rows[1]).to(DEV), alpha)
        tok = int(idx.item())
        state = g.walk([tok], state)[0]
        ids.append(tok)
        if tok == EOS:
            break
    return ids


@pytest.fixture(scope="module")
def pair_models():
    with torch.no_grad():
        mi = _transformer(ModelConfig(**NO_DROP), max_seq=MAX_SEQ, seed=61)
        ma = _transformer(ModelConfig(**NO_DROP), max_seq=MAX_SEQ, hw=(64, 900), seed=67)
        pairs = [(rnd((1, 1, hi, wi), 970 + i).to(DEV), rnd((1, 1, ha, wa), 980 + i).to(DEV))
                 for i, ((hi, wi), (ha, wa)) in enumerate(zip(SIZES, AUDIO_SIZES))]
        mems = [(mi.encode(xi), ma.encode(xa)) for xi, xa in pairs]
        g = alternating()
        _search_eos_bias([mi, ma], lambda: [_host_weighted_greedy(mi, ma, a, b, g, 0.3) for a, b in mems])
    return mi, ma, pairs, mems, g


@pytest.mark.parametrize("alpha", [0.0, 0.3, 1.0])
def test_weighted_routes_equal_their_host_restatements(pair_models, alpha):
    mi, ma, pairs, mems, g = pair_models
    want = [mi._words([_host_weighted_greedy(mi, ma, a, b, g, alpha)])[0] for a, b in mems]
    free = weighted_predict(pairs, mi, ma, alpha, batch_size=4)
    assert any(not g.prefix_ok(_ids(mi, seq)) for seq in free)
    assert weighted_predict(pairs, mi, ma, alpha, batch_size=4, grammar=g) == want
    assert weighted_predict(pairs, mi, ma, alpha, batch_size=2, refill=True, grammar=g) == want
    assert weighted_prediction(pairs[1][0], pairs[1][1], mi, ma, alpha, grammar=g) == want[1]
    assert all(g.prefix_ok(_ids(mi, seq)) for seq in want)
    beam_want = [_host_beam([mi, ma], [a, b], g, 3, alpha) for a, b in mems]
    words = [mi._words([ids])[0] for ids, _ in beam_want]
    assert weighted_predict(pairs, mi, ma, alpha, batch_size=6, beam=3, grammar=g) == words
    got = weighted_beam_search_batch([a for a, _ in mems], [b for _, b in mems], mi, ma, alpha, 3, grammar=g)
    assert got == [(w, s) for w, (_, s) in zip(words, beam_want)]
    assert weighted_beam_search(pairs[2][0], pairs[2][1], mi, ma, alpha, 3, grammar=g) == got[2]      # a 24-token memory: the host route


def test_weighted_permissive_and_evaluate(pair_models):
    mi, ma, pairs, mems, g = pair_models
    p = Grammar.permissive(V, EOS)
    for kw in (dict(), dict(refill=True), dict(beam=3)):
        assert weighted_predict(pairs, mi, ma, 0.3, batch_size=4, grammar=p, **kw) == weighted_predict(pairs, mi, ma, 0.3, batch_size=4, **kw), kw
    mi_list, ma_list = [a for a, _ in mems], [b for _, b in mems]
    assert weighted_beam_search_batch(mi_list, ma_list, mi, ma, 0.3, 3, grammar=p) == weighted_beam_search_batch(mi_list, ma_list, mi, ma, 0.3, 3)
    ys = [torch.tensor([[SOS] + [3 + (i + k) % 27 for k in range(4 + i)] + [EOS]]) for i in range(len(pairs))]
    truth = [[mi.ytest_i2w[t] for t in y[0][1:].tolist()] for y in ys]
    batches = [(xi, xa, y) for (xi, xa), y in zip(pairs, ys)]
    sweep = weighted_predict(pairs, mi, ma, [0.3, 1.0], batch_size=4, grammar=g)          # a sweep: the states rewind to `start` per alpha
    assert sweep[1.0] == weighted_predict(pairs, mi, ma, 1.0, batch_size=4, grammar=g)
    assert weighted_evaluate(batches, mi, ma, 0.3, batch_size=4, grammar=g) == compute_metrics(y_true=truth, y_pred=sweep[0.3])
    mi.decode_grammar = g
    try:
        assert weighted_predict(pairs, mi, ma, 0.3, batch_size=4) == sweep[0.3]           # the image model's attribute is the fallback
    finally:
        mi.decode_grammar = None
