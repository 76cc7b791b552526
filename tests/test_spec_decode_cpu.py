"""CPU-only: speculative greedy decoding without a GPU -- the acceptance rule restated in numpy against hand-written cases, the
host driver (evaluation.decode_spec) against a fake pair of models that replays fixed sequences, every refusal of the new C
entries (no case gets as far as a launch: the device pointers inside the descriptors stay NULL), and the ValueErrors of the
`draft=` keywords, which answer before the route or the hardware is looked at."""
import ctypes

import numpy as np
import pytest

import spec_refs as R
from omr_a2s_multimodal_transformer_amd import _lib
from omr_a2s_multimodal_transformer_amd.decoder import MAX_DRAFT_LEN, _DecodeDesc, _SpecDesc
from omr_a2s_multimodal_transformer_amd.evaluation import decode_spec

ARG, UNSUPPORTED = -1, -3
EOS, SOS = 1, 2


# ------------------------------------------------------------------------------------------------------------ the accept rule
def _one(tokens, picks, k, max_out=20, out_len=1, done=0):
    st = R.new_state(1, max_out, [tokens[0]], SOS, EOS)
    st["out_len"][0] = st["pos"][0] = out_len
    st["done"][0] = done
    top1 = np.arange(k + 1, dtype=np.float32)[None] + 0.5
    R.accept(np.array([tokens], np.int64), np.array([picks], np.int64), top1, st, k, EOS, max_out)
    n = int(st["out_len"][0]) - out_len
    return st, st["out_tokens"][0, out_len:out_len + n].tolist(), st["out_top1"][0, out_len:out_len + n].tolist()


def test_accept_rule_hand_written_cases():
    # j = 0: the first proposal is wrong -> one token, the target's own pick
    st, new, vals = _one([10, 11, 12, 13], [21, 22, 23, 24], 3)
    assert new == [21] and vals == [0.5] and st["accepted"][0] == 0 and st["pos"][0] == 2 and st["first"][0] == 21 and st["prev"][0] == 10
    assert st["totals"].tolist() == [3, 0] and st["done"][0] == 0
    # j = 2 of 3
    st, new, _ = _one([10, 21, 22, 99], [21, 22, 23, 24], 3)
    assert new == [21, 22, 23] and st["accepted"][0] == 2 and st["pos"][0] == 4 and st["first"][0] == 23 and st["prev"][0] == 22
    # a later match after a mismatch does not count
    st, new, _ = _one([10, 99, 22, 23], [21, 22, 23, 24], 3)
    assert new == [21] and st["accepted"][0] == 0
    # j = k: everything accepted, k + 1 tokens (the last one is the pick after the last proposal)
    st, new, vals = _one([10, 21, 22, 23], [21, 22, 23, 24], 3)
    assert new == [21, 22, 23, 24] and vals == [0.5, 1.5, 2.5, 3.5] and st["accepted"][0] == 3 and st["totals"].tolist() == [3, 3]
    assert st["first"][0] == 24 and st["prev"][0] == 23 and st["pos"][0] == 5
    # <eos> inside the accepted prefix: the run is cut after it and the slot is done; j still counts the matches
    st, new, _ = _one([10, 21, EOS, 23], [21, EOS, 23, 24], 3)
    assert new == [21, EOS] and st["done"][0] == 1 and st["accepted"][0] == 3 and st["pos"][0] == 3
    # <eos> as the first rejected pick is kept too (it is the target's own token)
    st, new, _ = _one([10, 21, 99, 23], [21, EOS, 23, 24], 3)
    assert new == [21, EOS] and st["done"][0] == 1 and st["accepted"][0] == 1
    # the run's capacity cuts as well
    st, new, _ = _one([10, 21, 22, 23], [21, 22, 23, 24], 3, max_out=6, out_len=4)
    assert new == [21, 22] and st["done"][0] == 1 and st["out_len"][0] == 6
    # a finished slot is frozen
    st, new, _ = _one([10, 21, 22, 23], [21, 22, 23, 24], 3, out_len=5, done=1)
    assert new == [] and st["pos"][0] == 5 and st["totals"].tolist() == [0, 0] and st["done"][0] == 1


# ------------------------------------------------------------------------------------------------------------ the host driver
def _sequences(budget):
    rng = np.random.RandomState(5)
    truth = [rng.randint(3, 30, size=budget + 8).tolist() for _ in range(4)]
    truth[0][17] = EOS                 # ends early
    truth[1][0] = EOS                  # ends at position 0
    truth[2][budget - 2] = EOS         # ends inside the plain-step tail (or the last cycle)
    guess = [list(seq) for seq in truth]            # row 0: a perfect draft; the others wrong at scattered positions
    for b in (1, 2, 3):
        for t in range(2 + b, budget, 3 + b):
            guess[b][t] = 31
    return truth, guess


def _expected(truth, budget):
    out = []
    for seq in truth:
        seq = seq[:budget]
        out.append(seq[:seq.index(EOS) + 1] if EOS in seq else seq)
    return out


@pytest.mark.parametrize("k", [1, 2, 4, 7])
@pytest.mark.parametrize("sync_every", [1, 3, 50])
def test_driver_gives_the_same_outputs_for_any_k_and_sync_every(k, sync_every):
    budget = 60
    truth, guess = _sequences(budget)
    fake = R.Replay(truth, guess, k, EOS, budget)
    out, values = decode_spec(fake.first(), fake.cycles, fake.plain, 4, EOS, budget, k + 1, sync_every, want_probs=True)
    assert out == _expected(truth, budget)
    assert values == [[1000.0 * b + t for t in range(len(seq))] for b, seq in enumerate(out)]
    assert len(out[3]) == budget and out[3][-1] != EOS                # one row runs into the budget ...
    assert all(c[1] <= sync_every for c in fake.calls)
    fake = R.Replay(truth, guess, k, EOS, budget)                      # without values: the same tokens, empty value lists
    out2, values2 = decode_spec(fake.first(), fake.cycles, fake.plain, 4, EOS, budget, k + 1, sync_every)
    assert out2 == out and values2 == [[], [], [], []]


def test_driver_edges():
    truth, guess = _sequences(12)
    fake = R.Replay(truth, guess, 3, EOS, 12)
    assert decode_spec(fake.first(), fake.cycles, fake.plain, 4, EOS, 0, 4, 2) == ([[], [], [], []], [[], [], [], []])
    fake = R.Replay(truth, guess, 3, EOS, 1)
    out, _ = decode_spec(fake.first(), fake.cycles, fake.plain, 4, EOS, 1, 4, 2)
    assert out == [seq[:1] for seq in truth] and fake.calls == []
    fake = R.Replay(truth, guess, 3, EOS, 3)              # budget < 1 + R: no cycle fits, plain steps only
    out, _ = decode_spec(fake.first(), fake.cycles, fake.plain, 4, EOS, 3, 4, 2)
    assert out == _expected(truth, 3) and all(c[0] == "plain" for c in fake.calls)
    with pytest.raises(ValueError):
        decode_spec(fake.first(), fake.cycles, fake.plain, 4, EOS, 3, 1, 2)
    # a perfect draft, k = 3, budget 10: positions 1 -> 5 -> 9 by two cycles, then no cycle fits and ONE plain step ends the row
    seq = [[3 + t for t in range(20)]]
    fake = R.Replay(seq, seq, 3, EOS, 10)
    out, _ = decode_spec(fake.first(), fake.cycles, fake.plain, 1, EOS, 10, 4, 8)
    assert out == [seq[0][:10]] and fake.calls == [("cycles", 2, 1), ("plain", 1, [9])]


# ------------------------------------------------------------------------------------------------------------ the C entries
_HOST = ctypes.create_string_buffer(1 << 20)
P = ctypes.addressof(_HOST)


def desc(**kw):
    """Widths of a model the row kernel takes; every pointer NULL."""
    d = _DecodeDesc()
    vals = dict(dtype=_lib.BF16, B=3, L=2, d=128, nhead=4, ff=256, V=97, ldv=104, max_len=64, S=100, window=-1, fp8=0, cross_ld=512, cross_bs=51200)
    vals.update(kw)
    for key, v in vals.items():
        setattr(d, key, v)
    return d


def spec_desc(state=P, **kw):
    s = _SpecDesc()
    vals = dict(B=3, k=4, eos=EOS, max_out=64, t_max=1)
    vals.update(kw)
    for key, v in vals.items():
        setattr(s, key, v)
    s.state = state
    n = _lib.lib().query("omr_spec_workspace_bytes", ctypes.byref(s))
    s.state_bytes = max(n, 0)
    s.ws_t, s.ws_t_bytes = P, 1 << 40
    return s, n


def verify(d, R_=5, t_max=10, pos=P, tokens=P, out=P, ws=P, ws_bytes=1 << 40):
    return _lib.lib().query("omr_decode_verify_rows", None if d is None else ctypes.byref(d), None, pos, t_max, R_, tokens, out, None, ws, ws_bytes, None)


def test_verify_rows_refusals():
    assert verify(None) == ARG
    for bad in (dict(d=192), dict(d=1024), dict(ff=2304), dict(ff=200)):          # outside the row kernel: answered first, NULL pointers and all
        assert verify(desc(**bad), pos=None, tokens=None, out=None, ws=None, R_=0) == UNSUPPORTED
    for R_ in (-1, 0, 1, 33, 100):
        assert verify(desc(), R_=R_) == ARG
    assert verify(desc(), R_=5, t_max=60) == ARG and verify(desc(), R_=5, t_max=-1) == ARG          # t_max + R > max_len
    assert verify(desc(), R_=32, t_max=33) == ARG
    for null in ("pos", "tokens", "out", "ws"):
        assert verify(desc(), **{null: None}) == ARG
    assert verify(desc(), ws_bytes=16) == ARG
    assert verify(desc(S=64)) == UNSUPPORTED and verify(desc(S=65)) == ARG      # shared memory K|V: the key-split kernel (S > 64), before any launch
    assert verify(desc()) == ARG                        # nothing wrong but the NULL pointers inside the descriptor: refused, no launch
    assert verify(desc(B=0)) == ARG and verify(desc(ldv=96)) == ARG


def test_group_workspace_bytes():
    q = lambda d, R_: _lib.lib().query("omr_decode_group_workspace_bytes", None if d is None else ctypes.byref(d), R_)
    assert q(None, 4) == ARG
    for R_ in (0, 1, 33):
        assert q(desc(), R_) == ARG
    one = _lib.lib().query("omr_decode_workspace_bytes", ctypes.byref(desc()))
    assert one < q(desc(), 2) < q(desc(), 8) < q(desc(), 32)
    assert q(desc(B=6), 4) == _lib.lib().query("omr_decode_workspace_bytes", ctypes.byref(desc(B=24)))      # B * R rows of scratch


def test_spec_workspace_and_accept_refusals():
    assert _lib.lib().query("omr_spec_workspace_bytes", None) == ARG
    for bad in (dict(k=0), dict(k=32), dict(B=0), dict(max_out=0)):
        assert spec_desc(**bad)[1] == ARG
    s, n = spec_desc(state=None)
    assert n > 0
    offs = [int(getattr(s, f) or 0) for f in _SpecDesc.STATE_FIELDS]
    assert offs == sorted(offs) and len(set(offs)) == len(offs) and offs[0] == 0 and all(o % 256 == 0 for o in offs) and offs[-1] < n
    assert _lib.lib().query("omr_spec_workspace_bytes", ctypes.byref(s)) == n and MAX_DRAFT_LEN == 31
    accept = lambda sd: _lib.lib().query("omr_spec_accept", None if sd is None else ctypes.byref(sd), None)
    assert accept(None) == ARG and accept(s) == ARG                  # no state block
    s, n = spec_desc()
    s.state_bytes = n - 1
    assert accept(s) == ARG
    s, n = spec_desc()
    s.picks = s.tokens                                                # fields that are not the block's
    assert accept(s) == ARG
    s, n = spec_desc()
    s.k = 0
    assert accept(s) == ARG


def cycles(t, d, s, k=4, n=2):
    ref = lambda x: None if x is None else ctypes.byref(x)
    return _lib.lib().query("omr_spec_decode_cycles", ref(t), ref(d), None, None, ref(s), k, n, None)


def test_spec_decode_cycles_refusals():
    s, _ = spec_desc()
    assert cycles(None, desc(), s) == ARG and cycles(desc(), None, s) == ARG
    assert cycles(desc(d=192), desc(), None) == UNSUPPORTED and cycles(desc(), desc(ff=2304), None) == UNSUPPORTED
    assert cycles(desc(), desc(), None) == ARG
    assert cycles(desc(), desc(), s, k=3) == ARG                      # not the block's k
    assert cycles(desc(), desc(), s, n=0) == ARG
    assert cycles(desc(), desc(), spec_desc(t_max=0)[0]) == ARG       # position 0 belongs to the plain step
    assert cycles(desc(), desc(), spec_desc(t_max=55)[0]) == ARG      # 55 + 2 * 5 > 64
    assert cycles(desc(), desc(max_len=10), s) == ARG                 # the draft's table is the shorter one
    assert cycles(desc(B=4), desc(), s) == ARG and cycles(desc(), desc(V=98), s) == ARG
    assert cycles(desc(), desc(), spec_desc(eos=97)[0]) == ARG
    assert cycles(desc(S=64), desc(), s) == UNSUPPORTED and cycles(desc(), desc(S=10), s) == ARG      # the draft without mem_len takes any S
    s2, _ = spec_desc()
    s2.ws_t = None
    assert cycles(desc(), desc(), s2) == ARG
    assert cycles(desc(), desc(), s) == ARG                           # only the NULL pointers inside the descriptors are left: refused, no launch


# ------------------------------------------------------------------------------------------------------------ the keywords
def _models():
    from omr_a2s_multimodal_transformer_amd import model as M
    from omr_a2s_multimodal_transformer_amd import synthetic as syn
    from omr_a2s_multimodal_transformer_amd.config import ModelConfig
    w2i, i2w = syn.make_vocab(30)
    cfg = ModelConfig(d_model=128, ff_dim=256, num_layers=1)
    uni = lambda **kw: M.Transformer(64, 256, kw.pop("max_seq", 16), kw.pop("w2i", w2i), i2w, config=kw.pop("cfg", cfg))
    multi = lambda: M.MultimodalTransformer(64, 256, 64, 256, 16, w2i, i2w, config=cfg)
    return M, syn, ModelConfig, uni, multi


def test_draft_keyword_refusals_need_no_gpu():
    M, syn, ModelConfig, uni, multi = _models()
    target, draft = uni(), uni()
    xs = [object()]                                   # never encoded: every refusal comes first
    other_w2i, _ = syn.make_vocab(31)
    for call in (target.predict, target.predict_with_probs, target.evaluate):
        with pytest.raises(ValueError, match="vocabulary"):
            call(xs, draft=uni(w2i=other_w2i))
        for bad in (0, 32, -1, 2.0, True):
            with pytest.raises(ValueError, match="draft_len"):
                call(xs, draft=draft, draft_len=bad)
        with pytest.raises(ValueError, match="refill"):
            call(xs, draft=draft, refill=True)
        with pytest.raises(ValueError, match="grammar"):
            call(xs, draft=draft, grammar=object())
        with pytest.raises(ValueError, match="draft_source"):
            call(xs, draft=draft, draft_source="image")
        with pytest.raises(ValueError, match="draft_source"):
            call(xs, draft_source="image")
        with pytest.raises(ValueError, match="max_seq_len"):
            call(xs, draft=uni(max_seq=8))
        with pytest.raises(ValueError, match="Transformer"):
            call(xs, draft=object())
    for call in (target.predict, target.evaluate):
        with pytest.raises(ValueError, match="beam"):
            call(xs, draft=draft, beam=2)
    target.decode_grammar = object()
    with pytest.raises(ValueError, match="grammar"):
        target.predict(xs, draft=draft)
    target.decode_grammar = None
    with pytest.raises(ValueError, match="draft's decoder widths .d = 64"):
        target.predict(xs, draft=uni(cfg=ModelConfig(d_model=64, nhead=2, ff_dim=256, num_layers=1)))
    with pytest.raises(ValueError, match="target's decoder widths .d = 128, ff = 2304"):
        uni(cfg=ModelConfig(d_model=128, ff_dim=2304, num_layers=1)).predict(xs, draft=draft)
    pair = multi()
    for call in (pair.predict, pair.evaluate):
        with pytest.raises(ValueError, match="draft_source"):
            call(xs, draft=draft)
        with pytest.raises(ValueError, match="draft_source"):
            call(xs, draft=draft, draft_source="video")
        with pytest.raises(ValueError, match="draft_source"):
            call(xs, draft=multi(), draft_source="image")
    with pytest.raises(ValueError, match="MultimodalTransformer"):
        target.predict(xs, draft=multi())
    # the late-fusion calls: two models in lock-step, no draft for the pair yet -- ValueError, before anything is encoded
    from omr_a2s_multimodal_transformer_amd.late_fusion import sw_evaluate, sw_predict
    from omr_a2s_multimodal_transformer_amd.weighted_fusion import weighted_evaluate, weighted_predict
    for call in (weighted_predict, weighted_evaluate, sw_predict, sw_evaluate):
        with pytest.raises(ValueError, match="does not take draft="):
            call(xs, target, draft, draft=draft)
        with pytest.raises(ValueError, match="does not take draft="):
            call(xs, target, draft, draft_len=4)


def test_the_methods_keep_their_own_parameter_lists():
    import inspect
    M = _models()[0]
    for cls in (M.Transformer, M.MultimodalTransformer):
        for name in ("predict", "evaluate"):
            assert [p for p in inspect.signature(getattr(cls, name)).parameters][1:] in (["xs", "batch_size"], ["pairs", "batch_size"], ["batches", "batch_size"])
    assert M.Transformer.last_spec_stats is None
