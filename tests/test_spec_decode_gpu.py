"""Speculative greedy decoding against the one-position route the reference runs (src/transformer/model.py:171-199, 226-262): a
grouped position (omr_decode_verify_rows) and the acceptance (omr_spec_accept) against omr_decode_steps_rows, and predict /
predict_with_probs / evaluate with draft= against the same calls without one.  Every comparison is exact: token ids are equal,
top-1 values and cache rows are compared as bits.  Tiny models: d = 128, 4 heads, ff = 256, V = 97, max_len = 300; target of 2
layers, draft of 1."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from omr_a2s_multimodal_transformer_amd import decoder as D  # noqa: E402
from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd._lib import cur_stream, lib, ptr  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402

DEV = "cuda:0"
V, MAX_SEQ = 97, 300
NAN = float("nan")
# image sizes -> memory lengths ceil(H/16) * ceil(W/8): 70, 300 and 128 keys
SIZES = [(32, 280), (32, 1200), (32, 512)]


def rnd(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _cfg(layers, dtype="fp32", fp8=False):
    return ModelConfig(d_model=128, nhead=4, ff_dim=256, num_layers=layers, compute_dtype=dtype, fp8_decode=fp8, dropout=0.0, encoder_dropout=0.0)


def _transformer(cfg, win=-1, seed=61):
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    w2i, i2w = syn.make_vocab(V)
    m = Transformer(64, 1600, MAX_SEQ, w2i, i2w, attn_window=win, config=cfg)
    m.load_state_dict(syn.seeded_state_dict(syn.transformer_shapes(V, cfg.d_model, cfg.ff_dim, cfg.num_layers), seed), strict=False)
    m.flatten_parameters()
    m.eval()
    return m


def _multimodal(cfg, seed=71):
    from omr_a2s_multimodal_transformer_amd.model import MultimodalTransformer
    w2i, i2w = syn.make_vocab(V)
    m = MultimodalTransformer(64, 1200, 64, 900, MAX_SEQ, w2i, i2w, mixer_type="concat", config=cfg)
    m.load_state_dict(syn.seeded_state_dict(syn.multimodal_shapes(V, "concat", cfg.d_model, cfg.ff_dim, cfg.num_layers), seed), strict=False)
    m.flatten_parameters()
    m.eval()
    return m


def _head_bias(m):
    return m.decoder.out_layer.bias.omr_phys


def _inputs():
    return [rnd((1, 1) + s, 900 + i).to(DEV) for i, s in enumerate(SIZES)]


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------- verify + accept against the sequential route
POS = [58, 250, 3]           # groups of up to 8 rows straddle the 64-key (58 .. 65) and the 256-key (250 .. 257) boundary of the split
N_SEQ = 262


@pytest.mark.parametrize("dtype,fp8", [("fp32", False), ("bf16", False), ("bf16", True)])
@pytest.mark.parametrize("win", [-1, 5])
def test_grouped_position_and_accept_equal_the_sequential_route(dtype, fp8, win):
    m, draft = _transformer(_cfg(2, dtype, fp8), win), _transformer(_cfg(1, dtype), win, seed=77)
    dec, sos, eos = m.decoder, m.w2i["<sos>"], m.w2i["<eos>"]
    _head_bias(m)[eos] = -1e4                                  # the run never ends: every position has a successor to compare with
    xs = _inputs()
    mems, dmems = [m.encode(x) for x in xs], [draft.encode(x) for x in xs]
    assert [x.shape[1] for x in mems] == [70, 300, 128]
    B = 3
    # the true greedy run g: N_SEQ positions of every slot from position 0, and the cache it leaves
    seq = dec.init_decode(mems)
    seq.tok.fill_(sos)
    g = torch.empty((N_SEQ, B), dtype=torch.int64, device=DEV)
    g1 = torch.empty((N_SEQ, B), dtype=torch.float32, device=DEV)
    zero = torch.zeros(B, dtype=torch.int32, device=DEV)
    lib().call("omr_decode_steps_rows", ctypes.byref(seq.desc), ptr(seq.mem_len), ptr(zero), 0, ptr(seq.tok), N_SEQ, ptr(g), ptr(g1), None, cur_stream())
    gh = g.cpu()
    pos = torch.tensor(POS, dtype=torch.int32, device=DEV)
    for k in (1, 4, 7):
        R = k + 1
        spec = dec.init_spec_decode(draft.decoder, mems, dmems, k, sos, eos, max_out=MAX_SEQ)
        st = spec.target
        for b_, x in enumerate(mems):                             # the same projection of every memory (the rows behind it are padding)
            assert torch.equal(bits(st.cross_kv[b_, :x.shape[1]]), bits(seq.cross_kv[b_, :x.shape[1]]))
        wanted = list(range(k + 1))
        wanted += [0] * (-len(wanted) % B)
        seen = set()
        for c0 in range(0, len(wanted), B):
            js = wanted[c0:c0 + B]
            st.self_kv.fill_(NAN)                              # what the group does not write itself, outside its window, is never read
            for b, p in enumerate(POS):
                lo = max(0, p - win) if win > 0 else 0
                st.self_kv[:, b, lo:p] = seq.self_kv[:, b, lo:p]
            tokens = torch.stack([gh[p - 1:p + k, b] for b, p in enumerate(POS)])          # [B][R]: the fed token, then the true continuations
            for b, j in enumerate(js):
                if j < k:
                    tokens[b, j + 1] = (tokens[b, j + 1] + 1 + b) % V                        # the first wrong proposal
                    if tokens[b, j + 1] == eos:
                        tokens[b, j + 1] = (tokens[b, j + 1] + 1) % V
            spec.state.zero_()
            spec._dev("pos", torch.int32, B).copy_(pos)
            spec._dev("out_len", torch.int32, B).copy_(pos)
            spec._dev("first", torch.int64, B).copy_(tokens[:, 0])
            spec._dev("tokens", torch.int64, B * R).copy_(tokens.reshape(-1))
            lib().call("omr_decode_verify_rows", ctypes.byref(st.desc), ptr(st.mem_len), ptr(spec._dev("pos", torch.int32, B)), max(POS), R,
                       ptr(spec._dev("tokens", torch.int64, B * R)), ptr(spec._dev("picks", torch.int64, B * R)),
                       ptr(spec._dev("top1", torch.float32, B * R)), ptr(spec.ws_t), spec.ws_t.numel(), cur_stream())
            before = spec.snapshot()
            assert before["pos"].tolist() == POS                                            # verify advances nothing
            lib().call("omr_spec_accept", ctypes.byref(spec.sdesc), cur_stream())
            snap = spec.snapshot()
            for b, (p, j) in enumerate(zip(POS, js)):
                n = j + 1
                want_t, want_v = gh[p:p + n, b].tolist(), g1[p:p + n, b].cpu()
                assert snap["picks"][b, :n].tolist() == want_t, (k, b, j)
                assert torch.equal(bits(torch.from_numpy(snap["top1"][b, :n].copy())), bits(want_v)), (k, b, j)
                assert snap["accepted"][b] == j and snap["pos"][b] == p + n and snap["out_len"][b] == p + n and snap["done"][b] == 0
                assert snap["out_tokens"][b, p:p + n].tolist() == want_t and snap["first"][b] == want_t[-1]
                assert snap["prev"][b] == (want_t[-2] if n >= 2 else int(tokens[b, 0]))
                assert torch.equal(bits(torch.from_numpy(snap["out_top1"][b, p:p + n].copy())), bits(want_v))
                # the cache rows up to the accepted position are the sequential run's, byte for byte
                assert torch.equal(bits(st.self_kv[:, b, p:p + n]), bits(seq.self_kv[:, b, p:p + n])), (k, b, j)
                seen.add(j)
            assert snap["totals"].tolist() == [B * k, sum(js)]
        assert seen == set(range(k + 1))


# ------------------------------------------------------------------------------------------------------------------- end to end
class _Spy:
    """Counts the speculative states and their plain-step calls."""

    def __init__(self, monkeypatch):
        self.states, self.plain = 0, 0
        init, plain = D.SpecDecodeState.__init__, D.SpecDecodeState.plain

        def spy_init(state, *a, **kw):
            self.states += 1
            return init(state, *a, **kw)

        def spy_plain(state, *a, **kw):
            self.plain += 1
            return plain(state, *a, **kw)

        monkeypatch.setattr(D.SpecDecodeState, "__init__", spy_init)
        monkeypatch.setattr(D.SpecDecodeState, "plain", spy_plain)


def _targets(n):
    g = torch.Generator().manual_seed(5)
    return [torch.randint(3, V, (1, 12), generator=g) for _ in range(n)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_predict_with_a_draft_equals_predict_without(dtype, monkeypatch):
    m = _transformer(_cfg(2, dtype))
    copy = _transformer(_cfg(2, dtype))                         # (a) the target's own weights: every proposal is accepted
    other = _transformer(_cfg(1, dtype), seed=77)               # (b) an unrelated random draft
    xs = _inputs() + [rnd((1, 1, 32, 96), 950).to(DEV)]          # the last one: 24 keys, decoded alone by the plain route
    want = m.predict(xs, batch_size=4)
    want_p = m.predict_with_probs(xs, batch_size=4)
    assert want_p[0] == want
    spy = _Spy(monkeypatch)
    assert m.predict(xs, batch_size=4) == want and spy.states == 0 and m.last_spec_stats is None      # no draft: nothing new
    for k in (1, 4, 7):
        assert m.predict(xs, batch_size=4, draft=copy, draft_len=k) == want
        s = m.last_spec_stats
        assert s["cycles"] > 0 and s["accepted"] == s["drafted"] > 0 and s["tokens"] == sum(len(w) for w in want[:3])
    assert m.predict_with_probs(xs, batch_size=4, draft=copy) == want_p                      # floats from the same fp32 bits
    assert m.predict(xs, batch_size=2, draft=other, draft_len=3) == want                      # groups of two rows
    assert m.last_spec_stats["accepted"] <= m.last_spec_stats["drafted"]
    assert m.predict_with_probs(iter(xs), batch_size=4, draft=other) == want_p
    # (c) the target with one token's head bias pushed down: it proposes the target's token except where that token is due
    flat = [w for seq in want[:3] for w in seq]
    victim = max(set(flat), key=flat.count)
    assert len(set(flat)) >= 2, "the baseline decodes one token only: no mixed acceptance to be had"
    near = _transformer(_cfg(2, dtype))
    _head_bias(near)[m.w2i[victim]] = -1e4
    assert m.predict_with_probs(xs, batch_size=4, draft=near, draft_len=4) == want_p
    s = m.last_spec_stats
    assert 0 < s["accepted"] < s["drafted"], s
    batches = [(x, y) for x, y in zip(xs, _targets(len(xs)))]
    assert m.evaluate(iter(batches), batch_size=4, draft=near) == m.evaluate(iter(batches), batch_size=4)
    assert spy.states > 0


def test_a_run_that_reaches_max_len_takes_the_plain_step_tail(monkeypatch):
    m, copy, other = _transformer(_cfg(2)), _transformer(_cfg(2)), _transformer(_cfg(1), seed=77)
    for x in (m, copy):
        _head_bias(x)[m.w2i["<eos>"]] = -1e4                   # no <eos>: every row runs into max_seq_len
    xs = _inputs()
    want, want_v = m.predict_with_probs(xs, batch_size=4)
    assert [len(w) for w in want] == [MAX_SEQ] * 3
    spy = _Spy(monkeypatch)
    assert m.predict_with_probs(xs, batch_size=4, draft=copy, draft_len=4) == (want, want_v)      # 1 -> 296 by cycles of 5, then 4 plain steps
    assert spy.plain >= 1 and m.last_spec_stats["tokens"] == 3 * MAX_SEQ
    assert m.predict_with_probs(xs, batch_size=4, draft=other, draft_len=6) == (want, want_v)
    m._spec_sync_every = 1
    assert m.predict(xs, batch_size=4, draft=other, draft_len=2) == want


def test_a_window_and_fp8_weights_end_to_end():
    m = _transformer(_cfg(2, "bf16", True), win=5)
    copy, other = _transformer(_cfg(2, "bf16", True), win=5), _transformer(_cfg(1, "bf16"), win=7, seed=77)
    xs = _inputs()
    want = m.predict_with_probs(xs, batch_size=4)
    assert m.predict_with_probs(xs, batch_size=4, draft=copy, draft_len=4) == want
    assert m.last_spec_stats["accepted"] == m.last_spec_stats["drafted"]
    assert m.predict_with_probs(xs, batch_size=4, draft=other, draft_len=7) == want


def test_multimodal_targets_take_a_pair_draft_or_a_unimodal_one():
    m = _multimodal(_cfg(2))
    pair_draft = _multimodal(_cfg(1), seed=73)
    image_draft = _transformer(_cfg(1), seed=77)
    img, aud = [(32, 400), (32, 1040), (48, 640)], [(32, 600), (48, 880), (32, 520)]
    pairs = [(rnd((1, 1) + img[i], 1100 + i).to(DEV), rnd((1, 1) + aud[i], 1150 + i).to(DEV)) for i in range(3)]
    want = m.predict(pairs, batch_size=4)
    assert m.predict(pairs, batch_size=4, draft=pair_draft) == want
    assert m.last_spec_stats["cycles"] > 0
    assert m.predict(pairs, batch_size=4, draft=image_draft, draft_source="image", draft_len=2) == want
    assert m.predict(pairs, batch_size=4, draft=image_draft, draft_source="audio", draft_len=2) == want
    batches = [(xi, xa, y) for (xi, xa), y in zip(pairs, _targets(3))]
    assert m.evaluate(iter(batches), batch_size=4, draft=pair_draft) == m.evaluate(iter(batches), batch_size=4)


# ---------------------------------------------------------------------------------------------------------------------- no draft
NEW_ENTRIES = {"omr_decode_verify_rows", "omr_spec_accept", "omr_spec_decode_cycles", "omr_spec_workspace_bytes", "omr_decode_group_workspace_bytes"}


def test_without_a_draft_the_entries_called_are_the_parents():
    """The library entries a plain predict calls -- names, counts, order -- are those recorded from the commit before the feature
    (tests/golden/spec_no_draft_entries.json, tools/record_predict_entries.py).  The project has no kernel-level launch trace; an
    entry issues a fixed chain of launches for given arguments, and the bits of the kernels behind it are pinned elsewhere."""
    import json
    import os
    import spec_refs
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spec_no_draft_entries.json")) as f:
        golden = json.load(f)
    assert golden["case"] == json.loads(json.dumps(spec_refs.PREDICT_CASE))
    m, xs = spec_refs.build_predict_case(DEV)
    words = []
    plain = spec_refs.record_entries(lambda: words.extend(m.predict(xs, batch_size=spec_refs.PREDICT_CASE["batch_size"])))
    assert [len(w) for w in words] == golden["tokens"]
    assert plain == golden["entries"] and not NEW_ENTRIES & set(plain)
    assert spec_refs.record_entries(lambda: m.predict(xs, batch_size=4, draft=None)) == plain
    assert m.last_spec_stats is None
    with_draft = spec_refs.record_entries(lambda: m.predict(xs, batch_size=4, draft=_transformer(_cfg(1), seed=77)))
    assert "omr_spec_decode_cycles" in with_draft


# ------------------------------------------------------------------------------------------------- the accept kernel, every path
def test_accept_kernel_equals_the_numpy_rule_on_every_path():
    """omr_spec_accept against spec_refs.accept, field by field, on slots that cover what the model tests cannot steer: <eos> among
    the accepted picks and as the first rejected one, a run that fills up (max_out), slots frozen before the call, every j; 300
    slots, so that a thread of the one workgroup takes more than one."""
    import numpy as np
    import spec_refs
    B, k, eos, max_out = 300, 4, 1, 12
    R = k + 1
    sd = D._SpecDesc()
    sd.B, sd.k, sd.eos, sd.max_out, sd.t_max = B, k, eos, max_out, 1
    sd.state = None
    nbytes = lib().query("omr_spec_workspace_bytes", ctypes.byref(sd))
    off = {n: int(getattr(sd, n) or 0) for n in D._SpecDesc.STATE_FIELDS}
    rng = np.random.RandomState(11)
    picks = rng.randint(2, 9, size=(B, R)).astype(np.int64)
    picks[rng.rand(B, R) < 0.15] = eos
    tokens = np.concatenate([rng.randint(2, 9, size=(B, 1)), picks[:, :k]], axis=1).astype(np.int64)      # proposals = the picks before them ...
    for b in range(B):                                                                                       # ... up to a first wrong one at j = b % (k + 1)
        j = b % (k + 1)
        if j < k:
            tokens[b, j + 1] = 20 + b % 7
    top1 = rng.rand(B, R).astype(np.float32)
    st = dict(pos=rng.randint(1, max_out, size=B).astype(np.int32), done=(rng.rand(B) < 0.2).astype(np.int32), accepted=np.full(B, 9, np.int32),
              totals=np.array([1000, 10], np.int64), first=tokens[:, 0].copy(), prev=rng.randint(2, 9, size=B).astype(np.int64),
              out_tokens=rng.randint(2, 9, size=(B, max_out)).astype(np.int64), out_top1=rng.rand(B, max_out).astype(np.float32))
    st["out_len"] = st["pos"].copy()
    dtypes = dict(pos=np.int32, out_len=np.int32, done=np.int32, accepted=np.int32, totals=np.int64, first=np.int64, prev=np.int64,
                  out_tokens=np.int64, out_top1=np.float32)
    host = np.zeros(nbytes, np.uint8)

    def put(name, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        host[off[name]:off[name] + raw.size] = raw

    for name in dtypes:
        put(name, st[name])
    put("tokens", tokens), put("picks", picks), put("top1", top1)
    dev = torch.from_numpy(host).to(DEV)
    sd.state, sd.state_bytes = dev.data_ptr(), nbytes
    assert lib().query("omr_spec_workspace_bytes", ctypes.byref(sd)) == nbytes
    lib().call("omr_spec_accept", ctypes.byref(sd), cur_stream())
    got = dev.cpu().numpy()
    spec_refs.accept(tokens, picks, top1, st, k, eos, max_out)
    for name, dt in dtypes.items():
        want = np.ascontiguousarray(st[name]).view(np.uint8).reshape(-1)
        assert np.array_equal(got[off[name]:off[name] + want.size], want), name            # bytes: the fp32 values are copies
    live = st["done"] == 0
    assert 0 < live.sum() < B and (st["out_len"] == max_out).any() and set(st["accepted"].tolist()) >= set(range(k + 1))
