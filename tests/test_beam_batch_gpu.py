"""Batched on-device beam search against the batch-size-1 host loop `_Base.beam_search` (the yardstick, unchanged): the
selection kernel alone against a restatement of that loop's body, the cache reorder against DecodeState.reorder_rows,
beam_search_batch / predict(beam=) / evaluate(beam=) of both model classes against per-input beam_search.  Every comparison
is exact: word lists identical, scores `==` (fp64 bit patterns for the kernel)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from omr_a2s_multimodal_transformer_amd import kernels as K  # noqa: E402
from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd._lib import cur_stream, lib, ptr  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402
from omr_a2s_multimodal_transformer_amd.decoder import _BeamDesc  # noqa: E402
from omr_a2s_multimodal_transformer_amd.metrics import compute_metrics  # noqa: E402

DEV = "cuda:0"
NO_DROP = dict(dropout=0.0, encoder_dropout=0.0)
NINF = float("-inf")
# image sizes -> memory lengths ceil(H/16) * ceil(W/8): 24 (<= 64: searched alone), 128 and 250 (one split of 256 keys),
# 260, 400 and 450 (several splits) -- the SIZES of tests/test_ragged_decode_gpu.py
SIZES = [(32, 96), (32, 512), (32, 1000), (32, 1040), (64, 800), (48, 1200)]
# <eos> head-bias increments searched for a set of inputs on which the comparison means something (see _search_eos_bias)
# (random-weight models answer all inputs much alike: the band of biases in which some inputs end and others run out of
# positions is narrow, hence the fine steps)
EOS_BIAS_STEPS = [round(0.05 * i, 2) for i in range(61)] + [3.5, 4.0, 4.5, 5.0, 6.0, 7.0, 8.0]


def rnd(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


# ------------------------------------------------------------------------------------------------------ selection kernel
class _SelState:
    """The search state of omr_beam_select on its own: N inputs, `beam` rows each, filled from Python lists."""
    INT_FIELDS = ("best_row", "best_pos", "done", "exhausted")

    def __init__(self, N, beam, max_len, eos, scores, best_score, best_row, best_pos, done, exhausted, tokens):
        self.N, self.beam, self.max_len, self.rows = N, beam, max_len, N * beam
        bd = self.bd = _BeamDesc()
        bd.beam, bd.N, bd.eos, bd.max_len, bd.state = beam, N, eos, max_len, None
        self.nbytes = lib().query("omr_beam_workspace_bytes", ctypes.byref(bd))
        assert self.nbytes > 0
        self.off = {f: int(getattr(bd, f) or 0) for f in _BeamDesc.STATE_FIELDS}
        host = np.zeros(self.nbytes, dtype=np.uint8)
        v = self.views(host)
        v["scores"][:], v["best_score"][:], v["tokens"][:] = scores, best_score, tokens
        v["best_row"][:], v["best_pos"][:], v["done"][:], v["exhausted"][:] = best_row, best_pos, done, exhausted
        v["parents"][:] = -7                               # sentinels: what the kernel does not write stays recognisable
        v["hist_parent"][:] = -7
        v["hist_token"][:] = -7
        self.initial = host.copy()
        self.dev = torch.from_numpy(host).to(DEV)
        bd.state, bd.state_bytes = self.dev.data_ptr(), self.nbytes
        assert lib().query("omr_beam_workspace_bytes", ctypes.byref(bd)) == self.nbytes

    def views(self, host):
        def view(name, dtype, count):
            o = self.off[name]
            return host[o:o + count * np.dtype(dtype).itemsize].view(dtype)
        out = {"scores": view("scores", np.float64, self.rows), "best_score": view("best_score", np.float64, self.N),
               "tokens": view("tokens", np.int64, self.rows), "parents": view("parents", np.int32, self.rows)}
        for f in self.INT_FIELDS:
            out[f] = view(f, np.int32, self.N)
        for f in ("hist_parent", "hist_token"):
            out[f] = view(f, np.int32, self.max_len * self.rows).reshape(self.max_len, self.rows)
        return out

    def select(self, logits, V, t):
        lib().call("omr_beam_select", ptr(logits), logits.stride(0), V, ctypes.byref(self.bd), t, cur_stream())
        torch.cuda.synchronize()
        return self.views(self.dev.cpu().numpy())


def _host_select(idx_h, val_h, beam, eos, scores, best_done, t):
    """The body of the position loop of _Base.beam_search (model.py), line by line, on the top-k lists of ONE input's rows.
    scores: list of Python floats; best_done: (score, parent row, position) in place of (score, sequence).
    -> (stopped, best_done, parents, new_tok, new_scores, notes)."""
    cands = [(scores[b] + val_h[b][j], b, idx_h[b][j]) for b in range(beam) if scores[b] > NINF for j in range(beam)]
    cands.sort(key=lambda c: (-c[0], c[1], c[2]))
    notes = {"eos_considered": 0, "eos_ignored": sum(1 for c in cands if c[2] == eos), "cands": cands}
    parents, new_tok, new_scores = [], [], []
    for sc, b, tk in cands:
        if tk == eos:
            notes["eos_considered"] += 1
            if sc > best_done[0]:
                best_done = (sc, b, t)
            continue
        parents.append(b); new_tok.append(tk); new_scores.append(sc)
        if len(parents) == beam:
            break
    notes["eos_ignored"] -= notes["eos_considered"]
    if not parents or new_scores[0] <= best_done[0]:
        return True, best_done, parents, new_tok, new_scores, notes
    while len(parents) < beam:
        parents.append(parents[0]); new_tok.append(new_tok[0]); new_scores.append(NINF)
    return False, best_done, parents, new_tok, new_scores, notes


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64).tolist()


def _run_selection_scenario(V, beam, eos, logits, scores, best, done, t=5, max_len=9):
    """One omr_beam_select launch over N inputs against _host_select per input; -> the notes of every input."""
    N = len(done)
    tokens0 = list(range(3, 3 + N * beam))
    st = _SelState(N, beam, max_len, eos, scores, [b[0] for b in best], [b[1] for b in best], [b[2] for b in best], done,
                   [1 - d for d in done], tokens0)
    dev_logits = logits.to(DEV).contiguous()
    idx, val = K.topk_logprob(dev_logits, beam)             # the host route's own top-k: what beam_search reads back
    idx_h, val_h = idx.cpu().tolist(), val.cpu().tolist()
    got = st.select(dev_logits, V, t)
    init = st.views(st.initial)
    all_notes = []
    for n in range(N):
        r = slice(n * beam, (n + 1) * beam)
        if done[n]:                                          # frozen: not one byte of the input's state moves
            for f in ("scores", "tokens", "parents"):
                assert got[f][r].tolist() == init[f][r].tolist(), (n, f)
            for f in ("best_score", "best_row", "best_pos", "done", "exhausted"):
                assert _bits(got[f][n:n + 1]) == _bits(init[f][n:n + 1]), (n, f)
            assert (got["hist_parent"][:, r] == -7).all() and (got["hist_token"][:, r] == -7).all()
            all_notes.append(None)
            continue
        stopped, bd, parents, new_tok, new_scores, notes = _host_select(idx_h[r], val_h[r], beam, eos, [float(s) for s in scores[r]], best[n], t)
        all_notes.append(notes)
        ctx = (V, beam, n)
        assert _bits([got["best_score"][n]]) == _bits([bd[0]]), ctx
        assert (int(got["best_row"][n]), int(got["best_pos"][n])) == (bd[1], bd[2]), ctx
        assert int(got["done"][n]) == int(stopped) and int(got["exhausted"][n]) == int(not stopped), ctx
        if stopped:                                          # the host loop breaks before it reorders anything
            assert _bits(got["scores"][r]) == _bits(scores[r]) and got["tokens"][r].tolist() == tokens0[r], ctx
            assert (got["parents"][r] == -7).all() and (got["hist_parent"][:, r] == -7).all(), ctx
        else:
            assert got["parents"][r].tolist() == parents and got["tokens"][r].tolist() == new_tok, ctx
            assert _bits(got["scores"][r]) == _bits(new_scores), ctx
            assert got["hist_parent"][t, r].tolist() == parents and got["hist_token"][t, r].tolist() == new_tok, ctx
            other = [p for p in range(max_len) if p != t]
            assert (got["hist_parent"][other][:, r] == -7).all() and (got["hist_token"][other][:, r] == -7).all(), ctx
    return all_notes


@pytest.mark.parametrize("V", [30, 6997])
@pytest.mark.parametrize("beam", [1, 2, 3, 4, 8])
def test_beam_select_equals_the_host_loop_body(V, beam):
    N, eos, rows = 3, 1, 3 * beam
    none = (NINF, 0, 0)

    def base(seed):
        x = rnd((rows, V), seed, -3.0, 3.0)
        x[:, eos] = -30.0                                    # <eos> out of every row's top-k unless a scenario puts it there
        return x

    def falling(n0):                                         # all rows of an input alive, distinct scores
        return [-0.5 * k - 0.125 * n0 for k in range(beam)]

    # ---- scenario 1: ties.  input 0: two equal logits at the top of a row; input 1: two parents with identical logit rows and
    #      equal scores (the parent order decides); input 2: dead rows (only row 0 lives)
    x = base(1)
    x[0, 7], x[0, 4] = 5.0, 5.0
    if beam > 1:
        x[beam + 1] = x[beam]
    scores = np.array(falling(0) + ([-1.0, -1.0] + [-2.0 - k for k in range(beam - 2)])[:beam] + [-0.75] + [NINF] * (beam - 1))
    notes = _run_selection_scenario(V, beam, eos, x, scores, [none, none, none], [0, 0, 0])
    if beam > 1:
        c0 = [c for c in notes[0]["cands"] if c[1] == 0]
        assert c0[0][0] == c0[1][0] and (c0[0][2], c0[1][2]) == (4, 7)                # equal values: the smaller token id first
        c1 = notes[1]["cands"]
        assert c1[0][0] == c1[1][0] and (c1[0][1], c1[1][1]) == (0, 1) and c1[0][2] == c1[1][2]      # same score and token: parent 0 first
    assert len(notes[2]["cands"]) == beam                    # dead rows gave no candidates

    # ---- scenario 2: <eos> inside the top-`beam` of a live row (a finished record, the search goes on); <eos> ranked after the
    #      beam-th live candidate (ignored); an input that is already done (state untouched)
    x = base(2)
    x[0, 5], x[0, eos] = 6.0, 5.75                           # <eos> is the second best of the best row
    x[2 * beam - 1, eos] = 9.0                               # the top of input 1's last, far-behind row
    scores = np.array(falling(0) + [-0.25 * k for k in range(beam - 1)] + [-60.0] + falling(2))
    best = [(-1000.0, 0, 0), (-2000.0, 1, 1), (-3.5, 2, 3)]
    notes = _run_selection_scenario(V, beam, eos, x, scores, best, [0, 0, 1])
    if beam > 1:
        assert notes[0]["eos_considered"] == 1 and notes[0]["cands"][0][2] != eos
        assert notes[1]["eos_considered"] == 0 and notes[1]["eos_ignored"] == 1
    assert notes[2] is None

    # ---- scenario 3: stops.  input 0: <eos> leads the only live row -- at beam 1 every candidate is <eos> (no survivor), wider
    #      beams stop because no survivor can overtake it; input 1: the stored best finished score is out of reach; input 2 goes on
    x = base(3)
    x[0, eos] = 9.0
    scores = np.array([-0.5] + [NINF] * (beam - 1) + falling(1) + falling(2))
    best = [none, (-0.001, 0, 2), (-500.0, 1, 4)]
    notes = _run_selection_scenario(V, beam, eos, x, scores, best, [0, 0, 0])
    assert notes[0]["cands"][0][2] == eos and notes[0]["eos_considered"] == 1
    if beam == 1:
        assert all(c[2] == eos for c in notes[0]["cands"])


def test_beam_entries_refuse_bad_arguments_before_launching():
    st = _SelState(2, 4, 8, 1, [0.0] * 8, [NINF] * 2, [0] * 2, [0] * 2, [0] * 2, [1] * 2, [2] * 8)
    x = torch.zeros((8, 32), device=DEV)
    assert lib().query("omr_beam_select", ptr(x), 32, 30, ctypes.byref(st.bd), 8, cur_stream()) == -1        # t beyond the history
    assert lib().query("omr_beam_select", ptr(x), 32, 3, ctypes.byref(st.bd), 0, cur_stream()) == -1         # fewer tokens than beams
    st.bd.beam = 9
    assert lib().query("omr_beam_select", ptr(x), 32, 30, ctypes.byref(st.bd), 0, cur_stream()) == -1
    m = _transformer(ModelConfig(**NO_DROP))
    bs = m.decoder.init_beam_decode([rnd((100, 256), 1).to(DEV), rnd((300, 256), 2).to(DEV)], 4, sos=m.w2i["<sos>"], eos=m.w2i["<eos>"])
    call = lambda t0, n: lib().query("omr_beam_decode_steps", ctypes.byref(bs.desc), ctypes.byref(bs.bdesc), ptr(bs.mem_len), t0, n, cur_stream())
    assert call(0, bs.max_len + 1) == -1 and call(bs.max_len, 1) == -1                                       # t0 + n_steps > max_len
    bs.bdesc.N = 3
    assert call(0, 1) == -1                                                                                  # rows != N * beam
    bs.bdesc.N, bs.bdesc.beam = 2, 9
    assert call(0, 1) == -1
    with pytest.raises(RuntimeError, match="max_seq_len"):
        bs.run(bs.max_len + 1)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------- model
def _transformer(cfg, win=-1, max_seq=24, hw=(64, 1600), V=30, seed=61):
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    w2i, i2w = syn.make_vocab(V)
    m = Transformer(hw[0], hw[1], max_seq, w2i, i2w, attn_window=win, config=cfg)
    sd = syn.seeded_state_dict(syn.transformer_shapes(V, cfg.d_model, cfg.ff_dim, cfg.num_layers), seed)
    m.load_state_dict(sd, strict=False)
    m.flatten_parameters()
    m.eval()
    return m


def _multimodal(mixer, V=30, max_seq=20):
    from omr_a2s_multimodal_transformer_amd.model import MultimodalTransformer
    w2i, i2w = syn.make_vocab(V)
    cfg = ModelConfig(num_layers=2, **NO_DROP)
    m = MultimodalTransformer(64, 1200, 64, 900, max_seq, w2i, i2w, mixer_type=mixer, config=cfg)
    sd = syn.seeded_state_dict(syn.multimodal_shapes(V, mixer, cfg.d_model, cfg.ff_dim, cfg.num_layers), 71)
    m.load_state_dict(sd, strict=False)
    m.flatten_parameters()
    m.eval()
    return m


def _images(seed, reps=2):
    """Inputs of the six SIZES, `reps` different images of each."""
    return [rnd((1, 1, h, w), seed + 10 * r + i).to(DEV) for r in range(reps) for i, (h, w) in enumerate(SIZES)]


def _batched_history(m, mems, beam):
    """The batched run driven by hand: -> (results as token ids, per position the [N, beam] parents of inputs still live)."""
    big = [x for x in mems if x.shape[1] > 64]
    st = m.decoder.init_beam_decode(big, beam, sos=m.w2i["<sos>"], eos=m.w2i["<eos>"])
    live_parents = []
    for _ in range(m.max_seq_len):
        before = st.done()
        st.run(1)
        after = st.done()
        par = st.parents().cpu().tolist()
        live_parents.append([par[n] for n in range(len(big)) if not before[n] and not after[n]])
        if all(after):
            break
    return st.results(), live_parents


def _search_eos_bias(m, mems, beam=4):
    """Raise the head bias of <eos> (a fixed list of increments) until the BATCH-SIZE-1 results at `beam` make the comparison
    with the batched route meaningful: (a) some input's beam result differs from its greedy sequence, (b) some position after
    the first has a non-identity `parents` for a live input, (c) two inputs end by <eos> at different lengths below
    max_seq_len, (d) some input runs out of positions.  Fails, never skips, when no increment gives all four."""
    bias = m.decoder.out_layer.bias.omr_phys
    eos = m.w2i["<eos>"]
    base = bias[eos].item()
    seen = []
    for add in EOS_BIAS_STEPS:
        bias[eos] = base + add
        singles = [m.beam_search(x, beam) for x in mems]
        greedy = [m._greedy(x)[0] for x in mems]
        a = any(s[0] != g for s, g in zip(singles, greedy))
        ended = {len(s[0]) for s in singles if s[0][-1] == "<eos>" and len(s[0]) < m.max_seq_len}
        c = len(ended) >= 2
        d = any(s[0][-1] != "<eos>" and len(s[0]) == m.max_seq_len for s in singles)
        b = False
        if a and c and d:
            _, live_parents = _batched_history(m, mems, beam)
            b = any(p != list(range(beam)) for step in live_parents[1:] for p in step)
        seen.append((add, a, b, c, d))
        print(f"eos bias +{add}: differs-from-greedy {a}, non-identity parents {b}, eos lengths {sorted(ended)}, exhausted {d}")
        if a and b and c and d:
            return add
    bias[eos] = base
    raise AssertionError(f"no <eos> bias increment of {EOS_BIAS_STEPS} gave inputs that exercise the beam search "
                         f"(increment, differs from greedy, non-identity parents, two <eos> lengths, one exhausted): {seen}")


@pytest.mark.parametrize("dtype,win,fp8", [("fp32", -1, False), ("bf16", -1, False), ("fp32", 4, False), ("bf16", 4, False),
                                           ("bf16", -1, True), ("fp32", 4, True)])
def test_beam_search_batch_equals_per_input_beam_search(dtype, win, fp8):
    m = _transformer(ModelConfig(compute_dtype=dtype, fp8_decode=fp8, **NO_DROP), win)
    mems = [m.encode(x) for x in _images(800)]
    lens = [x.shape[1] for x in mems]
    assert len(set(lens)) == 6 and min(lens) <= 64 and any(64 < n <= 256 for n in lens) and max(lens) > 256
    _search_eos_bias(m, mems)
    for beam in (2, 4, 8):
        want = [m.beam_search(x, beam) for x in mems]
        got = m.beam_search_batch(mems, beam)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g[0] == w[0], (beam, i, lens[i])
            assert g[1] == w[1], (beam, i, lens[i], g[1], w[1])
    got = m.beam_search_batch([x[0] for x in reversed(mems)], 4)                  # [S, d] memories, another order
    assert got == [m.beam_search(x, 4) for x in reversed(mems)]
    assert [w for w, _ in m.beam_search_batch(mems, 1)] == m.greedy_batch(mems)     # beam 1 is the greedy decode


def test_beam_search_batch_does_not_depend_on_sync_every():
    m = _transformer(ModelConfig(compute_dtype="bf16", **NO_DROP))
    mems = [m.encode(x) for x in _images(800)]
    _search_eos_bias(m, mems)
    want = [m.beam_search(x, 4) for x in mems]
    for sync in (1, 3, 8):
        assert m.beam_search_batch(mems, 4, sync_every=sync) == want, sync
    assert m.beam_search_batch(mems[3:4], 4) == want[3:4]                          # one input: a batch of one


@pytest.mark.parametrize("dtype,win", [("fp32", -1), ("bf16", -1), ("fp32", 4), ("bf16", 4)])
def test_beam_cache_reorder_equals_reorder_rows(dtype, win):
    """Position by position: the logits of every row of the batched state are bit-equal to a batch-size-1 beam state (the host
    route's: share_memory_between + reorder_rows) that is fed the batched state's tokens and parents."""
    beam = 4
    m = _transformer(ModelConfig(compute_dtype=dtype, **NO_DROP), win)
    m.decoder.out_layer.bias.omr_phys[m.w2i["<eos>"]] -= 30.0                      # nobody finishes: every input stays live
    mems = [m.encode(rnd((1, 1, h, w), 900 + i).to(DEV)) for i, (h, w) in enumerate(SIZES[1:])]
    N = len(mems)
    st = m.decoder.init_beam_decode(mems, beam, sos=m.w2i["<sos>"], eos=m.w2i["<eos>"])
    refs = []
    for x in mems:
        r = m.decoder.init_decode(x)
        r.share_memory_between(beam)
        refs.append(r)
    tok = torch.full((N * beam,), m.w2i["<sos>"], dtype=torch.int64, device=DEV)
    compared_after_shuffle = 0
    shuffled = [False] * N
    for t in range(12):
        st.run(1)
        lb = st.logits[:, :st.V].clone()
        for n in range(N):
            ln = refs[n].step_logits(tok[n * beam:(n + 1) * beam].view(beam, 1))
            assert torch.equal(lb[n * beam:(n + 1) * beam], ln), (t, n)
            compared_after_shuffle += shuffled[n]
        snap = st.snapshot()
        assert not snap["done"].any()
        par = snap["parents"].reshape(N, beam)
        for n in range(N):
            shuffled[n] = t > 0 and par[n].tolist() != list(range(beam))
            refs[n].reorder_rows(torch.tensor(par[n].tolist(), dtype=torch.int64, device=DEV))
        tok = torch.from_numpy(snap["tokens"].copy()).to(DEV)
    assert compared_after_shuffle > 0, "no position after the first had a non-identity parents: the reorder was not exercised"


# ------------------------------------------------------------------------------------------------------------ evaluation
def _targets(n, V, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.cat([torch.tensor([[2]]), torch.randint(3, V, (1, 4 + i % 9), generator=g), torch.tensor([[1]])], dim=1) for i in range(n)]


def test_transformer_predict_and_evaluate_with_a_beam():
    m = _transformer(ModelConfig(**NO_DROP))
    xs = _images(1000)[:11]
    _search_eos_bias(m, [m.encode(x) for x in xs])
    want = [m.beam_search(m._encode_input(x), 4)[0] for x in xs]
    assert m.predict(xs, beam=4, batch_size=8) == want
    assert m.predict(iter(xs), beam=4, batch_size=3) == want                       # fewer rows than one beam: one input per group
    ys = _targets(len(xs), 30, 1400)
    truth = [[m.ytest_i2w[i] for i in y[0][1:].tolist()] for y in ys]
    assert m.evaluate(list(zip(xs, ys)), beam=4) == compute_metrics(y_true=truth, y_pred=want)


def test_multimodal_predict_and_evaluate_with_a_beam():
    m = _multimodal("concat")
    img = [(32, 400), (32, 1040), (48, 640), (32, 96), (64, 1200), (32, 720), (48, 200)]
    aud = [(32, 600), (48, 880), (32, 96), (32, 520), (64, 400), (32, 300), (48, 720)]
    pairs = [(rnd((1, 1) + img[i % 7], 1100 + i).to(DEV), rnd((1, 1) + aud[(i * 3) % 7], 1150 + i).to(DEV)) for i in range(9)]
    _search_eos_bias(m, [m._encode_input(p) for p in pairs])
    want = [m.beam_search(m._encode_input(p), 4)[0] for p in pairs]
    assert m.predict(pairs, beam=4, batch_size=8) == want
    ys = _targets(len(pairs), 30, 1200)
    truth = [[m.ytest_i2w[i] for i in y[0][1:].tolist()] for y in ys]
    batches = [(xi, xa, y) for (xi, xa), y in zip(pairs, ys)]
    assert m.evaluate(iter(batches), beam=4, batch_size=8) == compute_metrics(y_true=truth, y_pred=want)
