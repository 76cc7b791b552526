"""Beam search over the weighted late fusion (an extension: the reference decodes the fusion greedily).  Two anchors: beam 1
is the reference-pinned weighted greedy decode (weighted_prediction, tests/golden/f15_weighted.npz), and the batched on-device
route (omr_weighted_beam_decode_steps, weighted_beam_search_batch, weighted_predict(beam=)) equals the per-pair host loop
weighted_beam_search exactly: word lists identical, scores `==`.  Below them the top-k kernel of the mixed distribution
against a float64 restatement and the selection kernel against the host loop's body."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_beam_batch_gpu import EOS_BIAS_STEPS, NINF, SIZES, _bits, _host_select, _SelState, _transformer, rnd  # noqa: E402

from omr_a2s_multimodal_transformer_amd import kernels as K  # noqa: E402
from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd._lib import cur_stream, lib, ptr  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402
from omr_a2s_multimodal_transformer_amd.decoder import WeightedBeamState  # noqa: E402
from omr_a2s_multimodal_transformer_amd.metrics import compute_metrics  # noqa: E402
from omr_a2s_multimodal_transformer_amd.weighted_fusion import (weighted_beam_search, weighted_beam_search_batch, weighted_evaluate,  # noqa: E402
                                                                weighted_predict, weighted_prediction)

DEV = "cuda:0"
NO_DROP = dict(dropout=0.0, encoder_dropout=0.0)
EXHAUSTED = "positional-encoding table exhausted"
# audio inputs of the six pairs -> memory lengths 150, 270, 24, 130, 330, 200 beside the image side's 24, 128, 250, 260, 400, 450
AUDIO_SIZES = [(32, 600), (48, 720), (32, 96), (32, 520), (48, 880), (64, 400)]


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


# ---------------------------------------------------------------------------------------------------------------- kernel
TIE_ROW, TIE_A, TIE_B = 2, 7, 19
# per-row seeds of the two logit matrices for which the gap condition asserted in the test holds
ROW_SEEDS = {30: ([30000, 30100, 30200, 30300, 30400], [35000, 35100, 35200, 35300, 35400]),
             6997: ([6997000, 6997100, 6997200, 6997301, 6997400], [7002000, 7002100, 7002200, 7002301, 7002403])}
KERNEL_ALPHAS = (0.0, 0.3, 1.0)


def _logit_rows(V, seeds):
    x = torch.stack([rnd((V,), s) * 8 - 4 for s in seeds])
    x[TIE_ROW, TIE_A] = x[TIE_ROW, TIE_B] = 4.5              # with the same in the other matrix: one exact tie, at the top of the row
    return x


def _padded(x, ld):
    out = torch.full((x.shape[0], ld), float("nan"))            # the padding of a row is never read
    out[:, :x.shape[1]] = x
    return out.to(DEV)[:, :x.shape[1]]


@pytest.fixture(scope="module", params=[30, 6997])
def mixed_rows(request):
    """(V, logits a, logits b on the device with padded row strides, {alpha: (sorted float64 log-probabilities, indices)})."""
    V = request.param
    a, b = (_logit_rows(V, s) for s in ROW_SEEDS[V])
    ref = {}
    for alpha in KERNEL_ALPHAS:
        p = alpha * torch.softmax(a.double(), dim=1) + (1.0 - alpha) * torch.softmax(b.double(), dim=1)
        ps, pi = torch.sort(p, dim=1, descending=True, stable=True)
        gaps = (ps[:, :8] - ps[:, 1:9]) / ps[:, :8]            # among the top k + 1 for the largest k
        assert gaps[TIE_ROW, 0] == 0.0 and pi[TIE_ROW, :2].tolist() == [TIE_A, TIE_B]
        gaps[TIE_ROW, 0] = 1.0
        assert float(gaps.min()) > 1e-4, (V, alpha, float(gaps.min()))
        ref[alpha] = (torch.log(ps), pi)
    return V, _padded(a, K.round_up(V, 8) + 8), _padded(b, K.round_up(V, 8) + 24), ref


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_weighted_topk_logprob_matches_the_float64_restatement(mixed_rows, k):
    V, a, b, ref = mixed_rows
    assert a.stride(0) > V and b.stride(0) > V and a.stride(0) != b.stride(0)
    for alpha in KERNEL_ALPHAS:
        idx, val = K.weighted_topk_logprob(a, b, alpha, k)
        want_val, want_idx = ref[alpha]
        assert torch.equal(idx.cpu(), want_idx[:, :k]), (V, k, alpha)
        torch.testing.assert_close(val.cpu(), want_val[:, :k].float(), rtol=1e-5, atol=1e-5)
        assert idx[TIE_ROW, 0] == TIE_A and (k == 1 or idx[TIE_ROW, 1] == TIE_B)      # the smaller index first
        for r in (0, TIE_ROW, 4):                              # a row does not depend on the grid: bit for bit
            i1, v1 = K.weighted_topk_logprob(a[r:r + 1], b[r:r + 1], alpha, k)
            assert torch.equal(i1, idx[r:r + 1]) and torch.equal(v1.view(torch.int32), val[r:r + 1].view(torch.int32)), (V, k, alpha, r)
        if k == 1:
            i0, prob = K.weighted_argmax_rows(a, b, alpha, n=V)
            assert torch.equal(idx[:, 0], i0), (V, alpha)
            assert float((val[:, 0] - torch.log(prob)).abs().max()) <= 1e-6, (V, alpha)


def test_weighted_topk_logprob_refuses_bad_arguments(mixed_rows):
    V, a, b, _ = mixed_rows
    idx = torch.empty((5, 8), dtype=torch.int64, device=DEV)
    val = torch.empty((5, 8), dtype=torch.float32, device=DEV)
    lda, ldb = a.stride(0), b.stride(0)
    # (rows, n, k, lda, ldb): no rows, fewer entries than k, k outside 1..8, a row stride below n on either side
    for rows, n, k, la_, lb_ in ((0, V, 4, lda, ldb), (5, 3, 4, lda, ldb), (5, V, 0, lda, ldb), (5, V, 9, lda, ldb), (5, V, 4, V - 1, ldb),
                                 (5, V, 4, lda, V - 1)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            lib().call("omr_weighted_topk_logprob", ptr(a), la_, ptr(b), lb_, rows, n, 0.3, k, ptr(idx), ptr(val), cur_stream())


# ------------------------------------------------------------------------------------------------------ selection kernel
def _run_weighted_selection(V, beam, eos, xa, xb, alpha, scores, best, done, t=5, max_len=9):
    """One omr_weighted_beam_select launch over N inputs against _host_select (the body of the host loop) per input, fed
    with K.weighted_topk_logprob of the same device logits; -> the notes of every input."""
    N = len(done)
    tokens0 = list(range(3, 3 + N * beam))
    st = _SelState(N, beam, max_len, eos, scores, [b[0] for b in best], [b[1] for b in best], [b[2] for b in best], done,
                   [1 - d for d in done], tokens0)
    da, db = _padded(xa, K.round_up(V, 8)), _padded(xb, K.round_up(V, 8) + 16)
    idx, val = K.weighted_topk_logprob(da, db, alpha, beam)
    idx_h, val_h = idx.cpu().tolist(), val.cpu().tolist()
    lib().call("omr_weighted_beam_select", ptr(da), da.stride(0), ptr(db), db.stride(0), V, alpha, ctypes.byref(st.bd), t, cur_stream())
    torch.cuda.synchronize()
    got, init = st.views(st.dev.cpu().numpy()), st.views(st.initial)
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
def test_weighted_beam_select_equals_the_host_loop_body(V, beam):
    eos, rows, alpha = 1, 3 * beam, 0.3
    none = (NINF, 0, 0)

    def base(seed):
        xa, xb = rnd((rows, V), seed, -3.0, 3.0), rnd((rows, V), seed + 100, -3.0, 3.0)
        xa[:, eos] = xb[:, eos] = -30.0                      # <eos> out of every row's top-k unless a scenario puts it there
        return xa, xb

    def falling(n0):                                         # all rows of an input alive, distinct scores
        return [-0.5 * k - 0.125 * n0 for k in range(beam)]

    # ---- scenario 1: a finished record, dead rows, a frozen input.  input 0: <eos> is the second best of the best row in both
    #      models (a finished record, the search goes on), and an exact tie below it; input 1: only row 0 lives; input 2 is done
    xa, xb = base(11)
    xa[0, 5], xb[0, 5], xa[0, eos], xb[0, eos] = 6.0, 6.0, 5.75, 5.75
    xa[0, 9] = xa[0, 4] = xb[0, 9] = xb[0, 4] = 5.0
    scores = np.array(falling(0) + [-0.75] + [NINF] * (beam - 1) + falling(2))
    best = [(-1000.0, 0, 0), none, (-3.5, 2, 3)]
    notes = _run_weighted_selection(V, beam, eos, xa, xb, alpha, scores, best, [0, 0, 1])
    if beam > 1:
        assert notes[0]["eos_considered"] == 1 and notes[0]["cands"][0][2] != eos
    if beam > 3:
        c0 = [c for c in notes[0]["cands"] if c[1] == 0]
        assert c0[2][0] == c0[3][0] and (c0[2][2], c0[3][2]) == (4, 9)                # equal values: the smaller token id first
    assert len(notes[1]["cands"]) == beam and notes[2] is None

    # ---- scenario 2: stops.  input 0: <eos> leads the only live row -- at beam 1 every candidate is <eos> (no survivor), wider
    #      beams stop because no survivor can overtake it; input 1: the stored best finished score is out of reach; input 2 goes on
    xa, xb = base(12)
    xa[0, eos] = xb[0, eos] = 9.0
    scores = np.array([-0.5] + [NINF] * (beam - 1) + falling(1) + falling(2))
    best = [none, (-0.001, 0, 2), (-500.0, 1, 4)]
    notes = _run_weighted_selection(V, beam, eos, xa, xb, alpha, scores, best, [0, 0, 0])
    assert notes[0]["cands"][0][2] == eos and notes[0]["eos_considered"] == 1


# ----------------------------------------------------------------------------------------------------------------- model
def _two_models(cfg, win=-1, cfg_audio=None, max_seq=(24, 24)):
    return _transformer(cfg, win, max_seq[0], seed=61), _transformer(cfg_audio or cfg, win, max_seq[1], seed=62)


def _six_pairs(seed=3000):
    return [(rnd((1, 1) + hi, seed + i).to(DEV), rnd((1, 1) + ha, seed + 50 + i).to(DEV)) for i, (hi, ha) in enumerate(zip(SIZES, AUDIO_SIZES))]


def _check_lengths(len_i, len_a):
    assert len(set(len_i)) == 6 and min(len_i) <= 64 and any(64 < n <= 256 for n in len_i) and sum(n > 256 for n in len_i) >= 3
    assert len(set(len_a)) == 6 and sum(n <= 64 for n in len_a) == 1
    assert len_i[len_a.index(min(len_a))] > 64                 # the pair that is a single because of its audio side alone
    assert any(i > 256 and 64 < a <= 256 for i, a in zip(len_i, len_a)) and any(64 < i <= 256 and a > 256 for i, a in zip(len_i, len_a))


def _ids(m, words):
    return [m.w2i[w] for w in words]


def _drive(img, aud, mems_i, mems_a, beam, alpha, poison=False):
    """A WeightedBeamState over the pairs whose memories both take a ragged state, run one position at a time: -> (results as
    token ids, per position the [N, beam] parents of pairs still live).  poison: NaN in all four self-attention caches and in
    the cross-attention K|V rows past each memory's length, before the run."""
    big = [k for k in range(len(mems_i)) if mems_i[k].shape[1] > 64 and mems_a[k].shape[1] > 64]
    st = WeightedBeamState(img.decoder, [mems_i[k] for k in big], aud.decoder, [mems_a[k] for k in big], beam, img.w2i["<sos>"],
                           img.w2i["<eos>"], alpha)
    if poison:
        for cache in (st.st_a.self_kv, st.kv2_a, st.st_b.self_kv, st.kv2_b):
            cache.fill_(float("nan"))
        for s, mems in ((st.st_a, mems_i), (st.st_b, mems_a)):
            for slot, k in enumerate(big):
                s.cross_kv[slot, mems[k].shape[1]:] = float("nan")
    live_parents = []
    for _ in range(st.max_len):
        before = st.done()
        st.run(1)
        after = st.done()
        par = st.search.parents().cpu().tolist()
        live_parents.append([par[n] for n in range(len(big)) if not before[n] and not after[n]])
        if all(after):
            break
    return big, st.results(), live_parents


def _search_eos_bias(img, aud, pairs, mems_i, mems_a, alpha=0.3, beam=4):
    """Raise the <eos> head bias of BOTH models (a fixed list of increments) until the per-pair results at `beam` make the
    comparison with the batched route meaningful: (a) some pair's beam result differs from its weighted greedy decode, (b) some
    position after the first has a non-identity `parents` for a live pair, (c) two pairs end by <eos> at different lengths
    below max_seq_len, (d) some pair runs out of positions.  Fails, never skips, when no increment gives all four."""
    eos = img.w2i["<eos>"]
    biases = [m.decoder.out_layer.bias.omr_phys for m in (img, aud)]
    base = [b[eos].item() for b in biases]
    limit = max(img.max_seq_len, aud.max_seq_len)
    seen = []
    for add in EOS_BIAS_STEPS:
        for b, b0 in zip(biases, base):
            b[eos] = b0 + add
        singles = [weighted_beam_search(xi, xa, img, aud, alpha, beam) for xi, xa in pairs]
        ended = {len(s[0]) for s in singles if s[0][-1] == "<eos>" and len(s[0]) < limit}
        c = len(ended) >= 2
        d = any(s[0][-1] != "<eos>" and len(s[0]) == limit for s in singles)
        a = b_ = False
        if c and d:
            a = any(s[0] != weighted_prediction(xi, xa, img, aud, alpha) for s, (xi, xa) in zip(singles, pairs))
        if a:
            _, _, live_parents = _drive(img, aud, mems_i, mems_a, beam, alpha)
            b_ = any(p != list(range(beam)) for step in live_parents[1:] for p in step)
        seen.append((add, a, b_, c, d))
        print(f"eos bias +{add}: differs-from-greedy {a}, non-identity parents {b_}, eos lengths {sorted(ended)}, exhausted {d}")
        if a and b_ and c and d:
            return add
    raise AssertionError(f"no <eos> bias increment of {EOS_BIAS_STEPS} gave pairs that exercise the beam search "
                         f"(increment, differs from greedy, non-identity parents, two <eos> lengths, one exhausted): {seen}")


def _prepared(dtype="fp32", win=-1, fp8=False, audio=None):
    """Two models, the six pairs and their memories, the <eos> biases raised by _search_eos_bias."""
    cfg = ModelConfig(compute_dtype=dtype, fp8_decode=fp8, **NO_DROP)
    cfg_audio = ModelConfig(compute_dtype=dtype, fp8_decode=fp8, **NO_DROP, **audio) if audio else None
    img, aud = _two_models(cfg, win, cfg_audio)
    pairs = _six_pairs()
    mems_i, mems_a = [img.encode(xi) for xi, _ in pairs], [aud.encode(xa) for _, xa in pairs]
    _check_lengths([m.shape[1] for m in mems_i], [m.shape[1] for m in mems_a])
    _search_eos_bias(img, aud, pairs, mems_i, mems_a)
    return img, aud, pairs, mems_i, mems_a


@pytest.mark.parametrize("alpha", [0.0, 0.3, 0.5, 1.0])
def test_beam_1_is_the_weighted_greedy_decode(alpha):
    img, aud = _two_models(ModelConfig(**NO_DROP))
    for m in (img, aud):
        m.decoder.out_layer.bias.omr_phys[m.w2i["<eos>"]] += 2.0
    pairs = _six_pairs()
    want = [weighted_prediction(xi, xa, img, aud, alpha) for xi, xa in pairs]
    assert [weighted_beam_search(xi, xa, img, aud, alpha, beam=1)[0] for xi, xa in pairs] == want
    assert weighted_predict(pairs, img, aud, alpha=alpha, beam=1, batch_size=4) == weighted_predict(pairs, img, aud, alpha=alpha, batch_size=4) == want


def test_beam_1_gives_the_reference_tokens_of_the_f15_pair(golden):
    """The F15 pair of tests/golden/f15_weighted.npz (the reference's tokens), loaded the way
    test_f15_pair_inside_a_mixed_list_gives_the_reference_tokens loads it."""
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    g = golden("f15_weighted")
    V = 30
    w2i, i2w = syn.make_vocab(V)
    models = []
    for hw, seed in (((64, 1200), 81), ((195, 880), 82)):
        mm = Transformer(hw[0], hw[1], 14, w2i, i2w).eval()
        mm.load_state_dict(syn.seeded_state_dict(syn.transformer_shapes(V), seed), strict=False)
        mm.flatten_parameters()
        models.append(mm)
    img, aud = models
    xi, xa = rnd((1, 1, 64, 128), 801).to(DEV), rnd((1, 1, 195, 64), 802).to(DEV)
    for alpha in (0.3, 0.5):
        ref = [int(t) for t in g[f"a{alpha}_tokens"]]
        assert _ids(img, weighted_beam_search(xi, xa, img, aud, alpha=alpha, beam=1)[0]) == ref, alpha


BATCH_CASES = [("fp32", -1, False, None), ("bf16", -1, False, None), ("fp32", 4, False, None), ("bf16", 4, False, None),
               ("bf16", -1, True, None), ("fp32", 4, True, None), ("fp32", -1, False, dict(d_model=128, num_layers=2))]


@pytest.mark.parametrize("dtype,win,fp8,audio", BATCH_CASES)
def test_weighted_beam_search_batch_equals_the_per_pair_loop(dtype, win, fp8, audio):
    img, aud, pairs, mems_i, mems_a = _prepared(dtype, win, fp8, audio)
    if audio:
        assert (aud.decoder.embedding.weight.shape[1], len(aud.decoder.transformer_decoder.layers)) == (128, 2) != \
               (img.decoder.embedding.weight.shape[1], len(img.decoder.transformer_decoder.layers))
    want = {}
    for beam in (2, 4, 8):
        for alpha in (0.3, 0.7):
            want[beam, alpha] = [weighted_beam_search(xi, xa, img, aud, alpha, beam) for xi, xa in pairs]
            got = weighted_beam_search_batch(mems_i, mems_a, img, aud, alpha, beam)
            for i, (g, w) in enumerate(zip(got, want[beam, alpha])):
                assert g[0] == w[0], (beam, alpha, i)
                assert g[1] == w[1], (beam, alpha, i, g[1], w[1])
    got = weighted_beam_search_batch([m[0] for m in reversed(mems_i)], [m[0] for m in reversed(mems_a)], img, aud, 0.3, 4)      # [S, d], another order
    assert got == want[4, 0.3][::-1]
    assert weighted_beam_search_batch(mems_i, mems_a, img, aud, 0.7, 4, sync_every=1) == want[4, 0.7]      # the default above is 8


def test_poisoned_caches_do_not_change_the_results():
    img, aud, pairs, mems_i, mems_a = _prepared("bf16", 4)
    for alpha in (0.3, 0.7):
        big, clean, _ = _drive(img, aud, mems_i, mems_a, 4, alpha)
        assert _drive(img, aud, mems_i, mems_a, 4, alpha, poison=True)[1] == clean
        loop = [weighted_beam_search(*pairs[k], img, aud, alpha, 4) for k in big]
        assert clean == [(_ids(img, words), score) for words, score in loop]


# ------------------------------------------------------------------------------------------------------------ evaluation
def test_weighted_predict_and_evaluate_with_a_beam():
    img, aud, pairs, mems_i, mems_a = _prepared()
    want = {a: [weighted_beam_search(xi, xa, img, aud, a, 4)[0] for xi, xa in pairs] for a in (0.3, 0.7)}
    assert want[0.3] != want[0.7]                              # the mix matters
    assert weighted_predict(pairs, img, aud, alpha=0.3, beam=4, batch_size=8) == want[0.3]
    assert weighted_predict(iter(pairs), img, aud, alpha=0.7, beam=4, batch_size=16, sync_every=3) == want[0.7]
    got = weighted_predict(pairs, img, aud, alpha=[0.3, 0.7], beam=4, batch_size=16)      # one state per group, rewound per alpha
    assert list(got.keys()) == [0.3, 0.7] and got == want
    g = torch.Generator().manual_seed(1300)
    ys = [torch.cat([torch.tensor([[2]]), torch.randint(3, 30, (1, 4 + i), generator=g), torch.tensor([[1]])], dim=1) for i in range(6)]
    truth = [[img.ytest_i2w[i] for i in y[0][1:].tolist()] for y in ys]
    batches = [(xi, xa, y) for (xi, xa), y in zip(pairs, ys)]
    assert weighted_evaluate(iter(batches), img, aud, alpha=0.3, beam=4) == compute_metrics(y_true=truth, y_pred=want[0.3])
    assert weighted_evaluate(batches, img, aud, alpha=[0.3, 0.7], beam=4, batch_size=16) == {a: compute_metrics(y_true=truth, y_pred=want[a]) for a in (0.3, 0.7)}


# ---------------------------------------------------------------------------------------------------------------- refusals
def _state(img, aud, n=2, beam=4):
    mems_i = [rnd((100 + 200 * k, 256), 1 + k).to(DEV) for k in range(n)]
    mems_a = [rnd((300 - 100 * k, 256), 11 + k).to(DEV) for k in range(n)]
    return WeightedBeamState(img.decoder, mems_i, aud.decoder, mems_a, beam, img.w2i["<sos>"], img.w2i["<eos>"])


def _steps(st, t0, n):
    return lib().query("omr_weighted_beam_decode_steps", ctypes.byref(st.st_a.desc), ptr(st.st_a.mem_len), ctypes.byref(st.st_b.desc), ptr(st.st_b.mem_len),
                       ctypes.byref(st.bdesc), ptr(st.kv2_b), 0.3, t0, n, cur_stream())


def test_the_executor_refuses_bad_arguments_before_launching():
    img, aud = _two_models(ModelConfig(**NO_DROP))
    st = _state(img, aud)
    before = st.search.state.clone()
    assert _steps(st, 0, st.max_len + 1) == -1 and _steps(st, st.max_len, 1) == -1       # t0 + n_steps > max_len
    st.st_b.desc.V = 31
    assert _steps(st, 0, 1) == -1                                                        # the models do not share V
    st.st_b.desc.V = 30
    st.bdesc.N = 3
    assert _steps(st, 0, 1) == -1                                                        # rows != N * beam
    st.bdesc.N, st.bdesc.beam = 2, 9
    assert _steps(st, 0, 1) == -1
    st.bdesc.beam = 4
    with pytest.raises(RuntimeError, match="max_seq_len"):
        st.run(st.max_len + 1)
    torch.cuda.synchronize()
    assert torch.equal(st.search.state, before)                                          # nothing was launched
    st.run(1)                                                                            # the state itself is in order
    torch.cuda.synchronize()


@pytest.mark.parametrize("max_seq", [(24, 16), (16, 24)])
def test_a_search_that_outgrows_the_shorter_positional_table_raises(max_seq):
    img, aud = _two_models(ModelConfig(**NO_DROP), max_seq=max_seq)
    st = _state(img, aud)
    assert st.max_len == 16
    assert _steps(st, 0, 17) == -1 and _steps(st, 16, 1) == -1                           # past either model's max_len
    for m in (img, aud):
        m.decoder.out_layer.bias.omr_phys[m.w2i["<eos>"]] -= 30.0                        # nobody finishes: every pair is live at position 16
    pairs = _six_pairs()[3:5]
    with pytest.raises(RuntimeError, match=EXHAUSTED):
        weighted_beam_search(*pairs[0], img, aud, 0.5, 2)
    with pytest.raises(RuntimeError, match=EXHAUSTED):
        weighted_beam_search_batch([img.encode(xi) for xi, _ in pairs], [aud.encode(xa) for _, xa in pairs], img, aud, 0.5, 2)
    with pytest.raises(RuntimeError, match=EXHAUSTED):
        weighted_predict(pairs, img, aud, beam=2)
    torch.cuda.synchronize()
