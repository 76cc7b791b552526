"""Attention maps at the model level: CrossAttention.need_weights against torch's nn.MultiheadAttention, Decoder.cross_attention_maps
against the CPU oracle's pieces (tests/attention_map_refs.decoder_maps_ref), Transformer.align / MultimodalTransformer.align
against their batch-size-1 runs and the host arithmetic of evaluation.cells_and_boxes.  fp32 tolerance: the one the model tests
hold the same modules to (tests/test_model_gpu.py `close`: 1e-3 relative, 2e-4 absolute)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_map_refs as M  # noqa: E402
from omr_a2s_multimodal_transformer_amd import evaluation as EV  # noqa: E402
from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402
from omr_a2s_multimodal_transformer_amd.runtime import seed_dropout, trace_dropout  # noqa: E402
from oracle import attention_refs as AR  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

DEV = "cuda:0"
NO_DROP = dict(dropout=0.0, encoder_dropout=0.0)
RTOL, ATOL = 1e-3, 2e-4                      # tests/test_model_gpu.py `close`
BF16_TOL = 3e-2                              # the bf16-against-fp32 tolerance of the model tests (test_bf16_step_tracks_fp32_oracle)


def rnd(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def close(got, ref, what=""):
    got = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = ref.detach().double().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert np.isfinite(got).all(), f"{what}: non-finite"
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=what)


def flat_module(module, dtype=torch.float32):
    from omr_a2s_multimodal_transformer_amd.params import FlatParams
    module._test_flat = FlatParams(list(module.named_parameters()), torch.device(DEV), dtype)
    for mod in module.modules():
        for name, buf in list(mod._buffers.items()):
            if buf is not None:
                mod._buffers[name] = buf.to(DEV)
    return module


# ================================================================================================ CrossAttention.need_weights

F4 = dict(B=3, T=9, S=11, d=256, H=4, lq=(5, 3, 2), lkv=(7, 4, 2))


def _cross_attention(dropout=0.1):
    from omr_a2s_multimodal_transformer_amd.model import CrossAttention
    ca = CrossAttention(F4["d"], dropout=dropout)
    sd = syn.seeded_state_dict(syn.mha_shapes("attention.", F4["d"]), 31)
    ca.load_state_dict(sd)
    flat_module(ca)
    q, kv = rnd((3, 9, 256), 401, -1, 1), rnd((3, 11, 256), 402, -1, 1)
    return ca, sd, q, kv, torch.tensor(F4["lq"]), torch.tensor(F4["lkv"])


def _tiled_block_mask():
    """bool [B * H, T, S], True = hidden, built the way oracle.ref_cpu.cross_attention builds its tiled bias: head (b, h) takes
    the block [lq:, lkv:] of sample (b * H + h) % B."""
    B, H, T, S = F4["B"], F4["H"], F4["T"], F4["S"]
    m = torch.zeros(B, T, S, dtype=torch.bool)
    for i, (lq, lkv) in enumerate(zip(F4["lq"], F4["lkv"])):
        m[i, lq:, lkv:] = True
    return m[torch.arange(B * H) % B]


def test_need_weights_off_returns_none_and_on_equals_torch():
    ca, sd, q, kv, lq, lkv = _cross_attention()
    ca.eval()
    assert type(ca).need_weights is False
    out0, none = ca(q.to(DEV), lq, kv.to(DEV), lkv)
    assert none is None
    ref = torch.nn.MultiheadAttention(F4["d"], F4["H"], batch_first=True).eval()
    ref.load_state_dict({k[len("attention."):]: v for k, v in sd.items()})
    ca.need_weights = True
    for lens, mask in (((lq, lkv), _tiled_block_mask()), ((None, None), None)):
        out, w = ca(q.to(DEV), lens[0], kv.to(DEV), lens[1])
        with torch.no_grad():
            o_ref, w_ref = ref(q, kv, kv, attn_mask=mask, need_weights=True)
        assert w.dtype == torch.float32 and tuple(w.shape) == (3, 9, 11)
        close(w, w_ref, what="weights against nn.MultiheadAttention")
        close(out, o_ref, what="output against nn.MultiheadAttention")
        close(w.sum(dim=-1), torch.ones(3, 9), what="rows sum to 1")
        if mask is not None:
            assert torch.equal(out, out0), "need_weights changed the attention output"
            hidden = mask.view(3, 4, 9, 11).all(dim=1)            # hidden in every head: exactly 0 in the average
            assert float(w.cpu()[hidden].abs().max()) == 0.0


def test_need_weights_in_training_is_the_post_dropout_average():
    """dropout 0.5: the weights are the fp64 reference under the keep mask of the seed the call drew (the dropout trace names it),
    the output is the need_weights = False output of the same seed bit for bit, and the backward runs through the tapped node."""
    ca, sd, q, kv, lq, lkv = _cross_attention(dropout=0.5)
    ca.train()
    qd = q.to(DEV).requires_grad_(True)
    seed_dropout(123)
    out0, _ = ca(qd, lq, kv.to(DEV), lkv)
    ca.need_weights = True
    seed_dropout(123)
    with trace_dropout() as tr:
        out, w = ca(qd, lq, kv.to(DEV), lkv)
    assert torch.equal(out, out0)
    sites = [t for t in tr if t[0] == "attn"]
    assert len(sites) == 1 and sites[0][1] == 0.5
    B, H, T, S, d = F4["B"], F4["H"], F4["T"], F4["S"], F4["d"]
    case = AR.AttnCase("f4-drop", "fwd", B, H, T, S, d // H, blk=(F4["lq"], F4["lkv"]), drop=(0.5, sites[0][2]))
    w_in, b_in = sd["attention.in_proj_weight"].double(), sd["attention.in_proj_bias"].double()
    qp = q.double() @ w_in[:d].t() + b_in[:d]
    kp = kv.double() @ w_in[d:2 * d].t() + b_in[d:2 * d]
    w_ref, _ = M.weights_ref(qp, kp, H, case=case, dtype=torch.float32, keep=AR.keep_mask(B, H, T, S, 0.5, sites[0][2]))
    close(w, w_ref, what="post-dropout weights")
    dropped = float((w_ref == 0).double().mean())
    assert 0.0 < dropped < 0.5                                    # entries every head dropped (or the block mask hides)
    out.float().sum().backward()
    torch.cuda.synchronize()
    assert qd.grad is not None and bool(torch.isfinite(qd.grad).all())


# ================================================================================================ Decoder.cross_attention_maps

V, D, L = 64, 128, 2


def _transformer(dtype, seed=21, hw=(32, 64), max_seq=32):
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    w2i, i2w = syn.make_vocab(V)
    cfg = ModelConfig(d_model=D, ff_dim=D, num_layers=L, compute_dtype=dtype, **NO_DROP)
    m = Transformer(hw[0], hw[1], max_seq, w2i, i2w, attn_window=-1, config=cfg)
    sd = syn.seeded_state_dict(syn.transformer_shapes(V, D, D, L), seed)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected
    m.flatten_parameters()
    return m.eval(), sd


def _decoder_inputs():
    g = torch.Generator().manual_seed(5)
    tgt = torch.randint(1, V, (3, 10), generator=g)
    tgt[1, 7:] = 0
    tgt[2, 4:] = 0
    mem = rnd((3, 20, D), 301, -1, 1)
    bmask = torch.arange(20)[None, :] >= torch.tensor([20, 13, 6])[:, None]
    return tgt, mem, bmask


CFG = O.OracleCfg(d_model=D, nhead=4, ff_dim=D, num_layers=L)


@pytest.fixture(scope="module")
def fp32_maps():
    """The fp32 model, its inputs, the oracle's maps per memory-mask form (computed once) and the kernel path's results."""
    m, sd = _transformer("fp32")
    tgt, mem, bmask = _decoder_inputs()
    forms = {"bool": bmask, "none": None, "lens": torch.tensor([20, 13, 6])}
    res = {}
    for name, ml in forms.items():
        ref = M.decoder_maps_ref(sd, "decoder.", tgt, mem, ml, CFG)
        ml_dev = None if ml is None else ml.to(DEV)
        logits, maps = m.decoder.cross_attention_maps(tgt.to(DEV), mem.to(DEV), ml_dev)
        res[name] = dict(ml=ml_dev, ref=ref, logits=logits, maps=maps)
    return m, sd, tgt, mem, res


@pytest.mark.parametrize("form", ["bool", "none", "lens"])
def test_decoder_maps_equal_the_oracle_and_logits_are_forwards(fp32_maps, form):
    m, sd, tgt, mem, res = fp32_maps
    r = res[form]
    with torch.no_grad():
        fwd = m.decoder(tgt.to(DEV), mem.to(DEV), r["ml"])
    assert r["logits"].shape == fwd.shape == (3, V, 10)
    assert torch.equal(r["logits"], fwd), "cross_attention_maps' logits are not forward's bit for bit"
    ref_logits, ref_maps, _ = r["ref"]
    assert r["maps"].dtype == torch.float32 and tuple(r["maps"].shape) == (3, 10, 20)
    close(r["maps"], ref_maps, what=f"maps ({form})")
    close(r["logits"], ref_logits, what=f"logits ({form})")
    sums = r["maps"].sum(dim=-1).cpu()
    assert float((sums - 1.0).abs().max()) <= 20 * 2.0 ** -8
    if form == "bool":
        hidden = (torch.arange(20)[None, :] >= torch.tensor([20, 13, 6])[:, None])[:, None, :].expand(3, 10, 20)
        assert float(r["maps"].cpu()[hidden].abs().max()) == 0.0      # -inf keys: exactly 0


def test_decoder_maps_of_selected_layers(fp32_maps):
    m, sd, tgt, mem, res = fp32_maps
    r = res["bool"]
    per_layer = r["ref"][2]
    for layers, want in (([1], per_layer[1]), ((0,), per_layer[0]), (range(2), r["ref"][1])):
        logits, maps = m.decoder.cross_attention_maps(tgt.to(DEV), mem.to(DEV), r["ml"], layers=layers)
        close(maps, want, what=f"layers={list(layers)}")
        assert torch.equal(logits, r["logits"])
    assert float((per_layer[0] - per_layer[1]).abs().max()) > 10 * ATOL       # the two layers' maps can be told apart
    for bad in ([], [2], [-1]):
        with pytest.raises(ValueError):
            m.decoder.cross_attention_maps(tgt.to(DEV), mem.to(DEV), r["ml"], layers=bad)


def test_padded_memory_rows_have_no_influence(fp32_maps):
    """The memory rows behind the bool mask filled with 1e4 in place of the inputs' values: maps and logits are the same bits.
    (Finite stand-ins, not NaN: a -inf bias cannot hide a NaN key, NaN - inf is NaN in every attention kernel's score chain.)"""
    m, sd, tgt, mem, res = fp32_maps
    r = res["bool"]
    hidden = torch.arange(20)[None, :] >= torch.tensor([20, 13, 6])[:, None]
    loud = mem.clone()
    loud[hidden] = 1.0e4
    assert not torch.equal(loud, mem)
    logits, maps = m.decoder.cross_attention_maps(tgt.to(DEV), loud.to(DEV), r["ml"])
    assert torch.equal(maps, r["maps"]) and torch.equal(logits, r["logits"])


def test_target_padding_bias_switch_of_align(fp32_maps):
    """A target with token 0 in FRONT of its padding (row 0, position 2).  The public entry is `forward` (its +1.0 on target keys
    equal to 0, quirk 1): logits bit-equal, maps the oracle's.  The private switch `_align` uses leaves the +1.0 out: rows in
    front of the first 0 key are the same bits, later rows are not, and every row equals its batch-size-1 pass without a mask."""
    m, sd, tgt, mem, res = fp32_maps
    tgt0 = tgt.clone()
    tgt0[0, 2] = 0
    ml = res["bool"]["ml"]
    logits, maps = m.decoder.cross_attention_maps(tgt0.to(DEV), mem.to(DEV), ml)
    with torch.no_grad():
        assert torch.equal(logits, m.decoder(tgt0.to(DEV), mem.to(DEV), ml))
    close(maps, M.decoder_maps_ref(sd, "decoder.", tgt0, mem, ml.cpu(), CFG)[1], what="maps with a 0 token, public entry")
    with torch.no_grad():
        _, plain = m.decoder._cross_attention_maps(tgt0.to(DEV), mem.to(DEV), ml, None, False)
    close(plain, M.decoder_maps_ref(sd, "decoder.", tgt0, mem, ml.cpu(), CFG, tgt_padding_bias=False)[1], what="maps without the +1.0")
    assert torch.equal(plain[0, :2], maps[0, :2]) and not torch.equal(plain[0, 2:], maps[0, 2:])
    _, alone = m.decoder.cross_attention_maps(tgt0[:1].to(DEV), mem[:1].to(DEV), None)        # row 0 has no padded memory row
    close(plain[0], alone[0], what="row 0 of the batch against its batch-size-1 pass")


def test_decoder_maps_refuse_training_mode(fp32_maps):
    m, sd, tgt, mem, res = fp32_maps
    m.decoder.train()
    try:
        with pytest.raises(ValueError):
            m.decoder.cross_attention_maps(tgt.to(DEV), mem.to(DEV), None)
    finally:
        m.decoder.eval()


def test_decoder_maps_bf16_track_fp32(fp32_maps):
    _, _, tgt, mem, res = fp32_maps
    mb, _ = _transformer("bf16")
    assert mb.compute_dtype() == torch.bfloat16
    logits, maps = mb.decoder.cross_attention_maps(tgt.to(DEV), mem.to(DEV), res["bool"]["ml"])
    with torch.no_grad():
        assert torch.equal(logits, mb.decoder(tgt.to(DEV), mem.to(DEV), res["bool"]["ml"]))
    ref = res["bool"]["maps"]
    peak = ref.max(dim=-1, keepdim=True).values
    err = float(((maps - ref).abs() / peak).max())
    print(f"bf16 maps against fp32 maps: largest |difference| / row peak {err:.4f}")
    assert maps.dtype == torch.float32 and err <= BF16_TOL
    assert float((maps.sum(dim=-1) - 1.0).abs().max()) <= 20 * 2.0 ** -8


# ================================================================================================ align

SIZES = ((64, 96), (37, 50), (17, 9))


@pytest.fixture(scope="module")
def aligned():
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    w2i, i2w = syn.make_vocab(V)
    torch.manual_seed(0)                     # random init, the same in every run
    m = Transformer(80, 200, 16, w2i, i2w, config=ModelConfig(num_layers=2, **NO_DROP))
    m.flatten_parameters()
    m.eval()
    xs = [rnd((1, 1, h, w), 900 + i) for i, (h, w) in enumerate(SIZES)]
    words = m.predict(xs, batch_size=3)
    batch = m.align(xs, batch_size=3, return_maps=True)
    singles = [m.align([x], return_maps=True)[0] for x in xs]
    return m, xs, words, batch, singles


def test_align_words_maps_and_picks(aligned):
    m, xs, words, batch, singles = aligned
    assert len(batch) == 3
    for (h, w), x, wd, a, s in zip(SIZES, xs, words, batch, singles):
        gh, gw = EV.grid_of(h, w)
        n = len(wd)
        assert a.words == wd == s.words and n >= 1
        assert tuple(a.maps.shape) == (n, gh * gw) == tuple(s.maps.shape) and a.maps.dtype == torch.float32 and a.maps.is_cuda
        close(a.maps, s.maps, what=f"{h}x{w}: maps in the batch against batch size 1")
        close(a.maps.sum(dim=-1), torch.ones(n), what="rows sum to 1")
        for al in (a, s):
            mp = al.maps.cpu().numpy()
            assert np.array_equal(al.index, mp.argmax(axis=-1))               # numpy: the first index on ties, like omr_argmax
            assert np.array_equal(al.weight, mp[np.arange(n), al.index])
            cell, box, source = EV.cells_and_boxes(al.index, (("image", h, w),))
            assert np.array_equal(al.cell, cell) and np.array_equal(al.box, box) and al.source == source == ["image"] * n
            assert (al.box[:, 2] <= h).all() and (al.box[:, 3] <= w).all() and (al.box[:, 0] < al.box[:, 2]).all() and (al.box[:, 1] < al.box[:, 3]).all()
    plain = m.align(xs, words=words, batch_size=3)
    assert all(p.maps is None and np.array_equal(p.index, a.index) and np.array_equal(p.weight, a.weight) for p, a in zip(plain, batch))


def test_align_map_byte_limit_cuts_the_groups(aligned, monkeypatch):
    """With the 1 GiB constant at 64 bytes no two of the inputs share a group (two rows of the smallest input, 4 memory rows and at
    least 1 token each, are 2 x 1 x 4 x 4 = 32 bytes, and the other two have 21 and 48 memory rows), and every input then is its
    batch-size-1 run, bit for bit."""
    m, xs, words, batch, singles = aligned
    assert EV.ALIGN_MAP_BYTES == 1 << 30
    monkeypatch.setattr(EV, "ALIGN_MAP_BYTES", 64)
    assert EV.plan_align_groups([len(w) for w in words], [48, 21, 4], 3) == [[0], [1], [2]]
    cut = m.align(xs, batch_size=3, return_maps=True)
    for c, s, a in zip(cut, singles, batch):
        assert c.words == s.words and np.array_equal(c.index, s.index) and np.array_equal(c.weight, s.weight)
        assert torch.equal(c.maps, s.maps)
        close(c.maps, a.maps, what="cut groups against the one batch")


def test_align_follows_given_words_and_layers(aligned):
    m, xs, words, batch, singles = aligned
    other = [list(reversed(w)) for w in words]
    a1 = m.align(xs, words=other, batch_size=2, layers=[1], return_maps=True)
    for i, (x, o) in enumerate(zip(xs, other)):
        ids = torch.tensor([[m.w2i["<sos>"]] + [m.w2i[w] for w in o[:-1]]])
        _, maps = m.decoder.cross_attention_maps(ids.to(DEV), m.encode(x), None, layers=[1])
        assert a1[i].words == o
        close(a1[i].maps, maps[0], what="teacher-forced pass over the given words")


def test_multimodal_align_concat_sources_and_audio_boxes():
    from omr_a2s_multimodal_transformer_amd.model import MultimodalTransformer
    w2i, i2w = syn.make_vocab(V)
    torch.manual_seed(1)
    m = MultimodalTransformer(80, 200, 80, 200, 16, w2i, i2w, mixer_type="concat", config=ModelConfig(num_layers=2, **NO_DROP))
    m.flatten_parameters()
    m.eval()
    shapes = (((64, 96), (37, 50)), ((17, 9), (33, 20)))
    pairs = [(rnd((1, 1, *si), 950 + i), rnd((1, 1, *sa), 960 + i)) for i, (si, sa) in enumerate(shapes)]
    out = m.align(pairs, batch_size=2, return_maps=True)
    assert [a.words for a in out] == m.predict(pairs, batch_size=2)
    for (si, sa), a in zip(shapes, out):
        s_img = int(np.prod(EV.grid_of(*si)))
        s_aud = int(np.prod(EV.grid_of(*sa)))
        assert a.maps.shape[1] == s_img + s_aud
        assert a.source == ["image" if i < s_img else "audio" for i in a.index.tolist()]
        cell, box, source = EV.cells_and_boxes(a.index, (("image", *si), ("audio", *sa)), s_img)
        assert np.array_equal(a.cell, cell) and np.array_equal(a.box, box) and a.source == source
        for src, bx in zip(a.source, a.box):
            hh, ww = si if src == "image" else sa                 # audio boxes are in spectrogram coordinates
            assert 0 <= bx[0] < bx[2] <= hh and 0 <= bx[1] < bx[3] <= ww
    # a token that leans on the audio part: the pick restricted to the audio columns maps into the spectrogram
    a, (si, sa) = out[0], shapes[0]
    s_img = int(np.prod(EV.grid_of(*si)))
    aud_pick = a.maps[:, s_img:].argmax(dim=-1).cpu().numpy() + s_img
    cell, box, source = EV.cells_and_boxes(aud_pick, (("image", *si), ("audio", *sa)), s_img)
    assert source == ["audio"] * len(aud_pick) and (box[:, 2] <= sa[0]).all() and (box[:, 3] <= sa[1]).all()


def test_align_rows_with_the_pad_token_equal_their_batch_size_1_runs(aligned):
    """Given words that hold <PAD> (token 0) in front of their end: in the padded batch (a memory mask, padded targets) every
    input's maps are those of its run alone, which has neither."""
    m, xs, _, _, _ = aligned
    pad, eos = m.i2w[0], "<eos>"
    given = [["tok00001", pad, "tok00002", "tok00003", eos], ["tok00004", "tok00005", pad, pad, "tok00006", "tok00007", eos], [pad, "tok00008", eos]]
    batch = m.align(xs, words=given, batch_size=3, return_maps=True)
    for x, g, a in zip(xs, given, batch):
        s = m.align([x], words=[g], return_maps=True)[0]
        assert a.words == g == s.words and tuple(a.maps.shape) == tuple(s.maps.shape)
        close(a.maps, s.maps, what="words with <PAD>: batch against batch size 1")
