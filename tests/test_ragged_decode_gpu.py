"""Batched greedy decoding over memories of different lengths (a ragged decode state) against the batch-size-1 loop the
reference runs (src/transformer/model.py:171-199): the key-split attention with a key count per row, the decode executor
with per-row memory lengths, greedy_batch / predict / evaluate of both model classes."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd._lib import cur_stream, lib, ptr  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402

DEV = "cuda:0"
NO_DROP = dict(dropout=0.0, encoder_dropout=0.0)
# image sizes -> memory lengths ceil(H/16) * ceil(W/8): 24 (<= 64: decoded alone), 128 and 250 (one split of 256 keys),
# 260, 400 and 450 (several splits)
SIZES = [(32, 96), (32, 512), (32, 1000), (32, 1040), (64, 800), (48, 1200)]


def rnd(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


# ---------------------------------------------------------------------------------------------------------------- kernel
def _split(q, k, v, H, S, kv_len=None):
    """omr_attn_fwd_split (kv_len None) / omr_attn_fwd_split_varlen on q [B,1,d], k/v [B,>=S,d] views -> (o, lse)."""
    B, T, d = q.shape
    hd = d // H
    o = torch.empty((B, T, d), dtype=q.dtype, device=DEV)
    lse = torch.empty((B, H, T), dtype=torch.float32, device=DEV)
    n = lib().query("omr_attn_split_workspace_floats", B, H, T, S, hd)
    ws = torch.empty(max(n, 1), dtype=torch.float32, device=DEV)
    code = 0 if q.dtype == torch.float32 else 1
    args = (code, ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), q.stride(1), k.stride(1), v.stride(1), o.stride(1), q.stride(0), k.stride(0),
            v.stride(0), o.stride(0), B, H, T, S, hd, None)
    if kv_len is None:
        lib().call("omr_attn_fwd_split", *args, ptr(ws), n, cur_stream())
    else:
        lib().call("omr_attn_fwd_split_varlen", *args, ptr(kv_len), ptr(ws), n, cur_stream())
    return o, lse


def _check_varlen(lens, dtype, hd, H=2, seed=0):
    B, S, d = len(lens), max(lens), H * hd
    q = rnd((B, 1, d), seed, -1, 1).to(DEV, dtype)
    k = rnd((B, S, d), seed + 1, -2, 2).to(DEV, dtype)
    v = rnd((B, S, d), seed + 2, -1, 1).to(DEV, dtype)
    for b, n in enumerate(lens):                     # anything read past a row's end turns its output into NaN
        k[b, n:] = float("nan")
        v[b, n:] = float("nan")
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    o, lse = _split(q, k, v, H, S, kv_len)
    torch.cuda.synchronize()
    for b, n in enumerate(lens):
        o1, lse1 = _split(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], H, n)
        assert torch.isfinite(o1).all()
        assert torch.equal(o[b:b + 1], o1), (dtype, hd, b, n, (o[b:b + 1].float() - o1.float()).abs().max().item())
        assert torch.equal(lse[b:b + 1], lse1), (dtype, hd, b, n)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hd", [32, 64])
def test_varlen_split_attention_rows_equal_their_own_run(dtype, hd):
    _check_varlen([65, 200, 256, 257, 511, 512, 3000], dtype, hd, seed=10)
    _check_varlen([300, 12696, 1000], dtype, hd, seed=20)          # the reference's largest memory: 50 splits, most rows empty past theirs


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hd", [32, 64])
def test_varlen_attention_without_a_split(dtype, hd):
    _check_varlen(list(range(65, 257)), dtype, hd, seed=30)        # S <= 256: one workgroup per row, normalised in the kernel


def test_varlen_attention_refuses_shapes_without_the_key_split():
    B, H, hd, S = 2, 2, 32, 64
    q = torch.zeros((B, 1, H * hd), device=DEV)
    k = torch.zeros((B, S, H * hd), device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        _split(q, k, k, H, S, torch.tensor([10, 64], dtype=torch.int32, device=DEV))


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


def _eos_bias_for_varied_lengths(m, mems, max_seq):
    """Raise the head bias of <eos> until the batch-size-1 decodes end at >= 3 different lengths below max_seq_len."""
    bias = m.decoder.out_layer.bias.omr_phys
    eos = m.w2i["<eos>"]
    base = bias[eos].item()
    for add in (0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0, 8.0):
        bias[eos] = base + add
        singles = [m._greedy(x)[0] for x in mems]
        ended = {len(s) for s in singles if s[-1] == "<eos>" and len(s) < max_seq}
        if len(ended) >= 3:
            return singles
    raise AssertionError("no <eos> bias gave three different sequence lengths")


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.mark.parametrize("dtype,win,fp8", [("fp32", -1, False), ("bf16", -1, False), ("fp32", 4, False), ("bf16", 4, False),
                                           ("bf16", -1, True), ("fp32", 4, True)])
def test_ragged_greedy_batch_equals_per_sample_greedy(dtype, win, fp8):
    m = _transformer(ModelConfig(compute_dtype=dtype, fp8_decode=fp8, **NO_DROP), win)
    mems = [m.encode(rnd((1, 1, h, w), 800 + i).to(DEV)) for i, (h, w) in enumerate(SIZES)]
    lens = [x.shape[1] for x in mems]
    assert len(set(lens)) == 6 and min(lens) <= 64 and any(64 < n <= 256 for n in lens) and max(lens) > 256
    singles = _eos_bias_for_varied_lengths(m, mems, m.max_seq_len)
    for sync in (3, 8):
        assert m.greedy_batch(mems, sync_every=sync) == singles
    assert m.greedy_batch([x[0] for x in reversed(mems)]) == singles[::-1]      # [S, d] memories, another order


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ragged_decode_step_logits_equal_batch_size_1(dtype):
    m = _transformer(ModelConfig(compute_dtype=dtype, **NO_DROP))
    mems = [m.encode(rnd((1, 1, h, w), 900 + i).to(DEV)) for i, (h, w) in enumerate(SIZES[1:])]
    _ragged_steps_match(m.decoder, mems, m.w2i["<sos>"])


def _ragged_steps_match(dec, mems, sos):
    B = len(mems)
    st = dec.init_decode(mems)
    assert st.S == max(x.shape[1] for x in mems)
    st1 = [dec.init_decode(x) for x in mems]
    for i in range(B):                                # the cross-attention K|V of each row is its bs-1 projection
        assert torch.equal(st.cross_kv[i, :mems[i].shape[1]], st1[i].cross_kv[0])
    tok = torch.full((B, 1), sos, dtype=torch.int64, device=DEV)
    for _ in range(3):
        lb = dec.decode_step(tok, st)
        rows = [dec.decode_step(tok[i:i + 1], st1[i]) for i in range(B)]
        for i in range(B):
            assert torch.equal(lb[i], rows[i]), i
        assert not torch.equal(lb[0], lb[1])
        tok = lb.argmax(dim=1, keepdim=True)
    with pytest.raises(RuntimeError, match="ragged"):
        st.reorder_rows(torch.zeros(B, dtype=torch.int64, device=DEV))


def test_ragged_decode_on_the_generic_executor():
    """A feed-forward width the row kernel does not take (ff 2304 > 2048: the per-kernel path of decode.hip), synthetic memories.
    (d_model 64 is no option: omr_add_layernorm_fwd takes widths 128 / 256 / 512 only.)"""
    from omr_a2s_multimodal_transformer_amd.decoder import Decoder
    from omr_a2s_multimodal_transformer_amd.params import FlatParams
    torch.manual_seed(5)
    dec = Decoder(output_size=30, max_seq_len=16, num_embeddings=30, embedding_dim=128, ff_dim=2304, dropout_p=0.0, nhead=4,
                  num_transformer_layers=2).eval()
    dec._test_flat = FlatParams(list(dec.named_parameters()), torch.device(DEV), torch.float32)
    for mod in dec.modules():
        for name, buf in list(mod._buffers.items()):
            if buf is not None:
                mod._buffers[name] = buf.to(DEV)
    mems = [rnd((1, n, 128), 950 + n, -1, 1).to(DEV) for n in (300, 70, 1000, 256, 513)]
    _ragged_steps_match(dec, mems, 2)


def test_transformer_predict_restores_input_order():
    m = _transformer(ModelConfig(**NO_DROP))
    sizes = [SIZES[i % 6] for i in range(11)]
    xs = [rnd((1, 1, h, w), 1000 + i).to(DEV) for i, (h, w) in enumerate(sizes)]
    singles = _eos_bias_for_varied_lengths(m, [m.encode(x) for x in xs], m.max_seq_len)
    assert m.predict(xs, batch_size=4) == singles
    assert m.predict(iter(xs), batch_size=1) == singles


def _multimodal(mixer, V=30, max_seq=20):
    from omr_a2s_multimodal_transformer_amd.model import MultimodalTransformer
    w2i, i2w = syn.make_vocab(V)
    cfg = ModelConfig(num_layers=2, **NO_DROP)
    m = MultimodalTransformer(64, 1200, 64, 900, max_seq, w2i, i2w, mixer_type=mixer, config=cfg)
    sd = syn.seeded_state_dict(syn.multimodal_shapes(V, mixer, cfg.d_model, cfg.ff_dim, cfg.num_layers), 71)
    m.load_state_dict(sd, strict=False)
    m.flatten_parameters()
    m.eval()
    m.decoder.out_layer.bias.omr_phys[w2i["<eos>"]] += 2.0
    return m


def _pairs(n, seed):
    img = [(32, 400), (32, 1040), (48, 640), (32, 96), (64, 1200), (32, 720), (48, 200)]
    aud = [(32, 600), (48, 880), (32, 96), (32, 520), (64, 400), (32, 300), (48, 720)]
    return [(rnd((1, 1) + img[i % 7], seed + i).to(DEV), rnd((1, 1) + aud[(i * 3) % 7], seed + 50 + i).to(DEV)) for i in range(n)]


def _targets(n, V, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.cat([torch.tensor([[2]]), torch.randint(3, V, (1, 4 + i % 9), generator=g), torch.tensor([[1]])], dim=1) for i in range(n)]


@pytest.mark.parametrize("mixer", ["concat", "attn_img"])
def test_multimodal_predict_and_evaluate_equal_validation_step(mixer):
    m = _multimodal(mixer)
    pairs = _pairs(9, 1100)
    ys = _targets(9, 30, 1200)
    batches = [(xi, xa, y) for (xi, xa), y in zip(pairs, ys)]
    for i, b in enumerate(batches):
        m.validation_step(b, i)
    want_pred = list(m.YHat)
    want = m.on_validation_epoch_end()
    assert m.predict(pairs, batch_size=4) == want_pred
    assert m.evaluate(iter(batches), batch_size=4) == want
    assert m.Y == [] and m.YHat == []


def test_transformer_evaluate_equals_validation_step_loop():
    m = _transformer(ModelConfig(**NO_DROP))
    m.decoder.out_layer.bias.omr_phys[m.w2i["<eos>"]] += 2.0
    xs = [rnd((1, 1) + SIZES[(i * 5) % 6], 1300 + i).to(DEV) for i in range(10)]
    batches = list(zip(xs, _targets(10, 30, 1400)))
    for i, b in enumerate(batches):
        m.validation_step(b, i)
    want = m.on_validation_epoch_end()
    m.Y.append(["kept"])
    assert m.evaluate(batches, batch_size=3) == want
    assert m.Y == [["kept"]] and m.YHat == []


def test_ragged_decode_rejects_bad_memories_before_launching():
    m = _transformer(ModelConfig(**NO_DROP))
    d = m.config.d_model
    ok = torch.zeros((1, 100, d), device=DEV)
    with pytest.raises(ValueError, match="empty"):
        m.greedy_batch([ok, torch.zeros((1, 0, d), device=DEV)])
    with pytest.raises(ValueError, match="16384"):
        m.greedy_batch([ok, torch.zeros((1, 16385, d), device=DEV)])
    with pytest.raises(ValueError, match="empty"):
        m.decoder.init_decode([torch.zeros((0, d), device=DEV)])
