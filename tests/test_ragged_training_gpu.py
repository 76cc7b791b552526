"""Training and encoding on a padded batch of different-sized inputs (Transformer.forward with xl [B, 2], encode_ragged) against the
batch-size-1 runs of the same samples: the only way to get these semantics without the ragged route.  A small Transformer (2 decoder
layers, d_model 128, T = 12, 30 tokens) in eval() with gradients enabled: dropout off, no teacher-forcing noise.  Shapes: the three
samples of tests/extent_refs.py in a 64 x 96 plane; the targets have 11, 7 and 4 tokens."""
import functools
import json
import os
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

import extent_refs as E  # noqa: E402
from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402

DEV = "cuda:0"
V, T, D, LAYERS = 30, 12, 128, 2
TARGET_LENS = (11, 7, 4)
LOSS_RTOL, GRAD_RTOL, FEATURE_RTOL = 1e-4, 1e-3, 1e-3          # the project's model-level bounds (loss, gradients, logits)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ragged_dense_loss.json")


def rnd(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def make_model(dtype: str, dropout: float = 0.0, encoder_dropout: float = 0.0):
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    w2i, i2w = syn.make_vocab(V)
    cfg = ModelConfig(d_model=D, ff_dim=D, num_layers=LAYERS, dropout=dropout, encoder_dropout=encoder_dropout, compute_dtype=dtype)
    m = Transformer(E.PLANE[0], E.PLANE[1], T + 4, w2i, i2w, config=cfg)
    m.load_state_dict(syn.seeded_state_dict(syn.transformer_shapes(V, D, D, LAYERS), 23), strict=False)
    m.flatten_parameters()
    m.teacher_forcing_prob = 0.0
    m.eval()
    return m, w2i


@functools.lru_cache(maxsize=None)
def batch():
    """(crops [1, 1, h_b, w_b], x [B, 1, 64, 96] zero-padded, sizes [B, 2], y_in, y_out [B, T] 0-padded, tokens per sample)."""
    from omr_a2s_multimodal_transformer_amd.image import collate_ragged
    w2i, _ = syn.make_vocab(V)
    sos, eos = w2i["<sos>"], w2i["<eos>"]
    crops = [rnd((1, 1, h, w), 500 + b) for b, (h, w) in enumerate(E.SIZES)]
    x, sizes = collate_ragged([c[0] for c in crops])
    y_in = torch.zeros((len(crops), T), dtype=torch.int64)
    y_out = torch.zeros((len(crops), T), dtype=torch.int64)
    g = torch.Generator().manual_seed(77)
    for b, n in enumerate(TARGET_LENS):
        toks = torch.randint(1, V, (n,), generator=g)
        toks[(toks == sos) | (toks == eos)] = 1
        y = torch.cat([torch.tensor([sos]), toks, torch.tensor([eos])])
        y_in[b, :n + 1], y_out[b, :n + 1] = y[:-1], y[1:]
    counts = [int((y_out[b] != 0).sum()) for b in range(len(crops))]
    assert tuple(x.shape) == (3, 1) + E.PLANE and counts == [n + 1 for n in TARGET_LENS]
    return crops, x, sizes, y_in, y_out, counts


def loss_and_grad(m, x, xl, y_in, y_out):
    m.zero_grad()
    loss = m.compute_loss(m(x.to(DEV), xl, y_in), y_out.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach().double()), m._flat.grad.detach().double().cpu()


def memory_lengths(sizes):
    return [h * w for h, w in E.extent_levels([tuple(s) for s in sizes.tolist()])[-1]]


@functools.lru_cache(maxsize=None)
def runs(dtype: str):
    """{"ragged": (loss, flat gradient) of the padded batch through the ragged route, "alone": the combination of the three
    batch-size-1 runs: sum n_b loss_b / N and sum (n_b / N) grad_b, "model": the model} -- computed once per dtype."""
    m, _ = make_model(dtype)
    crops, x, sizes, y_in, y_out, counts = batch()
    ragged = loss_and_grad(m, x, sizes, y_in, y_out)
    N = float(sum(counts))
    loss1, grad1 = 0.0, torch.zeros_like(ragged[1])
    for b, (c, s_b) in enumerate(zip(crops, memory_lengths(sizes))):
        l_b, g_b = loss_and_grad(m, c, torch.tensor([s_b], dtype=torch.int32), y_in[b:b + 1], y_out[b:b + 1])
        loss1 += counts[b] / N * l_b
        grad1 += counts[b] / N * g_b
    return dict(ragged=ragged, alone=(loss1, grad1), model=m)


def per_tensor_rel(m, got, ref):
    """{parameter name: relative L2 of its gradient tensor}; a tensor whose reference gradient is zero must be zero."""
    out = {}
    for n, (o, c) in m._flat.offsets.items():
        a, r = got[o:o + c], ref[o:o + c]
        if float(r.norm()) == 0.0:
            assert float(a.norm()) == 0.0, f"{n}: gradient {float(a.norm()):.3e} where the reference has none"
            continue
        out[n] = float((a - r).norm() / r.norm())
    return out


def rel(a: float, b: float) -> float:
    return abs(a - b) / abs(b)


# ------------------------------------------------------------------------------------------------ 7. forward

def test_encode_ragged_equals_encode_of_each_crop_fp32():
    m = runs("fp32")["model"]
    crops, x, sizes, *_ = batch()
    mems = m.encode_ragged(x.to(DEV), sizes)
    assert [t.shape[0] for t in mems] == memory_lengths(sizes) == [48, 21, 4]
    for b, (c, got) in enumerate(zip(crops, mems)):
        with torch.no_grad():
            ref = m.encode(c.to(DEV))[0]
        assert got.shape == ref.shape
        err = float((got.double() - ref.double()).norm() / ref.double().norm())
        print(f"encode_ragged sample {b}: relative L2 {err:.3e}")
        assert err <= FEATURE_RTOL, (b, err)


# ------------------------------------------------------------------------------------------------ 8. training, fp32

def test_ragged_training_equals_the_batch_size_1_runs_fp32():
    """Batch loss = sum n_b loss_b / sum n_b (relative 1e-4); every parameter-gradient tensor = sum (n_b / N) grad_b (relative L2 1e-3)."""
    r = runs("fp32")
    (loss, grad), (loss1, grad1) = r["ragged"], r["alone"]
    rels = per_tensor_rel(r["model"], grad, grad1)
    worst = max(rels, key=rels.get)
    print(f"ragged fp32: loss {loss:.8f} vs {loss1:.8f} (rel {rel(loss, loss1):.3e}); worst gradient tensor {worst}: {rels[worst]:.3e}; "
          f"whole gradient {float((grad - grad1).norm() / grad1.norm()):.3e}")
    assert len(rels) > 80 and any(n.startswith("encoder.conv_blocks.0.") for n in rels)
    assert rel(loss, loss1) <= LOSS_RTOL, (loss, loss1)
    bad = {n: e for n, e in rels.items() if not e <= GRAD_RTOL}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 9. negative control

def test_the_dense_route_on_the_padded_batch_misses_that_bound_tenfold():
    """The same padded batch through the dense route (1-D xl): the padding moves the convs' borders and enters every InstanceNorm, so
    the gradients are those of another function.  Shows that test 8 can see the defect it guards against."""
    r = runs("fp32")
    m = r["model"]
    _, x, sizes, y_in, y_out, _ = batch()
    smax = max(memory_lengths(sizes))
    loss, grad = loss_and_grad(m, x, torch.full((x.shape[0],), smax, dtype=torch.int32), y_in, y_out)
    rels = per_tensor_rel(m, grad, r["alone"][1])
    print(f"dense route on the padded batch: loss rel {rel(loss, r['alone'][0]):.3e}, worst gradient tensor {max(rels.values()):.3e}")
    assert max(rels.values()) > 10 * GRAD_RTOL
    assert rel(loss, r["alone"][0]) > 10 * LOSS_RTOL


# ------------------------------------------------------------------------------------------------ 10. training, bf16

def test_ragged_training_bf16_is_as_close_to_fp32_as_the_batch_size_1_path():
    """bf16 ragged vs fp32 ragged, held to TWICE what the existing bf16 batch-size-1 path loses against its own fp32 run on the same
    samples (computed here): loss, the whole flat gradient and every gradient tensor.

    Measured on an MI355X (also in DESIGN.md "Ragged training"): whole gradient 1.088e-1 (ragged) against 1.081e-1 (batch-size-1), bound
    2.163e-1; loss 1.6e-4 against 2.0e-4; the tensor closest to its own bound is decoder layer 1's linear1.bias, 5.09e-2 against 2.78e-2."""
    f32, b16 = runs("fp32"), runs("bf16")
    m = f32["model"]
    base_loss = rel(b16["alone"][0], f32["alone"][0])
    got_loss = rel(b16["ragged"][0], f32["ragged"][0])
    base_all = float((b16["alone"][1] - f32["alone"][1]).norm() / f32["alone"][1].norm())
    got_all = float((b16["ragged"][1] - f32["ragged"][1]).norm() / f32["ragged"][1].norm())
    base_t = per_tensor_rel(m, b16["alone"][1], f32["alone"][1])
    got_t = per_tensor_rel(m, b16["ragged"][1], f32["ragged"][1])
    ratio = {n: got_t[n] / base_t[n] for n in got_t}
    worst = max(ratio, key=ratio.get)
    print(f"bf16 vs fp32, whole gradient: ragged {got_all:.4e}, batch-size-1 {base_all:.4e} (bound {2 * base_all:.4e}); "
          f"loss: ragged {got_loss:.3e}, batch-size-1 {base_loss:.3e}; worst tensor {worst}: {got_t[worst]:.3e} vs {base_t[worst]:.3e}")
    assert got_all <= 2 * base_all, (got_all, base_all)
    assert got_loss <= 2 * base_loss, (got_loss, base_loss)
    bad = {n: (got_t[n], base_t[n]) for n in got_t if not got_t[n] <= 2 * base_t[n]}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 11. train mode

def test_train_mode_step_bf16_with_dropout():
    """One training_step + FusedAdam step with every dropout on: finite loss and gradients, features outside every extent exactly
    zero, and Python's `random` left where a dense step from the same seed leaves it."""
    m, _ = make_model("bf16", dropout=0.1, encoder_dropout=0.5)
    m.teacher_forcing_prob = 0.5
    m.train()
    _, x, sizes, y_in, y_out, _ = batch()
    opt = m.configure_optimizers()
    states = {}
    for route, xl in (("ragged", sizes), ("dense", torch.tensor(memory_lengths(sizes), dtype=torch.int32))):
        random.seed(11)
        opt.zero_grad()
        loss = m.training_step((x.to(DEV), xl, y_in, y_out.to(DEV)), 0)
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and torch.isfinite(m._flat.grad).all() and float(m._flat.grad.abs().max()) > 0, route
        opt.step()
        torch.cuda.synchronize()
        assert torch.isfinite(m._flat.master).all(), route
        states[route] = random.getstate()
    assert states["ragged"] == states["dense"]
    with torch.no_grad():
        f = m.encoder.forward_nhwc(x.to(DEV), torch.bfloat16, extents=sizes)
    grid = E.extent_levels(E.SIZES)[-1]
    assert tuple(f.shape) == (3, 4, 12, D) and torch.isfinite(f).all()
    assert not f.cpu()[~E.inside_mask((4, 12), grid)].any(), "features outside an extent"
    assert all(bool(f[b, :h, :w].any()) for b, (h, w) in enumerate(grid))


def test_train_mode_forward_keeps_the_invariant_in_debug_mode(monkeypatch):
    """encoder.RAGGED_DEBUG (OMR_RAGGED_DEBUG=1) checks after every block and residual add that the activation is zero outside the
    extents: the route passes its own check with every dropout on, and the check does fire on a tensor that breaks the invariant."""
    from omr_a2s_multimodal_transformer_amd import encoder as enc
    m, _ = make_model("bf16", dropout=0.1, encoder_dropout=0.5)
    m.train()
    _, x, sizes, *_ = batch()
    monkeypatch.setattr(enc, "RAGGED_DEBUG", True)
    with torch.no_grad():
        f = m.encoder.forward_nhwc(x.to(DEV), torch.bfloat16, extents=sizes)
    grid = torch.tensor(E.extent_levels(E.SIZES)[-1], dtype=torch.int32)
    enc._assert_zero_outside(f, grid, "the features")
    f[2, 3, 11, 5] = 1.0
    with pytest.raises(AssertionError, match="not zero outside"):
        enc._assert_zero_outside(f, grid, "the features")


# ------------------------------------------------------------------------------------------------ 12. the dense path is untouched

def test_bool_key_padding_mask_as_xl_still_goes_to_the_decoder():
    """xl as a bool [B, S] key-padding mask (decoder.get_memory_key_padding_mask's second form) is no pixel-size table, also when S == 2:
    it takes the dense route as it always did.  An all-False mask masks nothing, so the loss is that of the 1-D call with full lengths
    (which builds no mask at all: the only difference is a bias of zeros added to the scores), to 1e-6 relative."""
    m, w2i = make_model("fp32")
    for hw, seed in (((32, 96), 3), ((16, 16), 4)):                       # memories of 24 and of 2 tokens
        x, _, y_in, y_out = syn.synthetic_unimodal_batch(2, hw[0], hw[1], T, V, w2i["<sos>"], w2i["<eos>"], seed=seed)
        S = ((hw[0] + 15) // 16) * ((hw[1] + 7) // 8)
        with torch.no_grad():
            ref = float(m.compute_loss(m(x.to(DEV), torch.full((2,), S, dtype=torch.int32), y_in), y_out.to(DEV)))
            got = float(m.compute_loss(m(x.to(DEV), torch.zeros((2, S), dtype=torch.bool), y_in), y_out.to(DEV)))
            half = torch.zeros((2, S), dtype=torch.bool)
            half[1, S // 2:] = True
            masked = float(m.compute_loss(m(x.to(DEV), half.to(DEV), y_in), y_out.to(DEV)))
        print(f"bool xl [2, {S}]: loss {got!r} vs 1-D {ref!r}; half of sample 1 masked: {masked!r}")
        assert rel(got, ref) <= 1e-6, (S, got, ref)
        assert masked == masked and masked != got, "a mask that hides keys must change the loss"


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dense_path_loss_is_bit_identical_to_the_recorded_one(dtype):
    """The dense route (1-D xl) at one small shape gives the loss it gave before the ragged route existed, to the bit
    (tests/golden/ragged_dense_loss.json, float32 bits as hex: recorded on an MI355X from a built checkout of the commit before,
    f3bd580, with tools/record_dense_loss.py, which imports the package from the checkout it is given; its docstring has the commands)."""
    m, w2i = make_model(dtype)
    x, xl, y_in, y_out = syn.synthetic_unimodal_batch(2, 32, 96, T, V, w2i["<sos>"], w2i["<eos>"], seed=3)
    with torch.no_grad():
        loss = m.compute_loss(m(x.to(DEV), xl, y_in), y_out.to(DEV)).float()
    bits = format(int(loss.cpu().view(torch.int32)) & 0xFFFFFFFF, "08x")
    print(f"dense loss {dtype}: {float(loss)!r} bits {bits}")
    with open(GOLDEN) as fh:
        assert bits == json.load(fh)[dtype], float(loss)
