"""The routes of Conv3x3Fn.backward (functional.FUSED_BWD) through a whole model: every route gives the gradients of the separate
kernels to within those kernels' own bf16 error."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402

DEV = "cuda:0"
ROUTES = (0, 1, 3, 7, 15)


def _gradients(dtype, x, xl, y_in, y_out, w2i, i2w, sd, routes):
    """{route: (flat parameter gradient, gradient w.r.t. ConvBlock 1's input)} and the dropout positions of ConvBlocks 0 and 1; the
    same weights, `random` draws and dropout seeds for every run."""
    from omr_a2s_multimodal_transformer_amd import functional as Fn
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    from omr_a2s_multimodal_transformer_amd.runtime import seed_dropout
    m = Transformer(80, 200, 16, w2i, i2w, config=ModelConfig(num_layers=1, compute_dtype=dtype, dropout=0.0, encoder_dropout=0.5))
    m.load_state_dict(sd, strict=False)
    m.flatten_parameters()
    m.train()
    m.teacher_forcing_prob = 0.0
    positions, seen = [], {}
    blocks = m.encoder.conv_blocks

    def spy(blk, keep_grad):
        inner = blk.nhwc

        def nhwc(x, *a, **kw):
            state = random.getstate()
            positions.append(random.randint(1, 3))          # the draw ConvBlock.nhwc is about to make
            random.setstate(state)
            if keep_grad:
                x.register_hook(lambda g: seen.__setitem__("dx", g.detach().float().clone()))
            return inner(x, *a, **kw)

        blk.nhwc = nhwc

    spy(blocks[0], False)
    spy(blocks[1], True)
    out = {}
    old = Fn.FUSED_BWD
    try:
        for r in routes:
            Fn.FUSED_BWD = r
            seed_dropout(31)
            random.seed(0)
            del positions[:]
            m.zero_grad()
            m.compute_loss(m(x, xl, y_in), y_out).backward()
            torch.cuda.synchronize()
            out[r] = (m._flat.grad.clone(), seen.pop("dx"))
    finally:
        Fn.FUSED_BWD = old
    return out, list(positions), m._flat.offsets


def test_every_backward_route_is_within_the_bf16_error_of_the_separate_kernels():
    """bf16 gradients of a small model (ConvBlock 0: 16 channels, stride 1; ConvBlock 1: 32 channels, stride (2, 2): all four bits of
    FUSED_BWD are on the path) with encoder dropout on, under FUSED_BWD = 0 (separate kernels), 1, 3, 7 and 15, and the fp32
    gradients of the same weights, draws and seeds as the yardstick: for every parameter with a non-zero fp32 gradient and for the
    gradient that enters ConvBlock 0 from ConvBlock 1, ||g_r - g_0|| <= ||g_0 - g_fp32||.  No free constant: a route may differ from
    the separate kernels by no more than they differ from fp32 themselves."""
    V = 40
    w2i, i2w = syn.make_vocab(V)
    sd = syn.seeded_state_dict(syn.transformer_shapes(V, 256, 256, 1), 7, mode="torch_default")
    x, xl, y_in, y_out = syn.synthetic_unimodal_batch(3, 80, 200, 12, V, w2i["<sos>"], w2i["<eos>"], seed=4)
    x, y_out = x.to(DEV), y_out.to(DEV)
    lowp, positions, offsets = _gradients("bf16", x, xl, y_in, y_out, w2i, i2w, sd, ROUTES)
    full, positions32, _ = _gradients("fp32", x, xl, y_in, y_out, w2i, i2w, sd, (0,))
    assert positions == positions32 and any(p in (2, 3) for p in positions), positions      # a fused dropout behind conv2 or conv3
    slices = {n: (lambda t, o=o, c=c: t[0][o:o + c]) for n, (o, c) in offsets.items()}
    slices["input gradient of ConvBlock 1"] = lambda t: t[1].flatten()
    worst, bad, yard = {r: (0.0, None) for r in ROUTES[1:]}, [], []
    for n, pick in slices.items():
        g32, g0 = pick(full[0]).float(), pick(lowp[0]).float()
        if g32.abs().max() == 0:
            continue
        own = (g0 - g32).norm().item()
        yard.append(own / g32.norm().item())
        for r in ROUTES[1:]:
            d = (pick(lowp[r]).float() - g0).norm().item()
            ratio = d / own if own > 0 else (0.0 if d == 0 else float("inf"))
            if ratio > worst[r][0]:
                worst[r] = (ratio, n)
            if not d <= own:
                bad.append((r, n, d, own))
    for r, (ratio, n) in worst.items():
        print(f"FUSED_BWD={r}: worst ||g_r - g_0|| / ||g_0 - g_fp32|| = {ratio:.4f} ({n})")
    print(f"yardstick ||g_0 - g_fp32|| / ||g_fp32||: {min(yard):.4f} .. {max(yard):.4f} over {len(yard)} slices")
    assert not bad, bad
