"""Every parameter gradient of the bf16 training step (the benchmark's compute path) against the fp64 oracle, per tensor.

The bf16 backward takes its own host route (functional.py, conv_plan.py): the one-pass conv backward kernels, the InstanceNorm gradient
handed from conv3 to conv2, the DMA weight gradient, the attention backward over pre-generated dropout words, the side-stream weight
gradients.  Their kernels have their own suites; what is checked here is the glue -- which x, statistics, mask, in_scale, workspace and
slots each launch is handed, in which order, on which stream -- by the only thing that sees all of it: the gradients of a whole model.

As in tests/test_dropout_parity_gpu.py the run's own dropout masks and ReLU masks (runtime.trace_relu: stored output > 0) are injected
into oracle/ref_cpu.py, which then differentiates the same piecewise-linear function in fp64.  The bound of every tensor comes from the
reference alone (tests/bf16_grad_refs.py): the error of the oracle's own bf16-storage emulations, fp64 and fp32 accumulation, times the
margins of check_gradients.  DESIGN.md "bf16 gradient parity" has the storage-point mapping and the measured ratios.

gemm_panel and gemm_tall are not on these cases' path (they need >= 51 200 memory rows); their arithmetic has all-element exact tests
(tests/test_gemm_tall_gpu.py, test_gemm_branches_gpu.py) and their call site is the FusedCrossKVFn these cases run through the tile kernel.
"""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16_grad_refs as G  # noqa: E402
from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402

DEV = "cuda:0"
FUSED = {("fused", "none"), ("fused_apply", "none"), ("fused_xn", "hand_on"), ("fused_s2", "hand_on")}


def run_and_check(model, sd, step, fwd, rseed, label, n_trace, n_relu, routes=None):
    """One traced forward + backward of `model` (step() -> (logits, loss)), then the three oracle passes and check_gradients."""
    from omr_a2s_multimodal_transformer_amd import functional as Fn
    from omr_a2s_multimodal_transformer_amd.runtime import trace_dropout, trace_relu
    plans, inner = [], Fn.plan_conv3x3_bwd

    def recording(*a):
        plans.append(inner(*a))
        return plans[-1]

    random.seed(rseed)
    model.zero_grad()
    Fn.plan_conv3x3_bwd = recording
    try:
        with trace_dropout() as trace, trace_relu() as relus:
            logits, loss = step()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        Fn.plan_conv3x3_bwd = inner
    assert len(trace) == n_trace and len(relus) == n_relu, (len(trace), len(relus))
    drop_mask, relu_masks = G.materialise(trace, relus, DEV)

    def seeded(sdx, plan):
        random.seed(rseed)                    # the MixDropout draws of every pass
        return fwd(sdx, plan)

    g64 = G.reference(seeded, sd, drop_mask, relu_masks)
    assert g64.sites == (len(trace), len(relu_masks)), g64.sites          # the oracle met every site the run recorded, in its order
    e_ref = G.yardstick(g64, [G.emulate(seeded, sd, dt, drop_mask, relu_masks) for dt in (torch.float64, torch.float32)])
    got = G.Result({n: None if p.grad is None else p.grad.detach().float().cpu() for n, p in model.named_parameters()}, logits.detach().float().cpu(), loss.detach())
    assert all(torch.isfinite(g).all() for g in got.grads.values() if g is not None) and torch.isfinite(got.logits).all()
    seen = {(p.dgrad, p.finish) for p in plans}
    print(f"{label} routes {sorted(seen)}")
    if routes is not None:
        routes(seen)
    report = G.check_gradients(got, g64, e_ref, label)
    assert report["checked"] == sum(g is not None for g in g64.grads.values())
    assert abs(got.loss - g64.loss) / abs(g64.loss) < 2e-2, (got.loss, g64.loss)
    return report


def default_routes(seen):
    assert seen >= FUSED | {("conv_stat2", "apply"), ("conv", "none")}, sorted(seen)


def separate_routes(seen):
    assert not any(d.startswith("fused") for d, _ in seen) and ("conv_stat2", "apply") in seen and ("conv", "none") in seen, sorted(seen)


def two_pass_routes(seen):
    assert ("two_pass", "none") in seen and seen >= FUSED, sorted(seen)      # conv3 of the blocks that hand on keeps its one-pass kernel


@pytest.mark.parametrize("rseed,window,fused_bwd,two_pass,routes", [
    (2, -1, 15, False, default_routes), (6, -1, 15, False, default_routes), (9, -1, 15, False, default_routes),
    (6, 5, 15, False, default_routes), (6, -1, 0, False, separate_routes), (6, -1, 15, True, two_pass_routes)],
    ids=["seed2", "seed6", "seed9", "seed6-window5", "seed6-separate-kernels", "seed6-two-pass-norm"])
def test_unimodal_bf16_gradients_match_the_fp64_oracle(rseed, window, fused_bwd, two_pass, routes):
    """MixDropout at position 1 / 2 / 3 (seeds 2, 6, 9), the windowed self-attention, FUSED_BWD = 0 (separate data- and weight-gradient
    kernels, the stand-alone InstanceNorm apply) and TWO_PASS_NORM_BWD."""
    from omr_a2s_multimodal_transformer_amd import functional as Fn
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    from omr_a2s_multimodal_transformer_amd.runtime import seed_dropout
    V, H, W, T, L, B = 50, 80, 200, 12, 2, 3
    w2i, i2w = syn.make_vocab(V)
    saved = (Fn.FUSED_BWD, Fn.TWO_PASS_NORM_BWD)
    try:
        Fn.FUSED_BWD, Fn.TWO_PASS_NORM_BWD = fused_bwd, two_pass
        m = Transformer(H, W, 16, w2i, i2w, attn_window=window, config=ModelConfig(num_layers=L, compute_dtype="bf16"))
        sd = G.load(m, syn.transformer_shapes(V, layers=L), 41)
        m.flatten_parameters()
        m.train()
        x, xl, y_in, y_out = syn.synthetic_unimodal_batch(B, H, W, T, V, w2i["<sos>"], w2i["<eos>"], seed=9)
        seed_dropout(100 + rseed)

        def step():
            logits = m(x.to(DEV), xl, y_in)
            return logits, m.compute_loss(logits, y_out.to(DEV))

        ocfg = R.OracleCfg(num_layers=L, attn_window=window)

        def fwd(sdx, plan):
            lo = R.transformer_forward(sdx, x.to(next(iter(sdx.values())).dtype), xl, y_in, ocfg, H, W, drop=plan)
            return lo, R.ce_loss(lo, y_out)

        run_and_check(m, sd, step, fwd, rseed, f"unimodal seed {rseed} window {window} FUSED_BWD {fused_bwd} two_pass {two_pass}:",
                      9 + 1 + 1 + 6 * L, 5 * 3 + 4 * 2 + L, routes)
    finally:
        Fn.FUSED_BWD, Fn.TWO_PASS_NORM_BWD = saved


@pytest.mark.parametrize("mt,modality,rseed", [("attn_both", "both", 6), ("concat", "both", 2), ("attn_both", "audio", 9)])
def test_multimodal_bf16_gradients_match_the_fp64_oracle(mt, modality, rseed):
    """Both encoders, the mixer's probability dropout, the concatenated memory with its bool key mask, and the audio-only step (the image
    encoder and the mixer get no gradient: exactly zero)."""
    from omr_a2s_multimodal_transformer_amd.model import MultimodalTransformer
    from omr_a2s_multimodal_transformer_amd.runtime import seed_dropout
    V, L, B = 40, 2, 3
    IMG, AUD = (64, 160), (195, 96)
    w2i, i2w = syn.make_vocab(V)
    m = MultimodalTransformer(IMG[0], IMG[1], AUD[0], AUD[1], 12, w2i, i2w, mixer_type=mt, config=ModelConfig(num_layers=L, compute_dtype="bf16"))
    sd = G.load(m, syn.multimodal_shapes(V, mt, layers=L), 51)
    m.flatten_parameters()
    m.train()
    xi, xli, y_in, y_out = syn.synthetic_unimodal_batch(B, IMG[0], IMG[1], 11, V, w2i["<sos>"], w2i["<eos>"], seed=16)
    xa, xla, _, _ = syn.synthetic_unimodal_batch(B, AUD[0], AUD[1], 11, V, w2i["<sos>"], w2i["<eos>"], seed=17, pad_value=0.0)
    m.apply_teacher_forcing_modality = lambda: modality
    seed_dropout(200 + rseed)

    def step():
        logits = m(xi.to(DEV), xli, xa.to(DEV), xla, y_in, apply_teacher_forcing_modality=True)
        return logits, m.compute_loss(logits, y_out.to(DEV))

    ocfg = R.OracleCfg(num_layers=L)

    def fwd(sdx, plan):
        dt = next(iter(sdx.values())).dtype
        lo = R.multimodal_forward(sdx, xi.to(dt), xli, xa.to(dt), xla, y_in, ocfg, mt, IMG, AUD, modality, drop=plan)
        return lo, R.ce_loss(lo, y_out)

    n_mixer = {"concat": 0, "attn_both": 2}[mt] if modality == "both" else 0
    run_and_check(m, sd, step, fwd, rseed, f"multimodal {mt} {modality} seed {rseed}:", 2 * 10 + n_mixer + 1 + 6 * L, 2 * (5 * 3 + 4 * 2) + L)
