"""The guarded optimizer step on the GPU: omr_grad_norm's record against fp64, non-finite detection, omr_adam_guarded against
omr_adam (bit for bit) and against an fp64 clip_grad_norm_ + Adam restatement, FusedAdam's skip / lagged step counts over a
FlatParams, and the model-level path through Trainer.fit.

Bounds (u = 2^-24, K = kernels.GRAD_NORM_K fp32 additions per thread, everything above that in fp64; csrc/optim.hip):
  all terms of the sum of squares are >= 0, so K fp32 squares-and-adds cost at most K u relative on the sum;
  range_sumsq[r] (fp64, no further rounding that matters):   |got - ref| <= (K + 2) u ref     (the norm's bound without the halving)
  norm = (float)(sqrt(sumsq) * scale): the root halves the error, the scale and the rounding to fp32 add 2 u:
                                                             |got - ref| <= (K / 2 + 2) u ref
  clip = min(1, max / (norm + 1e-6)) in fp32, max_norm given as an fp32 value: the norm's bound plus an addition and a division:
                                                             |got - ref| <= (K / 2 + 4) u ref
"""
import random

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from omr_a2s_multimodal_transformer_amd import kernels as K  # noqa: E402
from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402
from omr_a2s_multimodal_transformer_amd.params import FlatParams, FusedAdam  # noqa: E402
from omr_a2s_multimodal_transformer_amd.runtime import WgradStream  # noqa: E402

DEV = "cuda:0"
NO_DROP = dict(dropout=0.0, encoder_dropout=0.0)
U = 2.0 ** -24
KK, CHUNK = K.GRAD_NORM_K, K.GRAD_NORM_CHUNK
NORM_TOL = (KK / 2 + 2) * U
RANGE_TOL = (KK + 2) * U
CLIP_TOL = NORM_TOL + 2 * U
SIZES = [4, 8, 60, 64, 68, CHUNK - 4, CHUNK, CHUNK + 4, 3 * CHUNK + 20]
SCALES = [1.0, 0.5, 0.125]
NAN, INF = float("nan"), float("inf")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8 if t.dtype == torch.uint8 else torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b, what=""):
    assert torch.equal(bits(a), bits(b)), f"{what}: bits differ"


def run_norm(g, ranges, scale=1.0, max_norm=None):
    """-> (decoded record, its bytes).  The record is pre-filled with 0xAB: a field the kernel leaves out would show."""
    ws = torch.empty(K.grad_norm_workspace_bytes(g.numel(), len(ranges)), dtype=torch.uint8, device=DEV)
    ctl = K.new_step_ctl(DEV).fill_(0xAB)
    K.grad_norm(g, ranges, scale, max_norm, ws, ctl)
    host = ctl.cpu()
    return K.read_step_ctl(host), host


def layout(n, kind):
    """Element ranges for range length n: one range; three ranges with gaps (the middle one ends off a multiple of 4); 16 ranges
    (every third one a little shorter).  Begins are multiples of 4, gaps are 4 .. 7 elements."""
    lens = {"one": [n], "three": [n, max(1, n - 3), n], "sixteen": [n if r % 3 else max(1, n - 1) for r in range(16)]}[kind]
    ranges, pos = [], 0
    for ln in lens:
        ranges.append((pos, pos + ln))
        pos = (pos + ln + 3) // 4 * 4 + 4
    return ranges, pos


def gradient(total, ranges, seed):
    """NaN everywhere outside the ranges (must not be read); N(0, 1) times a per-range magnitude inside."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.full((total,), NAN)
    for r, (b, e) in enumerate(ranges):
        g[b:e] = torch.randn(e - b, generator=gen) * (10.0 ** (r % 3 - 1))
    return g


# ------------------------------------------------------------------------------------------------ norm and record against fp64
@pytest.mark.parametrize("kind", ["one", "three", "sixteen"])
@pytest.mark.parametrize("n", SIZES)
def test_norm_and_record_against_fp64(n, kind):
    ranges, total = layout(n, kind)
    g = gradient(total, ranges, seed=n + len(ranges))
    ref_ranges = [float((g[b:e].double() ** 2).sum()) for b, e in ranges]
    ref_sumsq = sum(ref_ranges)
    gd = g.to(DEV)
    first = None
    for scale in SCALES:
        rec, raw = run_norm(gd, ranges, scale)
        ref = ref_sumsq ** 0.5 * scale
        print(f"n={n} {kind} scale={scale}: norm {rec.norm!r} ref {ref!r} rel {abs(rec.norm - ref) / ref:.3e} (bound {NORM_TOL:.3e})")
        assert rec.apply == 1 and rec.nonfinite == 0 and rec.clip == 1.0
        assert abs(rec.norm - ref) <= NORM_TOL * ref
        assert abs(rec.sumsq - ref_sumsq) <= RANGE_TOL * ref_sumsq
        for r, want in enumerate(ref_ranges):
            assert abs(rec.range_sumsq[r] - want) <= RANGE_TOL * want, r
        assert all(rec.range_sumsq[r] == 0.0 for r in range(len(ranges), 16))
        assert rec.sumsq == sum(rec.range_sumsq[r] for r in range(len(ranges)))            # the ranges, added in index order
        if first is None:
            first = raw
    again = run_norm(gd, ranges, SCALES[0])[1]
    same_bits(first, again, "two runs of omr_grad_norm")


def test_clip_factor():
    ranges, total = layout(3 * CHUNK + 20, "three")
    g = gradient(total, ranges, seed=5)
    ref = float(sum((g[b:e].double() ** 2).sum() for b, e in ranges)) ** 0.5
    gd = g.to(DEV)
    for max_norm in (ref / 10, ref, 10 * ref):
        max_norm = torch.tensor(max_norm, dtype=torch.float32).item()                       # the C ABI takes a float: no rounding of the argument
        rec, _ = run_norm(gd, ranges, 1.0, max_norm)
        want = min(1.0, max_norm / (ref + 1e-6))
        print(f"max_norm={max_norm!r}: clip {rec.clip!r} want {want!r}")
        assert abs(rec.clip - want) <= CLIP_TOL * want and rec.clip <= 1.0 and rec.apply == 1
    for max_norm in (0.0, INF, -1.0, None):
        assert run_norm(gd, ranges, 1.0, max_norm)[0].clip == 1.0
    max_norm = torch.tensor(ref / 10, dtype=torch.float32).item()
    rec, _ = run_norm(gd, ranges, 0.5, max_norm)                                            # the clip acts on the SCALED norm
    assert abs(rec.clip - max_norm / (0.5 * ref + 1e-6)) <= CLIP_TOL * 0.2


@pytest.mark.parametrize("n", [4, CHUNK + 4])
def test_all_zero_gradient(n):
    rec, _ = run_norm(torch.zeros(n, device=DEV), [(0, n)], 1.0, 1.0)
    assert rec.norm == 0.0 and rec.sumsq == 0.0 and rec.clip == 1.0 and rec.apply == 1 and rec.nonfinite == 0


# ------------------------------------------------------------------------------------------------ non-finite detection
@pytest.mark.parametrize("n", [3 * CHUNK + 20, 3 * CHUNK + 22])
def test_one_nonfinite_element_anywhere_stops_the_step(n):
    """n = 3 chunks + 20: the tail is whole 16-byte vectors; + 22: its last vector is partial (element-wise loads)."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(3))
    gd = g.to(DEV)
    spots = {"first": 0, "last": n - 1, "first of the last partial chunk": 3 * CHUNK, "3 mod 4 in the tail": 3 * CHUNK + 19,
             "last element of a full chunk": 2 * CHUNK - 1}
    assert spots["3 mod 4 in the tail"] % 4 == 3
    for what, i in spots.items():
        for bad in (NAN, INF, -INF):
            gd[i] = bad
            rec, _ = run_norm(gd, [(0, n)])
            assert rec.apply == 0 and rec.nonfinite == 1, (what, bad, rec.apply, rec.nonfinite)
            gd[i] = g[i].item()
    rec, _ = run_norm(gd, [(0, n)])
    assert rec.apply == 1 and rec.nonfinite == 0


def test_nonfinite_count_and_fp32_overflow():
    n = 3 * CHUNK + 20
    g = torch.randn(n, generator=torch.Generator().manual_seed(4))
    gd = g.to(DEV)
    for i, bad in ((7, NAN), (CHUNK + 1, INF), (3 * CHUNK + 5, -INF)):                     # three different slots
        gd[i] = bad
    rec, _ = run_norm(gd, [(0, n)], 1.0, 1.0)
    assert rec.apply == 0 and rec.nonfinite == 3
    ranges = [(0, CHUNK), (CHUNK + 4, n)]                                                   # the same through two ranges
    rec, _ = run_norm(gd, ranges)
    assert rec.apply == 0 and rec.nonfinite == 2                                            # (element CHUNK + 1 lies in the gap)
    gd = g.to(DEV)
    gd[CHUNK + 9] = 3e19                                # finite, but its square is not (fp32): skipped, and not counted as non-finite
    rec, _ = run_norm(gd, [(0, n)])
    assert rec.apply == 0 and rec.nonfinite == 0


# ------------------------------------------------------------------------------------------------ guarded kernel
def make_ctl(apply, clip):
    rec = K.StepCtl(sumsq=1.0, norm=1.0, clip=clip, apply=apply, nonfinite=0 if apply else 1)
    return torch.frombuffer(bytearray(bytes(rec)), dtype=torch.uint8).to(DEV)


def adam_state(n, seed, lowp):
    gen = torch.Generator().manual_seed(seed)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    m, v = 0.1 * torch.randn(n, generator=gen), 0.01 * torch.rand(n, generator=gen)
    lp = p.to(torch.bfloat16) if lowp else None
    return [None if t is None else t.to(DEV) for t in (p, g, m, v, lp)]


@pytest.mark.parametrize("lowp", [False, True], ids=["fp32-only", "bf16-copy"])
def test_guarded_with_clip_one_is_omr_adam_bit_for_bit(lowp):
    one = make_ctl(1, 1.0)
    for n in (1, 63, 64, 65, 4099):
        for step in (1, 2, 1000):
            p, g, m, v, lp = adam_state(n, 100 * n + step, lowp)
            p2, m2, v2, lp2 = p.clone(), m.clone(), v.clone(), None if lp is None else lp.clone()
            K.adam_step(p, g, m, v, step, 1e-3, grad_scale=0.5, p_lowp=lp)
            K.adam_step(p2, g, m2, v2, step, 1e-3, grad_scale=0.5, p_lowp=lp2, ctl=one)
            for a, b, what in ((p, p2, "p"), (m, m2, "m"), (v, v2, "v")) + (((lp, lp2, "p_bf16"),) if lowp else ()):
                same_bits(a, b, f"n={n} step={step} {what}")
            assert not torch.equal(p, adam_state(n, 100 * n + step, lowp)[0])                # (the step did move p)


@pytest.mark.parametrize("lowp", [False, True], ids=["fp32-only", "bf16-copy"])
def test_guarded_with_apply_zero_writes_nothing(lowp):
    skip = make_ctl(0, NAN)
    for n in (1, 63, 64, 65, 4099):
        for step in (1, 2, 1000):
            before = adam_state(n, 7 * n + step, lowp)
            p, g, m, v, lp = [None if t is None else t.clone() for t in before]
            K.adam_step(p, g, m, v, step, 1e-3, p_lowp=lp, ctl=skip)
            for a, b, what in zip((p, g, m, v, lp), before, ("p", "g", "m", "v", "p_bf16")):
                if a is not None:
                    same_bits(a, b, f"n={n} step={step} {what}")


def test_guarded_clipping_equals_omr_adam_on_the_clipped_gradient():
    n = 4099
    p, g, m, v, lp = adam_state(n, 11, True)
    ref = float(g.double().norm())
    ws = torch.empty(K.grad_norm_workspace_bytes(n, 1), dtype=torch.uint8, device=DEV)
    ctl = K.new_step_ctl(DEV)
    K.grad_norm(g, [(0, n)], 1.0, ref / 10, ws, ctl)
    clip = K.read_step_ctl(ctl.cpu()).clip
    assert abs(clip - 0.1) < 1e-5
    p2, m2, v2, lp2 = p.clone(), m.clone(), v.clone(), lp.clone()
    K.adam_step(p, g, m, v, 3, 1e-3, p_lowp=lp, ctl=ctl)
    K.adam_step(p2, g * clip, m2, v2, 3, 1e-3, p_lowp=lp2)                                   # g' = g * clip in fp32 (clip is an fp32 value)
    for a, b, what in ((p, p2, "p"), (m, m2, "m"), (v, v2, "v"), (lp, lp2, "p_bf16")):
        same_bits(a, b, what)


def test_guarded_clipping_tracks_fp64_clip_grad_norm_and_adam():
    """Five steps of torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in fp64 against grad_norm + adam_step(ctl=...), at the
    tolerance of the existing Adam parity test (tests/test_kernels_gpu.py::test_colsum_adam_argmax: rtol 1e-5, atol 1e-7)."""
    n, lr, steps = 5000, 1e-3, 5
    gen = torch.Generator().manual_seed(21)
    p0 = torch.rand(n, generator=gen)
    grads = [torch.rand(n, generator=gen) * (1 + t) for t in range(steps)]
    max_norm = float(grads[0].double().norm()) / 10
    ref = nn.Parameter(p0.double())
    opt = torch.optim.Adam([ref], lr=lr)
    for gt in grads:
        ref.grad = gt.double().clone()
        torch.nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ws = torch.empty(K.grad_norm_workspace_bytes(n, 1), dtype=torch.uint8, device=DEV)
    ctl = K.new_step_ctl(DEV)
    for t, gt in enumerate(grads):
        gd = gt.to(DEV)
        K.grad_norm(gd, [(0, n)], 1.0, max_norm, ws, ctl)
        K.adam_step(p, gd, m, v, t + 1, lr, ctl=ctl)
    torch.testing.assert_close(p.cpu(), ref.detach().float(), rtol=1e-5, atol=1e-7)
    assert (p.cpu() - p0).abs().max() > 1e-3


# ------------------------------------------------------------------------------------------------ FusedAdam over a FlatParams
SHAPES = [("enc.w", (300, 70)), ("enc.b", (7,)), ("dec.w", (33, 9)), ("dec.b", (5,))]          # enc spans two slots of the reduction


def make_flat():
    gen = torch.Generator().manual_seed(1)
    named = [(n, nn.Parameter(torch.randn(s, generator=gen))) for n, s in SHAPES]
    flat = FlatParams(named, torch.device(DEV), torch.bfloat16)
    return flat, FusedAdam(flat, lr=1e-3)


def step_gradient(flat, t):
    return torch.randn(flat.total, generator=torch.Generator().manual_seed(50 + t)).to(DEV)


def state_of(flat):
    return [t.clone() for t in (flat.master, flat.exp_avg, flat.exp_avg_sq, flat.lowp)]


def assert_state(flat, want, what):
    for a, b, name in zip(state_of(flat), want, ("master", "exp_avg", "exp_avg_sq", "lowp")):
        same_bits(a, b, f"{what}: {name}")


def run_steps(guard, script):
    """script: [(step id t, touched or None, poison)].  -> (flat, opt, state before each step, state after each step)."""
    flat, opt = make_flat()
    if guard:
        opt.enable_guard()
    before, after = [], []
    for t, touched, poison in script:
        opt.zero_grad()
        flat.grad.copy_(step_gradient(flat, t))
        if poison:
            flat.grad[flat.offsets["enc.w"][0] + 5] = NAN
        before.append(state_of(flat))
        opt.step(touched=touched)
        after.append(state_of(flat))
    return flat, opt, before, after


def test_fused_adam_skips_a_nonfinite_step_and_its_count():
    flat, opt, before, after = run_steps(True, [(1, None, False), (2, None, True), (3, None, False), (4, None, False)])
    for a, b, name in zip(after[1], before[1], ("master", "exp_avg", "exp_avg_sq", "lowp")):
        same_bits(a, b, f"step 2 must not write {name}")
    assert not torch.equal(after[0][0], before[0][0])
    assert opt.skipped == 1 and opt.steps == dict(enc=3, dec=3) and opt.step_count == 3
    sd = opt.state_dict()
    assert sd["skipped"] == 1 and sd["step"] == 3
    plain_flat, plain, _, plain_after = run_steps(False, [(1, None, False), (3, None, False), (4, None, False)])
    assert_state(flat, plain_after[2], "guarded run with step 2 skipped == unguarded run of steps 1, 3, 4")
    assert plain.steps == dict(enc=3, dec=3) and "skipped" not in plain.state_dict()
    assert torch.isfinite(flat.master).all() and torch.isfinite(flat.exp_avg_sq).all()


def test_fused_adam_skipped_modality_drop_step_counts_for_nobody():
    script = [(1, None, False), (2, ("enc",), True), (3, ("dec",), False), (4, None, False)]
    flat, opt, before, after = run_steps(True, script)
    for a, b, name in zip(after[1], before[1], ("master", "exp_avg", "exp_avg_sq", "lowp")):
        same_bits(a, b, f"the skipped enc-only step must not write {name}")
    assert opt.steps == dict(enc=2, dec=3) and opt.skipped == 1
    plain_flat, plain, _, plain_after = run_steps(False, [s for s in script if s[0] != 2])
    assert plain.steps == dict(enc=2, dec=3)
    assert_state(flat, plain_after[2], "guarded run with the enc-only step skipped == unguarded run without it")
    # the other way round: a skipped step that touched only `dec`, then one that touches only `enc`
    script = [(1, None, False), (2, ("dec",), False), (3, ("enc",), True), (4, ("enc",), False), (5, None, False)]
    flat, opt, _, _ = run_steps(True, script)
    _, plain, _, plain_after = run_steps(False, [s for s in script if s[0] != 3])
    assert opt.steps == plain.steps == dict(enc=3, dec=3) and opt.skipped == 1
    assert_state(flat, plain_after[3], "second modality script")


def test_fused_adam_reports_the_scaled_norm():
    flat, opt = make_flat()
    opt.enable_guard(max_norm=1e9)
    assert opt.last_grad_norm is None
    g = step_gradient(flat, 9)
    flat.grad.copy_(g)
    opt.step(grad_scale=0.5)
    ref = float(g.double().norm())
    assert abs(opt.last_grad_norm - 0.5 * ref) <= NORM_TOL * 0.5 * ref
    per = opt.last_range_norms
    assert set(per) == {"enc", "dec"}
    for name, (b, e) in opt.ranges.items():
        want = 0.5 * float(g[b:e].double().norm())
        assert abs(per[name] - want) <= NORM_TOL * want, name
    assert opt.skipped == 0 and opt.steps == dict(enc=1, dec=1)
    opt.disable_guard()
    flat.grad.copy_(step_gradient(flat, 10))
    opt.step()                                                                               # the unguarded path again
    assert opt.steps == dict(enc=2, dec=2) and "skipped" not in opt.state_dict()


# ------------------------------------------------------------------------------------------------ model level
V, T, HW = 50, 12, (64, 160)


def small_transformer(seed=47):
    from test_model_gpu import make_transformer
    m, w2i = make_transformer(V, ModelConfig(num_layers=2, compute_dtype="bf16", **NO_DROP), seed, hw=HW, max_seq=T)
    m.train()
    m.teacher_forcing_prob = 0.0
    return m, w2i


def batches(w2i, count):
    return [syn.synthetic_unimodal_batch(3, HW[0], HW[1], T, V, w2i["<sos>"], w2i["<eos>"], seed=30 + i) for i in range(count)]


def on_device(batch):
    x, xl, y_in, y_out = batch
    return x.to(DEV), xl, y_in, y_out


def test_model_survives_a_poisoned_step():
    m, w2i = small_transformer()
    flat = m._flat
    opt = m.configure_optimizers()
    opt.enable_guard()
    data = [on_device(b) for b in batches(w2i, 4)]
    for step in range(3):
        random.seed(step)
        opt.zero_grad()
        loss = m.training_step(data[step], step)
        loss.backward()
        if step == 1:
            WgradStream.join()                                                               # every weight gradient is in: now poison one element
            flat.grad[flat.total // 2] = NAN
            torch.cuda.synchronize()
            master, lowp = flat.master.clone(), flat.lowp.clone()
        opt.step()
        if step == 1:
            same_bits(flat.master, master, "the poisoned step must not write master")
            same_bits(flat.lowp, lowp, "the poisoned step must not write the bf16 copy")
    assert opt.skipped == 1 and set(opt.steps.values()) == {2}
    assert torch.isfinite(flat.master).all() and torch.isfinite(flat.exp_avg).all() and torch.isfinite(flat.exp_avg_sq).all()
    assert not torch.equal(flat.master, master)                                              # step 3 was applied
    opt.zero_grad()
    assert torch.isfinite(m.training_step(data[3], 3)).item()


def test_trainer_clips_and_logs_the_gradient_norm():
    from omr_a2s_multimodal_transformer_amd.lightning_shim import Trainer
    m, w2i = small_transformer()
    data = batches(w2i, 3)
    random.seed(0)
    m.zero_grad()
    m.training_step(on_device(data[0]), 0).backward()
    WgradStream.join()
    torch.cuda.synchronize()
    first_norm = float(m._flat.grad.double().norm())
    assert first_norm > 0
    m, _ = small_transformer()
    start = m._flat.master.clone()
    random.seed(0)
    trainer = Trainer(max_epochs=1, gradient_clip_val=first_norm / 10)
    trainer.fit(m, data)
    norm = m.logged_metrics["grad_norm"]
    assert isinstance(norm, float) and norm > 0 and norm < INF
    assert trainer.callback_metrics["skipped_steps"] == 0
    assert torch.isfinite(m._flat.master).all() and not torch.equal(m._flat.master, start)
    with pytest.raises(ValueError):
        Trainer(gradient_clip_algorithm="value", gradient_clip_val=1.0)
