"""References for the optimizer recipe (omr_adamw_ema, config.lr_at, FusedAdam's EMA): an fp64 restatement of one step, an fp32
numpy transcription of the kernel's operation order, the error bound the GPU tests use, hand-written schedule values and the
inputs the kernel-level tests share.  No GPU here: tests/test_optim_refs_cpu.py checks all of it against torch on the CPU.

The bound, u = 2^-24, first order, for inputs whose gradient g > 0 and first moment m >= 0 (`inputs` below builds such): every term
of m = b1 m + (1 - b1) g and of v is then non-negative, so the relative error of m and v is the COUNT of roundings a term passes
through -- no cancellation.  Roundings of the kernel per element in step j of a run of k steps (adam_update in csrc/optim.hip),
against exact arithmetic on the same fp32 arguments:
  gi = (g * scale) * clip                                    2
  m  = fma(b1, m, (1 - b1) * gi)      1 - b1: 1, product: 1, plus gi's 2 = 4 on the new term; the fma rounds the sum once per
                                      step it lives through                                    m: 4 + k
  v  = fma(b2, v, ((1 - b2) * gi) * gi)   1 - b2: 1, two products: 2, gi twice: 4 = 7; the fma as above       v: 7 + k
  denom = fma(sqrt(v), 1/sqrt(bc2), eps)  half of v's, sqrt: 1, the host's rounding of 1/sqrt(bc2): 1, fma: 1   (7 + k) / 2 + 3
  t  = (lr / bc1) * (m / denom)       m's, denom's, the division: 1, the host's rounding of lr / bc1: 1 (the product itself is
                                      inside the last fma)                                     t: 1.5 k + 12.5
  p' = p * f                          the host's rounding of f = 1 - lr wd: 1, the product: 1   2 on |p|
  p_new = fma(-lr/bc1, m / denom, p') one rounding of the result, at most u (|p'| + |t|)        1 on |p| + |t|
So one step adds at most  (1.5 k + 13.5) u |t| + 3 u |p|  <=  P_OPS(k) u (|p| + |t|),  P_OPS(k) = 14 + 2 k  (rounded up, which also
covers the second-order terms), t = (lr / bc1) m / denom.  An error p already carries is multiplied by f <= 1 and passed on,
so over k steps the errors add:  |p_k - exact| <= sum_j P_OPS(k) u (|p_j| + |t_j|)  -- `p_bound` accumulates exactly this along the
fp64 trajectory.
  ema = fma(d, ema, omd * p_new)      the host's rounding of omd = 1 - d: 1, the product: 1 (both on |omd p| <= max), the result: 1,
                                      and |result| <= max(|ema|, |p_new|)                       E_OPS = 3 on max(|ema|, |p_new|)
An error ema carries is multiplied by d <= 1, the error of p_new comes in multiplied by omd <= 1:
  |ema_k - exact| <= sum_j (E_OPS u max(|ema_(j-1)|, |p_j|) + omd * (p's bound at step j)).
When the reference recursion runs over RECORDED fp32 weights (the model-level test) the second term is absent.
"""
import math

import numpy as np

U = 2.0 ** -24
E_OPS = 3


def P_OPS(k: int) -> int:
    """Rounded fp32 operations per element charged to one step of a k-step run (see the module docstring)."""
    return 14 + 2 * k


def f32(x: float) -> float:
    """The value a C `float` argument takes: tests hand the kernel and the fp64 restatement the SAME number."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ fp64 restatement
def ref_step(state, g, step, lr, b1, b2, eps, wd=0.0, decay_mask=None, ema_decay=None, grad_scale=1.0, clip=1.0, apply=True):
    """One step in fp64.  state = (p, m, v, ema or None) as float64 arrays; decay_mask: per-element bool (None: all decay).
    -> (new state, |t|) with t the update term (lr / bc1) m / denom.  apply=False (the guard's skip): nothing changes.
    torch optim/adamw.py single-tensor order: decay, moments, bias corrections, update; then swa_utils' EMA."""
    p, m, v, ema = state
    if not apply:
        return (p, m, v, ema), np.zeros_like(p)
    gi = g.astype(np.float64) * grad_scale * clip
    if wd != 0.0:
        f = 1.0 - lr * wd
        p = p * f if decay_mask is None else np.where(decay_mask, p * f, p)
    m = b1 * m + (1.0 - b1) * gi
    v = b2 * v + (1.0 - b2) * gi * gi
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = np.sqrt(v) / math.sqrt(bc2) + eps
    t = (lr / bc1) * (m / denom)
    p = p - t
    if ema is not None and ema_decay is not None:
        ema = ema_decay * ema + (1.0 - ema_decay) * p
    return (p, m, v, ema), np.abs(t)


def ref_run(p0, m0, v0, ema0, grads, first_step, lr, b1, b2, eps, **kw):
    """k = len(grads) steps of ref_step from fp32 inputs -> (state, p's bound, ema's bound) after the last one, the bounds
    accumulated along the trajectory as the module docstring derives them."""
    k = len(grads)
    state = (p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64), None if ema0 is None else ema0.astype(np.float64))
    pb = np.zeros(p0.shape, np.float64)
    eb = np.zeros(p0.shape, np.float64)
    d = kw.get("ema_decay")
    for j, g in enumerate(grads):
        p_before, ema_before = state[0], state[3]
        state, t = ref_step(state, g, first_step + j, lr, b1, b2, eps, **kw)
        step_err = P_OPS(k) * U * (np.abs(p_before) + t)
        pb = pb + step_err
        if ema_before is not None and d is not None:
            eb = eb + E_OPS * U * np.maximum(np.abs(ema_before), np.abs(state[0])) + (1.0 - d) * pb
    return state, pb, eb


def ema_recursion(snapshots, ema0, d):
    """fp64 EMA over recorded weights: -> (ema, bound); bound = sum_j E_OPS u max(|ema_(j-1)|, |p_j|)."""
    ema = ema0.astype(np.float64)
    bound = np.zeros(ema.shape, np.float64)
    for p in snapshots:
        p = p.astype(np.float64)
        bound = bound + E_OPS * U * np.maximum(np.abs(ema), np.abs(p))
        ema = d * ema + (1.0 - d) * p
    return ema, bound


# ------------------------------------------------------------------------------------------------ the kernel's order, in fp32 numpy
def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64; the sum is rounded to fp64 and then to fp32 (a double rounding
    that differs from the hardware's single one in rare ties only -- this transcription checks the BOUND, never bits)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def kernel_f32_step(state, g, step, lr, b1, b2, eps, wd=0.0, decay_mask=None, ema_decay=None, grad_scale=1.0, clip=1.0):
    """omr_adamw_ema's operations, one rounded fp32 operation per line, on float32 arrays."""
    F = np.float32
    p, m, v, ema = state
    lr, b1, b2, eps = F(lr), F(b1), F(b2), F(eps)
    bc1, bc2 = 1.0 - float(b1) ** step, 1.0 - float(b2) ** step
    lrb, isb2 = F(float(lr) / bc1), F(1.0 / math.sqrt(bc2))
    gi = (g * F(grad_scale)) * F(clip)
    if wd != 0.0:
        f = F(1.0 - float(lr) * float(F(wd)))
        pd = p * f
        p = pd if decay_mask is None else np.where(decay_mask, pd, p)
    m = _fma(b1, m, (F(1) - b1) * gi)
    v = _fma(b2, v, ((F(1) - b2) * gi) * gi)
    denom = _fma(np.sqrt(v), isb2, eps)
    p = _fma(-lrb, m / denom, p)
    if ema is not None and ema_decay is not None:
        d = F(ema_decay)
        omd = F(1.0 - float(d))
        ema = _fma(d, ema, omd * p)
    return (p, m, v, ema)


# ------------------------------------------------------------------------------------------------ shared inputs
HYPER = dict(lr=f32(1e-3), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8))
WD = f32(0.1)
GRAD_SCALE = 0.5
FIRST_STEP = 3          # the run starts at optimizer step 3: both bias corrections are away from their first-step values


def inputs(n: int, seed: int, steps: int):
    """(p, m, v, ema, [g_1 .. g_steps]) as float32 arrays: p and ema signed, g > 0, m >= 0, v >= 0 (the bound's premise)."""
    rng = np.random.RandomState(seed)
    p = rng.standard_normal(n).astype(np.float32)
    m = (0.1 * rng.rand(n)).astype(np.float32)
    v = (0.01 * rng.rand(n)).astype(np.float32)
    ema = (p + 0.05 * rng.standard_normal(n)).astype(np.float32)
    grads = [((0.1 + rng.rand(n)) * (1 + j)).astype(np.float32) for j in range(steps)]
    return p, m, v, ema, grads


def block_mask(n: int, block: int = 64):
    """An alternating decay-block map (block 0 decays, block 1 does not, ...) -> (bytes [ceil(n / block)], per-element bool [n])."""
    nb = (n + block - 1) // block
    blocks = (np.arange(nb) % 2 == 0).astype(np.uint8)
    return blocks, np.repeat(blocks, block)[:n].astype(bool)


# ------------------------------------------------------------------------------------------------ schedule, by hand
LR0 = 1e-3
_COS_7_8 = 0.1 + 0.9 * 0.03806023374435663          # (1 + cos(7 pi / 8)) / 2 = 0.0380602337...
SCHEDULE = dict(warmup_steps=4, total_steps=12, min_lr_ratio=0.1)
LR_CASES = [
    # (OptimConfig arguments besides lr, {k: lr_at / LR0})
    (dict(schedule="cosine", **SCHEDULE), {0: 0.25, 3: 1.0, 4: 1.0, 8: 0.55, 11: _COS_7_8, 12: 0.1, 100: 0.1}),
    (dict(schedule="linear", **SCHEDULE), {0: 0.25, 3: 1.0, 4: 1.0, 8: 0.55, 11: 0.2125, 12: 0.1, 100: 0.1}),
    (dict(schedule="constant", warmup_steps=4), {0: 0.25, 1: 0.5, 3: 1.0, 4: 1.0, 100: 1.0}),
    (dict(schedule="constant"), {0: 1.0, 1: 1.0, 100: 1.0}),
]
