// The per-element Adam update, written ONCE for adam_kernel (elementwise.hip) and adam_guarded_kernel (optim.hip).
// torch optim/adam.py:347 single-tensor math (model.py:134-139: lr 1e-4, betas (0.9,0.999), eps 1e-8):
//   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// gi is the gradient as the update sees it (scaled, and clipped in the guarded step).  Optionally writes the bf16 compute copy of
// the updated parameter in the same pass.
//
// The library is built with -ffp-contract=fast, under which two copies of `a * b + c` -- or one copy inlined into two kernels --
// are not guaranteed to contract into the same fma chain (moving the expression into this function did change adam_kernel's
// chain).  So every multiply-add is spelled out as the fma omr_adam has always executed (read off adam_kernel's ISA):
//   m = fma(b1, m, (1-b1) g)   v = fma(b2, v, ((1-b2) g) g)   denom = fma(sqrt(v), 1/sqrt(bc2), eps)   p = fma(-lr/bc1, m / denom, p)
// No fmul -> fadd pair is left for the contraction pass: both kernels execute these roundings, whatever surrounds the call.
#pragma once
#include "omr_common.h"

__device__ __forceinline__ void adam_update(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, bf16* __restrict__ p_lp, long i,
                                            float gi, float lr_over_bc1, float b1, float b2, float eps, float inv_sqrt_bc2) {
    float mi = __builtin_fmaf(b1, m[i], (1.f - b1) * gi);
    float vi = __builtin_fmaf(b2, v[i], ((1.f - b2) * gi) * gi);
    float denom = __builtin_fmaf(sqrtf(vi), inv_sqrt_bc2, eps);
    float pi = __builtin_fmaf(-lr_over_bc1, mi / denom, p[i]);
    m[i] = mi; v[i] = vi; p[i] = pi;
    if (p_lp) p_lp[i] = (bf16)pi;
}

// The same update on values held in registers, for adamw_ema_kernel (optim.hip), which loads and stores 16 bytes at a time and
// wraps the update in two more fused steps (torch optim/adamw.py single-tensor math; optim/swa_utils.py get_ema_multi_avg_fn):
//   before:  p' = p * f, f = (float)(1 - lr wd) from the host, only where the element decays -- the caller passes p' as `pi`
//   after:   ema = fma(d, ema, (1-d) p_new)                                                  -- ema_update below
// The four roundings of m, v, denom and p are the ones above, operand for operand, so with p' = p this function leaves
// adam_update's bits.  Neither wrapper leaves an fmul -> fadd pair either: a product only ever feeds an explicit fma.
__device__ __forceinline__ void adam_update_reg(float& pi, float& mi, float& vi, float gi, float lr_over_bc1, float b1, float b2, float eps,
                                                float inv_sqrt_bc2) {
    mi = __builtin_fmaf(b1, mi, (1.f - b1) * gi);
    vi = __builtin_fmaf(b2, vi, ((1.f - b2) * gi) * gi);
    float denom = __builtin_fmaf(sqrtf(vi), inv_sqrt_bc2, eps);
    pi = __builtin_fmaf(-lr_over_bc1, mi / denom, pi);
}

// d = (float)decay and omd = (float)(1 - decay) come from the host.  d = 0: omd = 1, fma(0, ema, p) = p's bits (a finite ema);
// d = 1: omd = 0, fma(1, ema, 0 * p) = ema's bits (a finite p).
__device__ __forceinline__ float ema_update(float ema, float p_new, float d, float omd) { return __builtin_fmaf(d, ema, omd * p_new); }
