// What the CTC loss (ctc.hip) and the CTC prefix scores of the joint beam search (ctc_prefix.hip) share, each written once: the clamp of a
// device-side frame count, the frames' log-sum-exp pass and the two-term log-add.
#pragma once
#include "loss_rows.h"

namespace {

__device__ __forceinline__ int clamp_len(int n, int Fmax) { return min(max(n, 0), Fmax); }

// One workgroup per frame: the row pass of ce_fwd_kernel (loss_rows.h).  Frames >= F_b are skipped.
template <typename T>
__global__ __launch_bounds__(256) void ctc_lse_kernel(const T* __restrict__ logits, const int* __restrict__ frame_len, float* __restrict__ lse, int Fmax,
                                                      int V, long ldv) {
    __shared__ float red_m[4], red_s[4];
    const int b = blockIdx.y, f = blockIdx.x;
    if (f >= clamp_len(frame_len[b], Fmax)) return;
    const long row = (long)b * Fmax + f;
    float mx = -INFINITY, s = 0.f, rs = 0.f;
    row_online_pass<T, false>(logits + row * ldv, row_vec_ok<T>(logits, ldv), V, mx, s, rs);
    const float l = block_lse(mx, s, 1.f, red_m, red_s);
    if (threadIdx.x == 0) lse[row] = l;
}

__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    return m == -INFINITY ? -INFINITY : m + log1pf(expf(fminf(a, b) - m));
}

}  // namespace
