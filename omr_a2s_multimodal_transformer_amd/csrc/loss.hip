// Cross-entropy over the vocabulary with ignore_index (gfx950).
// Reference: CrossEntropyLoss(ignore_index=PAD) on logits [B,V,T] (model.py:109,166) =
// mean over targets != PAD of  logsumexp_v(logits) - logits[target].
// With label smoothing eps (torch's label_smoothing; an extension, the reference trains with 0) a live row's objective is
//   lse - (1 - eps) * logits[target] - (eps / V) * sum_{v < V} logits[v],
// and the plain mean above is reported next to it.  SMOOTH = false instantiates exactly the kernels of the unsmoothed loss.
// Internally logits are row-major [M = B*T][ldv >= V] (the [B,V,T] view is a stride permutation).
// The steps shared with distill.hip, the finalize (ce_finalize_kernel) among them, are in loss_rows.h.
#include <type_traits>
#include "loss_rows.h"
#include "omr_hip.h"

namespace {

// One workgroup per row: a single vectorised pass keeps a running (max, sum of exp) per thread (online softmax), then
// combines across the workgroup (block_lse at k = 1).  Only lse[row] is written: the loss itself is reduced by ce_finalize_kernel.
// SMOOTH: the same loop also carries rs, the fp32 sum of the thread's logits (columns < V only: the padding may hold anything), added
// in column order; rowsum[row] = block_sum of the 256 rs.
template <typename T, bool SMOOTH>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const T* __restrict__ logits, float* __restrict__ lse, int V, long ldv, float* __restrict__ rowsum) {
    __shared__ float red_m[4], red_s[4], red_r[4];
    const long row = blockIdx.x;
    float mx = -INFINITY, s = 0.f, rs = 0.f;
    row_online_pass<T, SMOOTH>(logits + row * ldv, row_vec_ok<T>(logits, ldv), V, mx, s, rs);
    if constexpr (SMOOTH) {
        rs = block_sum(rs, red_r);
        if (threadIdx.x == 0) rowsum[row] = rs;
    }
    const float l = block_lse(mx, s, 1.f, red_m, red_s);
    if (threadIdx.x == 0) lse[row] = l;
}

// dlogits = (softmax - onehot) * gscale / count on rows whose target != PAD, else 0.
// SMOOTH (launched for bf16; fp32 logits take ce_smooth_bwd_f32_kernel): (softmax - (1 - eps) * onehot - eps / V) * gscale / count, in fp32
// before the one rounding to T.
template <typename T, bool SMOOTH>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const T* __restrict__ logits, const long* __restrict__ target, const float* __restrict__ lse,
                                                     const double* __restrict__ acc, T* __restrict__ dlogits, int V, long ldv, int pad_idx,
                                                     float gscale, const float* __restrict__ grad_out, float eps) {
    const long row = blockIdx.x;
    const long t = target[row];
    const bool live = row_live(t, pad_idx, V);
    const float l = lse[row];
    const float sc = live ? gscale * (grad_out ? grad_out[0] : 1.f) / (float)acc[1] : 0.f;
    const T* lr = logits + row * ldv;
    T* dr = dlogits + row * ldv;
    const float keep = 1.f - eps, uni = eps / (float)V;
    for (int v = threadIdx.x; v < ldv; v += 256) {
        float d = 0.f;
        if constexpr (SMOOTH) {
            if (live && v < V) d = (__expf(to_f32(lr[v]) - l) - (v == t ? keep : 0.f) - uni) * sc;
        } else {
            if (live && v < V) d = (__expf(to_f32(lr[v]) - l) - (v == t ? 1.f : 0.f)) * sc;
        }
        dr[v] = from_f32<T>(d);
    }
}

// The smoothed gradient of fp32 logits.  The exact gradient of a live row sums to 0 over v < V (1 - (1 - eps) - V eps / V), and the fp32 rows
// keep that to the rounding of the values themselves, |sum_v dlogits[row, v]| <= 2^-24 sum_v |dlogits[row, v]|: the softmax is normalised by
// the row's own Z = sum_v exp(x_v - lse) instead of trusting the fp32 lse (whose rounding alone moves every term by 2^-24 |lse|), and the
// formula is applied in fp64 before the one rounding to fp32.  Z: per thread in column order, then block_sum.
// The second sweep reads the row from cache.  bf16 rows round at 2^-8 and keep the fp32 arithmetic of ce_bwd_kernel.
__global__ __launch_bounds__(256) void ce_smooth_bwd_f32_kernel(const float* __restrict__ logits, const long* __restrict__ target, const float* __restrict__ lse,
                                                                const double* __restrict__ acc, float* __restrict__ dlogits, int V, long ldv, int pad_idx,
                                                                float gscale, const float* __restrict__ grad_out, float eps) {
    __shared__ double red_z[4];
    const long row = blockIdx.x;
    const long t = target[row];
    const float* lr = logits + row * ldv;
    float* dr = dlogits + row * ldv;
    if (!row_live(t, pad_idx, V)) {                               // the same for the whole workgroup
        for (int v = threadIdx.x; v < ldv; v += 256) dr[v] = 0.f;
        return;
    }
    const double l = (double)lse[row];
    double z = 0.0;
    for (int v = threadIdx.x; v < V; v += 256) z += exp((double)lr[v] - l);
    const double inv = 1.0 / block_sum(z, red_z);
    const double sc = (double)gscale * (double)(grad_out ? grad_out[0] : 1.f) / acc[1];
    const double keep = 1.0 - (double)eps, uni = (double)eps / (double)V;
    for (int v = threadIdx.x; v < ldv; v += 256)
        dr[v] = v < V ? (float)((exp((double)lr[v] - l) * inv - (v == t ? keep : 0.0) - uni) * sc) : 0.f;
}

// CE_SMOOTH at eps == 0 still runs the unsmoothed row kernel (rowsum is not written), and the finalize that also reports the plain mean.
template <typename T, int MODE>
void launch_ce_fwd(const void* logits, const long* target, float* lse, float* rowsum, double* acc, float* loss_out, float* nll_out, long M, int V,
                   long ldv, int pad_idx, float eps, hipStream_t s) {
    if (eps > 0.f) hipLaunchKernelGGL((ce_fwd_kernel<T, true>), (int)M, 256, 0, s, (const T*)logits, lse, V, ldv, rowsum);
    else hipLaunchKernelGGL((ce_fwd_kernel<T, false>), (int)M, 256, 0, s, (const T*)logits, lse, V, ldv, (float*)nullptr);
    hipLaunchKernelGGL((ce_finalize_kernel<T, MODE>), 1, 1024, 0, s, (const T*)logits, target, (const float*)lse, (const float*)rowsum, acc, loss_out,
                       nll_out, (float*)nullptr, M, V, ldv, pad_idx, eps);
}

template <typename T>
void launch_ce_bwd(const void* logits, const long* target, const float* lse, const double* acc, void* dlogits, long M, int V, long ldv, int pad_idx,
                   float eps, float grad_scale, const float* grad_out, hipStream_t s) {
    if (eps > 0.f) {
        if constexpr (std::is_same<T, float>::value)
            hipLaunchKernelGGL(ce_smooth_bwd_f32_kernel, (int)M, 256, 0, s, (const float*)logits, target, lse, acc, (float*)dlogits, V, ldv, pad_idx, grad_scale, grad_out, eps);
        else
            hipLaunchKernelGGL((ce_bwd_kernel<T, true>), (int)M, 256, 0, s, (const T*)logits, target, lse, acc, (T*)dlogits, V, ldv, pad_idx, grad_scale, grad_out, eps);
    }
    else hipLaunchKernelGGL((ce_bwd_kernel<T, false>), (int)M, 256, 0, s, (const T*)logits, target, lse, acc, (T*)dlogits, V, ldv, pad_idx, grad_scale, grad_out, 0.f);
}

bool eps_ok(float eps) { return eps >= 0.f && eps <= 1.f; }      // NaN fails

}  // namespace

extern "C" int omr_ce_fwd(int dtype, const void* logits, const long* target, float* lse, double* acc2, float* loss_out, long M, int V, long ldv,
                          int pad_idx, void* stream) {
    if (!loss_rows_ok(M, V, ldv)) return OMR_ERR_ARG;
    DISPATCH_T(dtype, (launch_ce_fwd<T, CE_PLAIN>(logits, target, lse, nullptr, acc2, loss_out, nullptr, M, V, ldv, pad_idx, 0.f, (hipStream_t)stream)))
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_ce_bwd(int dtype, const void* logits, const long* target, const float* lse, const double* acc2, void* dlogits, long M, int V,
                          long ldv, int pad_idx, float grad_scale, const float* grad_out, void* stream) {
    return omr_ce_smooth_bwd(dtype, logits, target, lse, acc2, dlogits, M, V, ldv, pad_idx, 0.f, grad_scale, grad_out, stream);
}

extern "C" int omr_ce_smooth_fwd(int dtype, const void* logits, const long* target, float* lse, float* rowsum, double* acc3, float* loss_out,
                                 float* nll_out, long M, int V, long ldv, int pad_idx, float eps, void* stream) {
    if (!loss_rows_ok(M, V, ldv) || !eps_ok(eps) || (eps > 0.f && rowsum == nullptr)) return OMR_ERR_ARG;
    DISPATCH_T(dtype, (launch_ce_fwd<T, CE_SMOOTH>(logits, target, lse, rowsum, acc3, loss_out, nll_out, M, V, ldv, pad_idx, eps, (hipStream_t)stream)))
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_ce_smooth_bwd(int dtype, const void* logits, const long* target, const float* lse, const double* acc3, void* dlogits, long M, int V,
                                 long ldv, int pad_idx, float eps, float grad_scale, const float* grad_out, void* stream) {
    if (!loss_rows_ok(M, V, ldv) || !eps_ok(eps)) return OMR_ERR_ARG;
    DISPATCH_T(dtype, launch_ce_bwd<T>(logits, target, lse, acc3, dlogits, M, V, ldv, pad_idx, eps, grad_scale, grad_out, (hipStream_t)stream))
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}
