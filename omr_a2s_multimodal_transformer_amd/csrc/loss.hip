// Cross-entropy over the vocabulary with ignore_index (gfx950).
// Reference: CrossEntropyLoss(ignore_index=PAD) on logits [B,V,T] (model.py:109,166) =
// mean over targets != PAD of  logsumexp_v(logits) - logits[target].
// With label smoothing eps (torch's label_smoothing; an extension, the reference trains with 0) a live row's objective is
//   lse - (1 - eps) * logits[target] - (eps / V) * sum_{v < V} logits[v],
// and the plain mean above is reported next to it.  SMOOTH = false instantiates exactly the kernels of the unsmoothed loss.
// Internally logits are row-major [M = B*T][ldv >= V] (the [B,V,T] view is a stride permutation).
#include <type_traits>
#include "omr_common.h"
#include "omr_hip.h"

namespace {

// One workgroup per row: a single vectorised pass keeps a running (max, sum of exp) per thread (online softmax), then
// combines across the workgroup.  Only lse[row] is written: the loss itself is reduced by ce_finalize_kernel in a fixed
// order (no atomics: device-scope atomics on one address serialise at the memory side, and the sum stays deterministic).
// SMOOTH: the same loop also carries rs, the fp32 sum of the thread's logits (columns < V only: the padding may hold anything), added
// in column order; rowsum[row] = the xor-butterfly wave_sum of the 64 rs, then ((w0 + w1) + w2) + w3 over the four waves.
template <typename T, bool SMOOTH>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const T* __restrict__ logits, float* __restrict__ lse, int V, long ldv, float* __restrict__ rowsum) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = Frag<T>::N;
    __shared__ float red_m[4], red_s[4], red_r[4];
    const long row = blockIdx.x;
    const T* lr = logits + row * ldv;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float mx = -INFINITY, s = 0.f, rs = 0.f;
    const bool vec_ok = (ldv % VEC) == 0 && (((uintptr_t)logits) & 15) == 0;
    if (vec_ok) {
        for (int v0 = threadIdx.x * VEC; v0 < V; v0 += 256 * VEC) {
            const F f = *reinterpret_cast<const F*>(lr + v0);      // v0 + VEC <= ldv: the padding columns are readable
            float x[VEC], cm = -INFINITY;
#pragma unroll
            for (int e = 0; e < VEC; ++e) { x[e] = (v0 + e < V) ? to_f32(f[e]) : -INFINITY; cm = fmaxf(cm, x[e]); }
            const float nm = fmaxf(mx, cm);
            const float sub = nm == -INFINITY ? 0.f : nm;      // only -inf so far: exp(-inf - -inf) is NaN, exp(-inf - 0) = 0 keeps s
            float add = 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) add += __expf(x[e] - sub);
            s = s * __expf(mx - sub) + add;
            mx = nm;
            if constexpr (SMOOTH) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) rs += (v0 + e < V) ? to_f32(f[e]) : 0.f;
            }
        }
    } else {
        for (int v = threadIdx.x; v < V; v += 256) {
            const float x = to_f32(lr[v]), nm = fmaxf(mx, x);
            const float sub = nm == -INFINITY ? 0.f : nm;      // as above
            s = s * __expf(mx - sub) + __expf(x - sub);
            mx = nm;
            if constexpr (SMOOTH) rs += x;
        }
    }
    const float wm = wave_max(mx);
    s = wave_sum(mx == -INFINITY ? 0.f : s * __expf(mx - wm));
    if (lane == 0) { red_m[wv] = wm; red_s[wv] = s; }
    if constexpr (SMOOTH) {
        rs = wave_sum(rs);
        if (lane == 0) red_r[wv] = rs;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) t += red_m[i] == -INFINITY ? 0.f : red_s[i] * __expf(red_m[i] - m);
        lse[row] = m + logf(t);
        if constexpr (SMOOTH) rowsum[row] = ((red_r[0] + red_r[1]) + red_r[2]) + red_r[3];
    }
}

// acc[0] = sum over live rows of lse - logit[target], acc[1] = number of live rows, loss = mean.  One workgroup, fixed order.
template <typename T>
__global__ __launch_bounds__(1024) void ce_finalize_kernel(const T* __restrict__ logits, const long* __restrict__ target, const float* __restrict__ lse,
                                                           double* __restrict__ acc, float* __restrict__ loss, long M, int V, long ldv, int pad_idx) {
    __shared__ double rs[16], rc[16];
    double s = 0.0, c = 0.0;
    for (long row = threadIdx.x; row < M; row += 1024) {
        const long t = target[row];
        if (t != pad_idx && t >= 0 && t < V) { s += (double)(lse[row] - to_f32(logits[row * ldv + t])); c += 1.0; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); c += __shfl_xor(c, o, 64); }
    if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = s; rc[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ts = 0.0, tc = 0.0;
        for (int i = 0; i < 16; ++i) { ts += rs[i]; tc += rc[i]; }
        acc[0] = ts; acc[1] = tc;
        loss[0] = (float)(ts / tc);
    }
}

// The finalize of the smoothed loss, in the order of the one above: acc[0] = sum over live rows of the objective
// lse - (1 - eps) logit[target] - (eps / V) rowsum (formed in fp64), acc[1] = number of live rows, acc[2] = sum of the plain
// lse - logit[target]; loss and nll are the two means.  eps == 0 adds the very fp32 difference the kernel above adds and never reads
// rowsum: 0 * rowsum would be NaN on a row that holds -inf.
template <typename T>
__global__ __launch_bounds__(1024) void ce_smooth_finalize_kernel(const T* __restrict__ logits, const long* __restrict__ target, const float* __restrict__ lse,
                                                                  const float* __restrict__ rowsum, double* __restrict__ acc, float* __restrict__ loss,
                                                                  float* __restrict__ nll, long M, int V, long ldv, int pad_idx, float eps) {
    __shared__ double rs[16], rc[16], rn[16];
    double s = 0.0, c = 0.0, n = 0.0;
    const double keep = 1.0 - (double)eps, uni = (double)eps / (double)V;
    for (long row = threadIdx.x; row < M; row += 1024) {
        const long t = target[row];
        if (t != pad_idx && t >= 0 && t < V) {
            const float l = lse[row], xt = to_f32(logits[row * ldv + t]);
            const double plain = (double)(l - xt);
            s += eps > 0.f ? (double)l - keep * (double)xt - uni * (double)rowsum[row] : plain;
            n += plain;
            c += 1.0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); c += __shfl_xor(c, o, 64); n += __shfl_xor(n, o, 64); }
    if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = s; rc[threadIdx.x >> 6] = c; rn[threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ts = 0.0, tc = 0.0, tn = 0.0;
        for (int i = 0; i < 16; ++i) { ts += rs[i]; tc += rc[i]; tn += rn[i]; }
        acc[0] = ts; acc[1] = tc; acc[2] = tn;
        loss[0] = (float)(ts / tc);
        nll[0] = (float)(tn / tc);
    }
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
    const bool live = (t != pad_idx && t >= 0 && t < V);
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
// formula is applied in fp64 before the one rounding to fp32.  Z: per thread in column order, xor butterfly over the wave, ((w0 + w1) + w2) + w3.
// The second sweep reads the row from cache.  bf16 rows round at 2^-8 and keep the fp32 arithmetic of ce_bwd_kernel.
__global__ __launch_bounds__(256) void ce_smooth_bwd_f32_kernel(const float* __restrict__ logits, const long* __restrict__ target, const float* __restrict__ lse,
                                                                const double* __restrict__ acc, float* __restrict__ dlogits, int V, long ldv, int pad_idx,
                                                                float gscale, const float* __restrict__ grad_out, float eps) {
    __shared__ double red_z[4];
    const long row = blockIdx.x;
    const long t = target[row];
    const bool live = (t != pad_idx && t >= 0 && t < V);      // the same for the whole workgroup
    const float* lr = logits + row * ldv;
    float* dr = dlogits + row * ldv;
    if (!live) {
        for (int v = threadIdx.x; v < ldv; v += 256) dr[v] = 0.f;
        return;
    }
    const double l = (double)lse[row];
    double z = 0.0;
    for (int v = threadIdx.x; v < V; v += 256) z += exp((double)lr[v] - l);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
    if ((threadIdx.x & 63) == 0) red_z[threadIdx.x >> 6] = z;
    __syncthreads();
    const double inv = 1.0 / (((red_z[0] + red_z[1]) + red_z[2]) + red_z[3]);
    const double sc = (double)gscale * (double)(grad_out ? grad_out[0] : 1.f) / acc[1];
    const double keep = 1.0 - (double)eps, uni = (double)eps / (double)V;
    for (int v = threadIdx.x; v < ldv; v += 256)
        dr[v] = v < V ? (float)((exp((double)lr[v] - l) * inv - (v == t ? keep : 0.0) - uni) * sc) : 0.f;
}

template <typename T>
void launch_ce_fwd(const void* logits, const long* target, float* lse, double* acc2, float* loss_out, long M, int V, long ldv, int pad_idx, hipStream_t s) {
    hipLaunchKernelGGL((ce_fwd_kernel<T, false>), (int)M, 256, 0, s, (const T*)logits, lse, V, ldv, (float*)nullptr);
    hipLaunchKernelGGL((ce_finalize_kernel<T>), 1, 1024, 0, s, (const T*)logits, target, (const float*)lse, acc2, loss_out, M, V, ldv, pad_idx);
}

// eps == 0: the unsmoothed row kernel (rowsum is not written), and the finalize that also reports the plain mean.
template <typename T>
void launch_ce_smooth_fwd(const void* logits, const long* target, float* lse, float* rowsum, double* acc3, float* loss_out, float* nll_out, long M, int V,
                          long ldv, int pad_idx, float eps, hipStream_t s) {
    if (eps > 0.f) hipLaunchKernelGGL((ce_fwd_kernel<T, true>), (int)M, 256, 0, s, (const T*)logits, lse, V, ldv, rowsum);
    else hipLaunchKernelGGL((ce_fwd_kernel<T, false>), (int)M, 256, 0, s, (const T*)logits, lse, V, ldv, (float*)nullptr);
    hipLaunchKernelGGL((ce_smooth_finalize_kernel<T>), 1, 1024, 0, s, (const T*)logits, target, (const float*)lse, (const float*)rowsum, acc3, loss_out,
                       nll_out, M, V, ldv, pad_idx, eps);
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

}  // namespace

extern "C" int omr_ce_fwd(int dtype, const void* logits, const long* target, float* lse, double* acc2, float* loss_out, long M, int V, long ldv,
                          int pad_idx, void* stream) {
    if (M <= 0 || V <= 0 || ldv < V) return OMR_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == OMR_F32) launch_ce_fwd<float>(logits, target, lse, acc2, loss_out, M, V, ldv, pad_idx, s);
    else if (dtype == OMR_BF16) launch_ce_fwd<bf16>(logits, target, lse, acc2, loss_out, M, V, ldv, pad_idx, s);
    else return OMR_ERR_UNSUPPORTED;
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_ce_bwd(int dtype, const void* logits, const long* target, const float* lse, const double* acc2, void* dlogits, long M, int V,
                          long ldv, int pad_idx, float grad_scale, const float* grad_out, void* stream) {
    if (M <= 0 || V <= 0 || ldv < V) return OMR_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == OMR_F32) launch_ce_bwd<float>(logits, target, lse, acc2, dlogits, M, V, ldv, pad_idx, 0.f, grad_scale, grad_out, s);
    else if (dtype == OMR_BF16) launch_ce_bwd<bf16>(logits, target, lse, acc2, dlogits, M, V, ldv, pad_idx, 0.f, grad_scale, grad_out, s);
    else return OMR_ERR_UNSUPPORTED;
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_ce_smooth_fwd(int dtype, const void* logits, const long* target, float* lse, float* rowsum, double* acc3, float* loss_out,
                                 float* nll_out, long M, int V, long ldv, int pad_idx, float eps, void* stream) {
    if (M <= 0 || V <= 0 || ldv < V || !(eps >= 0.f && eps <= 1.f) || (eps > 0.f && rowsum == nullptr)) return OMR_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == OMR_F32) launch_ce_smooth_fwd<float>(logits, target, lse, rowsum, acc3, loss_out, nll_out, M, V, ldv, pad_idx, eps, s);
    else if (dtype == OMR_BF16) launch_ce_smooth_fwd<bf16>(logits, target, lse, rowsum, acc3, loss_out, nll_out, M, V, ldv, pad_idx, eps, s);
    else return OMR_ERR_UNSUPPORTED;
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_ce_smooth_bwd(int dtype, const void* logits, const long* target, const float* lse, const double* acc3, void* dlogits, long M, int V,
                                 long ldv, int pad_idx, float eps, float grad_scale, const float* grad_out, void* stream) {
    if (M <= 0 || V <= 0 || ldv < V || !(eps >= 0.f && eps <= 1.f)) return OMR_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == OMR_F32) launch_ce_bwd<float>(logits, target, lse, acc3, dlogits, M, V, ldv, pad_idx, eps, grad_scale, grad_out, s);
    else if (dtype == OMR_BF16) launch_ce_bwd<bf16>(logits, target, lse, acc3, dlogits, M, V, ldv, pad_idx, eps, grad_scale, grad_out, s);
    else return OMR_ERR_UNSUPPORTED;
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}
