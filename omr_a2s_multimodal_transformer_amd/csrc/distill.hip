// Knowledge distillation: cross-entropy on the hard labels plus the KL divergence to one or two teachers, fused (gfx950).
// An extension: the reference trains from hard labels alone (model.py:109,166).  Rows as in loss.hip: student logits x row-major
// [M][ldv >= V], teacher logits a (and optionally b) row-major [M][ldt >= V], a row is live when its target is not pad and lies in [0, V).
// Per live row, over the columns v < V only (the padding may hold anything in all three tensors):
//   p = softmax(x)   pt = softmax(x / tau)   q = alpha softmax(a / tau) + (1 - alpha) softmax(b / tau)
//   nll = lse(x) - x_t      kd = tau^2 sum_v q_v (log q_v - log pt_v)   (terms with q_v = 0 are 0: torch's xlogy / kl_div rule)
//   objective = (1 - lam) nll + lam kd
//   dx_v = ((1 - lam)(p_v - [v = t]) + lam tau (pt_v - q_v)) grad_scale grad_out / count
// loss, nll, kd are the means over the live rows.  lam == 0 is the plain loss and goes to omr_ce_fwd / omr_ce_bwd as they are.
//
// Every row kernel walks the row in chunks of 8 columns per thread (thread i owns columns 8 i .. 8 i + 7, then 2048 further on), the
// same chunks in all three tensors whatever their dtypes: one 16-byte load per chunk in bf16, two in fp32, where the tensor's pitch and
// base allow, else 8 scalar loads -- decided per tensor.  Every sum: per thread in column order, xor butterfly over the wave,
// ((w0 + w1) + w2) + w3 over the four waves (loss_rows.h, which holds every step shared with loss.hip).  No atomics: two runs give the same bits.
#include "loss_rows.h"
#include "omr_hip.h"

namespace {

template <typename T> __device__ __forceinline__ bool row_vec_ok(const T* base, long ld) {
    return (ld % Frag<T>::N) == 0 && (((uintptr_t)base) & 15) == 0;
}

// o[e] = row[v0 + e] for v0 + e < V, -inf past V (never the padding's value).  v0 is a multiple of 8, so with vec (row_vec_ok) every 16-byte
// load is aligned; it stays inside the row's pitch: ld is a multiple of the fragment and v0 < V <= ld (bf16: v0 + 8 <= ld; fp32: the upper
// half is loaded only when v0 + 4 < V, hence v0 + 8 <= ld).
__device__ __forceinline__ void load8(const float* __restrict__ r, int v0, int V, bool vec, float (&o)[8]) {
    if (vec) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(r + v0);
        f32x4 hi = {0.f, 0.f, 0.f, 0.f};
        if (v0 + 4 < V) hi = *reinterpret_cast<const f32x4*>(r + v0 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] = (v0 + e < V) ? lo[e] : -INFINITY; o[4 + e] = (v0 + 4 + e < V) ? hi[e] : -INFINITY; }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (v0 + e < V) ? r[v0 + e] : -INFINITY;
    }
}
__device__ __forceinline__ void load8(const bf16* __restrict__ r, int v0, int V, bool vec, float (&o)[8]) {
    if (vec) {
        const bf16x8 f = *reinterpret_cast<const bf16x8*>(r + v0);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (v0 + e < V) ? (float)f[e] : -INFINITY;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (v0 + e < V) ? (float)r[v0 + e] : -INFINITY;
    }
}

// d[e] -> row[v0 + e] for v0 + e < ld (the caller has put +0 in the columns >= V).
__device__ __forceinline__ void store8(float* __restrict__ r, int v0, long ld, bool vec, const float (&d)[8]) {
    if (vec) {
        *reinterpret_cast<f32x4*>(r + v0) = f32x4{d[0], d[1], d[2], d[3]};
        if (v0 + 4 < ld) *reinterpret_cast<f32x4*>(r + v0 + 4) = f32x4{d[4], d[5], d[6], d[7]};
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) if (v0 + e < ld) r[v0 + e] = d[e];
    }
}
__device__ __forceinline__ void store8(bf16* __restrict__ r, int v0, long ld, bool vec, const float (&d)[8]) {
    if (vec) {
        bf16x8 f;
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (bf16)d[e];
        *reinterpret_cast<bf16x8*>(r + v0) = f;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) if (v0 + e < ld) r[v0 + e] = (bf16)d[e];
    }
}

// One workgroup per row.  Sweep 1 keeps, per thread and online, the student's maximum with its two sums of exponentials (at 1 and at
// 1 / tau: they share the maximum) and each teacher's maximum and sum at 1 / tau; the four row constants follow.  Sweep 2 re-reads the
// three rows (from cache: they were just read) and sums q_v (log q_v - log pt_v).  One teacher: log q_v = a_v / tau - lse_a exactly, no
// logf.  A column with q_v = 0 (a teacher logit of -inf, a grammar-masked teacher) adds nothing, whatever the student holds there.
// Ignored rows read nothing and store zeros.
template <typename TS, typename TT, bool TWO>
__global__ __launch_bounds__(256) void distill_fwd_kernel(const TS* __restrict__ logits, long ldv, const TT* __restrict__ ta, const TT* __restrict__ tb,
                                                          long ldt, const long* __restrict__ target, float* __restrict__ lse4,
                                                          float* __restrict__ rowkd, long M, int V, int pad_idx, float alpha, float tau) {
    __shared__ float red_m[4], red_s[4];
    const long row = blockIdx.x;
    const long t = target[row];
    if (!row_live(t, pad_idx, V)) {                               // the same for the whole workgroup
        if (threadIdx.x < 4) lse4[threadIdx.x * M + row] = 0.f;
        if (threadIdx.x == 4) rowkd[row] = 0.f;
        return;
    }
    const TS* xr = logits + row * ldv;
    const TT* ar = ta + row * ldt;
    const TT* br = TWO ? tb + row * ldt : nullptr;
    const bool vx = row_vec_ok(logits, ldv), va = row_vec_ok(ta, ldt), vb = TWO ? row_vec_ok(tb, ldt) : false;
    const float k = 1.f / tau;
    float mx = -INFINITY, s1 = 0.f, st = 0.f, ma = -INFINITY, sa = 0.f, mb = -INFINITY, sb = 0.f;
    for (int v0 = threadIdx.x * 8; v0 < V; v0 += 2048) {
        float x[8];
        load8(xr, v0, V, vx, x);
        float nm = fmaxf(mx, chunk_max(x));
        online_add(x, mx, nm, 1.f, s1);
        online_add(x, mx, nm, k, st);
        mx = nm;
        load8(ar, v0, V, va, x);
        nm = fmaxf(ma, chunk_max(x));
        online_add(x, ma, nm, k, sa);
        ma = nm;
        if constexpr (TWO) {
            load8(br, v0, V, vb, x);
            nm = fmaxf(mb, chunk_max(x));
            online_add(x, mb, nm, k, sb);
            mb = nm;
        }
    }
    const float lse_x = block_lse(mx, s1, 1.f, red_m, red_s);
    const float lse_xt = block_lse(mx, st, k, red_m, red_s);
    const float lse_a = block_lse(ma, sa, k, red_m, red_s);
    const float lse_b = TWO ? block_lse(mb, sb, k, red_m, red_s) : 0.f;
    const float wb = 1.f - alpha;
    float kd = 0.f;
    for (int v0 = threadIdx.x * 8; v0 < V; v0 += 2048) {
        float x[8], a[8], b[8];
        load8(xr, v0, V, vx, x);
        load8(ar, v0, V, va, a);
        if constexpr (TWO) load8(br, v0, V, vb, b);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float term;
            if constexpr (TWO) {
                const float q = alpha * __expf(a[e] * k - lse_a) + wb * __expf(b[e] * k - lse_b);
                term = q > 0.f ? q * (logf(q) - (x[e] * k - lse_xt)) : 0.f;
            } else {
                const float lq = a[e] * k - lse_a, q = __expf(lq);
                term = q > 0.f ? q * (lq - (x[e] * k - lse_xt)) : 0.f;
            }
            kd += term;
        }
    }
    kd = block_sum(kd, red_s);
    if (threadIdx.x == 0) {
        lse4[row] = lse_x; lse4[M + row] = lse_xt; lse4[2 * M + row] = lse_a; lse4[3 * M + row] = lse_b;
        rowkd[row] = tau * tau * kd;
    }
}

// lam == 0 went through omr_ce_fwd, which wrote acc4[0..1] and means3[0]: the plain mean is also the nll, and there is no kd.
__global__ void distill_plain_fill_kernel(double* __restrict__ acc4, float* __restrict__ means3) {
    acc4[2] = acc4[0]; acc4[3] = 0.0;
    means3[1] = means3[0]; means3[2] = 0.f;
}

// One sweep over x, a, b and one write: p, pt and q again from the saved row constants.  +0 on ignored rows (which read nothing) and in the
// columns >= V.
template <typename TS, typename TT, bool TWO>
__global__ __launch_bounds__(256) void distill_bwd_kernel(const TS* __restrict__ logits, long ldv, const TT* __restrict__ ta, const TT* __restrict__ tb,
                                                          long ldt, const long* __restrict__ target, const float* __restrict__ lse4,
                                                          const double* __restrict__ acc4, TS* __restrict__ dlogits, long M, int V, int pad_idx,
                                                          float alpha, float tau, float lam, float gscale, const float* __restrict__ grad_out) {
    const long row = blockIdx.x;
    const long t = target[row];
    const bool live = row_live(t, pad_idx, V);                // the same for the whole workgroup
    TS* dr = dlogits + row * ldv;
    const bool vd = row_vec_ok(dlogits, ldv);
    if (!live) {
        const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int v0 = threadIdx.x * 8; v0 < ldv; v0 += 2048) store8(dr, v0, ldv, vd, z);
        return;
    }
    const TS* xr = logits + row * ldv;
    const TT* ar = ta + row * ldt;
    const TT* br = TWO ? tb + row * ldt : nullptr;
    const bool vx = row_vec_ok(logits, ldv), va = row_vec_ok(ta, ldt), vb = TWO ? row_vec_ok(tb, ldt) : false;
    const float k = 1.f / tau, wb = 1.f - alpha;
    const float lse_x = lse4[row], lse_xt = lse4[M + row], lse_a = lse4[2 * M + row], lse_b = lse4[3 * M + row];
    const float sc = gscale * (grad_out ? grad_out[0] : 1.f) / (float)acc4[1];
    const float hard = 1.f - lam, soft = lam * tau;
    for (int v0 = threadIdx.x * 8; v0 < ldv; v0 += 2048) {
        float d[8];
        if (v0 < V) {
            float x[8], a[8], b[8];
            load8(xr, v0, V, vx, x);
            load8(ar, v0, V, va, a);
            if constexpr (TWO) load8(br, v0, V, vb, b);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float q = __expf(a[e] * k - lse_a);
                if constexpr (TWO) q = alpha * q + wb * __expf(b[e] * k - lse_b);
                const float g = hard * (__expf(x[e] - lse_x) - (v0 + e == t ? 1.f : 0.f)) + soft * (__expf(x[e] * k - lse_xt) - q);
                d[e] = (v0 + e < V) ? g * sc : 0.f;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] = 0.f;
        }
        store8(dr, v0, ldv, vd, d);
    }
}

bool distill_args_ok(const void* logits, const void* ta, const void* tb, const long* target, long M, int V, long ldv, long ldt, float alpha, float tau,
                     float lam) {
    if (!loss_rows_ok(M, V, ldv) || ldt < V || logits == nullptr || target == nullptr) return false;
    if (!(tau > 0.f) || !(tau < INFINITY)) return false;                  // NaN fails both comparisons
    if (!(lam >= 0.f && lam <= 1.f) || !(alpha >= 0.f && alpha <= 1.f)) return false;
    if (tb == nullptr && alpha != 1.f) return false;
    if (lam > 0.f && ta == nullptr) return false;
    return true;
}

template <typename TS, typename TT>
void launch_distill_fwd(const void* logits, long ldv, const void* ta, const void* tb, long ldt, const long* target, float* lse4, float* rowkd, double* acc4,
                        float* means3, long M, int V, int pad_idx, float alpha, float tau, float lam, hipStream_t s) {
    if (tb) hipLaunchKernelGGL((distill_fwd_kernel<TS, TT, true>), (int)M, 256, 0, s, (const TS*)logits, ldv, (const TT*)ta, (const TT*)tb, ldt, target, lse4,
                               rowkd, M, V, pad_idx, alpha, tau);
    else hipLaunchKernelGGL((distill_fwd_kernel<TS, TT, false>), (int)M, 256, 0, s, (const TS*)logits, ldv, (const TT*)ta, (const TT*)nullptr, ldt, target,
                            lse4, rowkd, M, V, pad_idx, alpha, tau);
    hipLaunchKernelGGL((ce_finalize_kernel<TS, CE_DISTILL>), 1, 1024, 0, s, (const TS*)logits, target, (const float*)lse4, (const float*)rowkd, acc4, means3,
                       means3 + 1, means3 + 2, M, V, ldv, pad_idx, lam);
}

template <typename TS, typename TT>
void launch_distill_bwd(const void* logits, long ldv, const void* ta, const void* tb, long ldt, const long* target, const float* lse4, const double* acc4,
                        void* dlogits, long M, int V, int pad_idx, float alpha, float tau, float lam, float gscale, const float* grad_out, hipStream_t s) {
    if (tb) hipLaunchKernelGGL((distill_bwd_kernel<TS, TT, true>), (int)M, 256, 0, s, (const TS*)logits, ldv, (const TT*)ta, (const TT*)tb, ldt, target, lse4,
                               acc4, (TS*)dlogits, M, V, pad_idx, alpha, tau, lam, gscale, grad_out);
    else hipLaunchKernelGGL((distill_bwd_kernel<TS, TT, false>), (int)M, 256, 0, s, (const TS*)logits, ldv, (const TT*)ta, (const TT*)nullptr, ldt, target,
                            lse4, acc4, (TS*)dlogits, M, V, pad_idx, alpha, tau, lam, gscale, grad_out);
}

}  // namespace

// Run CALL with TS, TT = the element types of the student's and the teachers' dtype codes.
#define DISPATCH_TS_TT(CALL) DISPATCH_T(dtype, { typedef T TS; DISPATCH_T(tdtype, { typedef T TT; CALL; }) })

extern "C" int omr_ce_distill_fwd(int dtype, const void* logits, long ldv, int tdtype, const void* teacher_a, const void* teacher_b, long ldt,
                                  const long* target, float* lse4, float* rowkd, double* acc4, float* means3, long M, int V, int pad_idx, float alpha,
                                  float tau, float lam, void* stream) {
    if (!distill_args_ok(logits, teacher_a, teacher_b, target, M, V, ldv, ldt, alpha, tau, lam)) return OMR_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (lam == 0.f) {                                              // the plain loss: its own kernels, its bits; the teachers are never read
        const int rc = omr_ce_fwd(dtype, logits, target, lse4, acc4, means3, M, V, ldv, pad_idx, stream);
        if (rc != OMR_OK) return rc;
        hipLaunchKernelGGL(distill_plain_fill_kernel, 1, 1, 0, s, acc4, means3);
        OMR_CHECK_LAUNCH();
        return OMR_OK;
    }
    DISPATCH_TS_TT((launch_distill_fwd<TS, TT>(logits, ldv, teacher_a, teacher_b, ldt, target, lse4, rowkd, acc4, means3, M, V, pad_idx, alpha, tau, lam, s)))
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_ce_distill_bwd(int dtype, const void* logits, long ldv, int tdtype, const void* teacher_a, const void* teacher_b, long ldt,
                                  const long* target, const float* lse4, const double* acc4, void* dlogits, long M, int V, int pad_idx, float alpha,
                                  float tau, float lam, float grad_scale, const float* grad_out, void* stream) {
    if (!distill_args_ok(logits, teacher_a, teacher_b, target, M, V, ldv, ldt, alpha, tau, lam)) return OMR_ERR_ARG;
    if (lam == 0.f) return omr_ce_bwd(dtype, logits, target, lse4, acc4, dlogits, M, V, ldv, pad_idx, grad_scale, grad_out, stream);
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_TS_TT((launch_distill_bwd<TS, TT>(logits, ldv, teacher_a, teacher_b, ldt, target, lse4, acc4, dlogits, M, V, pad_idx, alpha, tau, lam, grad_scale,
                                               grad_out, s)))
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}
