// The steps the loss kernels share (loss.hip, distill.hip), each written once: which rows count, the online-softmax step, the
// workgroup's log-sum-exp and sums, and the one-workgroup fp64 finalize.  The order of every operation here is part of the results'
// bits (tests/test_loss_bits_gpu.py): eps == 0 and lam == 0 give the plain loss's bits because all three losses run these very steps.
#pragma once
#include "omr_common.h"

// A row is live when its target is not pad and lies in [0, V); every other row is ignored: no loss, a gradient of +0.
__host__ __device__ __forceinline__ bool row_live(long t, int pad_idx, int V) { return t != pad_idx && t >= 0 && t < V; }

// What every entry asks of the student rows [M][ldv >= V].
inline bool loss_rows_ok(long M, int V, long ldv) { return M > 0 && V > 0 && ldv >= V; }

// One online-softmax step over a chunk of N columns (-inf where the row has none): with m the running maximum and
// nm = fmaxf(m, chunk_max(x)) the new one, s = sum exp((x - m) * k) is carried over to nm.  Several sums may share one maximum.
// N = Frag<T>::N on ce_fwd_kernel's 16-byte path, 1 on its scalar path, 8 in the distillation kernels; k = 1 folds away.
template <int N> __device__ __forceinline__ float chunk_max(const float (&x)[N]) {
    float cm = x[0];
#pragma unroll
    for (int e = 1; e < N; ++e) cm = fmaxf(cm, x[e]);
    return cm;
}
template <int N> __device__ __forceinline__ void online_add(const float (&x)[N], float m, float nm, float k, float& s) {
    const float sub = nm == -INFINITY ? 0.f : nm;      // only -inf so far: exp(-inf - -inf) is NaN, exp(-inf - 0) = 0 keeps s
    float add = __expf((x[0] - sub) * k);              // seeded with the first term: 0.f + e is e (e >= 0), but an add the compiler must keep
#pragma unroll
    for (int e = 1; e < N; ++e) add += __expf((x[e] - sub) * k);
    s = s * __expf((m - sub) * k) + add;
}

// One thread's share of a row's single pass (256 threads per row, k = 1): the running (mx, s) over its 16-byte chunks (vec_ok) or its
// strided columns, and with SMOOTH the fp32 sum rs of its logits (columns < V only: the padding may hold anything), added in column order.
// ce_fwd_kernel (loss.hip) and the frame rows of the CTC loss (ctc.hip) run this very loop.
template <typename T> __device__ __forceinline__ bool row_vec_ok(const T* logits, long ldv) {
    return (ldv % Frag<T>::N) == 0 && (((uintptr_t)logits) & 15) == 0;
}
template <typename T, bool SMOOTH>
__device__ __forceinline__ void row_online_pass(const T* __restrict__ lr, bool vec_ok, int V, float& mx, float& s, float& rs) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = Frag<T>::N;
    if (vec_ok) {
        for (int v0 = threadIdx.x * VEC; v0 < V; v0 += 256 * VEC) {
            const F f = *reinterpret_cast<const F*>(lr + v0);      // v0 + VEC <= ldv: the padding columns are readable
            float x[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) x[e] = (v0 + e < V) ? to_f32(f[e]) : -INFINITY;
            const float nm = fmaxf(mx, chunk_max(x));
            online_add(x, mx, nm, 1.f, s);
            mx = nm;
            if constexpr (SMOOTH) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) rs += (v0 + e < V) ? to_f32(f[e]) : 0.f;
            }
        }
    } else {
        for (int v = threadIdx.x; v < V; v += 256) {
            const float x[1] = {to_f32(lr[v])};
            const float nm = fmaxf(mx, x[0]);
            online_add(x, mx, nm, 1.f, s);
            mx = nm;
            if constexpr (SMOOTH) rs += x[0];
        }
    }
}

// log sum_v exp(k x_v) of the row from the 256 threads' (m, s): every thread gets the value.  red_m / red_s: 4 floats of LDS each, free on
// return.  ce_fwd_kernel needs the value on thread 0 alone; the second barrier and the other threads' arithmetic do not show in its time
// (DESIGN.md "Loss kernels: shared steps").
__device__ __forceinline__ float block_lse(float m, float s, float k, float* red_m, float* red_s) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float wm = wave_max(m);
    s = wave_sum(m == -INFINITY ? 0.f : s * __expf((m - wm) * k));
    if (lane == 0) { red_m[wv] = wm; red_s[wv] = s; }
    __syncthreads();
    const float mm = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) t += red_m[i] == -INFINITY ? 0.f : red_s[i] * __expf((red_m[i] - mm) * k);
    __syncthreads();
    return mm * k + logf(t);
}

// The sum of v over the 256 threads, on every thread: xor butterfly over the wave, then ((w0 + w1) + w2) + w3.  red: 4 T of LDS,
// still being read on return (one barrier only: a caller that writes red again puts a barrier in between).
template <typename T> __device__ __forceinline__ T block_sum(T v, T* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// The sums of N fp64 accumulators over one workgroup of 1024 threads, valid on thread 0: xor butterfly over the wave, then the
// 16 waves in order.
template <int N> __device__ __forceinline__ void block1024_sum(double (&a)[N]) {
    __shared__ double red[N][16];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int i = 0; i < N; ++i) a[i] += __shfl_xor(a[i], o, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) red[i][threadIdx.x >> 6] = a[i];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double t = 0.0;
            for (int w = 0; w < 16; ++w) t += red[i][w];
            a[i] = t;
        }
}

// The losses of the batch from the rows' constants: one workgroup, fp64, fixed order (no atomics: device-scope atomics on one address
// serialise at the memory side, and the sum stays deterministic).  acc = {sum of the objective, live rows[, sum of the plain
// nll = lse - logit[target][, sum of kd]]} over the live rows, and the means of the sums.
//   CE_PLAIN    objective = nll: acc[2], loss.
//   CE_SMOOTH   objective = lse - (1 - w) logit[target] - (w / V) aux, formed in fp64; w = eps, aux = rowsum: acc[3], loss, nll.
//               w == 0 adds the plain fp32 difference and never reads aux: 0 * rowsum would be NaN on a row that holds -inf.
//   CE_DISTILL  objective = (1 - w) nll + w aux, formed in fp64; w = lam, aux = rowkd: acc[4], loss, nll, kd.
//               w == 1 never multiplies nll (0 * inf on a row whose target logit is -inf).
enum { CE_PLAIN, CE_SMOOTH, CE_DISTILL };
template <typename T, int MODE>
__global__ __launch_bounds__(1024) void ce_finalize_kernel(const T* __restrict__ logits, const long* __restrict__ target, const float* __restrict__ lse,
                                                           const float* __restrict__ aux, double* __restrict__ acc, float* __restrict__ loss,
                                                           float* __restrict__ nll, float* __restrict__ kd, long M, int V, long ldv, int pad_idx,
                                                           float w) {
    constexpr int N = 2 + MODE;
    double a[N] = {};
    const double keep = 1.0 - (double)w, uni = (double)w / (double)V;
    for (long row = threadIdx.x; row < M; row += 1024) {
        const long t = target[row];
        if (!row_live(t, pad_idx, V)) continue;
        const float l = lse[row], xt = to_f32(logits[row * ldv + t]);
        const double plain = (double)(l - xt);
        if constexpr (MODE == CE_PLAIN) a[0] += plain;
        if constexpr (MODE == CE_SMOOTH) a[0] += w > 0.f ? (double)l - keep * (double)xt - uni * (double)aux[row] : plain;
        if constexpr (MODE == CE_DISTILL) {
            const double rk = (double)aux[row];
            a[0] += w < 1.f ? keep * plain + (double)w * rk : rk;
            a[3] += rk;
        }
        if constexpr (MODE != CE_PLAIN) a[2] += plain;
        a[1] += 1.0;
    }
    block1024_sum(a);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = a[i];
        loss[0] = (float)(a[0] / a[1]);
        if constexpr (MODE != CE_PLAIN) nll[0] = (float)(a[2] / a[1]);
        if constexpr (MODE == CE_DISTILL) kd[0] = (float)(a[3] / a[1]);
    }
}
