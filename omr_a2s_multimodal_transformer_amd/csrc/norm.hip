// Normalisation kernels (gfx950), all statistics in fp32/fp64:
//   InstanceNorm2d(eps=1e-3, affine=False, no running stats) on NHWC maps  -- encoder.py:151-156,210-215 (kernels: instnorm_slots.h)
//   residual + LayerNorm(eps=1e-5) of the post-norm decoder layer          -- torch nn/modules/transformer.py:1146-1154
#include "omr_common.h"
#include "omr_hip.h"
#include "instnorm_slots.h"

namespace {

// ------------------------------------------------------------------------------------------------
// out = LayerNorm(dropout(x) + res) * gamma + beta.  One wave per row; lane l owns the PER = d/64 CONSECUTIVE elements
// [l*PER, (l+1)*PER) so every tensor is touched with one vector load/store per lane per row.  Saves mean and rstd.
// The sublayer dropout that precedes every post-norm residual (torch nn/modules/transformer.py:1146-1154) is fused:
// drop_thresh != 0 applies the counter-based mask of omr_dropout (same seed/index convention, element index row*d + c)
// to x; the backward regenerates it.
template <typename T, int PER>
__global__ __launch_bounds__(256) void add_ln_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, T* __restrict__ out, float* __restrict__ mean,
                                                         float* __restrict__ rstd, long M, float eps, uint32_t drop_thresh, float drop_scale,
                                                         uint64_t drop_seed) {
    typedef __attribute__((ext_vector_type(PER))) T VT;
    constexpr int d = PER * 64;
    const int lane = threadIdx.x & 63;
    const long row = blockIdx.x * (long)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= M) return;
    const VT xv = *reinterpret_cast<const VT*>(x + row * d + lane * PER);
    float v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) v[i] = to_f32(xv[i]);
    if (drop_thresh) {
        // the unfused path rounds the dropped value to T before the add: keep that rounding so both paths agree to the bit
#pragma unroll
        for (int i = 0; i < PER; ++i)
            v[i] = drop_keep(drop_seed, (uint64_t)(row * d + lane * PER + i), drop_thresh) ? to_f32(from_f32<T>(v[i] * drop_scale)) : 0.f;
    }
    if (res) {
        const VT rv = *reinterpret_cast<const VT*>(res + row * d + lane * PER);
#pragma unroll
        for (int i = 0; i < PER; ++i) v[i] += to_f32(rv[i]);
    }
    float mu, rs;
    ln_row<PER>(v, gamma, beta, lane, eps, mu, rs);
    VT o;
#pragma unroll
    for (int i = 0; i < PER; ++i) o[i] = from_f32<T>(v[i]);
    *reinterpret_cast<VT*>(out + row * d + lane * PER) = o;
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
}

// Backward: s = dropout(x) + res, xhat = (s - mean) * rstd, gh = dy * gamma
//   ds = rstd * (gh - mean_d(gh) - xhat * mean_d(gh * xhat))      (gradient of res; of x too when there is no dropout)
//   dx = keep ? ds / (1-p) : 0                                     (second output, only with the fused dropout)
//   dgamma[c] += sum_rows dy * xhat ; dbeta[c] += sum_rows dy     (register partials per wave -> LDS -> one atomic per column per block)
template <typename T, int PER>
__global__ __launch_bounds__(256) void add_ln_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ res,
                                                         const float* __restrict__ gamma, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, T* __restrict__ ds, float* __restrict__ dgamma,
                                                         float* __restrict__ dbeta, long M, int rows_per_block, uint32_t drop_thresh, float drop_scale,
                                                         uint64_t drop_seed, T* __restrict__ dx) {
    typedef __attribute__((ext_vector_type(PER))) T VT;
    typedef __attribute__((ext_vector_type(PER))) float VF;
    constexpr int d = PER * 64;
    __shared__ float cg[d], cb[d];
    for (int i = threadIdx.x; i < d; i += blockDim.x) { cg[i] = 0.f; cb[i] = 0.f; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const long r0 = (long)blockIdx.x * rows_per_block;
    const VF gm = *reinterpret_cast<const VF*>(gamma + lane * PER);
    float ag[PER], ab[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) ag[i] = ab[i] = 0.f;
    // the next row's operands are requested before this row's math (a wave walks its rows one after another)
    const long rend = (r0 + rows_per_block < M) ? r0 + rows_per_block : M;
    VT xn, gn, rn;
    float mun = 0.f, rsn = 1.f;
    auto fetch = [&](long row) {
        if (row < rend) {
            mun = mean[row]; rsn = rstd[row];
            xn = *reinterpret_cast<const VT*>(x + row * d + lane * PER);
            gn = *reinterpret_cast<const VT*>(dy + row * d + lane * PER);
            if (res) rn = *reinterpret_cast<const VT*>(res + row * d + lane * PER);
        }
    };
    fetch(r0 + wv);
    for (long row = r0 + wv; row < rend; row += nw) {
        const float mu = mun, rs = rsn;
        const VT xv = xn, gv = gn, rv = rn;
        fetch(row + nw);
        float sv[PER];
        bool keep[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) { sv[i] = to_f32(xv[i]); keep[i] = true; }
        if (drop_thresh) {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                keep[i] = drop_keep(drop_seed, (uint64_t)(row * d + lane * PER + i), drop_thresh);
                sv[i] = keep[i] ? to_f32(from_f32<T>(sv[i] * drop_scale)) : 0.f;
            }
        }
        if (res) {
#pragma unroll
            for (int i = 0; i < PER; ++i) sv[i] += to_f32(rv[i]);
        }
        float xh[PER], gh[PER], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const float g = to_f32(gv[i]);
            xh[i] = (sv[i] - mu) * rs;
            gh[i] = g * gm[i];
            ag[i] += g * xh[i];
            ab[i] += g;
            s1 += gh[i]; s2 += gh[i] * xh[i];
        }
        s1 = wave_sum(s1) * (1.f / d); s2 = wave_sum(s2) * (1.f / d);
        VT o;
#pragma unroll
        for (int i = 0; i < PER; ++i) o[i] = from_f32<T>(rs * (gh[i] - s1 - xh[i] * s2));
        *reinterpret_cast<VT*>(ds + row * d + lane * PER) = o;
        if (drop_thresh) {
            VT od;
#pragma unroll
            for (int i = 0; i < PER; ++i) od[i] = keep[i] ? from_f32<T>(to_f32(o[i]) * drop_scale) : from_f32<T>(0.f);
            *reinterpret_cast<VT*>(dx + row * d + lane * PER) = od;
        }
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) { atomicAdd(&cg[lane * PER + i], ag[i]); atomicAdd(&cb[lane * PER + i], ab[i]); }
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        atomicAdd(&dgamma[c], cg[c]);
        atomicAdd(&dbeta[c], cb[c]);
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// InstanceNorm on dense maps x[B][HW][C] (NHWC): launchers over the slot protocol of instnorm_slots.h.  16-byte accesses only
// (VEC = Frag<T>::N, C / VEC a divisor of 256).  The forward apply is fused into the consumer's tile load (conv3 / depthwise conv3), never
// materialised.  Backward, with xhat = (x - mean) * rstd and g = dL/dxhat:  dx = rstd * (g - mean_hw(g) - xhat * mean_hw(g * xhat)),
// optionally times the ReLU(+dropout) backward of the producer of x: (x > 0) * relu_scale.
static bool dense_width_ok(int dtype, int C) {
    const int vec = dtype == OMR_BF16 ? 8 : 4;
    return C % vec == 0 && 256 % (C / vec) == 0;
}
// stage 1 over the whole map; returns the slots per image it filled
template <bool BWD>
static int launch_partial(int dtype, const void* x, const void* g, const float* mean, const float* rstd, double* ws, int B, long HW, int C, hipStream_t s) {
    const int ppb = instnorm_pixels_per_block(HW, B), slots = cdiv(HW, ppb);
    DISPATCH_T(dtype, hipLaunchKernelGGL((instnorm_partial_kernel<T, Frag<T>::N, BWD, false>), dim3(slots, B), 256, instnorm_partial_lds_bytes(C, Frag<T>::N), s,
                                         (const T*)x, (const T*)g, mean, rstd, (const int*)nullptr, ws, 0, 0, HW, C, ppb));
    return slots;
}
// stage 2: mean / rstd (FINAL) or the compact sums behind the slots
template <bool FINAL>
static void launch_reduce(double* ws, int slots, int B, long HW, int C, float* mean, float* rstd, float eps, hipStream_t s) {
    hipLaunchKernelGGL((instnorm_reduce_slots_kernel<FINAL>), B, 256, 0, s, (const double*)ws, (const int*)nullptr, slots, 0, 0, C, mean, rstd,
                       FINAL ? (double*)nullptr : ws + slot_compact_offset(B, slots, C), FINAL ? 1.0 / (double)HW : 0.0, eps);
}
static int launch_bwd_apply(int dtype, const void* dxhat, const void* x, const float* mean, const float* rstd, void* dx, int B, long HW, int C,
                            int relu_mask, float relu_scale, double* ws, int slots, hipStream_t s) {
    launch_reduce<false>(ws, slots, B, HW, C, nullptr, nullptr, 0.f, s);
    const int ppb2 = 1024;
    DISPATCH_T(dtype, hipLaunchKernelGGL((instnorm_apply_kernel<T, Frag<T>::N, true, false>), dim3(cdiv(HW, ppb2), B), 256, 0, s, (const T*)x, (const T*)dxhat, mean,
                                         rstd, (const double*)(ws + slot_compact_offset(B, slots, C)), (const int*)nullptr, (T*)dx, 0, 0, HW, C, ppb2,
                                         (float)(1.0 / (double)HW), relu_mask, relu_scale));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

/* slots per image of the stand-alone statistics passes (omr_instnorm_stats / omr_instnorm_bwd) */
extern "C" int omr_instnorm_slots(int B, long HW) { return (B <= 0 || HW <= 0) ? OMR_ERR_ARG : cdiv(HW, instnorm_pixels_per_block(HW, B)); }
/* bytes of a statistics workspace with `slots` slots per image: partials [B][slots][C][2] + compact sums [B][C][2], fp64 */
extern "C" long omr_instnorm_workspace_bytes(int B, int C, int slots) { return slot_workspace_bytes(B, C, slots); }

extern "C" int omr_instnorm_stats(int dtype, const void* x, float* mean, float* rstd, int B, long HW, int C, float eps, void* workspace,
                                  void* stream) {
    if (B <= 0 || HW <= 0 || C <= 0 || !workspace) return OMR_ERR_ARG;
    if (!dense_width_ok(dtype, C)) return OMR_ERR_UNSUPPORTED;
    const int slots = launch_partial<false>(dtype, x, nullptr, nullptr, nullptr, (double*)workspace, B, HW, C, (hipStream_t)stream);
    if (slots < 0) return slots;
    launch_reduce<true>((double*)workspace, slots, B, HW, C, mean, rstd, eps, (hipStream_t)stream);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

/* mean / rstd from the fp64 {sum, sum of squares} slots that a producer kernel filled (omr_conv3x3_fwd stat_mode 1) */
extern "C" int omr_instnorm_finalize(const void* workspace, int slots, float* mean, float* rstd, int B, long HW, int C, float eps, void* stream) {
    if (B <= 0 || HW <= 0 || C <= 0 || slots < 1 || !workspace) return OMR_ERR_ARG;
    launch_reduce<true>((double*)workspace, slots, B, HW, C, mean, rstd, eps, (hipStream_t)stream);      // FINAL reads the workspace only
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

/* the image-wise sums of the slots a producer kernel filled (omr_conv3x3_fwd stat_mode 2 / 4), added in slot order into the
 * compact region [B][C][2] behind them: what omr_conv3x3_fwd stat_mode 5 (and omr_instnorm_bwd_apply) read */
extern "C" int omr_instnorm_reduce_sums(void* workspace, int slots, int B, int C, void* stream) {
    if (B <= 0 || C <= 0 || slots < 1 || !workspace) return OMR_ERR_ARG;
    launch_reduce<false>((double*)workspace, slots, B, 0, C, nullptr, nullptr, 0.f, (hipStream_t)stream);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

/* apply step of the InstanceNorm backward with {sum g, sum g*xhat} already in the slots of `workspace`
 * (omr_conv3x3_fwd stat_mode 2 fuses that reduction into the data-gradient conv that produces dxhat) */
extern "C" int omr_instnorm_bwd_apply(int dtype, const void* dxhat, const void* x, const float* mean, const float* rstd, void* dx, int B, long HW,
                                      int C, int relu_mask, float relu_scale, void* workspace, int slots, void* stream) {
    if (B <= 0 || HW <= 0 || C <= 0 || slots < 1 || !workspace) return OMR_ERR_ARG;
    if (!dense_width_ok(dtype, C)) return OMR_ERR_UNSUPPORTED;
    return launch_bwd_apply(dtype, dxhat, x, mean, rstd, dx, B, HW, C, relu_mask, relu_scale, (double*)workspace, slots, (hipStream_t)stream);
}

extern "C" int omr_instnorm_bwd(int dtype, const void* dxhat, const void* x, const float* mean, const float* rstd, void* dx, int B, long HW,
                                int C, int relu_mask, float relu_scale, void* workspace, void* stream) {
    if (B <= 0 || HW <= 0 || C <= 0 || !workspace) return OMR_ERR_ARG;
    if (!dense_width_ok(dtype, C)) return OMR_ERR_UNSUPPORTED;
    const int slots = launch_partial<true>(dtype, x, dxhat, mean, rstd, (double*)workspace, B, HW, C, (hipStream_t)stream);
    if (slots < 0) return slots;
    return launch_bwd_apply(dtype, dxhat, x, mean, rstd, dx, B, HW, C, relu_mask, relu_scale, (double*)workspace, slots, (hipStream_t)stream);
}

#define LN_DISPATCH_PER(KERNEL, ...)                                                                       \
    switch (d / 64) {                                                                                      \
        case 2: hipLaunchKernelGGL((KERNEL<T, 2>), __VA_ARGS__); break;                                    \
        case 4: hipLaunchKernelGGL((KERNEL<T, 4>), __VA_ARGS__); break;                                    \
        case 8: hipLaunchKernelGGL((KERNEL<T, 8>), __VA_ARGS__); break;                                    \
        default: return OMR_ERR_UNSUPPORTED;                                                               \
    }

extern "C" int omr_add_layernorm_fwd(int dtype, const void* x, const void* res, const float* gamma, const float* beta, void* out, float* mean,
                                     float* rstd, long M, int d, float eps, float drop_p, unsigned long long drop_seed, void* stream) {
    if (M <= 0 || d <= 0 || d % 64 || drop_p < 0.f || drop_p >= 1.f) return OMR_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    int grid = cdiv(M, 4);
    const uint32_t thresh = OMR_DROP_THRESH16(drop_p);
    const float scale = 1.f / (1.f - drop_p);
    DISPATCH_T(dtype, { LN_DISPATCH_PER(add_ln_fwd_kernel, grid, 256, 0, s, (const T*)x, (const T*)res, gamma, beta, (T*)out, mean, rstd, M, eps, thresh, scale,
                                        (uint64_t)drop_seed) });
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_add_layernorm_bwd(int dtype, const void* dy, const void* x, const void* res, const float* gamma, const float* mean,
                                     const float* rstd, void* ds, float* dgamma, float* dbeta, long M, int d, float drop_p,
                                     unsigned long long drop_seed, void* dx, void* stream) {
    if (M <= 0 || d <= 0 || d % 64 || drop_p < 0.f || drop_p >= 1.f) return OMR_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    int rpb = 64;                        // fewer, longer workgroups: each ends with 2 d atomics onto the same 16 cache lines
    int grid = cdiv(M, rpb);
    const uint32_t thresh = OMR_DROP_THRESH16(drop_p);
    const float scale = 1.f / (1.f - drop_p);
    if (thresh && !dx) return OMR_ERR_ARG;
    DISPATCH_T(dtype, { LN_DISPATCH_PER(add_ln_bwd_kernel, grid, 256, 0, s, (const T*)dy, (const T*)x, (const T*)res, gamma, mean, rstd, (T*)ds, dgamma, dbeta, M, rpb,
                                        thresh, scale, (uint64_t)drop_seed, (T*)dx) });
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}
