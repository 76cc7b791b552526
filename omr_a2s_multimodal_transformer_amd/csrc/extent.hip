// Ragged batches (gfx950): B samples of different sizes share one padded NHWC plane [B][H][W][C]; sample b's real content is the
// top-left h_b x w_b corner, extents[b] = (h_b, w_b).  The encoder keeps every activation ZERO outside its sample's extent: then a
// 3x3 / pad-1 conv at a position inside the extent reads what the sample run alone at h_b x w_b reads (its zero padding), and weight
// and bias gradients come out right from the dense kernels because both operands are zero outside (DESIGN.md "Ragged training").
//   omr_extent_zero                  writes the zeros back after every conv (bias + ReLU made the outside non-zero); its own adjoint
//   omr_instnorm_extent_fwd / _bwd   InstanceNorm2d(eps=1e-3, affine=False) with its sums over the extent only, count h_b * w_b
//   omr_pack_memory_fwd / _bwd       [B][H'][W'][d] feature grid <-> [B][Smax][d] decoder memory, row i * w'_b + j = cell (i, j)
// All memory-bound: 16-byte accesses where C is a multiple of the fragment width (else one element per access: the 1-channel input
// image, odd widths), long offsets, statistics by the deterministic fp64 slot reduction of norm.hip (no atomics).  One sample holds at
// most 2^31 - 1 elements (the launchers check H * W * C), so positions INSIDE a sample are 32-bit and pixel -> (row, column) is a 32-bit
// division; only the offset into the batch is 64-bit.  A value outside an extent is never read: conv outputs there are unspecified,
// the caller's padding may be anything (NaN in the tests).
#include "omr_common.h"
#include "omr_hip.h"

namespace {

// VEC elements moved with one access (VEC * sizeof(T) = 16 bytes on the vector path, one element on the scalar path)
template <typename T, int VEC> struct alignas(sizeof(T) * VEC) Pack { T v[VEC]; };
template <typename T, int VEC> __device__ __forceinline__ Pack<T, VEC> pack_zero() {
    Pack<T, VEC> z;
#pragma unroll
    for (int e = 0; e < VEC; ++e) z.v[e] = from_f32<T>(0.f);
    return z;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------------------------
// x[b,i,j,:] = 0 for i >= h_b or j >= w_b, in place.  The outside of a sample is two regions: the strip right of the extent in its
// first h_b rows (h_b runs of (W - w_b) * C elements) and the rows below it (one contiguous run); the threads of blockIdx.y = b
// walk both with a grid-stride loop over fragments.  Nothing is loaded; a full-size sample has nothing to do.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void extent_zero_kernel(T* __restrict__ x, const int* __restrict__ ext, int H, int W, int C) {
    typedef Pack<T, VEC> P;
    const int b = blockIdx.y;
    const int h = clampi(ext[2 * b], 0, H), w = clampi(ext[2 * b + 1], 0, W);
    const unsigned cv = C / VEC;
    const unsigned right = (unsigned)(W - w) * cv;         // fragments right of the extent in one row
    const unsigned nA = (unsigned)h * right, nB = (unsigned)(H - h) * W * cv;
    T* xb = x + (long)b * H * W * C;
    const P z = pack_zero<T, VEC>();
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < nA + nB; i += gridDim.x * blockDim.x) {
        unsigned frag;
        if (i < nA) { const unsigned r = i / right; frag = (r * W + w) * cv + (i - r * right); }
        else frag = (unsigned)h * W * cv + (i - nA);
        *reinterpret_cast<P*>(xb + (long)frag * VEC) = z;
    }
}

// ------------------------------------------------------------------------------------------------
// Stage 1 of the statistics (norm.hip instnorm_partial_kernel over the extent): workgroup k of sample b reduces the extent's pixels
// [k * ppb, (k + 1) * ppb) in row-major order OF THE EXTENT (pixel p = (p / w_b, p % w_b)) for all channels and stores its sums into
// its own slot ws[b][k][C][2]; a workgroup past the extent's last pixel stores zeros, so the consumer adds all slots.
// !BWD: {sum x, sum x*x}.  BWD: {sum g, sum g * xhat} with xhat = (x - mean) * rstd.
// Thread t owns channel group t % (C / VEC) and every (256 / (C / VEC))-th pixel; threads left over (C / VEC no divisor of 256) idle.
template <typename T, int VEC, bool BWD>
__global__ __launch_bounds__(256) void extent_partial_kernel(const T* __restrict__ x, const T* __restrict__ g, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const int* __restrict__ ext, double* __restrict__ ws,
                                                             int H, int W, int C, int ppb) {
    typedef Pack<T, VEC> P;
    extern __shared__ __attribute__((aligned(16))) float red[];   // [nphase][C][2]
    const int b = blockIdx.y;
    const int h = clampi(ext[2 * b], 0, H), w = clampi(ext[2 * b + 1], 0, W);
    const unsigned n = (unsigned)h * w;
    const int ncg = C / VEC, nphase = blockDim.x / ncg;
    const int cg = threadIdx.x % ncg, phase = threadIdx.x / ncg;
    const bool active = phase < nphase;
    const unsigned p0 = blockIdx.x * (unsigned)ppb;
    const unsigned p1 = p0 + ppb < n ? p0 + ppb : n;
    const long base = (long)b * H * W * C + cg * VEC;
    float s[VEC], q[VEC], mu[VEC], rs[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        s[e] = q[e] = 0.f;
        mu[e] = BWD ? mean[(long)b * C + cg * VEC + e] : 0.f;
        rs[e] = BWD ? rstd[(long)b * C + cg * VEC + e] : 1.f;
    }
    if (active) {
        for (unsigned p = p0 + phase; p < p1; p += nphase) {
            const unsigned i = p / (unsigned)w, j = p - i * w;
            const long off = base + (long)(i * W + j) * C;
            const P xv = *reinterpret_cast<const P*>(x + off);
            if (BWD) {
                const P gv = *reinterpret_cast<const P*>(g + off);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float gg = to_f32(gv.v[e]);
                    s[e] += gg;
                    q[e] += gg * ((to_f32(xv.v[e]) - mu[e]) * rs[e]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float v = to_f32(xv.v[e]);
                    s[e] += v;
                    q[e] += v * v;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            red[(phase * C + cg * VEC + e) * 2 + 0] = s[e];
            red[(phase * C + cg * VEC + e) * 2 + 1] = q[e];
        }
    }
    __syncthreads();
    double* out = ws + ((long)b * gridDim.x + blockIdx.x) * C * 2;
    for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) {
        double acc = 0.0;
        for (int ph = 0; ph < nphase; ++ph) acc += (double)red[ph * 2 * C + i];
        out[i] = acc;
    }
}

// Stage 2 (norm.hip instnorm_reduce_slots_kernel with the count of each sample's own extent): one workgroup per sample adds its slots
// in a fixed order -- `parts` threads share a value, each adding the slots part, part + parts, ..., the partial sums then added in
// part order.  FINAL: mean / rstd by omr_instnorm_finalize's arithmetic with 1 / (h_b * w_b) (for sums that are exact in fp64 they
// are bit-equal to omr_instnorm_stats of the cropped sample); else the compact sums [b][C][2] that the backward apply reads.
template <bool FINAL>
__global__ __launch_bounds__(256) void extent_reduce_slots_kernel(const double* __restrict__ ws, const int* __restrict__ ext, int slots, int H, int W, int C,
                                                                  float* __restrict__ mean, float* __restrict__ rstd, double* __restrict__ compact, float eps) {
    __shared__ double red[512];
    const int b = blockIdx.x, NV = 2 * C, tid = threadIdx.x;
    const long n = (long)clampi(ext[2 * b], 0, H) * clampi(ext[2 * b + 1], 0, W);
    const double inv_hw = n > 0 ? 1.0 / (double)n : 0.0;
    const double* base = ws + (long)b * slots * NV;
    for (int v0 = 0; v0 < NV; v0 += 256) {
        const int nv = NV - v0 < 256 ? NV - v0 : 256;            // values of this round (even: NV and 256 are)
        const int parts = 256 / nv;
        const int v = tid % nv, part = tid / nv;
        double acc = 0.0;
        if (part < parts)
            for (int k = part; k < slots; k += parts) acc += base[(long)k * NV + v0 + v];
        __syncthreads();
        if (part < parts) red[part * nv + v] = acc;
        __syncthreads();
        if (tid < nv) {
            double s = 0.0;
            for (int q = 0; q < parts; ++q) s += red[q * nv + tid];
            red[256 + tid] = s;
        }
        __syncthreads();
        if (FINAL) {
            if (tid < nv / 2) {                                   // channel c = (v0 + 2 tid) / 2
                const double m = red[256 + 2 * tid] * inv_hw;
                double var = red[256 + 2 * tid + 1] * inv_hw - m * m;
                if (var < 0) var = 0;
                const long o = (long)b * C + v0 / 2 + tid;
                mean[o] = (float)m;
                rstd[o] = (float)(1.0 / sqrt(var + (double)eps));
            }
        } else if (tid < nv) {
            compact[(long)b * NV + v0 + tid] = red[256 + tid];
        }
    }
}

// Apply over the whole plane: thread owns one channel group (its statistics in registers) and walks the pixels of its workgroup's slab.
// !BWD: y = (x - mean) * rstd inside the extent, 0 outside.
// BWD : dx = rstd * (g - sum g / n - xhat * sum(g * xhat) / n) [* (x > 0) * relu_scale] inside, 0 outside (norm.hip
//       instnorm_bwd_apply_kernel's arithmetic); sums = the compact [b][C][2] of stage 2.
// Outside the extent nothing is loaded.
template <typename T, int VEC, bool BWD>
__global__ __launch_bounds__(256) void extent_norm_apply_kernel(const T* __restrict__ x, const T* __restrict__ g, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, const double* __restrict__ sums,
                                                                const int* __restrict__ ext, T* __restrict__ out, int H, int W, int C, int ppb,
                                                                int relu_mask, float relu_scale) {
    typedef Pack<T, VEC> P;
    const int b = blockIdx.y;
    const int h = clampi(ext[2 * b], 0, H), w = clampi(ext[2 * b + 1], 0, W);
    const int ncg = C / VEC, nphase = blockDim.x / ncg;
    const int cg = threadIdx.x % ncg, phase = threadIdx.x / ncg;
    if (phase >= nphase) return;
    const long n = (long)h * w;
    const double inv_hw = n > 0 ? 1.0 / (double)n : 0.0;
    float mu[VEC], rs[VEC], s1[VEC], s2[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const long bc = (long)b * C + cg * VEC + e;
        mu[e] = mean[bc]; rs[e] = rstd[bc];
        s1[e] = BWD ? (float)(sums[2 * bc] * inv_hw) : 0.f;
        s2[e] = BWD ? (float)(sums[2 * bc + 1] * inv_hw) : 0.f;
    }
    const unsigned HW = (unsigned)H * W;
    const unsigned p0 = blockIdx.x * (unsigned)ppb;
    const unsigned p1 = p0 + ppb < HW ? p0 + ppb : HW;
    const long base = (long)b * HW * C + cg * VEC;
    const P z = pack_zero<T, VEC>();
#pragma unroll 4
    for (unsigned p = p0 + phase; p < p1; p += nphase) {
        const unsigned i = p / (unsigned)W, j = p - i * W;
        P o = z;
        if (i < (unsigned)h && j < (unsigned)w) {
            const P xv = *reinterpret_cast<const P*>(x + base + (long)p * C);
            if (BWD) {
                const P gv = *reinterpret_cast<const P*>(g + base + (long)p * C);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float xf = to_f32(xv.v[e]);
                    float d = rs[e] * (to_f32(gv.v[e]) - s1[e] - (xf - mu[e]) * rs[e] * s2[e]);
                    if (relu_mask) d = xf > 0.f ? d * relu_scale : 0.f;
                    o.v[e] = from_f32<T>(d);
                }
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) o.v[e] = from_f32<T>((to_f32(xv.v[e]) - mu[e]) * rs[e]);
            }
        }
        *reinterpret_cast<P*>(out + base + (long)p * C) = o;
    }
}

// ------------------------------------------------------------------------------------------------
// Decoder memory of a ragged batch.  !BWD: out[b][r][:] = x[b][r / w_b][r % w_b][:] for r < S_b = h_b * w_b, 0 for S_b <= r < Smax.
// BWD: dx[b][i][j][:] = dout[b][i * w_b + j][:] inside the extent, 0 outside (rows >= S_b of dout are not read).  One fragment per
// thread and iteration, the destination walked linearly.
template <typename T, int VEC, bool BWD>
__global__ __launch_bounds__(256) void pack_memory_kernel(const T* __restrict__ src, const int* __restrict__ ext, T* __restrict__ dst, int H, int W, int C,
                                                          int Smax) {
    typedef Pack<T, VEC> P;
    const int b = blockIdx.y;
    const unsigned cv = C / VEC;
    const unsigned h = clampi(ext[2 * b], 0, H), w = clampi(ext[2 * b + 1], 0, W);
    const unsigned per = (BWD ? (unsigned)H * W : (unsigned)Smax) * cv;     // destination fragments of this sample
    const T* sb = src + (long)b * (BWD ? (long)Smax : (long)H * W) * C;
    T* db = dst + (long)b * (BWD ? (long)H * W : (long)Smax) * C;
    const P z = pack_zero<T, VEC>();
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < per; t += gridDim.x * blockDim.x) {
        const unsigned pix = t / cv, c = (t - pix * cv) * VEC;
        P o = z;
        if (BWD) {
            const unsigned i = pix / (unsigned)W, j = pix - i * W;
            const unsigned r = i * w + j;
            if (i < h && j < w && r < (unsigned)Smax) o = *reinterpret_cast<const P*>(sb + (long)r * C + c);
        } else if (pix < h * w) {
            const unsigned i = pix / w, j = pix - i * w;
            o = *reinterpret_cast<const P*>(sb + (long)(i * W + j) * C + c);
        }
        *reinterpret_cast<P*>(db + (long)t * VEC) = o;
    }
}

}  // namespace

// Pixels per workgroup of the statistics pass: norm.hip's rule on the padded plane (2048, fewer on small maps so that ~1000 workgroups fly).
static int extent_pixels_per_block(long HW, int B) {
    long ppb = 2048;
    while (ppb > 64 && cdiv(HW, ppb) * (long)B < 1024) ppb /= 2;
    return (int)ppb;
}
// elements per access: the 16-byte fragment when every pixel's channels and every given pointer allow it, else one element
static int extent_vec(int dtype, int C, const void* a, const void* b = nullptr, const void* c = nullptr) {
    const int vec = dtype == OMR_BF16 ? 8 : 4;
    const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c;
    return (C % vec == 0 && bits % 16 == 0) ? vec : 1;
}
static bool extent_args_ok(const void* p, const int* ext, int B, int H, int W, int C) {
    return p && ext && B > 0 && B <= 65535 && H > 0 && W > 0 && C > 0 && (long)H * W * C <= 0x7fffffffL;
}

// Run CALL with T and VEC (compile-time) for a dtype code and the access width `vec` chosen by extent_vec.
#define DISPATCH_T_VEC(dtype, vec, CALL)                                                                \
    if ((dtype) == OMR_F32) { typedef float T; if ((vec) == 4) { constexpr int VEC = 4; CALL; } else { constexpr int VEC = 1; CALL; } } \
    else if ((dtype) == OMR_BF16) { typedef bf16 T; if ((vec) == 8) { constexpr int VEC = 8; CALL; } else { constexpr int VEC = 1; CALL; } } \
    else return OMR_ERR_UNSUPPORTED;

extern "C" int omr_extent_zero(int dtype, void* x, const int* extents, int B, int H, int W, int C, void* stream) {
    if (!extent_args_ok(x, extents, B, H, W, C)) return OMR_ERR_ARG;
    const int vec = extent_vec(dtype, C, x);
    long gx = ((long)H * W * (C / vec) + 256 * 8 - 1) / (256 * 8);      // ~8 fragments per thread if the whole plane were outside
    gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
    DISPATCH_T_VEC(dtype, vec, hipLaunchKernelGGL((extent_zero_kernel<T, VEC>), dim3((unsigned)gx, B), 256, 0, (hipStream_t)stream, (T*)x, extents, H, W, C));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

/* slots per sample of the extent statistics passes; the workspace is omr_instnorm_workspace_bytes(B, C, slots) */
extern "C" int omr_instnorm_extent_slots(int B, long HW) { return (B <= 0 || HW <= 0) ? OMR_ERR_ARG : cdiv(HW, extent_pixels_per_block(HW, B)); }

extern "C" int omr_instnorm_extent_fwd(int dtype, const void* x, const int* extents, void* y, float* mean, float* rstd, int B, int H, int W, int C,
                                       float eps, void* workspace, void* stream) {
    if (!extent_args_ok(x, extents, B, H, W, C) || !y || !mean || !rstd || !workspace) return OMR_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int vec = extent_vec(dtype, C, x, y);
    const int ncg = C / vec;
    if (ncg > 256) return OMR_ERR_UNSUPPORTED;
    const long HW = (long)H * W;
    const int ppb = extent_pixels_per_block(HW, B), slots = cdiv(HW, ppb);
    const size_t lds = (size_t)(256 / ncg) * C * 2 * sizeof(float);
    double* ws = (double*)workspace;
    DISPATCH_T_VEC(dtype, vec, hipLaunchKernelGGL((extent_partial_kernel<T, VEC, false>), dim3(slots, B), 256, lds, s, (const T*)x, (const T*)nullptr,
                                                  (const float*)nullptr, (const float*)nullptr, extents, ws, H, W, C, ppb));
    hipLaunchKernelGGL((extent_reduce_slots_kernel<true>), B, 256, 0, s, (const double*)ws, extents, slots, H, W, C, mean, rstd, (double*)nullptr, eps);
    const int ppb2 = 1024;
    DISPATCH_T_VEC(dtype, vec, hipLaunchKernelGGL((extent_norm_apply_kernel<T, VEC, false>), dim3(cdiv(HW, ppb2), B), 256, 0, s, (const T*)x, (const T*)nullptr,
                                                  (const float*)mean, (const float*)rstd, (const double*)nullptr, extents, (T*)y, H, W, C, ppb2, 0, 1.f));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_instnorm_extent_bwd(int dtype, const void* dxhat, const void* x, const float* mean, const float* rstd, const int* extents, void* dx,
                                       int B, int H, int W, int C, int relu_mask, float relu_scale, void* workspace, void* stream) {
    if (!extent_args_ok(x, extents, B, H, W, C) || !dxhat || !dx || !mean || !rstd || !workspace) return OMR_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int vec = extent_vec(dtype, C, x, dxhat, dx);
    const int ncg = C / vec;
    if (ncg > 256) return OMR_ERR_UNSUPPORTED;
    const long HW = (long)H * W;
    const int ppb = extent_pixels_per_block(HW, B), slots = cdiv(HW, ppb);
    const size_t lds = (size_t)(256 / ncg) * C * 2 * sizeof(float);
    double* ws = (double*)workspace;
    double* compact = ws + (long)B * slots * C * 2;
    DISPATCH_T_VEC(dtype, vec, hipLaunchKernelGGL((extent_partial_kernel<T, VEC, true>), dim3(slots, B), 256, lds, s, (const T*)x, (const T*)dxhat, mean, rstd,
                                                  extents, ws, H, W, C, ppb));
    hipLaunchKernelGGL((extent_reduce_slots_kernel<false>), B, 256, 0, s, (const double*)ws, extents, slots, H, W, C, (float*)nullptr, (float*)nullptr, compact, 0.f);
    const int ppb2 = 1024;
    DISPATCH_T_VEC(dtype, vec, hipLaunchKernelGGL((extent_norm_apply_kernel<T, VEC, true>), dim3(cdiv(HW, ppb2), B), 256, 0, s, (const T*)x, (const T*)dxhat, mean,
                                                  rstd, (const double*)compact, extents, (T*)dx, H, W, C, ppb2, relu_mask, relu_scale));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

static unsigned pack_grid(long frags) { long g = (frags + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > 256 ? 256 : g)); }   // per sample (blockIdx.y)

extern "C" int omr_pack_memory_fwd(int dtype, const void* x, const int* extents, void* out, int B, int H, int W, int C, int Smax, void* stream) {
    if (!extent_args_ok(x, extents, B, H, W, C) || !out || Smax <= 0 || (long)Smax * C > 0x7fffffffL) return OMR_ERR_ARG;
    const int vec = extent_vec(dtype, C, x, out);
    DISPATCH_T_VEC(dtype, vec, hipLaunchKernelGGL((pack_memory_kernel<T, VEC, false>), dim3(pack_grid((long)Smax * (C / vec)), B), 256, 0, (hipStream_t)stream,
                                                  (const T*)x, extents, (T*)out, H, W, C, Smax));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_pack_memory_bwd(int dtype, const void* dout, const int* extents, void* dx, int B, int H, int W, int C, int Smax, void* stream) {
    if (!extent_args_ok(dout, extents, B, H, W, C) || !dx || Smax <= 0 || (long)Smax * C > 0x7fffffffL) return OMR_ERR_ARG;
    const int vec = extent_vec(dtype, C, dout, dx);
    DISPATCH_T_VEC(dtype, vec, hipLaunchKernelGGL((pack_memory_kernel<T, VEC, true>), dim3(pack_grid((long)H * W * (C / vec)), B), 256, 0, (hipStream_t)stream,
                                                  (const T*)dout, extents, (T*)dx, H, W, C, Smax));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}
