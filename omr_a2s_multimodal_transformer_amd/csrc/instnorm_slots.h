// The InstanceNorm statistics protocol (gfx950), written once: a DETERMINISTIC two-stage fp64 reduction, no atomics anywhere.
//   workspace   fp64: partial slots ws[B][slots][C][2] = {sum, second sum} per (image, slot, channel), then the compact sums [B][C][2]
//   stage 1     a block keeps per-thread fp32 partials over its pixels, adds them over its threads in a FIXED order in fp64 and stores
//               the result into ITS OWN slot (slot_store).  Producers: instnorm_partial_kernel below (dense maps and ragged extents),
//               the conv kernels' statistics epilogue (conv3x3_mfma.h flush_stats) and the fused conv backward (conv_bwd_fused.hip).
//   spare slots a persistent producer may run fewer blocks per image than the workspace has slots: block 0 of an image zeroes the slots
//               gridDim.x .. slots - 1, so the consumer always adds ALL slots and the caller never clears the workspace.
//   stage 2     instnorm_reduce_slots_kernel adds an image's slots in index order and writes mean / rstd or the compact sums.
//   apply       instnorm_apply_kernel: y = (x - mean) * rstd, or dx = rstd * (g - sum g / n - xhat * sum(g * xhat) / n) [* (x > 0) * relu_scale].
// 1 / n: the DENSE backward apply multiplies the fp64 sums by 1 / HW rounded to FLOAT (the host passes it in; conv_bwd_fused.hip's
// APPLY constants do the same), the EXTENT forms by 1 / (h_b * w_b) in DOUBLE (as does conv3x3_mfma.h's mode 5).  Results are pinned
// to the bit on both sides (tests/golden/instnorm_bits.json): the difference is kept, not fixed.
// DESIGN.md "InstanceNorm slot protocol".
#pragma once
#include <type_traits>
#include "omr_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ workspace layout
// element index of value k (0 sum, 1 second sum) of channel c in slot `slot` of image b
__host__ __device__ __forceinline__ long slot_index(int b, long slots, long slot, int C, int c, int k) { return (((long)b * slots + slot) * C + c) * 2 + k; }
// element index of the compact sums [B][C][2] behind the slots
__host__ __device__ __forceinline__ long slot_compact_offset(int B, int slots, int C) { return slot_index(B, slots, 0, C, 0, 0); }
// bytes of a workspace (what omr_instnorm_workspace_bytes returns)
__host__ __device__ __forceinline__ long slot_workspace_bytes(int B, int C, int slots) { return (slot_compact_offset(B, slots, C) + (long)B * C * 2) * (long)sizeof(double); }

// One finished fp64 value into the calling block's slot (slot blockIdx.x of image b); block 0 also zeroes the value in the spare slots.
__device__ __forceinline__ void slot_store(double* __restrict__ ws, int b, int slots, int C, int c, int k, double v) {
    ws[slot_index(b, slots, blockIdx.x, C, c, k)] = v;
    if (blockIdx.x == 0)
        for (int sl = gridDim.x; sl < slots; ++sl) ws[slot_index(b, slots, sl, C, c, k)] = 0.0;
}

// Pixels per workgroup of the stand-alone statistics passes: 2048 on the big maps, fewer on the small DSC maps so that at least ~1000
// workgroups are in flight (16 x 256 maps with 2048 pixels per workgroup left 3/4 of the CUs idle).
inline int instnorm_pixels_per_block(long HW, int B) {
    long ppb = 2048;
    while (ppb > 64 && cdiv(HW, ppb) * (long)B < 1024) ppb /= 2;
    return (int)ppb;
}
// dynamic LDS of stage 1: [nphase][C][2] floats, nphase = 256 / (C / vec)
inline size_t instnorm_partial_lds_bytes(int C, int vec) { return (size_t)(256 / (C / vec)) * C * 2 * sizeof(float); }

// VEC elements moved with one access (VEC * sizeof(T) = 16 bytes on the vector path, one element on the scalar path)
template <typename T, int VEC> struct alignas(sizeof(T) * VEC) Pack {
    T v[VEC];
    __device__ __forceinline__ T& operator[](int e) { return v[e]; }
    __device__ __forceinline__ const T& operator[](int e) const { return v[e]; }
};
template <typename T, int VEC, typename P = Pack<T, VEC>> __device__ __forceinline__ P pack_zero() {
    P z;
#pragma unroll
    for (int e = 0; e < VEC; ++e) z[e] = from_f32<T>(0.f);
    return z;
}
// what the statistics kernels move with one access: the dense maps keep omr_common.h's 16-byte fragment, the extents a Pack
template <typename T, int VEC, bool EXTENT>
using NormAccess = typename std::conditional<!EXTENT && VEC == Frag<T>::N, typename Frag<T>::type, Pack<T, VEC>>::type;
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------------------------ stage 1
// Workgroup k of image b reduces the pixels [k * ppb, (k + 1) * ppb) for all channels into its own slot ws[b][k][C][2].
//   !EXTENT: pixels of the dense map x[B][HW][C]; 64-bit pixel index, no division, `ext` is not read.
//    EXTENT: pixels of the sample's extent (h_b, w_b) = ext[b] inside its padded plane [H][W], in row-major order OF THE EXTENT (pixel
//            p = (p / w_b, p % w_b); one sample holds < 2^31 elements, so positions inside it are 32-bit); a workgroup past the extent's
//            last pixel stores zeros, so the consumer adds all slots.
//   !BWD: {sum x, sum x * x}.  BWD: {sum g, sum g * xhat} with xhat = (x - mean) * rstd.
// Thread t owns channel group t % (C / VEC) and walks the pixels p = p0 + phase, += nphase (phase = t / (C / VEC)) with VEC-wide loads
// (NHWC rows are contiguous: fully coalesced); EXTENT: threads left over (C / VEC no divisor of 256) idle.
template <typename T, int VEC, bool BWD, bool EXTENT>
__global__ __launch_bounds__(256) void instnorm_partial_kernel(const T* __restrict__ x, const T* __restrict__ g, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const int* __restrict__ ext, double* __restrict__ ws,
                                                               int H, int W, long HW, int C, int ppb) {
    typedef NormAccess<T, VEC, EXTENT> P;
    typedef typename std::conditional<EXTENT, unsigned, long>::type Pix;
    extern __shared__ __attribute__((aligned(16))) float red[];   // [nphase][C][2]
    const int b = blockIdx.y;
    int w = 0;
    Pix n = (Pix)HW;
    if constexpr (EXTENT) {
        w = clampi(ext[2 * b + 1], 0, W);
        n = (unsigned)clampi(ext[2 * b], 0, H) * w;
    }
    const int ncg = C / VEC, nphase = blockDim.x / ncg;            // channel groups; !EXTENT: ncg divides blockDim
    const int cg = threadIdx.x % ncg, phase = threadIdx.x / ncg;
    const bool active = !EXTENT || phase < nphase;
    const Pix p0 = (Pix)blockIdx.x * (Pix)ppb;
    const Pix p1 = p0 + ppb < n ? p0 + ppb : n;
    const long base = (EXTENT ? (long)b * H * W * C : (long)b * HW * C) + cg * VEC;
    float s[VEC], q[VEC], mu[VEC], rs[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        s[e] = q[e] = 0.f;
        mu[e] = BWD ? mean[(long)b * C + cg * VEC + e] : 0.f;
        rs[e] = BWD ? rstd[(long)b * C + cg * VEC + e] : 1.f;
    }
    if (active) {
        for (Pix p = p0 + phase; p < p1; p += nphase) {
            long off;
            if constexpr (EXTENT) {
                const unsigned i = p / (unsigned)w, j = p - i * w;
                off = base + (long)(i * W + j) * C;
            } else {
                off = base + p * C;
            }
            const P xv = *reinterpret_cast<const P*>(x + off);
            if (BWD) {
                const P gv = *reinterpret_cast<const P*>(g + off);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float gg = to_f32(gv[e]);
                    s[e] += gg;
                    q[e] += gg * ((to_f32(xv[e]) - mu[e]) * rs[e]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float v = to_f32(xv[e]);
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
    double* out = ws + slot_index(b, gridDim.x, blockIdx.x, C, 0, 0);
    for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) {
        double acc = 0.0;
        for (int ph = 0; ph < nphase; ++ph) acc += (double)red[ph * 2 * C + i];
        out[i] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ stage 2
// One workgroup per image: value v = (channel, {sum | second sum}) of slot k lives at ws[b][k][v]; the 256 threads are dealt out as
// (v, part) so that `parts` threads share a value, each adding the slots k = part, part + parts, ... in that order, and the partial
// sums are then added in part order -- fixed order, no atomics, and no thread walks more than slots / parts slots (a single thread per
// value was a 20-27 us latency chain per launch).
// FINAL: mean / rstd with 1 / n = inv_hw, or, with `ext`, 1 / (h_b * w_b) of the sample's own extent (for sums that are exact in fp64 the
// result is bit-equal to the dense statistics of the cropped sample); else: the compact sums [b][C][2] that the backward apply reads.
template <bool FINAL>
__global__ __launch_bounds__(256) void instnorm_reduce_slots_kernel(const double* __restrict__ ws, const int* __restrict__ ext, int slots, int H, int W, int C,
                                                                    float* __restrict__ mean, float* __restrict__ rstd, double* __restrict__ compact,
                                                                    double inv_hw, float eps) {
    __shared__ double red[512];
    const int b = blockIdx.x, NV = 2 * C, tid = threadIdx.x;
    if (ext) {
        const long n = (long)clampi(ext[2 * b], 0, H) * clampi(ext[2 * b + 1], 0, W);
        inv_hw = n > 0 ? 1.0 / (double)n : 0.0;
    }
    const double* base = ws + slot_index(b, slots, 0, C, 0, 0);
    for (int v0 = 0; v0 < NV; v0 += 256) {                       // NV <= 256 in one round (C <= 128), two rounds for C = 256
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

// ------------------------------------------------------------------------------------------------ apply
// Thread owns one channel group (its statistics in registers) and walks the pixels of its workgroup's slab: no index divisions on the
// dense map.  !BWD: y = (x - mean) * rstd.  BWD: dx = rstd * (g - s1 - xhat * s2) [* (x > 0) * relu_scale], s1 / s2 = the compact
// sums `sums` [b][C][2] of stage 2 times 1 / n -- !EXTENT: n = HW, the factor is the FLOAT inv_hw; EXTENT: n = h_b * w_b, in double
// (see the note at the top).  EXTENT walks the whole padded plane and stores 0 outside the extent, where nothing is loaded.
template <typename T, int VEC, bool BWD, bool EXTENT>
__global__ __launch_bounds__(256) void instnorm_apply_kernel(const T* __restrict__ x, const T* __restrict__ g, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const double* __restrict__ sums, const int* __restrict__ ext,
                                                             T* __restrict__ out, int H, int W, long HW, int C, int ppb, float inv_hw, int relu_mask,
                                                             float relu_scale) {
    typedef NormAccess<T, VEC, EXTENT> P;
    typedef typename std::conditional<EXTENT, unsigned, long>::type Pix;
    const int b = blockIdx.y;
    const int h = EXTENT ? clampi(ext[2 * b], 0, H) : 0, w = EXTENT ? clampi(ext[2 * b + 1], 0, W) : 0;
    const int ncg = C / VEC, nphase = blockDim.x / ncg;
    const int cg = threadIdx.x % ncg, phase = threadIdx.x / ncg;
    if (EXTENT && phase >= nphase) return;
    double inv_n = (double)inv_hw;
    if constexpr (EXTENT) {
        const long n = (long)h * w;
        inv_n = n > 0 ? 1.0 / (double)n : 0.0;
    }
    float mu[VEC], rs[VEC], s1[VEC], s2[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const long bc = (long)b * C + cg * VEC + e;
        mu[e] = mean[bc]; rs[e] = rstd[bc];
        s1[e] = BWD ? (float)(sums[2 * bc] * inv_n) : 0.f;
        s2[e] = BWD ? (float)(sums[2 * bc + 1] * inv_n) : 0.f;
    }
    const Pix np = EXTENT ? (Pix)((unsigned)H * W) : (Pix)HW;
    const Pix p0 = (Pix)blockIdx.x * (Pix)ppb;
    const Pix p1 = p0 + ppb < np ? p0 + ppb : np;
    const long base = (long)b * np * C + cg * VEC;
    const P z = pack_zero<T, VEC, P>();
#pragma unroll 4
    for (Pix p = p0 + phase; p < p1; p += nphase) {
        P o = z;
        unsigned i = 0, j = 0;
        if constexpr (EXTENT) { i = p / (unsigned)W; j = p - i * W; }
        if (!EXTENT || (i < (unsigned)h && j < (unsigned)w)) {
            const P xv = *reinterpret_cast<const P*>(x + base + (long)p * C);
            if (BWD) {
                const P gv = *reinterpret_cast<const P*>(g + base + (long)p * C);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float xf = to_f32(xv[e]);
                    float d = rs[e] * (to_f32(gv[e]) - s1[e] - (xf - mu[e]) * rs[e] * s2[e]);
                    if (relu_mask) d = xf > 0.f ? d * relu_scale : 0.f;
                    o[e] = from_f32<T>(d);
                }
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) o[e] = from_f32<T>((to_f32(xv[e]) - mu[e]) * rs[e]);
            }
        }
        *reinterpret_cast<P*>(out + base + (long)p * C) = o;
    }
}

}  // namespace
