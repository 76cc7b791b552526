// omr_gather_ragged_batch (batch_gather.hip) with a per-sample augmentation inside the same launch (gfx950): one OmrAugment record per
// batch row -- an affine map of the destination pixel into the source plane, a bilinear blend of four taps, gain / bias / hashed noise,
// fill-valued row and column bands (omr_hip.h states the contract step by step).  It stands where the reference reads a second,
// pre-rendered copy of every score (`image_distorted`, ar_dataset.py:377) before pad_batch_inputs (preprocessing.py:55-75).
//
// The value of a pixel is DEFINED operation by operation in fp32: with the identity record it is omr_gather_ragged_batch's to the bit, with
// any record that of a numpy float32 restatement (tests/augment_refs.py).  So no product may be fused into an add.  The Makefile's
// -ffp-contract=fast lets the backend fuse whatever it meets, whatever a `#pragma clang fp contract(off)` inside a function says (tried:
// the affine map and the lerps came out as v_fma_f32 / v_fmac_f32), and __fmul_rn / __fadd_rn are plain * and + to the compiler.  The
// choice made here: THIS FILE IS COMPILED WITH -ffp-contract=off (a per-file flag in the Makefile).  The v_fma_f32 that remain in its
// code belong to the expansion of the correctly rounded division.
//
// Structure of the plain gather: blockIdx.y = b, a grid-stride loop over destination fragments, one 16-byte store per iteration where W
// is a multiple of the fragment width and out is 16-byte aligned, else one element; 32-bit positions inside a plane (the destination's
// H * W and the source's h_n * w_n are <= 2^31 - 1); no LDS, no atomics.  A tap outside the h_n x w_n source plane is `fill` and is not
// read, a tap whose weight is exactly 0 is not read either: every byte read lies inside a listed sample.
#include <type_traits>
#include "omr_common.h"
#include "omr_hip.h"
#include "instnorm_slots.h"      // Pack, clampi
#include "batch_gather.h"        // gather_conv, gather_pad

namespace {

// start <= i < start + length for i >= 0 without overflow; length <= 0: no band
__device__ __forceinline__ bool in_band(int i, const int (&band)[2]) {
    return band[1] > 0 && (unsigned)i - (unsigned)band[0] < (unsigned)band[1];
}
// one tap in source units (a gray 0 .. 255, or the fp32 value)
template <typename S> __device__ __forceinline__ float gather_tap(const S* __restrict__ sb, int h, int w, int y, int x, float fill) {
    return (y >= 0 && y < h && x >= 0 && x < w) ? (float)sb[(unsigned)y * (unsigned)w + (unsigned)x] : fill;
}

// Steps 1-6 of the contract for destination pixel (i, j) inside the extent and outside every band: the value in SOURCE units.
template <typename S>
__device__ __forceinline__ float augment_value(const S* __restrict__ sb, int h, int w, const OmrAugment& a, int i, int j, int ow) {
    const float fi = (float)i, fj = (float)j;
    float y = a.m[0] * fi + a.m[1] * fj + a.m[2];
    float x = a.m[3] * fi + a.m[4] * fj + a.m[5];
    y = fminf(fmaxf(y, -1.0f), (float)h);               // fmaxf first: a NaN becomes -1
    x = fminf(fmaxf(x, -1.0f), (float)w);
    const float y0 = floorf(y), x0 = floorf(x);
    const float fy = y - y0, fx = x - x0;
    const int iy = (int)y0, ix = (int)x0;
    float g = gather_tap(sb, h, w, iy, ix, a.fill);
    if (fx != 0.0f) g = g * (1.0f - fx) + gather_tap(sb, h, w, iy, ix + 1, a.fill) * fx;
    if (fy != 0.0f) {
        float g1 = gather_tap(sb, h, w, iy + 1, ix, a.fill);
        if (fx != 0.0f) g1 = g1 * (1.0f - fx) + gather_tap(sb, h, w, iy + 1, ix + 1, a.fill) * fx;
        g = g * (1.0f - fy) + g1 * fy;
    }
    if (!(a.gain == 1.0f && a.bias == 0.0f)) g = a.gain * g + a.bias;
    if (a.noise != 0.0f) {
        const uint32_t bits = hash32(a.seed_lo, a.seed_hi, (uint32_t)i * (uint32_t)ow + (uint32_t)j);
        const float r = (float)(bits >> 8) * 1.1920928955078125e-07f - 1.0f;        // 2^-23: r in [-1, 1)
        g = g + a.noise * r;
    }
    if (std::is_same<S, unsigned char>::value) g = fminf(fmaxf(g, 0.0f), 255.0f);
    return g;
}
// conv of a value that is already a float in source units
template <typename S> __device__ __forceinline__ float augment_conv(float g) {
    return std::is_same<S, unsigned char>::value ? __fdiv_rn(g, 255.0f) : g;
}

template <typename S, typename T, int VEC>
__global__ __launch_bounds__(256) void gather_augmented_batch_kernel(const S* __restrict__ src, const long* __restrict__ offsets,
                                                                     const int* __restrict__ sizes, int N, const int* __restrict__ idx,
                                                                     const OmrAugment* __restrict__ aug, T* __restrict__ out, int H, int W,
                                                                     float pad_value) {
    typedef Pack<T, VEC> P;
    const int b = blockIdx.y;
    const int n = clampi(idx[b], 0, N - 1);
    const OmrAugment a = aug[b];
    const int h = sizes[2 * n] > 0 ? sizes[2 * n] : 0, w = sizes[2 * n + 1] > 0 ? sizes[2 * n + 1] : 0;     // the SOURCE plane: not clamped to H, W
    const int oh = clampi(a.out_h, 0, H), ow = clampi(a.out_w, 0, W);
    const unsigned per = (unsigned)H * W / VEC;            // destination fragments of this sample
    const S* sb = src + offsets[n];
    T* ob = out + (long)b * H * W;
    const T pad = gather_pad<T>(pad_value);
    const T band = from_f32<T>(augment_conv<S>(a.fill));
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < per; t += gridDim.x * blockDim.x) {
        const unsigned pix = t * VEC, i = pix / (unsigned)W, j = pix - i * W;
        const bool row_band = in_band((int)i, a.rows[0]) || in_band((int)i, a.rows[1]);
        P o;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int je = (int)j + e;
            if ((int)i >= oh || je >= ow) o[e] = pad;
            else if (row_band || in_band(je, a.cols[0]) || in_band(je, a.cols[1])) o[e] = band;
            else o[e] = from_f32<T>(augment_conv<S>(augment_value(sb, h, w, a, (int)i, je, ow)));
        }
        *reinterpret_cast<P*>(ob + (long)t * VEC) = o;
    }
}

template <typename S, typename T, int VEC>
void launch_augmented(const void* src, const long* offsets, const int* sizes, int N, const int* idx, const OmrAugment* aug, void* out, int B, int H,
                      int W, float pad_value, hipStream_t s) {
    long gx = ((long)H * W / VEC + 255) / 256;          // the plain gather's grid: at most 256 * 256 threads per sample (blockIdx.y)
    gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
    hipLaunchKernelGGL((gather_augmented_batch_kernel<S, T, VEC>), dim3((unsigned)gx, B), 256, 0, s, (const S*)src, offsets, sizes, N, idx, aug, (T*)out,
                       H, W, pad_value);
}

template <typename S>
int augmented_dst(const void* src, const long* offsets, const int* sizes, int N, const int* idx, const OmrAugment* aug, int dst_dtype, void* out, int B,
                  int H, int W, float pad_value, hipStream_t s) {
    const bool aligned = (uintptr_t)out % 16 == 0;
    if (dst_dtype == OMR_F32) {
        if (aligned && W % 4 == 0) launch_augmented<S, float, 4>(src, offsets, sizes, N, idx, aug, out, B, H, W, pad_value, s);
        else launch_augmented<S, float, 1>(src, offsets, sizes, N, idx, aug, out, B, H, W, pad_value, s);
    } else if (dst_dtype == OMR_BF16) {
        if (aligned && W % 8 == 0) launch_augmented<S, bf16, 8>(src, offsets, sizes, N, idx, aug, out, B, H, W, pad_value, s);
        else launch_augmented<S, bf16, 1>(src, offsets, sizes, N, idx, aug, out, B, H, W, pad_value, s);
    } else return OMR_ERR_UNSUPPORTED;
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

}  // namespace

extern "C" int omr_gather_augmented_batch(int src_dtype, const void* src, const long* offsets, const int* sizes, int N, const int* idx,
                                          const OmrAugment* aug, int dst_dtype, void* out, int B, int H, int W, float pad_value, void* stream) {
    if (!src || !offsets || !sizes || !idx || !aug || !out || N < 1 || B < 1 || B > 65535 || H < 1 || W < 1 || (long)H * W > 0x7fffffffL) return OMR_ERR_ARG;
    if (src_dtype == OMR_DTYPE_U8)
        return augmented_dst<unsigned char>(src, offsets, sizes, N, idx, aug, dst_dtype, out, B, H, W, pad_value, (hipStream_t)stream);
    if (src_dtype == OMR_F32) return augmented_dst<float>(src, offsets, sizes, N, idx, aug, dst_dtype, out, B, H, W, pad_value, (hipStream_t)stream);
    return OMR_ERR_UNSUPPORTED;
}
