// Ragged batches (gfx950): B samples of different sizes share one padded NHWC plane [B][H][W][C]; sample b's real content is the
// top-left h_b x w_b corner, extents[b] = (h_b, w_b).  The encoder keeps every activation ZERO outside its sample's extent: then a
// 3x3 / pad-1 conv at a position inside the extent reads what the sample run alone at h_b x w_b reads (its zero padding), and weight
// and bias gradients come out right from the dense kernels because both operands are zero outside (DESIGN.md "Ragged training").
//   omr_extent_zero                  writes the zeros back after every conv (bias + ReLU made the outside non-zero); its own adjoint
//   omr_instnorm_extent_fwd / _bwd   InstanceNorm2d(eps=1e-3, affine=False) with its sums over the extent only, count h_b * w_b
//   omr_pack_memory_fwd / _bwd       [B][H'][W'][d] feature grid <-> [B][Smax][d] decoder memory, row i * w'_b + j = cell (i, j)
//   omr_concat_memory_fwd / _bwd     two packed memories with per-sample lengths <-> their per-sample concatenation (multimodal mixers)
// All memory-bound: 16-byte accesses where C is a multiple of the fragment width (else one element per access: the 1-channel input
// image, odd widths), long offsets, statistics by the deterministic fp64 slot protocol of instnorm_slots.h (its EXTENT kernels; no
// atomics).  One sample holds at
// most 2^31 - 1 elements (the launchers check H * W * C), so positions INSIDE a sample are 32-bit and pixel -> (row, column) is a 32-bit
// division; only the offset into the batch is 64-bit.  A value outside an extent is never read: conv outputs there are unspecified,
// the caller's padding may be anything (NaN in the tests).
#include "omr_common.h"
#include "omr_hip.h"
#include "instnorm_slots.h"      // Pack, clampi and the statistics kernels

namespace {

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

// ------------------------------------------------------------------------------------------------
// Two packed memories a [B][La][C], b [B][Lb][C] with per-sample lengths la, lb -> one memory [B][Smax][C]: torch.cat([xi, xa], dim=1)
// of each sample alone.  !BWD (src = a, src2 = b, dst = out): out[r] = a[r] for r < la, b[r - la] for la <= r < la + lb, 0 behind.
// BWD (src = dout, dst = da, dst2 = db): da[r] = dout[r] for r < min(la, Smax), db[r] = dout[la + r] for r < lb and la + r < Smax, 0
// elsewhere; da, then db, each walked linearly.  Lb = 0 (b / db null, len_b not read): copy the first la rows and zero the rest.  Rows
// of a / b at or past their length and rows of dout at or past la + lb are not read.
template <typename T, int VEC, bool BWD>
__global__ __launch_bounds__(256) void concat_memory_kernel(const T* __restrict__ src, const T* __restrict__ src2, const int* __restrict__ len_a,
                                                            const int* __restrict__ len_b, T* __restrict__ dst, T* __restrict__ dst2, int La, int Lb, int C,
                                                            int Smax) {
    typedef Pack<T, VEC> P;
    const int b = blockIdx.y;
    const unsigned cv = C / VEC;
    const unsigned la = clampi(len_a[b], 0, La), lb = Lb > 0 ? clampi(len_b[b], 0, Lb) : 0;
    const unsigned first = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    const P z = pack_zero<T, VEC>();
    if (!BWD) {
        const T* ab = src + (long)b * La * C;
        const T* bb = src2 + (long)b * Lb * C;       // not dereferenced when Lb = 0
        T* ob = dst + (long)b * Smax * C;
        for (unsigned t = first; t < (unsigned)Smax * cv; t += step) {
            const unsigned r = t / cv, c = (t - r * cv) * VEC;
            P o = z;
            if (r < la) o = *reinterpret_cast<const P*>(ab + (long)r * C + c);
            else if (r < la + lb) o = *reinterpret_cast<const P*>(bb + (long)(r - la) * C + c);
            *reinterpret_cast<P*>(ob + (long)t * VEC) = o;
        }
    } else {
        const T* gb = src + (long)b * Smax * C;
        T* da = dst + (long)b * La * C;
        T* db = dst2 + (long)b * Lb * C;
        const unsigned na = la < (unsigned)Smax ? la : (unsigned)Smax;                 // rows of da that have a row of dout
        const unsigned nb = la >= (unsigned)Smax ? 0u : (lb < Smax - la ? lb : Smax - la);   // rows of db that have one
        for (unsigned t = first; t < (unsigned)La * cv; t += step) {
            const unsigned r = t / cv;
            *reinterpret_cast<P*>(da + (long)t * VEC) = r < na ? *reinterpret_cast<const P*>(gb + (long)t * VEC) : z;
        }
        for (unsigned t = first; t < (unsigned)Lb * cv; t += step) {
            const unsigned r = t / cv;
            *reinterpret_cast<P*>(db + (long)t * VEC) = r < nb ? *reinterpret_cast<const P*>(gb + (long)la * C + (long)t * VEC) : z;
        }
    }
}

}  // namespace

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
extern "C" int omr_instnorm_extent_slots(int B, long HW) { return (B <= 0 || HW <= 0) ? OMR_ERR_ARG : cdiv(HW, instnorm_pixels_per_block(HW, B)); }

// The three launches of instnorm_slots.h over the extents: stage 1 into the slots, stage 2 (!BWD: mean / rstd with each sample's own count;
// BWD: the compact sums), apply over the whole plane (!BWD: out = y from x; BWD: out = dx from g = dxhat and x).
template <bool BWD>
static int launch_extent_norm(int dtype, int vec, const void* x, const void* g, float* mean, float* rstd, const int* ext, void* out, int B, int H, int W,
                              int C, float eps, int relu_mask, float relu_scale, double* ws, hipStream_t s) {
    if (C / vec > 256) return OMR_ERR_UNSUPPORTED;
    const long HW = (long)H * W;
    const int ppb = instnorm_pixels_per_block(HW, B), slots = cdiv(HW, ppb), ppb2 = 1024;
    double* compact = ws + slot_compact_offset(B, slots, C);
    DISPATCH_T_VEC(dtype, vec, hipLaunchKernelGGL((instnorm_partial_kernel<T, VEC, BWD, true>), dim3(slots, B), 256, instnorm_partial_lds_bytes(C, vec), s, (const T*)x,
                                                  (const T*)g, (const float*)(BWD ? mean : nullptr), (const float*)(BWD ? rstd : nullptr), ext, ws, H, W, HW, C, ppb));
    hipLaunchKernelGGL((instnorm_reduce_slots_kernel<!BWD>), B, 256, 0, s, (const double*)ws, ext, slots, H, W, C, BWD ? nullptr : mean, BWD ? nullptr : rstd,
                       BWD ? compact : nullptr, 0.0, eps);
    DISPATCH_T_VEC(dtype, vec, hipLaunchKernelGGL((instnorm_apply_kernel<T, VEC, BWD, true>), dim3(cdiv(HW, ppb2), B), 256, 0, s, (const T*)x, (const T*)g,
                                                  (const float*)mean, (const float*)rstd, (const double*)(BWD ? compact : nullptr), ext, (T*)out, H, W, HW, C, ppb2,
                                                  0.f, relu_mask, relu_scale));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_instnorm_extent_fwd(int dtype, const void* x, const int* extents, void* y, float* mean, float* rstd, int B, int H, int W, int C,
                                       float eps, void* workspace, void* stream) {
    if (!extent_args_ok(x, extents, B, H, W, C) || !y || !mean || !rstd || !workspace) return OMR_ERR_ARG;
    return launch_extent_norm<false>(dtype, extent_vec(dtype, C, x, y), x, nullptr, mean, rstd, extents, y, B, H, W, C, eps, 0, 1.f, (double*)workspace,
                                     (hipStream_t)stream);
}

extern "C" int omr_instnorm_extent_bwd(int dtype, const void* dxhat, const void* x, const float* mean, const float* rstd, const int* extents, void* dx,
                                       int B, int H, int W, int C, int relu_mask, float relu_scale, void* workspace, void* stream) {
    if (!extent_args_ok(x, extents, B, H, W, C) || !dxhat || !dx || !mean || !rstd || !workspace) return OMR_ERR_ARG;
    return launch_extent_norm<true>(dtype, extent_vec(dtype, C, x, dxhat, dx), x, dxhat, const_cast<float*>(mean), const_cast<float*>(rstd), extents, dx, B, H, W,
                                    C, 0.f, relu_mask, relu_scale, (double*)workspace, (hipStream_t)stream);
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

// a / La: the first memory (in the backward: its gradient); b / Lb: the second one, absent (null, Lb = 0) in the tail-zeroing form
static bool concat_args_ok(const void* a, const int* len_a, int La, const void* b, const int* len_b, int Lb, const void* o, int B, int C, int Smax) {
    return a && len_a && o && B > 0 && B <= 65535 && La > 0 && Lb >= 0 && C > 0 && Smax > 0 && (Lb == 0 || (b && len_b)) &&
           (long)La * C <= 0x7fffffffL && (long)Lb * C <= 0x7fffffffL && (long)Smax * C <= 0x7fffffffL;
}

extern "C" int omr_concat_memory_fwd(int dtype, const void* a, const int* len_a, int La, const void* b, const int* len_b, int Lb, void* out, int B, int C,
                                     int Smax, void* stream) {
    if (!concat_args_ok(a, len_a, La, b, len_b, Lb, out, B, C, Smax)) return OMR_ERR_ARG;
    if (Lb == 0) b = nullptr;
    const int vec = extent_vec(dtype, C, a, b, out);
    DISPATCH_T_VEC(dtype, vec, hipLaunchKernelGGL((concat_memory_kernel<T, VEC, false>), dim3(pack_grid((long)Smax * (C / vec)), B), 256, 0, (hipStream_t)stream,
                                                  (const T*)a, (const T*)b, len_a, len_b, (T*)out, (T*)nullptr, La, Lb, C, Smax));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_concat_memory_bwd(int dtype, const void* dout, const int* len_a, int La, const int* len_b, int Lb, void* da, void* db, int B, int C,
                                     int Smax, void* stream) {
    if (!concat_args_ok(da, len_a, La, db, len_b, Lb, dout, B, C, Smax)) return OMR_ERR_ARG;
    if (Lb == 0) db = nullptr;
    const int vec = extent_vec(dtype, C, dout, da, db);
    const long frags = (long)(La > Lb ? La : Lb) * (C / vec);         // both destinations are walked by the same grid
    DISPATCH_T_VEC(dtype, vec, hipLaunchKernelGGL((concat_memory_kernel<T, VEC, true>), dim3(pack_grid(frags), B), 256, 0, (hipStream_t)stream,
                                                  (const T*)dout, (const T*)nullptr, len_a, len_b, (T*)da, (T*)db, La, Lb, C, Smax));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}
