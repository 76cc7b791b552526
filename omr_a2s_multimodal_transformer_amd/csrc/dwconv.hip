// Depthwise 3x3, stride 1, pad 1 on NHWC (DepthSepConv2D.depth_conv, encoder.py:56-64) on gfx950: forward, data gradient
// (flip = 1 applies the taps mirrored) and weight / bias gradient.  HBM-bound VALU kernels.  Optional fused InstanceNorm
// apply on the input and optional epilogue mask (ReLU/dropout backward of the producer).  Three forms per direction:
//   tile      a workgroup stages a halo tile through LDS (the DSC blocks' 16 x 256 maps: the hot path)
//   walk      a thread walks down an image column with a 3x3 register window (tiles that do not fit, unaligned weights)
//   per-pixel forward only: any height and channel count
// The pieces the forms share are written once: DwHalo (tile staging), DwRowWindow (register window) and dw_store (epilogue).
#include <type_traits>

#include "omr_common.h"
#include "omr_hip.h"

#include "launch_setup.h"

namespace {

constexpr int DW_TR = 8;      // output rows per tile

// Store epilogue of the forward kernels: s, masked by the producer's ReLU/dropout output when there is one, as one 16-byte store.
template <typename T>
__device__ __forceinline__ void dw_store(T* y, const T* mask, float mask_scale, long off, const float (&s)[Frag<T>::N]) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = Frag<T>::N;
    F o;
    if (mask) {
        const F mk = *reinterpret_cast<const F*>(mask + off);
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = from_f32<T>(to_f32(mk[e]) > 0.f ? s[e] * mask_scale : 0.f);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = from_f32<T>(s[e]);
    }
    *reinterpret_cast<F*>(y + off) = o;
}

// Halo tile [DW_TR + 2][IWt = TC + 2][C] of a 256-thread workgroup, origin (r0 - 1, j0 - 1) of image xb: thread tid owns the
// 16-byte chunks tid + 256 i, i < NLD (the host guarantees nchunk <= 256 NLD).  load() issues all of them before anything is
// consumed; store() normalises on the way into LDS (rounded to T like the MFMA convs; padding stays exactly 0).  What a caller
// puts between the two rides in flight with the halo.
template <typename T, int NLD> struct DwHalo {
    typedef typename Frag<T>::type F;
    static constexpr int VEC = Frag<T>::N;
    F ld[NLD];
    unsigned okbits;
    __device__ __forceinline__ void load(const T* xb, int tid, int cv, int IWt, int nchunk, int r0, int j0, int H, int Wd, int C) {
        okbits = 0;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int ch = tid + i * 256, pp = ch / cv, gi = ch - pp * cv;
            const int ti = pp / IWt, tj = pp - ti * IWt, r = r0 - 1 + ti, j = j0 - 1 + tj;
            const bool ok = ch < nchunk && r >= 0 && r < H && j >= 0 && j < Wd;
            ld[i] = frag_zero<T>();
            if (ok) ld[i] = *reinterpret_cast<const F*>(xb + ((long)r * Wd + j) * C + gi * VEC);
            okbits |= (unsigned)ok << i;
        }
    }
    __device__ __forceinline__ void store(T* tile, const float* mean, const float* rstd, int b, int tid, int cv, int nchunk, int C) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int ch = tid + i * 256;
            if (ch >= nchunk) break;
            if (mean && ((okbits >> i) & 1)) {
                const int gi = ch % cv;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float rs = rstd[b * C + gi * VEC + e], nb = -mean[b * C + gi * VEC + e] * rs;
                    ld[i][e] = from_f32<T>(fmaf(to_f32(ld[i][e]), rs, nb));
                }
            }
            *reinterpret_cast<F*>(tile + (long)ch * VEC) = ld[i];
        }
    }
};

// 3x3 register window of the row walkers: thread = (image column j, channel group), win[kh][kw] = the (normalised, zero-padded)
// input of rows r - 1 .. r + 1, columns j - 1 .. j + 1, kept in the compute dtype.  xb points at the thread's channel group of
// pixel (0, 0) of its image; sc is the index of that group in mean / rstd.
template <typename T> struct DwRowWindow {
    typedef typename Frag<T>::type F;
    static constexpr int VEC = Frag<T>::N;
    const T* xb;
    int j, H, Wd, C;
    bool cl, cr, norm;
    float rs[VEC], nb[VEC];
    F win[3][3];
    __device__ __forceinline__ DwRowWindow(const T* xb_, const float* mean, const float* rstd, long sc, int j_, int H_, int Wd_, int C_)
        : xb(xb_), j(j_), H(H_), Wd(Wd_), C(C_), cl(j_ > 0), cr(j_ + 1 < Wd_), norm(mean != nullptr) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            rs[e] = rstd ? rstd[sc + e] : 1.f;
            nb[e] = mean ? -mean[sc + e] * rs[e] : 0.f;
        }
    }
    // raw row r of the three columns j-1, j, j+1 (zero fragments outside the image); `ok` tells convert() which are real
    __device__ __forceinline__ void fetch(int r, F (&raw)[3], bool& ok) const {
        ok = r >= 0 && r < H;
        raw[0] = raw[1] = raw[2] = frag_zero<T>();
        if (ok) {
            const T* xr = xb + ((long)r * Wd + j) * C;
            raw[1] = *reinterpret_cast<const F*>(xr);
            if (cl) raw[0] = *reinterpret_cast<const F*>(xr - C);
            if (cr) raw[2] = *reinterpret_cast<const F*>(xr + C);
        }
    }
    // normalise (rounded to T, as the MFMA convs do); padding stays exactly 0: it lives in the normalised space
    __device__ __forceinline__ void convert(const F (&raw)[3], bool ok, F (&row)[3]) const {
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const bool v = ok && (kw == 1 || (kw == 0 ? cl : cr));
            if (norm) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) row[kw][e] = v ? from_f32<T>(fmaf(to_f32(raw[kw][e]), rs[e], nb[e])) : from_f32<T>(0.f);
            } else {
                row[kw] = raw[kw];                                  // fetch() already zero-filled what lies outside
            }
        }
    }
    __device__ __forceinline__ void fill(int kh, int r) { F raw[3]; bool ok; fetch(r, raw, ok); convert(raw, ok, win[kh]); }
    // one row down: the fetched row `raw` becomes the bottom row of the window
    __device__ __forceinline__ void shift_down(const F (&raw)[3], bool ok) {
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) { win[0][kw] = win[1][kw]; win[1][kw] = win[2][kw]; }
        convert(raw, ok, win[2]);
    }
};

// ------------------------------------------------------------------------------------------------
// Per-pixel form: one thread = one pixel x VEC channels.
template <typename T>
__global__ __launch_bounds__(256) void dwconv3x3_kernel(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias, T* __restrict__ y,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd, const T* __restrict__ mask, float mask_scale,
                                                        int B, int H, int Wd, int C, int flip) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = Frag<T>::N;
    extern __shared__ __attribute__((aligned(16))) float wsm[];   // [9][C] taps (already mirrored when flip) + [C] bias
    for (int i = threadIdx.x; i < 9 * C; i += blockDim.x) {
        const int t = i / C, c = i % C;
        wsm[i] = to_f32(w[c * 9 + (flip ? 8 - t : t)]);
    }
    for (int i = threadIdx.x; i < C; i += blockDim.x) wsm[9 * C + i] = bias ? bias[i] : 0.f;
    __syncthreads();
    const int cv = C / VEC;
    const long total = (long)B * H * Wd * cv;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % cv) * VEC; long p = i / cv;
        const int j = (int)(p % Wd); long q = p / Wd; const int ii = (int)(q % H); const long b = q / H;
        F xv[9];
        bool ok[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {          // issue all nine 16-byte loads before using any
            const int yy = ii + t / 3 - 1, xx = j + t % 3 - 1;
            ok[t] = yy >= 0 && yy < H && xx >= 0 && xx < Wd;
            if (ok[t]) xv[t] = *reinterpret_cast<const F*>(x + ((b * H + yy) * Wd + xx) * C + c);
        }
        float s[VEC], mu[VEC], rs[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            s[e] = wsm[9 * C + c + e];
            mu[e] = mean ? mean[b * C + c + e] : 0.f;
            rs[e] = rstd ? rstd[b * C + c + e] : 1.f;
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if (!ok[t]) continue;
#pragma unroll
            for (int e = 0; e < VEC; ++e) s[e] += wsm[t * C + c + e] * ((to_f32(xv[t][e]) - mu[e]) * rs[e]);
        }
        dw_store<T>(y, mask, mask_scale, p * C + c, s);
    }
}

// Row-walking form of the same op for the DSC blocks (16 x 256 maps, 128-256 channels: tensors of 30-70 MB where the
// per-pixel kernel above is latency-bound at ~1.3 TB/s).  Thread = (image column, channel group): it walks RC rows of one
// image with a 3x3 register window of the (normalised, zero-padded) input, so a pixel costs 3 new 16-byte loads
// (two rows ahead are in flight behind this row's FMAs) instead of 9, and the InstanceNorm apply is paid once per loaded element
// instead of once per tap.  Taps and bias sit in LDS as above.
template <typename T>
__global__ __launch_bounds__(256) void dwconv3x3_walk_kernel(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias, T* __restrict__ y,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd, const T* __restrict__ mask,
                                                             float mask_scale, int B, int H, int Wd, int C, int flip, int RC) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = Frag<T>::N;
    // taps [9][C] in the compute dtype (already mirrored when flip), read as ONE 16-byte fragment per tap per thread: lanes
    // step 16 bytes, conflict-free, where scalar fp32 reads at a 32-byte lane stride were 8-way bank conflicted and
    // dominated the kernel.  The fp32 bias follows (2 x 16 bytes per thread).
    extern __shared__ __attribute__((aligned(16))) unsigned char wraw[];
    T* wt = reinterpret_cast<T*>(wraw);
    float* wbias = reinterpret_cast<float*>(wraw + (size_t)9 * C * sizeof(T));
    for (int i = threadIdx.x; i < 9 * C; i += blockDim.x) {
        const int t = i / C, c = i % C;
        wt[i] = w[c * 9 + (flip ? 8 - t : t)];
    }
    for (int i = threadIdx.x; i < C; i += blockDim.x) wbias[i] = bias ? bias[i] : 0.f;
    __syncthreads();
    const int cv = C / VEC;
    const int c = (threadIdx.x % cv) * VEC, j = blockIdx.x * (blockDim.x / cv) + threadIdx.x / cv;
    if (j >= Wd) return;
    const int chunks = cdiv(H, RC);
    const int b = blockIdx.y / chunks, r0 = (blockIdx.y % chunks) * RC, r1 = min(H, r0 + RC);
    DwRowWindow<T> rw(x + (long)b * H * Wd * C + c, mean, rstd, b * C + c, j, H, Wd, C);
    F rawa[3], rawb[3];
    bool oka, okb;
    rw.fill(0, r0 - 1);
    rw.fill(1, r0);
    rw.fill(2, r0 + 1);
    rw.fetch(r0 + 2, rawa, oka);                                 // two rows of loads stay in flight behind the math
    for (int r = r0; r < r1; ++r) {
        rw.fetch(r + 3, rawb, okb);
        asm volatile("" ::: "memory");                          // keep the taps in LDS (72+ registers otherwise)
        float s[VEC];
#pragma unroll
        for (int e = 0; e < VEC; e += 4) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(wbias + c + e);
            s[e] = bv[0]; s[e + 1] = bv[1]; s[e + 2] = bv[2]; s[e + 3] = bv[3];
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const F wv = *reinterpret_cast<const F*>(wt + t * C + c);
#pragma unroll
            for (int e = 0; e < VEC; ++e) s[e] = fmaf(to_f32(wv[e]), to_f32(rw.win[t / 3][t % 3][e]), s[e]);
        }
        const long p = ((long)b * H + r) * Wd + j;
        dw_store<T>(y, mask, mask_scale, p * C + c, s);
        rw.shift_down(rawa, oka);
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) rawa[kw] = rawb[kw];
        oka = okb;
    }
}

// Tile form of the same op (the DSC blocks' 16 x 256 maps): the walker above keeps only two rows of loads in flight per thread
// and fetches every input element three times (columns j-1, j, j+1), so its 8-row walk is a chain of exposed latencies
// (1.4 TB/s).  Here a workgroup stages an (8+2) x (TC+2) x C halo tile through LDS -- every element requested once, ALL of a
// thread's requests in flight together, the InstanceNorm apply and the zero padding done on the way in -- and then each
// thread produces its (column, channel group)'s 8 outputs from 9 conflict-free 16-byte LDS reads per output against taps
// held in registers as fp32 (one contiguous 9 x VEC run of the [C][9] weight per thread).
template <typename T>
__global__ __launch_bounds__(256) void dwconv3x3_tile_kernel(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias, T* __restrict__ y,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd, const T* __restrict__ mask,
                                                             float mask_scale, int B, int H, int Wd, int C, int flip) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = Frag<T>::N, NLD = 16;                    // NLD: 16-byte halo chunks per thread (host guarantees the tile fits)
    extern __shared__ __attribute__((aligned(16))) unsigned char traw[];
    T* tile = reinterpret_cast<T*>(traw);                         // [DW_TR + 2][TC + 2][C]
    const int cv = C / VEC, TC = 256 / cv, IWt = TC + 2;
    const int tid = threadIdx.x, cg = tid % cv, col = tid / cv, c = cg * VEC;
    const int tiles_h = cdiv(H, DW_TR);
    const int b = blockIdx.y / tiles_h, r0 = (blockIdx.y % tiles_h) * DW_TR, j0 = blockIdx.x * TC;
    const T* xb = x + (long)b * H * Wd * C;
    // ---- all halo requests of this thread, then the taps, before anything is consumed
    const int nchunk = (DW_TR + 2) * IWt * cv;
    DwHalo<T, NLD> halo;
    halo.load(xb, tid, cv, IWt, nchunk, r0, j0, H, Wd, C);
    F wraw[9];                                                    // w[c*9 .. c*9 + 9*VEC): element e*9 + t is tap t of channel c + e
#pragma unroll
    for (int i = 0; i < 9; ++i) wraw[i] = *reinterpret_cast<const F*>(w + (long)c * 9 + i * VEC);
    float bv[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) bv[e] = bias ? bias[c + e] : 0.f;
    halo.store(tile, mean, rstd, b, tid, cv, nchunk, C);
    float wt[9][VEC];
    auto unpack = [&](auto fl) {                                  // (mirrored taps for the data gradient) -- indices are compile-time
        constexpr bool FL = decltype(fl)::value;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int idx = e * 9 + (FL ? 8 - t : t);
                wt[t][e] = to_f32(wraw[idx / VEC][idx % VEC]);
            }
    };
    if (flip) unpack(std::true_type()); else unpack(std::false_type());
    __syncthreads();
    const int j = j0 + col;
    if (j >= Wd) return;
#pragma unroll 2
    for (int rr = 0; rr < DW_TR; ++rr) {
        const int r = r0 + rr;
        if (r >= H) break;
        float sacc[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) sacc[e] = bv[e];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const F xv = *reinterpret_cast<const F*>(tile + ((long)((rr + t / 3) * IWt + col + t % 3) * cv + cg) * VEC);
#pragma unroll
            for (int e = 0; e < VEC; ++e) sacc[e] = fmaf(wt[t][e], to_f32(xv[e]), sacc[e]);
        }
        const long p = ((long)b * H + r) * Wd + j;
        dw_store<T>(y, mask, mask_scale, p * C + c, sacc);
    }
}

// Weight / bias gradient on the same tile: dW[c][tap] += sum_p dY[p][c] xin[p+tap][c], db[c] += sum_p dY[p][c].  The halo tile
// of the (normalised) input goes through LDS as above, the thread's 8 dY fragments ride in registers with it (one round
// trip for everything), 80 fp32 partial sums per thread.  Fold: the columns a wave holds for one channel group sit 16 / 32
// lanes apart -> v_permlane16_swap / v_permlane32_swap + add; the four waves through LDS; one atomic per weight per
// workgroup.  (The row walker below keeps a whole image column per thread: 512 workgroups, 7x its HBM time.)
template <typename T, int NLD>
__global__ __launch_bounds__(256, 2) void dwconv3x3_wgrad_tile_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ dw, float* __restrict__ db,
                                                                   const float* __restrict__ mean, const float* __restrict__ rstd, int B, int H, int Wd, int C) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = Frag<T>::N;                               // NLD: 16-byte halo chunks per thread (12 for the 128-channel bf16 tile, else 16)
    extern __shared__ __attribute__((aligned(16))) unsigned char traw[];
    T* tile = reinterpret_cast<T*>(traw);                         // [DW_TR + 2][TC + 2][C]; afterwards the cross-wave fold scratch
    const int cv = C / VEC, TC = 256 / cv, IWt = TC + 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cg = tid % cv, col = tid / cv, c = cg * VEC;
    const int tiles_h = cdiv(H, DW_TR), tiles_w = cdiv(Wd, TC), ntiles = B * tiles_h * tiles_w;
    const int nchunk = (DW_TR + 2) * IWt * cv;
    float acc[10][VEC];                                           // [tap 0..8 | bias][channel], kept over all tiles of this workgroup
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[t][e] = 0.f;
    // persistent over tiles: the fold and the atomics at the end are paid once per workgroup (a memory-side float atomic
    // serialises per cache line -- one per tile was 1.3 M atomics onto 40 lines, 3x the time of everything else)
    for (int tile_id = blockIdx.x; tile_id < ntiles; tile_id += gridDim.x) {
        const int b = tile_id / (tiles_h * tiles_w), rem = tile_id - b * tiles_h * tiles_w;
        const int r0 = (rem / tiles_w) * DW_TR, j0 = (rem % tiles_w) * TC, j = j0 + col;
        const T* xb = x + (long)b * H * Wd * C;
        DwHalo<T, NLD> halo;
        halo.load(xb, tid, cv, IWt, nchunk, r0, j0, H, Wd, C);
        const T* dyp = dy + (((long)b * H + r0) * Wd + j) * C + c;   // this thread's dY fragments, one row ahead of their use
        auto load_gy = [&](int rr) { return (j < Wd && r0 + rr < H) ? *reinterpret_cast<const F*>(dyp + (long)rr * Wd * C) : frag_zero<T>(); };
        F gnext = load_gy(0);
        __syncthreads();                                          // the previous tile's reads are done
        halo.store(tile, mean, rstd, b, tid, cv, nchunk, C);
        __syncthreads();
#pragma unroll 1
        for (int rr = 0; rr < DW_TR; ++rr) {                      // zero dY fragments (rows / columns past the image) add nothing
            const F gcur = gnext;
            if (rr + 1 < DW_TR) gnext = load_gy(rr + 1);
            float g[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) { g[e] = to_f32(gcur[e]); acc[9][e] += g[e]; }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const F xv = *reinterpret_cast<const F*>(tile + ((long)((rr + t / 3) * IWt + col + t % 3) * cv + cg) * VEC);
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[t][e] = fmaf(g[e], to_f32(xv[e]), acc[t][e]);
            }
        }
    }
    // ---- fold the columns of this wave that share the channel group (lanes cv apart: cv = 16 or 32; cv >= 64: one column per wave)
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (cv <= 32) acc[t][e] += __shfl_xor(acc[t][e], 32, 64);
            if (cv == 16) acc[t][e] += __shfl_xor(acc[t][e], 16, 64);
        }
    // ---- the waves through LDS (the tile is dead), then one atomic per weight per workgroup
    __syncthreads();
    float* red = reinterpret_cast<float*>(traw);                  // [wave-slot][cg][10][VEC]
    const bool wide = cv >= 64;                                   // a column spans whole waves: every thread is the only holder of its (column, group)
    const int slot = wide ? col : wave, nslot = wide ? TC : 4;
    if (wide || lane < cv) {
        float* rp = red + ((long)slot * cv + cg) * 10 * VEC;
#pragma unroll
        for (int t = 0; t < 10; ++t)
#pragma unroll
            for (int e = 0; e < VEC; ++e) rp[t * VEC + e] = acc[t][e];
    }
    __syncthreads();
    for (int i = tid; i < cv * 10 * VEC; i += 256) {
        float v = 0.f;
        for (int sl = 0; sl < nslot; ++sl) v += red[(long)sl * cv * 10 * VEC + i];
        const int g2 = i / (10 * VEC), rem = i - g2 * 10 * VEC, t = rem / VEC, e = rem - t * VEC, ch = g2 * VEC + e;
        if (t < 9) atomicAdd(&dw[(long)ch * 9 + t], v);
        else if (db) atomicAdd(&db[ch], v);
    }
}

// dW[c][tap] += sum_p dY[p][c] xin[p+tap][c];  db[c] += sum_p dY[p][c].
// Thread = (image column j, channel group): it walks DOWN the rows of one image with a 3x3 register window of the
// normalised input (kept in the compute dtype) -- per pixel 3 new 16-byte x loads + 1 dY load, issued a row ahead of their
// use, for 9*VEC FMAs.  The 10*VEC partial sums stay in registers for the whole column (splitting the rows over more
// workgroups was tried: the 80-value fold below then dominates); wave shuffles fold the columns, then LDS and one global
// atomic per weight per workgroup.
template <typename T>
__global__ __launch_bounds__(256) void dwconv3x3_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ dw, float* __restrict__ db,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd, int B, int H, int Wd, int C) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = Frag<T>::N;
    extern __shared__ __attribute__((aligned(16))) float red[];   // [C][10]
    for (int i = threadIdx.x; i < C * 10; i += blockDim.x) red[i] = 0.f;
    __syncthreads();
    const int ncg = C / VEC, cpb = blockDim.x / ncg;
    const int cg = threadIdx.x % ncg, j = blockIdx.x * cpb + threadIdx.x / ncg, b = blockIdx.y;
    float acc[10][VEC];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[t][e] = 0.f;
    if (j < Wd) {
        DwRowWindow<T> rw(x + (long)b * H * Wd * C + cg * VEC, mean, rstd, (long)b * C + cg * VEC, j, H, Wd, C);
        const T* dyp = dy + ((long)b * H * Wd + j) * C + cg * VEC;
        const long rstride = (long)Wd * C;
        F raw[3], gcur, gnext = frag_zero<T>();
        bool ok;
        rw.fill(0, -1);
        rw.fill(1, 0);
        rw.fill(2, 1);
        gcur = *reinterpret_cast<const F*>(dyp);
        for (int r = 0; r < H; ++r) {
            rw.fetch(r + 2, raw, ok);                               // next row's operands fly behind this row's FMAs
            if (r + 1 < H) gnext = *reinterpret_cast<const F*>(dyp + (long)(r + 1) * rstride);
            float g[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) { g[e] = to_f32(gcur[e]); acc[9][e] += g[e]; }
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[t][e] = fmaf(g[e], to_f32(rw.win[t / 3][t % 3][e]), acc[t][e]);
            rw.shift_down(raw, ok);
            gcur = gnext;
        }
    }
    // fold the columns that share this lane's channel group (lanes cg, cg+ncg, ...), then LDS, then global
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float v = acc[t][e];
            for (int o = ncg; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
            if (lane < ncg) atomicAdd(&red[(cg * VEC + e) * 10 + t], v);
        }
    __syncthreads();
    for (int i = threadIdx.x; i < C * 10; i += blockDim.x) {
        const int c = i / 10, tt = i % 10;
        if (tt < 9) atomicAdd(&dw[c * 9 + tt], red[i]);
        else if (db) atomicAdd(&db[c], red[i]);
    }
}

// Host-side plan of the LDS-tile kernels for C channels of `dtype` on H-row images: computed once per call by both entry points.
struct DwTilePlan {
    int vec, cv, tc, nchunk;     // elements per 16-byte chunk, chunks per pixel, tile columns (0: no whole split of 256 threads), chunks per halo tile
    size_t tile_bytes;           // dynamic LDS of the launch
    bool fits;                   // the tile kernel of this direction takes the shape
    DwTilePlan(int dtype, int C, int H, bool wgrad) {
        vec = dtype == OMR_BF16 ? 8 : 4;
        const size_t esz = dtype == OMR_BF16 ? 2 : 4;
        cv = C / vec;
        tc = cv <= 256 && 256 % cv == 0 ? 256 / cv : 0;
        nchunk = (DW_TR + 2) * (tc + 2) * cv;
        tile_bytes = (size_t)(DW_TR + 2) * (tc + 2) * C * esz;
        bool shape = tc >= 2;
        if (wgrad) {             // the cross-wave fold reuses the tile: [wave or column slot][cv][10][vec] floats
            const size_t red_bytes = (size_t)(cv >= 64 ? tc : 4) * cv * 10 * vec * sizeof(float);
            if (red_bytes > tile_bytes) tile_bytes = red_bytes;
            shape = (cv == 16 || cv == 32 || (cv >= 64 && cv <= 256)) && tc >= 1;
        }
        fits = shape && H >= 4 && tile_bytes <= 64 * 1024 && nchunk <= 16 * 256;     // at most 16 chunks per thread
    }
};

// Launch tile kernel KERN on the plan's LDS; tiles above 32 KB need the large-LDS opt-in, issued once per instantiation.
template <auto KERN, typename... A> int launch_dw_tiles(const DwTilePlan& p, dim3 grid, hipStream_t s, A... args) {
    static std::atomic<int> opt_in{0};
    if (p.tile_bytes > 32 * 1024 && !omr_launch_setup(opt_in, (const void*)KERN, 64 * 1024, true)) return OMR_ERR_LAUNCH;
    hipLaunchKernelGGL(KERN, grid, 256, p.tile_bytes, s, args...);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

}  // namespace

extern "C" int omr_dwconv3x3(int dtype, const void* x, const void* w, const float* bias, void* y, const float* in_mean, const float* in_rstd,
                             const void* out_mask, float mask_scale, int B, int H, int W, int C, int flip, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return OMR_ERR_ARG;
    if (C % (dtype == OMR_BF16 ? 8 : 4)) return OMR_ERR_UNSUPPORTED;
    const DwTilePlan p(dtype, C, H, false);
    hipStream_t s = (hipStream_t)stream;
    if (p.fits && ((uintptr_t)w & 15) == 0) {      // LDS tile (DSC blocks); the taps are read as 16-byte fragments
        const dim3 gridt(cdiv(W, p.tc), B * cdiv(H, DW_TR));
        DISPATCH_T(dtype, return launch_dw_tiles<dwconv3x3_tile_kernel<T>>(p, gridt, s, (const T*)x, (const T*)w, bias, (T*)y, in_mean, in_rstd, (const T*)out_mask,
                                                                           mask_scale, B, H, W, C, flip));
    }
    if (p.tc >= 1 && H >= 4 && (size_t)10 * C * sizeof(float) <= 48 * 1024) {      // row walker (tiles that do not fit the LDS budget)
        int RC = 8;                                              // rows per thread: 2 halo rows re-read per RC
        while (RC < H && (long)cdiv(W, p.tc) * B * cdiv(H, RC) > 4096) RC *= 2;
        dim3 gridw(cdiv(W, p.tc), B * cdiv(H, RC));
        DISPATCH_T(dtype, hipLaunchKernelGGL((dwconv3x3_walk_kernel<T>), gridw, 256, (size_t)9 * C * sizeof(T) + (size_t)C * sizeof(float), s, (const T*)x, (const T*)w, bias,
                                             (T*)y, in_mean, in_rstd, (const T*)out_mask, mask_scale, B, H, W, C, flip, RC));
        OMR_CHECK_LAUNCH();
        return OMR_OK;
    }
    long total = (long)B * H * W * p.cv;
    int grid = (int)((total + 1023) / 1024); if (grid > 2048) grid = 2048; if (grid < 1) grid = 1;   // >= 4 pixels x groups per thread amortise the weight staging
    DISPATCH_T(dtype, hipLaunchKernelGGL((dwconv3x3_kernel<T>), grid, 256, (size_t)10 * C * sizeof(float), s, (const T*)x, (const T*)w, bias, (T*)y,
                                         in_mean, in_rstd, (const T*)out_mask, mask_scale, B, H, W, C, flip));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_dwconv3x3_wgrad(int dtype, const void* x, const void* dy, float* dw, float* db, const float* in_mean, const float* in_rstd,
                                   int B, int H, int W, int C, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return OMR_ERR_ARG;
    const int vec = dtype == OMR_BF16 ? 8 : 4;
    if (C % vec || 256 % (C / vec)) return OMR_ERR_UNSUPPORTED;
    const DwTilePlan p(dtype, C, H, true);
    hipStream_t s = (hipStream_t)stream;
    if (p.fits) {
        const long ntiles = (long)cdiv(W, p.tc) * B * cdiv(H, DW_TR);
        const dim3 gridt((unsigned)(ntiles < OMR_NUM_CU ? ntiles : OMR_NUM_CU));   // persistent: one workgroup per CU (the closing atomics are per workgroup)
        if (p.nchunk <= 12 * 256) {     // NLD: 16-byte halo chunks per thread
            DISPATCH_T(dtype, return (launch_dw_tiles<dwconv3x3_wgrad_tile_kernel<T, 12>>(p, gridt, s, (const T*)x, (const T*)dy, dw, db, in_mean, in_rstd, B, H, W, C)));
        }
        DISPATCH_T(dtype, return (launch_dw_tiles<dwconv3x3_wgrad_tile_kernel<T, 16>>(p, gridt, s, (const T*)x, (const T*)dy, dw, db, in_mean, in_rstd, B, H, W, C)));
    }
    const int ncg = p.cv;
    if (ncg > 64 || 64 % ncg) return OMR_ERR_UNSUPPORTED;          // a wave holds whole channel-group sets
    dim3 grid(cdiv(W, 256 / ncg), B);
    DISPATCH_T(dtype, hipLaunchKernelGGL((dwconv3x3_wgrad_kernel<T>), grid, 256, (size_t)C * 10 * sizeof(float), s,
                                         (const T*)x, (const T*)dy, dw, db, in_mean, in_rstd, B, H, W, C));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}
