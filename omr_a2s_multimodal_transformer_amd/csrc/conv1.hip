// First layer of the CNN encoder on gfx950: the 1 -> 16 (or 32) 3x3 conv, forward and weight gradient.  K = 9, so both are
// HBM-bound VALU / single-MFMA kernels of their own, not the MFMA tile kernels of conv.hip.  NHWC, weights [COUT][3][3][1].
#include "omr_common.h"
#include "omr_hip.h"

#include "conv1.h"
#include "launch_setup.h"

namespace {

// First layer: Cin = 1 -> COUT (<= 32) with ReLU; K = 9, HBM-bound (2 B in, 2 COUT B out per pixel).
// Thread = one image column: it walks down RC rows of one image with a 3x3 register window (3 new 2-byte loads per
// pixel, the next row's already in flight while this row's 9 COUT FMAs run) and writes its pixel's COUT channels as 16-byte
// stores.  Weights sit in LDS tap-major and are read as broadcast float4s; ~50 VGPRs keep 8 waves per SIMD resident.
template <typename T, int COUT>
__global__ __launch_bounds__(256) void conv1_direct_kernel(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias, T* __restrict__ y, int B,
                                                           int H, int Wd, int relu, int RC) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = Frag<T>::N;
    __shared__ __attribute__((aligned(16))) float ws[10 * COUT];              // [tap][COUT] then bias
    for (int i = threadIdx.x; i < COUT * 9; i += blockDim.x) ws[(i % 9) * COUT + i / 9] = to_f32(w[i]);
    for (int i = threadIdx.x; i < COUT; i += blockDim.x) ws[9 * COUT + i] = bias ? bias[i] : 0.f;
    __syncthreads();
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= Wd) return;
    const int chunks = cdiv(H, RC);
    const int b = blockIdx.y / chunks, r0 = (blockIdx.y % chunks) * RC, r1 = min(H, r0 + RC);
    const T* xb = x + (long)b * H * Wd;
    T* yb = y + (long)b * H * Wd * COUT;
    auto load_row = [&](int r, float (&row)[3]) {
        row[0] = row[1] = row[2] = 0.f;
        if (r >= 0 && r < H) {
            const T* xr = xb + (long)r * Wd + j;
            row[1] = to_f32(xr[0]);
            if (j > 0) row[0] = to_f32(xr[-1]);
            if (j + 1 < Wd) row[2] = to_f32(xr[1]);
        }
    };
    float win[3][3], nxt[3];
    load_row(r0 - 1, win[0]);
    load_row(r0, win[1]);
    load_row(r0 + 1, win[2]);
    for (int r = r0; r < r1; ++r) {
        load_row(r + 2, nxt);                                   // in flight behind this row's math
        asm volatile("" ::: "memory");                          // re-read the weights from LDS every row: hoisting all 10 COUT of them costs the occupancy
        float acc[COUT];
#pragma unroll
        for (int n = 0; n < COUT; n += 4) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(&ws[9 * COUT + n]);
            acc[n] = bv[0]; acc[n + 1] = bv[1]; acc[n + 2] = bv[2]; acc[n + 3] = bv[3];
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float xv = win[t / 3][t % 3];
#pragma unroll
            for (int n = 0; n < COUT; n += 4) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(&ws[t * COUT + n]);
                acc[n] += wv[0] * xv; acc[n + 1] += wv[1] * xv; acc[n + 2] += wv[2] * xv; acc[n + 3] += wv[3] * xv;
            }
        }
        F* dst = reinterpret_cast<F*>(yb + ((long)r * Wd + j) * COUT);
#pragma unroll
        for (int v = 0; v < COUT / VEC; ++v) {
            F f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) f[e] = from_f32<T>(relu ? fmaxf(acc[v * VEC + e], 0.f) : acc[v * VEC + e]);
            dst[v] = f;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { win[0][c] = win[1][c]; win[1][c] = win[2][c]; win[2][c] = nxt[c]; }
    }
}
// dW[n][tap] += sum_p dY[p][n] x[p + tap]; db[n] += sum_p dY[p][n].  Workgroup = 3 waves x 64 image columns, wave = tap
// row kh: a thread keeps COUT x 3 partial sums in registers while walking image rows (16-byte dY loads, the next row's in
// flight behind this row's FMAs).  All lanes of a wave then hold sums for the SAME weights, so they fold with wave shuffles;
// one lane per wave adds to LDS, one global fp32 atomic per weight per workgroup.
template <typename T, int COUT>
__global__ __launch_bounds__(192) void conv1_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ dw, float* __restrict__ db, int B, int H, int Wd) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = Frag<T>::N, NV = COUT / VEC;
    __shared__ float red[COUT * 10];
    for (int i = threadIdx.x; i < COUT * 10; i += blockDim.x) red[i] = 0.f;
    __syncthreads();
    const int kh = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x * 64 + lane;
    float acc[3][COUT], accb[COUT];
#pragma unroll
    for (int n = 0; n < COUT; ++n) { acc[0][n] = acc[1][n] = acc[2][n] = 0.f; accb[n] = 0.f; }
    if (j < Wd) {
        const int rows = B * H;
        // Loads are unconditional (row clamped by the caller, out-of-image tap rows read a valid row and are zeroed by a
        // factor): a load behind a branch makes the compiler's vmcnt bookkeeping pessimistic and the ring collapses into
        // one round trip per row.
        auto load = [&](int row, float (&xv)[3], F (&gv)[NV]) {
            const int i = row % H;
            const int yy = i + kh - 1;
            const bool ok = yy >= 0 && yy < H;
            const float m = ok ? 1.f : 0.f;
            const T* xr = x + (long)(ok ? row + kh - 1 : row) * Wd;
            const int jl = j > 0 ? j - 1 : j, jr = j + 1 < Wd ? j + 1 : j;
            const T xl = xr[jl], xc = xr[j], xrr = xr[jr];          // three unconditional loads; the image border is a factor
            xv[0] = to_f32(xl) * (j > 0 ? m : 0.f);
            xv[1] = to_f32(xc) * m;
            xv[2] = to_f32(xrr) * (j + 1 < Wd ? m : 0.f);
            const F* gp = reinterpret_cast<const F*>(dy + ((long)row * Wd + j) * COUT);
#pragma unroll
            for (int v = 0; v < NV; ++v) gv[v] = gp[v];
        };
        // ring of PD rows in flight per lane (one row = 32 bytes of dy per lane: a single row ahead leaves the kernel waiting
        // on HBM latency at 1.4 TB/s)
        constexpr int PD = 4;
        float xq[PD][3];
        F gq[PD][NV];
#pragma unroll
        for (int d = 0; d < PD; ++d) {
            xq[d][0] = xq[d][1] = xq[d][2] = 0.f;
#pragma unroll
            for (int v = 0; v < NV; ++v) gq[d][v] = frag_zero<T>();
            load(min((int)(blockIdx.y + d * gridDim.y), rows - 1), xq[d], gq[d]);
        }
        for (int row0 = blockIdx.y; row0 < rows; row0 += PD * gridDim.y) {
#pragma unroll
            for (int d = 0; d < PD; ++d) {
                const int row = row0 + d * gridDim.y;
                if (row >= rows) break;
                float xv[3] = {xq[d][0], xq[d][1], xq[d][2]};
                F gv[NV];
#pragma unroll
                for (int v = 0; v < NV; ++v) gv[v] = gq[d][v];
                load(min(row + PD * (int)gridDim.y, rows - 1), xq[d], gq[d]);       // refill this slot: PD rows stay in flight behind the FMAs
#pragma unroll
                for (int v = 0; v < NV; ++v) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const float g = to_f32(gv[v][e]);
                        const int n = v * VEC + e;
                        acc[0][n] += g * xv[0]; acc[1][n] += g * xv[1]; acc[2][n] += g * xv[2];
                        if (kh == 1) accb[n] += g;
                    }
                }
            }
        }
    }
    // columns beyond the image hold zeros: every lane takes part in the wave reductions
#pragma unroll
    for (int n = 0; n < COUT; ++n) {
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const float v = wave_sum(acc[kw][n]);
            if (lane == 0) red[n * 9 + kh * 3 + kw] = v;        // (n, kh, kw) has exactly one writer
        }
        if (kh == 1) {
            const float v = wave_sum(accb[n]);
            if (lane == 0) red[COUT * 9 + n] = v;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < COUT * 9; i += blockDim.x) atomicAdd(&dw[i], red[i]);
    if (db) for (int i = threadIdx.x; i < COUT; i += blockDim.x) atomicAdd(&db[i], red[COUT * 9 + i]);
}

// The same weight gradient on the MFMA (bf16, 16 output channels: the benchmark's first layer; the last kernel of a backward pass, so
// its whole duration sits in front of the optimizer):  D[n][tap] += dY^T[n][pixels] . P[pixels][tap]  with K = 16 consecutive pixels of
// an image row per MFMA, P the im2col of the 1-channel image -- column `tap` of P is the image row shifted by the tap, so a lane's
// fragment (8 consecutive pixels of one tap) is one aligned 16-byte read from one of THREE copies of the image halo tile kept in LDS,
// pre-shifted by 0 / 1 / 2 pixels.  Column 9 of P is all ones: D[n][9] is the bias gradient.  dY^T comes out of the pixel-major dY
// tile with ds_read_b64_tr_b16 (lanes 16-31 of a half repeat lanes 0-15: rows 16-31 of D are a copy nobody stores).
// Workgroup = 4 waves on a tile of 8 rows x 32 pixels (a wave: two rows = four MFMAs); persistent over the tiles of its share; LDS is
// 10 KB, so a CU holds many workgroups and their load -> LDS -> MFMA phases overlap without a software pipeline.
typedef __attribute__((address_space(3))) bf16x4 C1LdsV4;
__global__ __launch_bounds__(256) void conv1_wgrad_mfma_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy, float* __restrict__ dw,
                                                                float* __restrict__ db, int B, int H, int Wd, int tiles_h, int tiles_w) {
    constexpr int TH1 = 8, TW1 = 32, IH1 = TH1 + 2, XP = 40;               // XP: row pitch of the shifted image copies (elements; 80 B)
    __shared__ __attribute__((aligned(16))) bf16 Ys[TH1 * TW1 * 16];        // dY tile, pixel-major 32-byte rows, chunk index ^ (col >> 3) & 1
    __shared__ __attribute__((aligned(16))) bf16 Xs[3][IH1][XP];            // Xs[s][r][c] = image(tile row r - 1, tile col c - 1 + s), zero outside
    __shared__ float red[4][16][10];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = (lane & 15) >> 2, p = lane & 3, hh = lane >> 5, ntap = lane & 31;
    const int kh = ntap / 3, kw = ntap - 3 * kh;                             // valid for ntap < 9
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const bf16x8 ones = {(bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f};
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const int ntiles = B * tiles_h * tiles_w;
    // global -> registers: two 16-byte dY chunks per thread (pixel tid / 2 + 128 j, chunk tid % 2) and up to four image halo values; the
    // next tile's loads are issued before the current tile's MFMAs
    bf16x8 gv[2];
    bf16 xv[4];
    auto load_tile = [&](int tile) {
        const int b = tile / (tiles_h * tiles_w), rem = tile - b * tiles_h * tiles_w;
        const int th = rem / tiles_w, tw = rem - th * tiles_w, oh0 = th * TH1, ow0 = tw * TW1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int pix = (tid >> 1) + 128 * j, oh = oh0 + (pix >> 5), ow = ow0 + (pix & 31);
            gv[j] = zero8;
            if (oh < H && ow < Wd) gv[j] = *reinterpret_cast<const bf16x8*>(dy + (((long)b * H + oh) * Wd + ow) * 16 + (tid & 1) * 8);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {                  // shifted copies: 3 x 10 x 32 = 960 values
            const int e = tid + 256 * j, sft = e / (IH1 * TW1), r = (e / TW1) % IH1, c = e % TW1;
            const int ih = oh0 - 1 + r, iw = ow0 - 1 + c + sft;
            xv[j] = (bf16)0.f;
            if (e < 3 * IH1 * TW1 && ih >= 0 && ih < H && iw >= 0 && iw < Wd) xv[j] = x[((long)b * H + ih) * Wd + iw];
        }
    };
    if ((int)blockIdx.x < ntiles) load_tile(blockIdx.x);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();                               // the previous tile's MFMAs are done with the LDS tiles
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int pix = (tid >> 1) + 128 * j;
            *reinterpret_cast<bf16x8*>(Ys + pix * 16 + (((tid & 1) ^ ((pix >> 3) & 1)) << 3)) = gv[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = tid + 256 * j, sft = e / (IH1 * TW1), r = (e / TW1) % IH1, c = e % TW1;
            if (e < 3 * IH1 * TW1) Xs[sft][r][c] = xv[j];
        }
        __syncthreads();
        if (tile + (int)gridDim.x < ntiles) load_tile(tile + gridDim.x);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int row = wave * 2 + (s4 >> 1), col0 = (s4 & 1) * 16;
            // A: dY^T, lane (q, p, hh) addresses pixel col0 + 8 hh + q (+4), channels 4 p .. 4 p + 3 (both 16-lane groups of a half the same)
            const int pa = row * TW1 + col0 + 8 * hh + q;
            const int offa = pa * 16 + ((((p >> 1) ^ (((pa & 31) >> 3) & 1)) << 3) | ((p & 1) << 2));
            const int pb = pa + 4;
            const int offb = pb * 16 + ((((p >> 1) ^ (((pb & 31) >> 3) & 1)) << 3) | ((p & 1) << 2));
            const bf16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((C1LdsV4*)(Ys + offa));
            const bf16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((C1LdsV4*)(Ys + offb));
            const bf16x8 af = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
            // B: column ntap of the im2col: pixels (row + kh - 1, col0 + 8 hh + 0..7 + kw - 1) = copy kw, tile row row + kh, columns col0 + 8 hh ..
            bf16x8 bfr = ntap == 9 ? ones : zero8;
            if (ntap < 9) bfr = *reinterpret_cast<const bf16x8*>(&Xs[kw][row + kh][col0 + 8 * hh]);
            mma32(acc, af, bfr);
        }
    }
    // D[n][tap]: column = lane & 31 = tap, row(reg) = channel; fold the four waves through LDS, one atomic per value per workgroup
    if (ntap < 10) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = acc_row(r, lane);
            if (n < 16) red[wave][n][ntap] = acc[r];
        }
    }
    __syncthreads();
    if (tid < 160) {
        const int n = tid / 10, t = tid - n * 10;
        const float v = red[0][n][t] + red[1][n][t] + red[2][n][t] + red[3][n][t];
        if (t < 9) atomicAdd(&dw[n * 9 + t], v);
        else if (db) atomicAdd(&db[n], v);
    }
}

}  // namespace

int omr_conv1_fwd(int dtype, const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int COUT, int relu, hipStream_t s) {
    const int RC = 32;                                   // rows per workgroup: 2 halo rows per 32 re-read
    dim3 g1(cdiv(W, 256), B * cdiv(H, RC));
    DISPATCH_T(dtype, {
        if (COUT == 16) hipLaunchKernelGGL((conv1_direct_kernel<T, 16>), g1, 256, 0, s, (const T*)x, (const T*)w, bias, (T*)y, B, H, W, relu, RC);
        else if (COUT == 32) hipLaunchKernelGGL((conv1_direct_kernel<T, 32>), g1, 256, 0, s, (const T*)x, (const T*)w, bias, (T*)y, B, H, W, relu, RC);
        else return OMR_ERR_UNSUPPORTED;
    });
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

int omr_conv1_wgrad(int dtype, const void* x, const void* dy, float* dw, float* db, int B, int H, int W, int COUT, hipStream_t s) {
    if (dtype == OMR_BF16 && COUT == 16 && (((uintptr_t)dy) & 15) == 0) {
        const int th = cdiv(H, 8), tw = cdiv(W, 32);
        long nt = (long)B * th * tw;
        const int nblk = (int)(nt < OMR_NUM_CU * 8 ? nt : OMR_NUM_CU * 8);   // persistent (8 workgroups per CU): each ends with 160 atomics onto the same cache lines
        hipLaunchKernelGGL(conv1_wgrad_mfma_kernel, dim3(nblk), dim3(256), 0, s, (const bf16*)x, (const bf16*)dy, dw, db, B, H, W, th, tw);
        OMR_CHECK_LAUNCH();
        return OMR_OK;
    }
    int gy = B * H; if (gy > 64) gy = 64;      // few, long-lived blocks: each ends with 10 COUT atomics onto the same five cache lines
    dim3 grid(cdiv(W, 64), gy);
    DISPATCH_T(dtype, {
        if (COUT == 16) hipLaunchKernelGGL((conv1_wgrad_kernel<T, 16>), grid, 192, 0, s, (const T*)x, (const T*)dy, dw, db, B, H, W);
        else if (COUT == 32) hipLaunchKernelGGL((conv1_wgrad_kernel<T, 32>), grid, 192, 0, s, (const T*)x, (const T*)dy, dw, db, B, H, W);
        else return OMR_ERR_UNSUPPORTED;
    });
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}
