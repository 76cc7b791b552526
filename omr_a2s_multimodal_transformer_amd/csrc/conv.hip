// Convolution kernels for the CNN encoder (reference: src/transformer/encoder.py) on gfx950.
// Activations are NHWC ([B][H][W][C], channel fastest) so that
//   * the 3x3 convs are nine shifted [pixels x Cin] . [Cin x Cout] MFMA GEMMs fed from ONE LDS halo tile,
//   * DepthSepConv2D's 1x1 point_conv is a plain GEMM (gemm.hip) and
//   * the encoder output IS the decoder memory [B, S, C] (model.py:147 flatten+permute) with no copy.
// Weights are [Cout][3][3][Cin] (= torch channels_last storage of the reference's [Cout,Cin,3,3] tensor).
//
//   conv3x3_mfma     forward (stride s, pad 1, optional fused InstanceNorm-apply on the input, bias, ReLU) and,
//                    with flipped/transposed weights + input dilation, the data gradient (transposed conv).
//   conv3x3_wgrad    dW[n][tap][c] += sum_pix dY[pix][n] X[pix+tap][c]  (MFMA, K = pixels, fp32 atomics)
// The 1 -> 16 first layer (K = 9) lives in conv1.hip, the depthwise 3x3 family in dwconv.hip, the bf16 LDS-DMA weight gradient
// in conv_wgrad_dma.hip and the fused backward in conv_bwd_fused.hip.
#include <type_traits>

#include "omr_common.h"
#include "omr_hip.h"

#include "conv3x3_mfma.h"
#include "conv_wgrad.h"
#include "conv1.h"

using omr_conv::ConvArgs;
using omr_conv::TW;
int omr_conv3x3_dispatch_bf16(const ConvArgs& a, hipStream_t s);
int omr_conv3x3_dispatch_f32(const ConvArgs& a, hipStream_t s);

namespace {

// ------------------------------------------------------------------------------------------------
// Weight re-layout for the data gradient: Wd[c][8 - tap][n] = W[n][tap][c]   (transposed conv = conv with
// flipped taps and swapped channel roles), for SEVERAL convs in one launch (blockIdx.y = conv): the flipped copies of all 3x3
// weights of a model are refreshed once per optimizer step, right behind omr_adam, instead of one launch in front of every data
// gradient of the backward pass.
constexpr int FLIP_MAX = 32;
struct FlipTable { const void* w[FLIP_MAX]; void* wd[FLIP_MAX]; int cout[FLIP_MAX]; int cin[FLIP_MAX]; };
template <typename T>
__global__ void weight_flip_grouped_kernel(FlipTable t) {
    const int g = blockIdx.y, COUT = t.cout[g], CIN = t.cin[g];
    const T* __restrict__ w = (const T*)t.w[g];
    T* __restrict__ wd = (T*)t.wd[g];
    const long total = (long)COUT * 9 * CIN;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int n = (int)(i % COUT); long q = i / COUT; int tapd = (int)(q % 9); int c = (int)(q / 9);
        wd[i] = w[((long)n * 9 + (8 - tapd)) * CIN + c];
    }
}

// ------------------------------------------------------------------------------------------------
// Weight gradient of the 3x3 conv.  Workgroup = 2x2 waves; wave (wn, wc) owns the 32 couts x 32 cins
// block (n0 + 32 wn, c0 + 32 wc) for all nine taps (9 x 16 accumulator registers).  K = output pixels:
// the block walks pixel tiles (grid-stride), stages dY[pix][64 n] and the X halo [pix][64 c] in LDS
// and reads k-strided operand fragments element-wise (dtype generic; bf16 tr-reads are a later step).
template <typename T, int TH, int CBN, int CBC, int SH, int SW>
__global__ __launch_bounds__(256) void conv3x3_wgrad_kernel(WgradArgs a) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = Frag<T>::N;
    constexpr int WN = CBN / 32, WC = CBC / 32, WK = 4 / (WN * WC);   // waves over couts, cins and pixel slices
    constexpr bool TR = std::is_same<T, bf16>::value;       // bf16: transposing LDS reads; fp32: element gathers
    // LDS pitches (elements).  tr path: 4 consecutive pixel rows x 16 dwords must tile the 64 banks -> 64 B rows for 32
    // channels, 192 B rows for 64 channels (conflict-free for unit pixel stride); scalar path: odd dword pitch.
    constexpr int NP = TR ? CBN + 8 : CBN + 4, CP = TR ? CBC + 8 : CBC + 4;   // +16 B: conflict-free 16-byte staging stores, 2-way at worst on the tr reads
    typedef __attribute__((address_space(3))) bf16x4 LdsV4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int IH = (TH - 1) * SH + 3, IW = (TW - 1) * SW + 3, NPIX = IH * IW;   // compile-time tile geometry
    T* Ys = reinterpret_cast<T*>(smem_raw);            // [TH*TW][NP]
    T* Xs = Ys + (long)TH * TW * NP;                   // [IH*IW][CP]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wk = wave / (WN * WC), wn = (wave % (WN * WC)) / WC, wc = wave % WC;
    const int ncb = cdiv(a.CIN, CBC);
    const int n0 = (blockIdx.y / ncb) * CBN, c0 = (blockIdx.y % ncb) * CBC;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const int ntiles = a.B * a.tiles_h * a.tiles_w;
    const bool do_bias = a.db != nullptr && (blockIdx.y % ncb) == 0;   // one cin-block column of the grid owns the bias sums
    float bsum = 0.f;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = tile / (a.tiles_h * a.tiles_w);
        const int rem = tile % (a.tiles_h * a.tiles_w);
        const int oh0 = (rem / a.tiles_w) * TH, ow0 = (rem % a.tiles_w) * TW;
        const int ih0 = oh0 * SH - 1, iw0 = ow0 * SW - 1;
        const T* X = (const T*)a.x + (long)b * a.Hr * a.Wr * a.CIN;
        const T* DY = (const T*)a.dy + (long)b * a.Ho * a.Wo * a.COUT;
        __syncthreads();
        // ---- stage dY tile [pix][CBN] and X halo [pix][CBC]: thread = one pixel per round (one bounds test + address for
        //      all of its 16-byte chunks); every load of every round is issued before the first LDS store
        {
            constexpr int CPN = CBN / VEC, CPC = CBC / VEC;
            constexpr int RY = (TH * TW + 255) / 256, RX = (NPIX + 255) / 256;
            F vy[RY][CPN], vx[RX][CPC];
#pragma unroll
            for (int r = 0; r < RY; ++r) {
                const int pix = tid + r * 256;
                const int oh = oh0 + pix / TW, ow = ow0 + pix % TW;
                const bool ok = pix < TH * TW && oh < a.Ho && ow < a.Wo;
                const T* src = DY + ((long)oh * a.Wo + ow) * a.COUT + n0;
#pragma unroll
                for (int k = 0; k < CPN; ++k) {
                    vy[r][k] = frag_zero<T>();
                    if (ok && n0 + k * VEC < a.COUT) vy[r][k] = *reinterpret_cast<const F*>(src + k * VEC);
                }
            }
#pragma unroll
            for (int r = 0; r < RX; ++r) {
                const int pix = tid + r * 256;
                const int il = pix / IW, jl = pix - il * IW;
                const int ih = ih0 + il, iw = iw0 + jl;
                const bool ok = pix < NPIX && ih >= 0 && ih < a.Hr && iw >= 0 && iw < a.Wr;
                const T* src = X + ((long)ih * a.Wr + iw) * a.CIN + c0;
#pragma unroll
                for (int k = 0; k < CPC; ++k) {
                    vx[r][k] = frag_zero<T>();
                    if (ok && c0 + k * VEC < a.CIN) vx[r][k] = *reinterpret_cast<const F*>(src + k * VEC);
                }
                if (ok && a.mean) {
#pragma unroll
                    for (int k = 0; k < CPC; ++k)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            const int ch = c0 + k * VEC + e;
                            if (ch < a.CIN) vx[r][k][e] = from_f32<T>((to_f32(vx[r][k][e]) - a.mean[b * a.CIN + ch]) * a.rstd[b * a.CIN + ch]);
                        }
                }
            }
#pragma unroll
            for (int r = 0; r < RY; ++r) {
                const int pix = tid + r * 256;
                if (pix < TH * TW)
#pragma unroll
                    for (int k = 0; k < CPN; ++k) *reinterpret_cast<F*>(Ys + (long)pix * NP + k * VEC) = vy[r][k];
            }
#pragma unroll
            for (int r = 0; r < RX; ++r) {
                const int pix = tid + r * 256;
                if (pix < NPIX)
#pragma unroll
                    for (int k = 0; k < CPC; ++k) *reinterpret_cast<F*>(Xs + (long)pix * CP + k * VEC) = vx[r][k];
            }
        }
        __syncthreads();
        if (do_bias) {   // bias gradient: column sums of the staged dY tile (thread = channel x pixel phase)
            constexpr int NPH = 256 / CBN;
            const int ch = tid % CBN;
            for (int pix = tid / CBN; pix < TH * TW; pix += NPH) bsum += to_f32(Ys[(long)pix * NP + ch]);
        }
        if constexpr (TR) {
            // bf16: k-major operand fragments straight out of the [pixel][channel] tiles with ds_read_b64_tr_b16.
            // Lane (q, p, cb, h) supplies the address of pixel row q, channels 16cb+4p.. of its 16-lane group's 4x16 block
            // and receives 4 consecutive pixels of channel 16cb + (lane & 15) (verified on hardware, scratch/trtest.hip).
            const int q = (lane & 15) >> 2, chan = ((lane >> 4) & 1) * 16 + (lane & 3) * 4, hh = lane >> 5;
            for (int k0 = wk * 16; k0 < TH * TW; k0 += WK * 16) {
                const int pk = k0 + 8 * hh + q;                // u = 0 block; the u = 1 block is 4 pixels further (same tile row)
                const bf16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LdsV4*)(Ys + (long)pk * NP + wn * 32 + chan));
                const bf16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LdsV4*)(Ys + (long)(pk + 4) * NP + wn * 32 + chan));
                const bf16x8 af = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
                const int r = pk >> 5, col = pk & 31;
                const T* xrow = Xs + (long)((r * SH) * IW + col * SW) * CP + wc * 32 + chan;
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int kh = tap / 3, kw = tap % 3;
                    const T* xp = xrow + (long)(kh * IW + kw) * CP;
                    const bf16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LdsV4*)xp);
                    const bf16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LdsV4*)(xp + (long)4 * SW * CP));
                    const bf16x8 bf = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
                    mma32(acc[tap], af, bf);
                }
            }
        } else {
            const int nl = wn * 32 + (lane & 31), cl = wc * 32 + (lane & 31);
            for (int k0 = wk * KStep<T>::value; k0 < TH * TW; k0 += WK * KStep<T>::value) {
                const int pbase = k0 + (lane >> 5) * VEC;     // VEC consecutive pixels of one tile row
                const int r = pbase / TW, col = pbase % TW;
                F af;
#pragma unroll
                for (int e = 0; e < VEC; ++e) af[e] = Ys[(long)(pbase + e) * NP + nl];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int kh = tap / 3, kw = tap % 3;
                    F bf;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) bf[e] = Xs[(long)((r * SH + kh) * IW + (col + e) * SW + kw) * CP + cl];
                    mma32(acc[tap], af, bf);
                }
            }
        }
    }
    if (do_bias) {   // combine the per-thread partial sums in LDS first: lanes of one wave hitting the same address serialise badly
        float* red = reinterpret_cast<float*>(smem_raw);
        __syncthreads();
        red[tid] = bsum;
        __syncthreads();
        if (tid < CBN) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 256 / CBN; ++k) v += red[k * CBN + tid];
            if (n0 + tid < a.COUT) atomicAdd(&a.db[n0 + tid], v);
        }
    }
    // accumulate: dw[n][tap][c] (fp32 atomics; the grad buffer is zeroed once per step)
    const int c = c0 + wc * 32 + (lane & 31);
    if (c < a.CIN) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wn * 32 + acc_row(r, lane);
                if (n < a.COUT) atomicAdd(&a.dw[((long)n * 9 + tap) * a.CIN + c], acc[tap][r]);
            }
    }
}

template <typename T, int TH, int CBN, int CBC, int SH, int SW> int launch_wgrad3(WgradArgs a, hipStream_t s) {
    a.tiles_w = cdiv(a.Wo, TW);
    a.tiles_h = cdiv(a.Ho, TH);
    constexpr int IH = (TH - 1) * SH + 3, IW = (TW - 1) * SW + 3;
    constexpr bool TR = std::is_same<T, bf16>::value;
    constexpr int NP = TR ? CBN + 8 : CBN + 4, CP = TR ? CBC + 8 : CBC + 4;   // +16 B: conflict-free 16-byte staging stores, 2-way at worst on the tr reads
    size_t shm = ((size_t)TH * TW * NP + (size_t)IH * IW * CP) * sizeof(T);
    if (shm > 160 * 1024) return OMR_ERR_UNSUPPORTED;
    auto kern = conv3x3_wgrad_kernel<T, TH, CBN, CBC, SH, SW>;
    const int gy = cdiv(a.COUT, CBN) * cdiv(a.CIN, CBC);
    const int ntiles = a.B * a.tiles_h * a.tiles_w;
    static std::atomic<int> occ_cache{0};   // resident blocks per CU of this instantiation
    const int occv = omr_launch_setup(occ_cache, (const void*)kern, shm, shm > 48 * 1024, 256, 2);
    if (occv == 0) return OMR_ERR_LAUNCH;
    int gx = (OMR_NUM_CU * occv + gy - 1) / gy; if (gx < 1) gx = 1; if (gx > ntiles) gx = ntiles;
    hipLaunchKernelGGL(kern, dim3(gx, gy), dim3(256), shm, s, a);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

template <typename T, int TH, int SH, int SW> int launch_wgrad2(const WgradArgs& a, hipStream_t s) {
    if (a.COUT > 32 && a.CIN > 32) return launch_wgrad3<T, TH, 64, 64, SH, SW>(a, s);
    if (a.COUT > 32) return launch_wgrad3<T, TH, 64, 32, SH, SW>(a, s);
    return launch_wgrad3<T, TH, 32, 32, SH, SW>(a, s);
}

// TH1: tile rows for stride 1, TH2: for the strided convs (bigger halo)
template <typename T, int TH1, int TH2> int launch_wgrad(const WgradArgs& a, hipStream_t s) {
    if (a.sh == 1 && a.sw == 1) return launch_wgrad2<T, TH1, 1, 1>(a, s);
    if (a.sh == 2 && a.sw == 2) return launch_wgrad2<T, TH2, 2, 2>(a, s);
    if (a.sh == 2 && a.sw == 1) return launch_wgrad2<T, TH2, 2, 1>(a, s);
    return OMR_ERR_UNSUPPORTED;
}

inline int ew_grid(long n) { long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }

}  // namespace

extern "C" int omr_conv3x3_fwd(int dtype, const void* x, const void* w, const float* bias, void* y, const float* in_mean, const float* in_rstd,
                               const void* out_mask, float mask_scale, int B, int H, int W, int CIN, int COUT, int stride_h, int stride_w,
                               int dil_h, int dil_w, int Ho, int Wo, int relu, float drop_p, unsigned long long drop_seed,
                               int drop_channel_mode, int stat_mode, double* stat_ws, int stat_slots, const void* stat_x,
                               const float* stat_mean, const float* stat_rstd, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0 || CIN <= 0 || COUT <= 0 || !x || !w || (!y && stat_mode != 4)) return OMR_ERR_ARG;
    if (stride_h < 1 || stride_w < 1 || dil_h < 1 || dil_w < 1 || dil_h > 2 || dil_w > 2) return OMR_ERR_ARG;
    if ((stride_h > 1 || stride_w > 1) && (dil_h > 1 || dil_w > 1)) return OMR_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (drop_p < 0.f || drop_p >= 1.f || stat_mode < 0 || stat_mode == 3 || stat_mode > 5) return OMR_ERR_ARG;
    if (stat_mode && (!stat_ws || stat_slots < 1)) return OMR_ERR_ARG;
    if (stat_mode >= 2 && (!stat_x || !stat_mean || !stat_rstd)) return OMR_ERR_ARG;
    if (stat_mode >= 4 && (out_mask || bias || drop_p > 0.f)) return OMR_ERR_ARG;      // data-gradient modes: `relu` / mask_scale describe stat_x's ReLU mask
    if (CIN == 1) {
        if (drop_p > 0.f || stat_mode) return OMR_ERR_UNSUPPORTED;
        if (dil_h != 1 || dil_w != 1 || stride_h != 1 || stride_w != 1 || in_mean || out_mask || Ho != H || Wo != W) return OMR_ERR_UNSUPPORTED;
        return omr_conv1_fwd(dtype, x, w, bias, y, B, H, W, COUT, relu, s);
    }
    ConvArgs a;
    a.x = x; a.w = w; a.bias = bias; a.y = y; a.mean = in_mean; a.rstd = in_rstd; a.mask = out_mask; a.mask_scale = mask_scale;
    a.B = B; a.Hr = H; a.Wr = W; a.CIN = CIN; a.Ho = Ho; a.Wo = Wo; a.COUT = COUT;
    a.sh = stride_h; a.sw = stride_w; a.dh = dil_h; a.dw = dil_w; a.relu = relu; a.tiles_w = a.tiles_h = 0;
    a.drop_thresh = OMR_DROP_THRESH16(drop_p); a.drop_scale = 1.f / (1.f - drop_p); a.drop_seed = drop_seed;
    a.drop_channel = drop_channel_mode;
    a.stat_mode = stat_mode; a.stat_ws = stat_ws; a.stat_x = stat_x; a.stat_mean = stat_mean; a.stat_rstd = stat_rstd; a.stat_slots = stat_slots;
    a.stat_relu = 0; a.stat_relu_scale = 1.f;
    if (stat_mode >= 4) { a.stat_relu = relu; a.stat_relu_scale = mask_scale; a.relu = 0; a.mask_scale = 1.f; }
    if (dtype == OMR_BF16) return omr_conv3x3_dispatch_bf16(a, s);
    if (dtype == OMR_F32) return omr_conv3x3_dispatch_f32(a, s);
    return OMR_ERR_UNSUPPORTED;
}

/* upper bound on the blocks per image of the persistent conv grid (<= 8 resident 256-thread blocks per CU on 256 CUs, and
 * never more than the 4-row x 32-column tiles of an image): the slot count of the fused-statistics workspace */
extern "C" int omr_conv3x3_stat_slots(int B, int Ho, int Wo) {
    if (B <= 0 || Ho <= 0 || Wo <= 0) return OMR_ERR_ARG;
    const long tiles = (long)cdiv(Ho, 4) * cdiv(Wo, TW), slots = ((long)OMR_NUM_CU * 8 + B - 1) / B;
    return (int)(tiles < slots ? tiles : slots);
}

extern "C" int omr_conv3x3_weight_flip(int dtype, const void* w, void* wd, int COUT, int CIN, void* stream) {
    if (COUT <= 0 || CIN <= 0) return OMR_ERR_ARG;
    FlipTable t = {};
    t.w[0] = w; t.wd[0] = wd; t.cout[0] = COUT; t.cin[0] = CIN;
    DISPATCH_T(dtype, hipLaunchKernelGGL((weight_flip_grouped_kernel<T>), ew_grid((long)COUT * 9 * CIN), 256, 0, (hipStream_t)stream, t));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_conv3x3_weight_flip_grouped(int dtype, int n, const omr_flip_desc* descs, void* stream) {
    if (n < 0 || (n && !descs)) return OMR_ERR_ARG;
    for (int base = 0; base < n; base += FLIP_MAX) {
        FlipTable t = {};
        const int cnt = n - base < FLIP_MAX ? n - base : FLIP_MAX;
        long most = 0;
        for (int i = 0; i < cnt; ++i) {
            const omr_flip_desc& d = descs[base + i];
            if (!d.w || !d.wd || d.cout <= 0 || d.cin <= 0) return OMR_ERR_ARG;
            t.w[i] = d.w; t.wd[i] = d.wd; t.cout[i] = d.cout; t.cin[i] = d.cin;
            const long total = (long)d.cout * 9 * d.cin;
            if (total > most) most = total;
        }
        const dim3 grid((unsigned)((most + 255) / 256 < 64 ? (most + 255) / 256 : 64), (unsigned)cnt);
        DISPATCH_T(dtype, hipLaunchKernelGGL((weight_flip_grouped_kernel<T>), grid, 256, 0, (hipStream_t)stream, t));
    }
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_conv3x3_wgrad(int dtype, const void* x, const void* dy, float* dw, float* db, const float* in_mean, const float* in_rstd, int B, int H,
                                 int W, int CIN, int COUT, int stride_h, int stride_w, int Ho, int Wo, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0 || CIN <= 0 || COUT <= 0 || !x || !dy || !dw) return OMR_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (CIN == 1) {
        if (stride_h != 1 || stride_w != 1 || in_mean) return OMR_ERR_UNSUPPORTED;
        return omr_conv1_wgrad(dtype, x, dy, dw, db, B, H, W, COUT, s);
    }
    const int vec = dtype == OMR_BF16 ? 8 : 4;
    if (CIN % vec || COUT % vec) return OMR_ERR_UNSUPPORTED;
    WgradArgs a;
    a.x = x; a.dy = dy; a.dw = dw; a.db = db; a.mean = in_mean; a.rstd = in_rstd; a.B = B; a.Hr = H; a.Wr = W; a.CIN = CIN; a.Ho = Ho; a.Wo = Wo;
    a.COUT = COUT; a.sh = stride_h; a.sw = stride_w; a.tiles_w = a.tiles_h = 0;
    if (dtype == OMR_BF16) {
        const int rc = omr_wgrad_dma_bf16(a, s);            // asynchronous-staging kernel (conv_wgrad_dma.hip) where it covers the shape
        if (rc != OMR_ERR_UNSUPPORTED) return rc;
        return launch_wgrad<bf16, 8, 4>(a, s);
    }
    if (dtype == OMR_F32) return launch_wgrad<float, 4, 2>(a, s);
    return OMR_ERR_UNSUPPORTED;
}

