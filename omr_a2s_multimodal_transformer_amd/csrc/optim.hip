// The optimizer step (gfx950): global gradient norm, clip factor and the apply / skip decision on the device, and the one Adam
// kernel -- AdamW decay, EMA and the guard's record all optional -- behind omr_adam, omr_adam_guarded and omr_adamw_ema.  The host
// never waits for the decision: it is a record in device memory (omr_step_ctl, omr_hip.h) that the step kernel reads in stream
// order and the host copies back one step late (params.FusedAdam).
//
// The norm is a two-stage slot reduction like the InstanceNorm statistics (norm.hip): no atomics, a fixed order at every level, a
// chunk size that is a compile-time constant -- the bits do not depend on the CU count or on the run.
//   stage 1  one workgroup per slot (GN_CHUNK = 256 threads x GN_K elements of ONE range): 16-byte loads, each thread adds its GN_K
//            squares in fp32 in load order, the workgroup combines the 256 partial sums in fp64 by a halving tree and writes
//            (sum of squares, number of inf / NaN elements) to its own slot.
//   stage 2  one workgroup: thread r adds range r's slots in index order (fp64); thread 0 adds the ranges in index order and fills
//            the record.
#include <limits.h>

#include "omr_common.h"
#include "omr_hip.h"

namespace {

constexpr int GN_BLOCK = 256;
constexpr int GN_K = OMR_GRAD_NORM_K;                  // elements per thread
constexpr int GN_CHUNK = OMR_GRAD_NORM_CHUNK;          // elements per slot
constexpr int GN_VECS = GN_K / 4;                      // 16-byte loads per thread
constexpr int GN_TILE = 1024;                          // slots staged in LDS per round of stage 2
constexpr int GN_MAXR = OMR_GRAD_NORM_MAX_RANGES;
static_assert(GN_CHUNK == GN_BLOCK * GN_K && GN_K % 4 == 0, "slot = one workgroup's threads x K elements");

struct GnSlot { double sumsq; long long bad; };        // 16 bytes
struct GnRanges {                                      // by value in the kernel arguments
    long begin[GN_MAXR], end[GN_MAXR];
    int slot0[GN_MAXR + 1];                            // range r owns slots [slot0[r], slot0[r + 1])
    int n_ranges;
};

__device__ __forceinline__ int is_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(GN_BLOCK) void grad_norm_slots_kernel(const float* __restrict__ g, GnRanges rg, GnSlot* __restrict__ ws) {
    __shared__ double ssum[GN_BLOCK];
    __shared__ int sbad[GN_BLOCK];
    const int slot = blockIdx.x, tid = threadIdx.x;
    int r = 0;
    while (r + 1 < rg.n_ranges && slot >= rg.slot0[r + 1]) ++r;          // uniform: scalar compares
    long rb = rg.begin[0], re = rg.end[0];
    int s0 = rg.slot0[0];
#pragma unroll
    for (int k = 1; k < GN_MAXR; ++k)                                    // static indices: the argument struct stays in SGPRs
        if (k == r) { rb = rg.begin[k]; re = rg.end[k]; s0 = rg.slot0[k]; }
    const long base = rb + (long)(slot - s0) * GN_CHUNK;                 // a multiple of 4: g + base is 16-byte aligned
    f32x4 x[GN_VECS];
#pragma unroll
    for (int j = 0; j < GN_VECS; ++j) {
        const long e = base + 4l * (j * GN_BLOCK + tid);
        if (e + 4 <= re) {
            x[j] = *reinterpret_cast<const f32x4*>(g + e);
        } else {                                                         // the range's last vector: nothing at or past `re` is read
#pragma unroll
            for (int c = 0; c < 4; ++c) x[j][c] = e + c < re ? g[e + c] : 0.f;
        }
    }
    float acc = 0.f;
    int bad = 0;
#pragma unroll
    for (int j = 0; j < GN_VECS; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) { acc += x[j][c] * x[j][c]; bad += is_nonfinite(x[j][c]); }
    ssum[tid] = (double)acc;
    sbad[tid] = bad;
    __syncthreads();
    for (int o = GN_BLOCK / 2; o > 0; o >>= 1) {
        if (tid < o) { ssum[tid] += ssum[tid + o]; sbad[tid] += sbad[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) { GnSlot s; s.sumsq = ssum[0]; s.bad = sbad[0]; ws[slot] = s; }
}

__global__ __launch_bounds__(GN_BLOCK) void grad_norm_finish_kernel(const GnSlot* __restrict__ ws, GnRanges rg, float grad_scale, float max_norm,
                                                                   omr_step_ctl* __restrict__ ctl) {
    __shared__ GnSlot tile[GN_TILE];
    __shared__ double rsum[GN_MAXR];
    __shared__ long long rbad[GN_MAXR];
    __shared__ int s0[GN_MAXR + 1];
    const int tid = threadIdx.x, nr = rg.n_ranges;
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k <= GN_MAXR; ++k) s0[k] = rg.slot0[k];          // static indices: the argument struct stays in SGPRs
    }
    __syncthreads();
    const int total = s0[nr];
    const int lo = tid < nr ? s0[tid] : 0, hi = tid < nr ? s0[tid + 1] : 0;
    double acc = 0.0;
    long long bad = 0;
    for (int t0 = 0; t0 < total; t0 += GN_TILE) {
        for (int i = tid; i < GN_TILE && t0 + i < total; i += GN_BLOCK) tile[i] = ws[t0 + i];
        __syncthreads();
        const int a = lo > t0 ? lo : t0, b = hi < t0 + GN_TILE ? hi : t0 + GN_TILE;
#pragma unroll 8
        for (int k = a; k < b; ++k) { acc += tile[k - t0].sumsq; bad += tile[k - t0].bad; }      // index order
        __syncthreads();
    }
    if (tid < GN_MAXR) { rsum[tid] = acc; rbad[tid] = bad; }             // threads >= nr hold zeros
    __syncthreads();
    if (tid == 0) {
        double sumsq = 0.0;
        long long nbad = 0;
        for (int r = 0; r < GN_MAXR; ++r) {
            ctl->range_sumsq[r] = rsum[r];
            if (r < nr) { sumsq += rsum[r]; nbad += rbad[r]; }
        }
        const float norm = (float)(sqrt(sumsq) * (double)grad_scale);
        float clip = 1.0f;
        if (max_norm > 0.f && !is_nonfinite(max_norm)) clip = fminf(1.0f, max_norm / (norm + 1e-6f));
        ctl->sumsq = sumsq;
        ctl->norm = norm;
        ctl->clip = clip;
        ctl->apply = (nbad == 0 && !(sumsq != sumsq) && sumsq <= 1.7976931348623157e308) ? 1 : 0;
        ctl->nonfinite = nbad > (long long)INT_MAX ? INT_MAX : (int)nbad;
    }
}

// ---------------------------------------------------------------- the optimizer step (omr_adam, omr_adam_guarded, omr_adamw_ema)
// ONE kernel behind the three entries.  torch optim/adam.py:347 single-tensor math (model.py:134-139: lr 1e-4, betas (0.9,0.999),
// eps 1e-8):
//   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// wrapped in two more fused steps (torch optim/adamw.py single-tensor math; optim/swa_utils.py get_ema_multi_avg_fn):
//   before:  p' = p * f, f = (float)(1 - lr wd) from the host, only where the element decays
//   after:   ema = fma(d, ema, (1-d) p_new), d = (float)decay and omd = (float)(1 - decay) from the host.  d = 0: omd = 1,
//            fma(0, ema, p) = p's bits (a finite ema); d = 1: omd = 0, fma(1, ema, 0 * p) = ema's bits (a finite p).
// The gradient the update sees is gi = (g * gscale) * clip, clip = the guard's record's or 1.0f.
//
// The library is built with -ffp-contract=fast, under which two copies of `a * b + c` -- or one copy inlined into two places --
// are not guaranteed to contract into the same fma chain (moving the expression into a function once did change the chain of the
// scalar kernel omr_adam had then).  So every multiply-add is spelled out as the fma omr_adam has always executed:
//   m = fma(b1, m, (1-b1) g)   v = fma(b2, v, ((1-b2) g) g)   denom = fma(sqrt(v), 1/sqrt(bc2), eps)   p = fma(-lr/bc1, m / denom, p)
// No fmul -> fadd pair is left for the contraction pass: a product only ever feeds an explicit fma, so the vector body and the
// scalar tail execute these roundings, whatever surrounds the call.
//
// A pure streaming kernel: 16-byte loads and stores, four elements per thread per trip (g, p, m, v [, ema] in; p, m, v [, ema]
// and 8 bytes of bf16 out), a grid-stride loop, no LDS, no atomics; the last n % 4 elements take the same update one at a time.
// decay_blocks: one byte per AW_BLOCK_ELEMS elements, relative to p; a thread's four elements share a byte.
// A block that does not decay takes p' = p through a select -- no multiply touches it.
constexpr int AW_THREADS = 256;
constexpr int AW_MAX_GRID = 2048;                      // 256 CUs x 8 workgroups
constexpr int AW_BLOCK_ELEMS = OMR_ADAM_DECAY_BLOCK;   // elements per decay byte
constexpr int AW_BLOCK_SHIFT = __builtin_ctz(AW_BLOCK_ELEMS);
static_assert((AW_BLOCK_ELEMS & (AW_BLOCK_ELEMS - 1)) == 0 && AW_BLOCK_ELEMS % 4 == 0, "a power of two, and a 16-byte vector never straddles a block");

struct AwArgs {                                        // by value in the kernel arguments
    float lr_over_bc1, b1, b2, eps, inv_sqrt_bc2, gscale;
    float decay_f;                                     // (float)(1 - lr wd)
    float ema_d, ema_omd;                              // (float)d, (float)(1 - d)
};

// The per-element sequence on registers, written once for the vector body and the scalar tail.  -> the bf16 copy of the new p.
template <bool DECAY, bool EMA>
__device__ __forceinline__ bf16 adam_update(float& pi, float& mi, float& vi, float& ei, float g, bool dec, float clip, const AwArgs& a) {
    const float gi = (g * a.gscale) * clip;
    if (DECAY) pi = dec ? pi * a.decay_f : pi;
    mi = __builtin_fmaf(a.b1, mi, (1.f - a.b1) * gi);
    vi = __builtin_fmaf(a.b2, vi, ((1.f - a.b2) * gi) * gi);
    const float denom = __builtin_fmaf(sqrtf(vi), a.inv_sqrt_bc2, a.eps);
    pi = __builtin_fmaf(-a.lr_over_bc1, mi / denom, pi);
    if (EMA) ei = __builtin_fmaf(a.ema_d, ei, a.ema_omd * pi);
    return (bf16)pi;
}

template <bool DECAY, bool EMA>
__global__ __launch_bounds__(AW_THREADS) void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, bf16* __restrict__ p_lp, float* __restrict__ ema,
                                                              const unsigned char* __restrict__ decay_blocks, long n, AwArgs a,
                                                              const omr_step_ctl* __restrict__ ctl) {
    float clip = 1.0f;
    if (ctl) {                                                           // uniform loads; a skipped step leaves before any access
        if (ctl->apply == 0) return;
        clip = ctl->clip;
    }
    const long gid = blockIdx.x * (long)AW_THREADS + threadIdx.x, stride = (long)gridDim.x * AW_THREADS;
    const long nvec = n >> 2;
    for (long j = gid; j < nvec; j += stride) {
        const long i = j << 2;
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(g + i);
        f32x4 p4 = *reinterpret_cast<const f32x4*>(p + i);
        f32x4 m4 = *reinterpret_cast<const f32x4*>(m + i);
        f32x4 v4 = *reinterpret_cast<const f32x4*>(v + i);
        f32x4 e4;
        if (EMA) e4 = *reinterpret_cast<const f32x4*>(ema + i);
        bool dec = DECAY;
        if (DECAY && decay_blocks) dec = decay_blocks[i >> AW_BLOCK_SHIFT] != 0;
        bf16x4 lp4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float pi = p4[c], mi = m4[c], vi = v4[c], ei = EMA ? e4[c] : 0.f;
            lp4[c] = adam_update<DECAY, EMA>(pi, mi, vi, ei, g4[c], dec, clip, a);
            p4[c] = pi; m4[c] = mi; v4[c] = vi;
            if (EMA) e4[c] = ei;
        }
        *reinterpret_cast<f32x4*>(p + i) = p4;
        *reinterpret_cast<f32x4*>(m + i) = m4;
        *reinterpret_cast<f32x4*>(v + i) = v4;
        if (EMA) *reinterpret_cast<f32x4*>(ema + i) = e4;
        if (p_lp) *reinterpret_cast<bf16x4*>(p_lp + i) = lp4;
    }
    for (long i = (nvec << 2) + gid; i < n; i += stride) {               // at most three elements, on the grid's first threads
        float pi = p[i], mi = m[i], vi = v[i], ei = EMA ? ema[i] : 0.f;
        const bool dec = DECAY && (!decay_blocks || decay_blocks[i >> AW_BLOCK_SHIFT] != 0);
        const bf16 lp = adam_update<DECAY, EMA>(pi, mi, vi, ei, g[i], dec, clip, a);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (p_lp) p_lp[i] = lp;
        if (EMA) ema[i] = ei;
    }
}

__global__ __launch_bounds__(AW_THREADS) void swap_f32_kernel(float* __restrict__ a, float* __restrict__ b, long n) {
    const long gid = blockIdx.x * (long)AW_THREADS + threadIdx.x, stride = (long)gridDim.x * AW_THREADS;
    const long nvec = n >> 2;
    for (long j = gid; j < nvec; j += stride) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(a + (j << 2));
        const f32x4 y = *reinterpret_cast<const f32x4*>(b + (j << 2));
        *reinterpret_cast<f32x4*>(a + (j << 2)) = y;
        *reinterpret_cast<f32x4*>(b + (j << 2)) = x;
    }
    for (long i = (nvec << 2) + gid; i < n; i += stride) { const float x = a[i]; a[i] = b[i]; b[i] = x; }
}

inline int aw_grid(long n) {
    const long blocks = ((n >> 2) + AW_THREADS - 1) / AW_THREADS;
    return (int)(blocks < 1 ? 1 : (blocks > AW_MAX_GRID ? AW_MAX_GRID : blocks));
}

inline long gn_slots(long len) { return (len + GN_CHUNK - 1) / GN_CHUNK; }

}  // namespace

// The one launch behind the three entries: checks, fp64 bias corrections, instance by what is asked for.
static int adam_launch(float* p, const float* g, float* m, float* v, void* p_bf16, float* ema, const unsigned char* decay_blocks, long n,
                       int step, float lr, float b1, float b2, float eps, float weight_decay, float ema_decay, float grad_scale,
                       const omr_step_ctl* ctl, void* stream) {
    if (n <= 0) return OMR_OK;
    if (step < 1 || !p || !g || !m || !v) return OMR_ERR_ARG;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)p_bf16 | (uintptr_t)ema) & 15) || ((uintptr_t)ctl & 7))
        return OMR_ERR_ARG;
    if (ema && !(ema_decay >= 0.f && ema_decay <= 1.f)) return OMR_ERR_ARG;
    const double bc1 = 1.0 - pow((double)b1, step), bc2 = 1.0 - pow((double)b2, step);
    AwArgs a;
    a.lr_over_bc1 = (float)(lr / bc1); a.b1 = b1; a.b2 = b2; a.eps = eps; a.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2)); a.gscale = grad_scale;
    a.decay_f = (float)(1.0 - (double)lr * (double)weight_decay);
    a.ema_d = ema_decay; a.ema_omd = (float)(1.0 - (double)ema_decay);
    const bool decay = weight_decay != 0.f;
    hipStream_t s = (hipStream_t)stream;
    const int grid = aw_grid(n);
#define AW_LAUNCH(D, E)                                                                                                          \
    hipLaunchKernelGGL((adamw_ema_kernel<D, E>), grid, AW_THREADS, 0, s, p, g, m, v, (bf16*)p_bf16, ema, decay_blocks, n, a, ctl)
    if (decay && ema) AW_LAUNCH(true, true);
    else if (decay) AW_LAUNCH(true, false);
    else if (ema) AW_LAUNCH(false, true);
    else AW_LAUNCH(false, false);
#undef AW_LAUNCH
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_adamw_ema(float* p, const float* g, float* m, float* v, void* p_bf16, float* ema, const unsigned char* decay_blocks, long n,
                             int step, float lr, float b1, float b2, float eps, float weight_decay, float ema_decay, float grad_scale,
                             const omr_step_ctl* ctl, void* stream) {
    return adam_launch(p, g, m, v, p_bf16, ema, decay_blocks, n, step, lr, b1, b2, eps, weight_decay, ema_decay, grad_scale, ctl, stream);
}

extern "C" int omr_adam(float* p, const float* g, float* m, float* v, void* p_bf16, long n, int step, float lr, float b1, float b2,
                        float eps, float grad_scale, void* stream) {
    return adam_launch(p, g, m, v, p_bf16, nullptr, nullptr, n, step, lr, b1, b2, eps, 0.f, 0.f, grad_scale, nullptr, stream);
}

extern "C" int omr_adam_guarded(float* p, const float* g, float* m, float* v, void* p_bf16, long n, int step, float lr, float b1, float b2,
                                float eps, float grad_scale, const omr_step_ctl* ctl, void* stream) {
    if (n > 0 && !ctl) return OMR_ERR_ARG;
    return adam_launch(p, g, m, v, p_bf16, nullptr, nullptr, n, step, lr, b1, b2, eps, 0.f, 0.f, grad_scale, ctl, stream);
}

extern "C" int omr_swap_f32(float* a, float* b, long n, void* stream) {
    if (n <= 0) return OMR_OK;
    if (!a || !b || (((uintptr_t)a | (uintptr_t)b) & 15)) return OMR_ERR_ARG;
    if (a < b + n && b < a + n) return OMR_ERR_ARG;                      // overlap (a == b included)
    hipLaunchKernelGGL(swap_f32_kernel, aw_grid(n), AW_THREADS, 0, (hipStream_t)stream, a, b, n);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" long omr_grad_norm_workspace_bytes(long n, int n_ranges) {
    if (n < 1 || n_ranges < 1 || n_ranges > GN_MAXR) return OMR_ERR_ARG;
    return (n / GN_CHUNK + n_ranges) * (long)sizeof(GnSlot);            // sum over ranges of ceil(len / CHUNK) <= n / CHUNK + n_ranges
}

extern "C" int omr_grad_norm(const float* g, long n, const long* range_begin, const long* range_end, int n_ranges, float grad_scale,
                             float max_norm, void* ws, omr_step_ctl* ctl, void* stream) {
    if (!g || !ws || !ctl || !range_begin || !range_end || n < 1 || n_ranges < 1 || n_ranges > GN_MAXR) return OMR_ERR_ARG;
    if (((uintptr_t)g & 15) || ((uintptr_t)ws & 15) || ((uintptr_t)ctl & 7)) return OMR_ERR_ARG;
    GnRanges rg = {};
    rg.n_ranges = n_ranges;
    long prev_end = 0, slots = 0;
    for (int r = 0; r < n_ranges; ++r) {
        const long b = range_begin[r], e = range_end[r];
        if (b < prev_end || e <= b || e > n || (b & 3)) return OMR_ERR_ARG;
        rg.begin[r] = b; rg.end[r] = e; rg.slot0[r] = (int)slots;
        slots += gn_slots(e - b);
        prev_end = e;
    }
    if (slots > INT_MAX) return OMR_ERR_UNSUPPORTED;
    rg.slot0[n_ranges] = (int)slots;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(grad_norm_slots_kernel, (int)slots, GN_BLOCK, 0, s, g, rg, (GnSlot*)ws);
    hipLaunchKernelGGL(grad_norm_finish_kernel, 1, GN_BLOCK, 0, s, (const GnSlot*)ws, rg, grad_scale, max_norm, ctl);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}
