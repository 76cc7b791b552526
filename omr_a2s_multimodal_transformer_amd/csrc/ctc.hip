// CTC auxiliary head (gfx950): encoder memory -> time-ordered frames, the CTC loss and its gradient on the head's logits, and the greedy
// (best-path) transcript.  An extension: the reference trains the encoder through the decoder's cross-attention alone.  Semantics are
// F.ctc_loss(log_softmax(logits), ..., blank, reduction="mean", zero_infinity=True); include/omr_hip.h states every entry.
//
// Lattice.  A sample with labels l_0 .. l_{L-1} has the states 0 .. 2L: state 2j is the blank in front of label j (2L: behind the last),
// state 2j + 1 is label j.  log alpha[t][s] includes the emission of frame t, as torch's does.  log beta is the same recursion on the
// reversed labels over the reversed frames (beta[t][s] = alpha'[F - 1 - t][2L - s]), so ONE sweep body serves both: workgroup (b, 0) runs
// it forwards, (b, 1) backwards, and both store their values under the frame t they belong to, in their own state order.
//
// Sweep.  Thread j owns the blank state 2j and the label state 2j + 1; per frame
//     a0' = e_blank + lse2(a0, left)        a1' = e_label + lse3(a1, a0, left if l_j != l_{j-1})        left = a1 of thread j - 1,
// which comes by a wave shuffle, and for lane 0 of a wave from a double-buffered LDS row that lane 63 of the wave before wrote in front
// of the frame's one barrier.  The emissions of the NEXT 8 frames are loaded (raw logit, blank logit, frame lse) into registers while the
// current 8 are computed; the barrier waits for LDS only, so those loads stay in flight across it.
// Offsets.  Every 8th frame (and the last) the workgroup's maximum m is taken out of all states and added to an fp64 offset: stored
// values stay within 8 frames' drift of 0 whatever F is, and log alpha[t][s] = offset[t] + stored[t][s].  expf / logf / log1pf are the
// accurate ones here; the fast intrinsics serve the V-wide softmax of the gradient only.
// Gradient.  One workgroup per frame writes s (softmax) over all columns, then takes the posterior off the blank column (a fixed-order
// block sum over the blank states) and off each distinct label's column: the thread of a label's FIRST occurrence walks the sample's
// "next state with this label" chain (ctc_prep_kernel) and adds in state order.  No float atomics anywhere.
#include "dma_common.h"
#include "ctc_rows.h"
#include "omr_hip.h"

namespace {

constexpr int CTC_K = 8;            // frames per prefetch block, and between two renormalisations
constexpr int CTC_TMAX = 1023;      // T + 1 threads must fit a workgroup

struct CtcWs {
    double* off;    // [2][B][Fmax]   fp64 offset of the stored values of (direction, sample, frame)
    double* logp;   // [2][B]         log P from either direction (-inf: infeasible); [0] is the one used
    float* lse;     // [B][Fmax]      log-sum-exp of each frame's logits
    float* ab;      // [2][B][Fmax][2T + 2]   stored log alpha (0) / reversed log beta (1)
    int* len;       // [B]            L_b
    int* next;      // [B][T]         next label index with the same label, -1: none
    int* first;     // [B][T]         1: no earlier label index has this label
};
inline long ctc_ws_layout(CtcWs* w, char* base, long B, long F, long T) {
    long o = 0;
    auto take = [&](long bytes) { char* p = base ? base + o : nullptr; o += (bytes + 15) & ~15L; return p; };
    w->off = (double*)take(2 * B * F * 8);
    w->logp = (double*)take(2 * B * 8);
    w->lse = (float*)take(B * F * 4);
    w->ab = (float*)take(2 * B * F * (2 * T + 2) * 4);
    w->len = (int*)take(B * 4);
    w->next = (int*)take(B * T * 4);
    w->first = (int*)take(B * T * 4);
    return o;
}

// ------------------------------------------------------------------------------------------------ frames

// Sample b's grid (h, w), its groups per column G and frame count F; an unusable grid is the empty sample.
__device__ __forceinline__ void sample_grid(const int* __restrict__ grid, int b, int gh, int gw, int S, int pool, int Fmax, int& h, int& w, int& G) {
    h = grid ? grid[2 * b] : gh;
    w = grid ? grid[2 * b + 1] : gw;
    bool ok = h >= 1 && w >= 1 && (long)h * w <= S;
    if (ok) {
        G = (h + pool - 1) / pool;
        ok = (long)G * w <= Fmax;
    }
    if (!ok) h = w = G = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void ctc_frames_fwd_kernel(const T* __restrict__ mem, const int* __restrict__ grid, T* __restrict__ out,
                                                             int* __restrict__ frame_len, int S, int d, int gh, int gw, int pool, int Fmax) {
    const int b = blockIdx.y, f = blockIdx.x;
    int h, w, G;
    sample_grid(grid, b, gh, gw, S, pool, Fmax, h, w, G);
    const int F = G * w;
    if (f == 0 && threadIdx.x == 0) frame_len[b] = F;
    T* o = out + ((long)b * Fmax + f) * d;
    if (f >= F) {
        for (int c = threadIdx.x; c < d; c += 256) o[c] = from_f32<T>(0.f);
        return;
    }
    const int j = f / G, q = f - j * G, r0 = q * pool, r1 = min(r0 + pool, h);
    const T* src = mem + (long)b * S * d;
    for (int c = threadIdx.x; c < d; c += 256) {
        if (r1 - r0 == 1) { o[c] = src[((long)r0 * w + j) * d + c]; continue; }
        float s = to_f32(src[((long)r0 * w + j) * d + c]);
        for (int i = r0 + 1; i < r1; ++i) s += to_f32(src[((long)i * w + j) * d + c]);
        o[c] = from_f32<T>(s / (float)(r1 - r0));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void ctc_frames_bwd_kernel(const T* __restrict__ g, const int* __restrict__ grid, T* __restrict__ dmem, int S, int d,
                                                             int gh, int gw, int pool, int Fmax) {
    const int b = blockIdx.y, r = blockIdx.x;
    int h, w, G;
    sample_grid(grid, b, gh, gw, S, pool, Fmax, h, w, G);
    T* o = dmem + ((long)b * S + r) * d;
    if (r >= h * w) {
        for (int c = threadIdx.x; c < d; c += 256) o[c] = from_f32<T>(0.f);
        return;
    }
    const int i = r / w, j = r - i * w, q = i / pool, cnt = min((q + 1) * pool, h) - q * pool;
    const T* src = g + ((long)b * Fmax + (long)j * G + q) * d;
    for (int c = threadIdx.x; c < d; c += 256) o[c] = cnt == 1 ? src[c] : from_f32<T>(to_f32(src[c]) / (float)cnt);
}

// ------------------------------------------------------------------------------------------------ loss

// One workgroup per sample: L_b, and for every label index the next one with the same label / whether it is the first with it.
__global__ __launch_bounds__(256) void ctc_prep_kernel(const long* __restrict__ tgt, int* __restrict__ len, int* __restrict__ next, int* __restrict__ first,
                                                       int T, int V, int blank, int eos) {
    __shared__ int sL;
    __shared__ int lab[CTC_TMAX + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long* y = tgt + (long)b * T;
    if (tid == 0) sL = T;
    __syncthreads();
    int mine = T;
    for (int j = tid; j < T; j += 256) {
        const long t = y[j];
        if (t == blank || t == eos || t < 0 || t >= V) { mine = j; break; }
    }
    atomicMin(&sL, mine);
    __syncthreads();
    const int L = sL;
    for (int j = tid; j < L; j += 256) lab[j] = (int)y[j];
    __syncthreads();
    for (int j = tid; j < L; j += 256) {
        int n = -1, fst = 1;
        for (int k = j + 1; k < L; ++k)
            if (lab[k] == lab[j]) { n = k; break; }
        for (int k = 0; k < j; ++k)
            if (lab[k] == lab[j]) { fst = 0; break; }
        next[(long)b * T + j] = n;
        first[(long)b * T + j] = fst;
    }
    if (tid == 0) len[b] = L;
}

__device__ __forceinline__ float lse3(float a, float b, float c) {
    const float m = fmaxf(fmaxf(a, b), c);
    return m == -INFINITY ? -INFINITY : m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

// Workgroup 2b + dir: the recursion of sample b forwards (dir 0) or backwards (dir 1); blockDim.x = the multiple of 64 that holds T + 1.
template <typename T>
__global__ __launch_bounds__(1024) void ctc_sweep_kernel(const T* __restrict__ logits, long ldv, const int* __restrict__ frame_len,
                                                         const long* __restrict__ tgt, const int* __restrict__ len, const float* __restrict__ lse,
                                                         float* __restrict__ ab, double* __restrict__ off, double* __restrict__ logp, int B, int Fmax, int Tt,
                                                         int blank) {
    __shared__ float edge[2][16];
    __shared__ float red[16];
    const int b = blockIdx.x >> 1, dir = blockIdx.x & 1, j = threadIdx.x, lane = j & 63, wv = j >> 6, nw = blockDim.x >> 6;
    const int L = len[b], F = clamp_len(frame_len[b], Fmax);
    if (F < 1) {
        if (j == 0) logp[(long)dir * B + b] = -INFINITY;
        return;
    }
    const long S2 = 2L * Tt + 2;
    float* A = ab + ((long)dir * B + b) * Fmax * S2;
    double* O = off + ((long)dir * B + b) * Fmax;
    const T* X = logits + (long)b * Fmax * ldv;
    const float* Z = lse + (long)b * Fmax;
    const bool has_lab = j < L;
    int lab = blank, labl = -1;
    if (has_lab) lab = (int)tgt[(long)b * Tt + (dir ? L - 1 - j : j)];
    if (has_lab && j >= 1) labl = (int)tgt[(long)b * Tt + (dir ? L - j : j - 1)];
    const bool skip = has_lab && j >= 1 && lab != labl;

    T rl[CTC_K], rb[CTC_K];
    float rz[CTC_K];
    auto load = [&](int i0, T (&xl)[CTC_K], T (&xb)[CTC_K], float (&xz)[CTC_K]) {
#pragma unroll
        for (int k = 0; k < CTC_K; ++k) {
            const int i = i0 + k;
            if (i < F) {
                const int t = dir ? F - 1 - i : i;
                const T* r = X + (long)t * ldv;
                xl[k] = r[lab];
                xb[k] = r[blank];
                xz[k] = Z[t];
            } else {
                xl[k] = xb[k] = from_f32<T>(0.f);
                xz[k] = 0.f;
            }
        }
    };
    load(0, rl, rb, rz);
    float a0 = -INFINITY, a1 = -INFINITY;
    double offs = 0.0;
    for (int i0 = 0; i0 < F; i0 += CTC_K) {
        T nl[CTC_K], nb[CTC_K];
        float nz[CTC_K];
        load(i0 + CTC_K, nl, nb, nz);
#pragma unroll
        for (int k = 0; k < CTC_K; ++k) {
            const int i = i0 + k;
            if (i < F) {
                const float z = rz[k];
                const float eb = to_f32(rb[k]) - z;
                const float el = has_lab ? to_f32(rl[k]) - z : -INFINITY;
                if (i == 0) {
                    a0 = j == 0 ? eb : -INFINITY;
                    a1 = j == 0 ? el : -INFINITY;
                } else {
                    float left = __shfl_up(a1, 1, 64);
                    if (lane == 0) left = wv > 0 ? edge[(i - 1) & 1][wv - 1] : -INFINITY;
                    const float n0 = eb + lse2(a0, left);
                    const float n1 = el + lse3(a1, a0, skip ? left : -INFINITY);
                    a0 = n0;
                    a1 = n1;
                }
                if (k == CTC_K - 1 || i == F - 1) {
                    float m = wave_max(fmaxf(a0, a1));
                    if (lane == 0) red[wv] = m;
                    lds_barrier();
                    m = red[0];
                    for (int w = 1; w < nw; ++w) m = fmaxf(m, red[w]);
                    if (m == -INFINITY || !(m == m)) m = 0.f;
                    a0 -= m;
                    a1 -= m;
                    offs += (double)m;
                }
                if (lane == 63) edge[i & 1][wv] = a1;
                const int t = dir ? F - 1 - i : i;
                if (j <= L) A[t * S2 + 2 * j] = a0;
                if (j < L) A[t * S2 + 2 * j + 1] = a1;
                if (j == 0) O[t] = offs;
                lds_barrier();
            }
        }
#pragma unroll
        for (int k = 0; k < CTC_K; ++k) { rl[k] = nl[k]; rb[k] = nb[k]; rz[k] = nz[k]; }
    }
    // log P = offset + lse2(final blank state 2L, final label state 2L - 1): thread L holds the first, its left neighbour the second
    float left = __shfl_up(a1, 1, 64);
    if (lane == 0) left = wv > 0 ? edge[(F - 1) & 1][wv - 1] : -INFINITY;
    if (j == L) {
        const double x0 = (double)a0, x1 = (double)left, m = fmax(x0, x1);
        logp[(long)dir * B + b] = m == -INFINITY ? -INFINITY : offs + m + log(exp(x0 - m) + exp(x1 - m));
    }
}

// One workgroup, fp64, fixed order (the way of ce_finalize_kernel): rows, loss, acc2 = {sum_b nll_b / max(L_b, 1), B}, infeasible.
__global__ __launch_bounds__(1024) void ctc_finalize_kernel(const double* __restrict__ logp, const int* __restrict__ len, double* __restrict__ acc,
                                                            float* __restrict__ loss, float* __restrict__ rows, int* __restrict__ infeasible, int B) {
    double a[2] = {};
    for (int b = threadIdx.x; b < B; b += 1024) {
        const double lp = logp[b];
        const bool ok = lp == lp && lp != -INFINITY && lp != INFINITY;
        rows[b] = ok ? (float)(-lp) : 0.f;
        if (ok) a[0] += -lp / (double)max(len[b], 1);
        else a[1] += 1.0;
    }
    block1024_sum(a);
    if (threadIdx.x == 0) {
        acc[0] = a[0];
        acc[1] = (double)B;
        loss[0] = (float)(a[0] / (double)B);
        infeasible[0] = (int)a[1];
    }
}

// One workgroup per frame (see the head of the file).
template <typename T>
__global__ __launch_bounds__(256) void ctc_bwd_kernel(const T* __restrict__ logits, long ldv, const int* __restrict__ frame_len, const long* __restrict__ tgt,
                                                      const int* __restrict__ len, const int* __restrict__ next, const int* __restrict__ first,
                                                      const float* __restrict__ lse, const float* __restrict__ ab, const double* __restrict__ off,
                                                      const double* __restrict__ logp, T* __restrict__ dlogits, int B, int Fmax, int Tt, int V, int blank,
                                                      float gscale, const float* __restrict__ grad_out) {
    __shared__ float red[4];
    const int b = blockIdx.y, f = blockIdx.x, tid = threadIdx.x;
    T* dr = dlogits + ((long)b * Fmax + f) * ldv;
    const int L = len[b], F = clamp_len(frame_len[b], Fmax);
    const double lp = logp[b];
    const bool live = f < F && lp == lp && lp != -INFINITY && lp != INFINITY;      // the same for the whole workgroup
    if (!live) {
        for (int v = tid; v < ldv; v += 256) dr[v] = from_f32<T>(0.f);
        return;
    }
    const T* xr = logits + ((long)b * Fmax + f) * ldv;
    const float z = lse[(long)b * Fmax + f];
    const float sc = gscale * (grad_out ? grad_out[0] : 1.f) / ((float)B * (float)max(L, 1));
    for (int v = tid; v < ldv; v += 256) dr[v] = from_f32<T>(v < V ? __expf(to_f32(xr[v]) - z) * sc : 0.f);
    const long S2 = 2L * Tt + 2;
    const float* al = ab + ((long)b * Fmax + f) * S2;
    const float* be = ab + (((long)B + b) * Fmax + f) * S2;
    const double c = off[(long)b * Fmax + f] + off[((long)B + b) * Fmax + f] - lp;
    // posterior of lattice state s, whose emission is e: alpha and beta both hold e
    auto post = [&](int s, float e) -> float {
        const float a = al[s], bt = be[2 * L - s];
        if (a == -INFINITY || bt == -INFINITY) return 0.f;
        return expf((float)((double)a + (double)bt + c - (double)e));
    };
    const long* y = tgt + (long)b * Tt;
    const float xb = to_f32(xr[blank]);
    float pb = 0.f;
    for (int j = tid; j <= L; j += 256) pb += post(2 * j, xb - z);
    pb = block_sum(pb, red);        // its barrier also orders the stores below behind the softmax pass above
    if (tid == 0) dr[blank] = from_f32<T>((__expf(xb - z) - pb) * sc);
    for (int j = tid; j < L; j += 256) {
        if (!first[(long)b * Tt + j]) continue;
        const int v = (int)y[j];
        const float x = to_f32(xr[v]);
        float p = 0.f;
        for (int k = j; k >= 0; k = next[(long)b * Tt + k]) p += post(2 * k + 1, x - z);
        dr[v] = from_f32<T>((__expf(x - z) - p) * sc);
    }
}

// ------------------------------------------------------------------------------------------------ greedy

template <typename T>
__global__ __launch_bounds__(256) void ctc_frame_argmax_kernel(const T* __restrict__ logits, long ldv, const int* __restrict__ frame_len,
                                                               int* __restrict__ arg, float* __restrict__ val, int Fmax, int V, int blank) {
    __shared__ float sv[256];
    __shared__ int si[256];
    const int b = blockIdx.y, f = blockIdx.x, tid = threadIdx.x;
    const long row = (long)b * Fmax + f;
    if (f >= clamp_len(frame_len[b], Fmax)) {
        if (tid == 0) { arg[row] = blank; val[row] = 0.f; }
        return;
    }
    const T* x = logits + row * ldv;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < V; i += 256) {
        const float v = to_f32(x[i]);
        if (v > best || (v == best && i < bi)) { best = v; bi = i; }
    }
    sv[tid] = best;
    si[tid] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const float v2 = sv[tid + o];
            const int i2 = si[tid + o];
            if (v2 > sv[tid] || (v2 == sv[tid] && i2 < si[tid])) { sv[tid] = v2; si[tid] = i2; }
        }
        __syncthreads();
    }
    if (tid == 0) { arg[row] = si[0] < V ? si[0] : blank; val[row] = sv[0]; }      // a row of NaN wins no comparison: blank
}

// One wave per sample: keep frame f when its pick is no blank and differs from frame f - 1's; ballot + prefix popcount per 64 frames.
__global__ __launch_bounds__(64) void ctc_collapse_kernel(const int* __restrict__ arg, const int* __restrict__ frame_len, int* __restrict__ tokens,
                                                          int* __restrict__ lengths, int Fmax, int blank) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int F = clamp_len(frame_len[b], Fmax);
    const int* a = arg + (long)b * Fmax;
    int* out = tokens + (long)b * Fmax;
    int base = 0;
    for (int f0 = 0; f0 < F; f0 += 64) {
        const int f = f0 + lane;
        const int tok = f < F ? a[f] : blank;
        const int prev = (f > 0 && f < F) ? a[f - 1] : -1;
        const bool keep = f < F && tok != blank && tok != prev;
        const unsigned long long mask = __ballot(keep);
        if (keep) out[base + __popcll(mask & ((1ull << lane) - 1ull))] = tok;
        base += __popcll(mask);
    }
    for (int f = base + lane; f < Fmax; f += 64) out[f] = blank;
    if (lane == 0) lengths[b] = base;
}

bool frames_ok(const void* a, const void* c, int B, int S, int d, int gh, int gw, int pool, int Fmax, const int* grid) {
    if (!a || !c || B < 1 || B > 65535 || S < 1 || d < 1 || pool < 1 || Fmax < 1) return false;
    return grid != nullptr || (gh >= 1 && gw >= 1 && (long)gh * gw <= S);
}
bool ctc_ok(const void* logits, long ldv, const int* frame_len, int B, int Fmax, int V, int blank) {
    return logits && frame_len && B >= 1 && B <= 32767 && Fmax >= 1 && V >= 1 && ldv >= V && blank >= 0 && blank < V;
}

}  // namespace

extern "C" int omr_ctc_frames_fwd(int dtype, const void* mem, const int* grid, void* frames, int* frame_len, int B, int S, int d, int gh, int gw,
                                  int pool, int Fmax, void* stream) {
    if (!frames_ok(mem, frames, B, S, d, gh, gw, pool, Fmax, grid) || !frame_len) return OMR_ERR_ARG;
    DISPATCH_T(dtype, hipLaunchKernelGGL((ctc_frames_fwd_kernel<T>), dim3(Fmax, B), 256, 0, (hipStream_t)stream, (const T*)mem, grid, (T*)frames,
                                         frame_len, S, d, gh, gw, pool, Fmax))
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_ctc_frames_bwd(int dtype, const void* dframes, const int* grid, void* dmem, int B, int S, int d, int gh, int gw, int pool,
                                  int Fmax, void* stream) {
    if (!frames_ok(dframes, dmem, B, S, d, gh, gw, pool, Fmax, grid)) return OMR_ERR_ARG;
    DISPATCH_T(dtype, hipLaunchKernelGGL((ctc_frames_bwd_kernel<T>), dim3(S, B), 256, 0, (hipStream_t)stream, (const T*)dframes, grid, (T*)dmem, S, d,
                                         gh, gw, pool, Fmax))
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" long omr_ctc_workspace_bytes(int B, int Fmax, int Tmax, int V) {
    if (B < 1 || B > 32767 || Fmax < 1 || Tmax < 1 || Tmax > CTC_TMAX || V < 1) return -1;
    CtcWs w;
    return ctc_ws_layout(&w, nullptr, B, Fmax, Tmax);
}

extern "C" int omr_ctc_fwd(int dtype, const void* logits, long ldv, const int* frame_len, const long* targets, void* ws, double* acc2, float* loss,
                           float* rows, int* infeasible, int B, int Fmax, int T, int V, int blank_idx, int eos_idx, void* stream) {
    if (!ctc_ok(logits, ldv, frame_len, B, Fmax, V, blank_idx) || !targets || !ws || !acc2 || !loss || !rows || !infeasible || T < 1 ||
        T > CTC_TMAX || eos_idx < -1 || eos_idx >= V)
        return OMR_ERR_ARG;
    if (dtype != OMR_F32 && dtype != OMR_BF16) return OMR_ERR_UNSUPPORTED;
    CtcWs w;
    ctc_ws_layout(&w, (char*)ws, B, Fmax, T);
    hipStream_t s = (hipStream_t)stream;
    const int Tt = T, nt = (T + 1 + 63) / 64 * 64;      // Tt: DISPATCH_T names the element type T
    hipLaunchKernelGGL(ctc_prep_kernel, B, 256, 0, s, targets, w.len, w.next, w.first, T, V, blank_idx, eos_idx);
    DISPATCH_T(dtype, {
        hipLaunchKernelGGL((ctc_lse_kernel<T>), dim3(Fmax, B), 256, 0, s, (const T*)logits, frame_len, w.lse, Fmax, V, ldv);
        hipLaunchKernelGGL((ctc_sweep_kernel<T>), 2 * B, nt, 0, s, (const T*)logits, ldv, frame_len, targets, (const int*)w.len, (const float*)w.lse,
                           w.ab, w.off, w.logp, B, Fmax, Tt, blank_idx);
    })
    hipLaunchKernelGGL(ctc_finalize_kernel, 1, 1024, 0, s, (const double*)w.logp, (const int*)w.len, acc2, loss, rows, infeasible, B);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_ctc_bwd(int dtype, const void* logits, long ldv, const int* frame_len, const long* targets, const void* ws, void* dlogits, int B,
                           int Fmax, int T, int V, int blank_idx, float grad_scale, const float* grad_out, void* stream) {
    if (!ctc_ok(logits, ldv, frame_len, B, Fmax, V, blank_idx) || !targets || !ws || !dlogits || T < 1 || T > CTC_TMAX) return OMR_ERR_ARG;
    CtcWs w;
    ctc_ws_layout(&w, (char*)ws, B, Fmax, T);
    const int Tt = T;
    DISPATCH_T(dtype, hipLaunchKernelGGL((ctc_bwd_kernel<T>), dim3(Fmax, B), 256, 0, (hipStream_t)stream, (const T*)logits, ldv, frame_len, targets,
                                         (const int*)w.len, (const int*)w.next, (const int*)w.first, (const float*)w.lse, (const float*)w.ab,
                                         (const double*)w.off, (const double*)w.logp, (T*)dlogits, B, Fmax, Tt, V, blank_idx, grad_scale, grad_out))
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_ctc_greedy(int dtype, const void* logits, long ldv, const int* frame_len, int* frame_arg, float* frame_val, int* tokens,
                              int* lengths, int B, int Fmax, int V, int blank_idx, void* stream) {
    if (!ctc_ok(logits, ldv, frame_len, B, Fmax, V, blank_idx) || !frame_arg || !frame_val || !tokens || !lengths) return OMR_ERR_ARG;
    DISPATCH_T(dtype, hipLaunchKernelGGL((ctc_frame_argmax_kernel<T>), dim3(Fmax, B), 256, 0, (hipStream_t)stream, (const T*)logits, ldv, frame_len,
                                         frame_arg, frame_val, Fmax, V, blank_idx))
    hipLaunchKernelGGL(ctc_collapse_kernel, B, 64, 0, (hipStream_t)stream, (const int*)frame_arg, frame_len, tokens, lengths, Fmax, blank_idx);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}
