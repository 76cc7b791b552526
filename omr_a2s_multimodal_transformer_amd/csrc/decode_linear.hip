// The row kernel of KV-cached decoding and what goes with it: the greedy pick's second half, the per-row-position tables,
// and the launch (decode_linear_impl, omr_decode_linear).  decode.hip describes the linears of a position and issues them.
#include <type_traits>

#include "decode_common.h"

namespace {

// Row linear of a decode position (omr_decode_linear).  A position is a chain of ~50 dependent launches of almost no work, so
// what counts is how FEW launches there are and how short each one's dependent latency is -- not MFMA throughput (M = the
// batch rows of one position).  Workgroup = 16 output columns x 16 k-lanes; the weight chunks of a thread are requested
// first, the input rows are built while they fly (LayerNorm of the previous sub-layer / embedding / merge of the key-split
// attention partials: the element-wise kernels that used to sit between the GEMMs), then a fixed-order fp32 dot product per
// (row, column): chunks in ascending k, the 16 k-lanes combined by a fixed cross-lane tree.  blockIdx.y picks RM rows; nothing in a row's
// arithmetic depends on M or on the other rows.
constexpr int RM = 8, NOUT = 16, KL = 16, WCH = 8;      // rows per workgroup, columns per workgroup, k-lanes, prefetched weight chunks per thread
constexpr int MAXSPLIT = 64, MAXHS = 512;                // key splits the merge prologue takes (attn_common.h choose_split caps a decode
                                                         // row at 64 splits of >= 256 keys: the reference's largest memory, 12 696 tokens,
                                                         // is 50); heads x splits

// Sum over the 16 k-lanes of a column (= one DPP row): four cross-lane adds, every lane ends with the total.  (The generic
// __shfl_xor butterfly is ~7 instructions per step through the LDS crossbar.)
__device__ __forceinline__ float klane_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
    return v;
}

// e4m3 (OCP) weight chunk -> fp32: 8 codes per lane and chunk (gfx950 converts two codes per v_cvt_pk_f32_fp8)
struct W8Chunk { uint2 v; };
__device__ __forceinline__ void w_unpack(const W8Chunk& c, float (&f)[8]) {
    const auto p0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.v.x, false), p1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.v.x, true);
    const auto p2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.v.y, false), p3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.v.y, true);
    f[0] = p0[0]; f[1] = p0[1]; f[2] = p1[0]; f[3] = p1[1]; f[4] = p2[0]; f[5] = p2[1]; f[6] = p3[0]; f[7] = p3[1];
}
__device__ __forceinline__ void w_unpack(const bf16x8& c, float (&f)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = to_f32(c[e]);
}
__device__ __forceinline__ void w_unpack(const f32x4& c, float (&f)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = c[e];
}

// The kernel's argument block: the public omr_decode_linear_args (its layout is pinned) plus what a decode state with per-row
// positions adds (ROWS): row m sits at position row_pos[m], so its positional row is pe_row + row_pos[m] * K and its out1 part
// (the K|V projection's cache row) lands out1_pos_ld elements further per position.  GROUP (a grouped position, `group`
// consecutive rows = consecutive positions of one slot; omr_decode_verify_rows): the out1 part of row m goes to the cache of slot
// m / group, not of row m.
struct LinArgs { omr_decode_linear_args a; const int* row_pos; long out1_pos_ld; int group; };

template <typename T, bool W8, bool ROWS, bool GROUP>
__global__ __launch_bounds__(256) void decode_linear_kernel(LinArgs la) {
    const omr_decode_linear_args& a = la.a;
    typedef typename Frag<T>::type F;
    constexpr int VEC = W8 ? 8 : Frag<T>::N;                            // weight elements per chunk (fp8: 8 codes = 8 bytes)
    typedef typename std::conditional<W8, W8Chunk, F>::type WF;
    extern __shared__ __attribute__((aligned(16))) float xs[];          // [RM][K]: the rows as the GEMM sees them (values rounded to T)
    __shared__ float mls[4 * 2 * MAXHS];                                 // prologue 3: per-wave (max | sum) strips
    __shared__ float cand[RM][NOUT];                                     // greedy pick: the workgroup's rounded outputs
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nl = tid / KL, kl = tid % KL;
    const int n = blockIdx.x * NOUT + nl, K = a.K, nch = K / VEC;
    typedef typename std::conditional<W8, unsigned char, T>::type WT;
    const WT* wrow = (W8 ? (const WT*)a.w8 : (const WT*)a.w) + (long)(n < a.N ? n : 0) * K;

    // K is a multiple of KL * VEC (host check): chunk kl + i * KL exists for every lane or for none, so the loops over a thread's
    // chunks have block-uniform bounds and the loads carry no per-lane test (columns past N read row 0 and are never stored)
    const int cpt = nch / KL;
    WF wv[WCH];
#pragma unroll
    for (int i = 0; i < WCH; ++i)
        if (i < cpt) wv[i] = *reinterpret_cast<const WF*>(wrow + (kl + i * KL) * VEC);
    const int per = K / 64;                                              // prologues 1-3: a wave builds a row, lane = `per` consecutive columns
    {
        const int r0 = blockIdx.y * RM, rm = min(RM, a.M - r0);
        for (int r = wave; r < rm; r += 4) {
            const long m = r0 + r;
            float* xr = xs + r * K;
            if (a.pro == 0) {
                const T* src = (const T*)a.x + m * a.ldx;
                for (int k = lane; k < K; k += 64) xr[k] = to_f32(src[k]);
            } else if (a.pro == 1) {        // add + LayerNorm, same lane layout and summation order as add_ln_fwd_kernel (norm.hip)
                const T* y = (const T*)a.x + m * a.ldx + lane * per;
                const T* rs_ = (const T*)a.res + m * a.ldres + lane * per;
                auto run = [&](auto per_c) {
                    constexpr int PER = decltype(per_c)::value;
                    float v[PER], mu, rstd;
#pragma unroll
                    for (int i = 0; i < PER; ++i) v[i] = to_f32(y[i]) + to_f32(rs_[i]);
                    ln_row<PER>(v, a.gamma, a.beta, lane, a.eps, mu, rstd);
#pragma unroll
                    for (int i = 0; i < PER; ++i) {
                        const T o = from_f32<T>(v[i]);
                        xr[lane * PER + i] = to_f32(o);
                        if (blockIdx.x == 0) ((T*)a.xn_out)[m * K + lane * PER + i] = o;
                    }
                };
                if (per == 2) run(std::integral_constant<int, 2>());
                else if (per == 4) run(std::integral_constant<int, 4>());
                else run(std::integral_constant<int, 8>());
            } else if (a.pro == 2) {        // embedding + positional row (embed_pe_kernel, elementwise.hip)
                const long t = a.tokens[m];
                const bool ok = t >= 0 && t < a.vocab;
                const float* pe_row = ROWS ? a.pe_row + (long)la.row_pos[m] * K : a.pe_row;
                for (int i = 0; i < per; ++i) {
                    const int k = lane * per + i;
                    const T o = from_f32<T>((ok ? to_f32(((const T*)a.emb)[t * K + k]) : 0.f) + pe_row[k]);
                    xr[k] = to_f32(o);
                    if (blockIdx.x == 0) ((T*)a.xn_out)[m * K + k] = o;
                }
            } else {                        // merge of the key-split partial softmaxes: attn_split_merge_kernel's arithmetic in its
                                            // order.  The (max, sum) pairs of the row's H * nsplit partials go through a per-wave LDS
                                            // strip first (one global round trip for all of them); a lane's `per` columns lie in one head
                const int hs = a.H * a.nsplit, stride = a.hd + 2;
                float* ml = mls + wave * (2 * MAXHS);
                for (int l = lane; l < hs; l += 64) {
                    const float* P = a.part + (m * hs + l) * stride;
                    ml[l] = P[a.hd];
                    ml[MAXHS + l] = P[a.hd + 1];
                }
                // the LDS queue of a wave is in order: the reads below follow the writes above
                const int h = (lane * per) / a.hd, dch = lane * per - h * a.hd;
                const float* mh = ml + h * a.nsplit;
                const float* P = a.part + ((m * a.H + h) * a.nsplit) * stride + dch;
                float mm = -INFINITY;
                for (int j = 0; j < a.nsplit; ++j) mm = fmaxf(mm, mh[j]);
                float l_tot = 0.f, o[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) o[i] = 0.f;
#pragma unroll 4
                for (int j = 0; j < a.nsplit; ++j) {
                    const float mj = mh[j];
                    const float wj = mj == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mj - mm);
                    l_tot += mh[MAXHS + j] * wj;
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        if (i < per) o[i] += P[j * stride + i] * wj;
                }
                const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (i < per) xr[lane * per + i] = to_f32(from_f32<T>(o[i] * inv));
            }
        }
        __syncthreads();
        float acc[RM];
#pragma unroll
        for (int r = 0; r < RM; ++r) acc[r] = 0.f;
        auto slice_rows = [&](auto nr_c) {       // one row (bs 1, the reference's loop) takes the lean single-row body
            constexpr int NR = decltype(nr_c)::value;
#pragma unroll
            for (int i = 0; i < WCH; ++i)
                if (i < cpt) {
                    const float* xc = xs + (kl + i * KL) * VEC;
                    float wf[VEC];
                    w_unpack(wv[i], wf);
#pragma unroll
                    for (int r = 0; r < NR; ++r)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) acc[r] = fmaf(wf[e], xc[r * K + e], acc[r]);
                }
            for (int i = WCH; i < cpt; ++i) {                            // K beyond the prefetched chunks
                const WF wx = *reinterpret_cast<const WF*>(wrow + (kl + i * KL) * VEC);
                const float* xc = xs + (kl + i * KL) * VEC;
                float wf[VEC];
                w_unpack(wx, wf);
#pragma unroll
                for (int r = 0; r < NR; ++r)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[r] = fmaf(wf[e], xc[r * K + e], acc[r]);
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[r] = klane_sum(acc[r]);
        };
        if (rm == 1) slice_rows(std::integral_constant<int, 1>());
        else slice_rows(std::integral_constant<int, RM>());             // rows past rm: arithmetic on stale LDS, never stored
        if (kl == 0 && n < a.N) {
            const float bv = a.bias ? a.bias[n] : 0.f, wsc = W8 ? a.w8_scale[n] : 1.f;
#pragma unroll
            for (int r = 0; r < RM; ++r) {
                if (r >= rm) break;
                float v = W8 ? fmaf(acc[r], wsc, bv) : acc[r] + bv;
                if (a.relu) v = fmaxf(v, 0.f);
                const T o = from_f32<T>(v);
                const long m = r0 + r;
                if (n < a.n0) ((T*)a.out0)[m * a.ld0 + n] = o;
                else ((T*)a.out1)[(GROUP ? m / la.group : m) * a.ld1 + (ROWS ? (long)la.row_pos[m] * la.out1_pos_ld : 0) + (n - a.n0)] = o;
                if (a.out32) a.out32[m * a.ld32 + n] = to_f32(o);
                cand[r][nl] = to_f32(o);
            }
        }
        // ---- greedy pick, first half: this workgroup's candidate per row (value, column); decode_pick_kernel reduces the
        //      ceil(N/16) candidates of a row.  (Letting the last workgroup to finish do that -- counter + agent-scope fences --
        //      was measured: 20 us slower per position than the second launch.)
        if (a.amax_part) {
            if (kl == 0 && n >= a.N)
#pragma unroll
                for (int r = 0; r < RM; ++r) cand[r][nl] = -INFINITY;
            __syncthreads();
            if (tid < rm) {
                float best = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
                for (int c = 0; c < NOUT; ++c) {
                    const float v = cand[tid][c];
                    if (v > best) { best = v; bi = blockIdx.x * NOUT + c; }            // ascending columns: the first maximum stays
                }
                float* pp = a.amax_part + ((long)(r0 + tid) * gridDim.x + blockIdx.x) * 2;
                pp[0] = best; pp[1] = __int_as_float(bi);
            }
        }
    }
}

// greedy pick, second half: one wave per row over the G (value, column) candidates; first index of the maximum (torch.argmax)
__global__ __launch_bounds__(64) void decode_pick_kernel(const float* __restrict__ part, int G, long* __restrict__ idx_out, float* __restrict__ val_out) {
    const int lane = threadIdx.x;
    const float* pp = part + (long)blockIdx.x * G * 2;
    float best = -INFINITY; int bi = 0x7fffffff;
    for (int i = lane; i < G; i += 64) {
        const float v = pp[2 * i]; const int ii = __float_as_int(pp[2 * i + 1]);
        if (v > best || (v == best && ii < bi)) { best = v; bi = ii; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float v = __shfl_xor(best, o, 64); const int ii = __shfl_xor(bi, o, 64);
        if (v > best || (v == best && ii < bi)) { best = v; bi = ii; }
    }
    // no comparison won (the row is all NaN, or all -inf: `v > best` alone in the first half): index 0, as argmax_kernel and torch.argmax
    if (lane == 0) { idx_out[blockIdx.x] = bi == 0x7fffffff ? 0 : bi; if (val_out) val_out[blockIdx.x] = best; }
}

// Per-row positions (omr_decode_steps_rows): ONE launch per host call turns pos[B] into the tables every kernel of position s
// indexes at [s][b] -- the position pos[b] + off + s, the first visible key lo_b (banded causal mask, decoder.py:213-214) and
// the key count.  A position is clamped into [0, max_len - n_steps]: whatever `pos` holds, no kernel leaves the caches.
// grouped (omr_decode_verify_rows): the n_steps consecutive positions of slot b are ROWS of one position, entry [b][s], not steps [s][b].
__global__ __launch_bounds__(256) void decode_rows_tables_kernel(const int* __restrict__ pos, int off, int B, int n_steps, int max_len, int window,
                                                                 int grouped, int* __restrict__ tpos, int* __restrict__ tstart, int* __restrict__ tcount) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * n_steps) return;
    const int b = grouped ? i / n_steps : i % B, s = grouped ? i % n_steps : i / B;
    const int t = min(max(pos[b] + off, 0), max_len - n_steps) + s;
    const int lo = (window > 0 && t - window > 0) ? t - window : 0;
    tpos[i] = t; tstart[i] = lo; tcount[i] = t + 1 - lo;
}

}  // namespace

namespace omr_dec {

// row_pos != NULL: the per-row-position form (LinArgs); group > 1 (with row_pos): the grouped form
int decode_linear_impl(const omr_decode_linear_args& a, const int* row_pos, long out1_pos_ld, void* stream, int group) {
    const int vec = (a.dtype == OMR_BF16 || a.w8) ? 8 : 4;
    if (a.M <= 0 || a.N <= 0 || a.K <= 0 || a.K % vec || a.K > 2048 || (!a.w && !a.w8) || !a.out0 || a.n0 < 0) return OMR_ERR_ARG;
    if (a.w8 ? (!a.w8_scale || ((uintptr_t)a.w8 & 7)) : (((uintptr_t)a.w & 15) != 0)) return OMR_ERR_ARG;
    if (a.n0 < a.N && !a.out1) return OMR_ERR_ARG;
    if (a.pro < 0 || a.pro > 3) return OMR_ERR_ARG;
    if (a.K % (KL * vec)) return OMR_ERR_UNSUPPORTED;                    // whole 16-lane chunk groups (128 bf16 / 64 fp32 columns)
    if (a.amax_idx && !a.amax_part) return OMR_ERR_ARG;
    if (a.pro && (a.K % 64 || a.K / 64 > 16)) return OMR_ERR_ARG;
    if (a.pro == 1 && a.K != 128 && a.K != 256 && a.K != 512) return OMR_ERR_UNSUPPORTED;      // the widths omr_add_layernorm_fwd takes
    if ((a.pro == 0 || a.pro == 1) && !a.x) return OMR_ERR_ARG;
    if (a.pro == 1 && (!a.res || !a.gamma || !a.beta || !a.xn_out)) return OMR_ERR_ARG;
    if (a.pro == 2 && (!a.tokens || !a.emb || !a.pe_row || !a.xn_out)) return OMR_ERR_ARG;
    if (a.pro == 3 && (!a.part || a.nsplit < 1 || a.nsplit > MAXSPLIT || a.H < 1 || a.hd < 1 || a.H * a.hd != a.K || a.H * a.nsplit > MAXHS || a.hd % (a.K / 64))) return OMR_ERR_ARG;
    const dim3 grid((unsigned)cdiv(a.N, NOUT), (unsigned)cdiv(a.M, RM)), block(256);
    const size_t shm = (size_t)RM * a.K * sizeof(float);
    if (a.dtype != OMR_BF16 && a.dtype != OMR_F32) return OMR_ERR_UNSUPPORTED;
    if (group < 1 || (group > 1 && (!row_pos || a.M % group))) return OMR_ERR_ARG;
    const LinArgs la = {a, row_pos, out1_pos_ld, group};
    auto launch = [&](auto rows_c, auto group_c) {
        constexpr bool ROWS = decltype(rows_c)::value, GROUP = decltype(group_c)::value;
        if (a.dtype == OMR_BF16 && a.w8) hipLaunchKernelGGL((decode_linear_kernel<bf16, true, ROWS, GROUP>), grid, block, shm, (hipStream_t)stream, la);
        else if (a.dtype == OMR_F32 && a.w8) hipLaunchKernelGGL((decode_linear_kernel<float, true, ROWS, GROUP>), grid, block, shm, (hipStream_t)stream, la);
        else if (a.dtype == OMR_BF16) hipLaunchKernelGGL((decode_linear_kernel<bf16, false, ROWS, GROUP>), grid, block, shm, (hipStream_t)stream, la);
        else hipLaunchKernelGGL((decode_linear_kernel<float, false, ROWS, GROUP>), grid, block, shm, (hipStream_t)stream, la);
    };
    if (group > 1) launch(std::true_type(), std::true_type());
    else if (row_pos) launch(std::true_type(), std::false_type());
    else launch(std::false_type(), std::false_type());
    if (a.amax_idx) hipLaunchKernelGGL(decode_pick_kernel, dim3((unsigned)a.M), dim3(64), 0, (hipStream_t)stream, a.amax_part, (int)grid.x, a.amax_idx, a.amax_val);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

// the model widths the row kernel takes (8 launches per layer); any other takes one kernel per step of the layer
bool takes_row_kernel(const omr_decode_desc& d) {
    const int smax = d.S > d.max_len ? d.S : d.max_len, splits_max = (smax + 255) / 256 < MAXSPLIT ? (smax + 255) / 256 : MAXSPLIT;
    return (d.d == 128 || d.d == 256 || d.d == 512) && d.ff <= 2048 && d.ff % (16 * ((d.dtype == OMR_BF16 || d.fp8) ? 8 : 4)) == 0 &&
           d.nhead * splits_max <= MAXHS;
}

void launch_rows_tables(const Model& m, const int* pos, int off, int n_steps, void* stream) {
    const omr_decode_desc& d = *m.d;
    const size_t tab = (size_t)m.rows * d.max_len;
    hipLaunchKernelGGL(decode_rows_tables_kernel, dim3((unsigned)cdiv((long)d.B * n_steps, 256)), dim3(256), 0, (hipStream_t)stream, pos, off, d.B,
                       n_steps, d.max_len, d.window, 0, m.w.rows_tab, m.w.rows_tab + tab, m.w.rows_tab + 2 * tab);
}

// The tables of ONE grouped position: row b * group + r sits at pos[b] + r (clamped like the steps of launch_rows_tables), entry
// [b][r] of the first position's part of each table.
Position launch_group_tables(const Model& m, const int* pos, int t_max, void* stream) {
    const omr_decode_desc& d = *m.d;
    const size_t tab = (size_t)m.rows * d.max_len;
    hipLaunchKernelGGL(decode_rows_tables_kernel, dim3((unsigned)cdiv((long)m.rows, 256)), dim3(256), 0, (hipStream_t)stream, pos, 0, d.B, m.group,
                       d.max_len, d.window, 1, m.w.rows_tab, m.w.rows_tab + tab, m.w.rows_tab + 2 * tab);
    return Position{t_max + m.group - 1, m.w.rows_tab, m.w.rows_tab + tab, m.w.rows_tab + 2 * tab};
}

// pos == NULL: every row at t.  Otherwise the rows of step s of the tables launch_rows_tables filled; t is the furthest row's.
Position position_at(const Model& m, const int* pos, int t, int s) {
    if (!pos) return Position{t, nullptr, nullptr, nullptr};
    const size_t tab = (size_t)m.rows * m.d->max_len, at = (size_t)s * m.d->B;
    return Position{t, m.w.rows_tab + at, m.w.rows_tab + tab + at, m.w.rows_tab + 2 * tab + at};
}

}  // namespace omr_dec

extern "C" int omr_decode_linear(const omr_decode_linear_args* ap, void* stream) {
    if (!ap) return OMR_ERR_ARG;
    return omr_dec::decode_linear_impl(*ap, nullptr, 0, stream, 1);
}

extern "C" int omr_decode_linear_rows(const omr_decode_linear_args* ap, const int* row_pos, long out1_pos_ld, void* stream) {
    if (!ap || !row_pos || out1_pos_ld < 0) return OMR_ERR_ARG;
    return omr_dec::decode_linear_impl(*ap, row_pos, out1_pos_ld, stream, 1);
}
