// Attention maps for gfx950: the head-averaged attention weights nn.MultiheadAttention returns beside its output
// (torch multi_head_attention_forward with need_weights = True, average_attn_weights = True; CrossAttention, model.py:323).
// The fused forward never holds P in memory; this is one more recompute pass from its `lse`, the pass both backward kernels
// already make:  P = exp2(score - lse * log2 e)  with the score chain, visibility range, augmented k-step and dropout words of
// attn_common.h, in the dQ kernel's orientation (lane = query row, keys on the accumulator's register axis).
//
//   w[b][t][s] (+)= out_scale * sum_h c * m_bhts * P_bhts        c = 1 / (1 - p), m = the keep bit (p = 0: c = m = 1)
//
// grid = (ceil(T / 128) * key ranges, 1, B).  Wave w of a workgroup owns query rows q0 + 32 w .. + 31 and, alone, the tile of
// `w` those rows have in the workgroup's key range: it walks the range in 64-key tiles and, per tile, the H heads IN ORDER,
// adding each head's P to 32 fp32 accumulator registers; the sum is scaled and stored once, through the wave's own LDS patch so
// that a store instruction writes whole 256-byte row segments (vector stores only).  Nothing is shared between
// workgroups and nothing is added atomically, so two runs give the same bits.  The four waves share the staged K tile of
// (tile, head) in LDS; the next (tile, head)'s K rows, Q fragments and lse are in flight while the current one is computed.
// Every s < S of every row t < T is written (keys nobody sees: exactly 0); columns S .. ldw - 1 are left alone.
#include "attn_common.h"

namespace {
using namespace attn;

struct MapOut {
    float* w; long ldw, bsw;          // [B][T][ldw] fp32
    float scale;                      // out_scale * c
    int accumulate;
    int vec4;                         // rows of w are 16-byte aligned: whole groups of 4 keys go out as one 16-byte store
    int range_len;                    // keys per workgroup, a multiple of 64
};

template <typename T, int HD, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_weights_kernel(AttnArgs a, MapOut m, const uint64_t* __restrict__ dmask,
                                                              const int* __restrict__ kv_len) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = ACfg<T>::VEC, KS = KStep<T>::value;
    constexpr int NKS = HD / KS, BKV = 64;
    constexpr int PK = HD + VEC;
    __shared__ __attribute__((aligned(16))) T Ks[BKV * PK];
    __shared__ __attribute__((aligned(16))) F Ka[BKV + 1];      // augmented k-step, key side: the key bias; entry BKV = zeros
    constexpr int WP = BKV + 4;                                 // pitch of the output patches: 272 bytes, rows 4 banks apart
    __shared__ __attribute__((aligned(16))) float Wt_[4 * 32 * WP];

    const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nqb = (a.T + 127) / 128;                          // blockIdx.x = query block + nqb * key range
    const int range = blockIdx.x / nqb, q0 = (blockIdx.x % nqb) * 128;
    const int b = blockIdx.z;
    const int qw0 = q0 + wave * 32;
    const int q = qw0 + (lane & 31);
    const int S = kv_len ? max(min(kv_len[b], a.S), 0) : a.S;   // this row's key count; keys S .. a.S - 1 are written as 0
    const T* Q = (const T*)a.q + (long)b * a.bsq;
    const T* K = (const T*)a.k + (long)b * a.bsk;
    const bool win_on = a.window > 0 && a.window < a.T;
    const float sc2 = a.scale * LOG2E;

    // the workgroup's keys [r_beg, r_end) and, inside them, the tiles some row of its 128 may see: [c_beg, c_end)
    const int r_beg = range * m.range_len, r_end = min(a.S, r_beg + m.range_len);
    int c_beg = r_beg, c_end = min(r_end, S);
    if (a.causal) {
        c_end = min(c_end, q0 + 128);
        if (win_on) c_beg = max(c_beg, max(0, q0 - a.window) / BKV * BKV);
    }

    // A wave's (32 queries x 64 keys) tile leaves through its own LDS patch, transposed: in the accumulator a lane holds 16-byte
    // pieces of ONE row, so a store instruction would touch 32 rows with 32 bytes each; read back with lane = (row, 16-byte
    // column) an instruction writes four whole 256-byte row segments.  The patch is the wave's alone: LDS serves a wave's
    // accesses in order, so a wave-level fence orders its writes and reads, no workgroup barrier.
    float* const Wt = Wt_ + wave * 32 * WP;
    const int kcol = 4 * (lane & 15), krow = lane >> 4;
    float* const wbase = m.w + (long)b * m.bsw;
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    auto put = [&](int kv0, const f32x16* acc) {                // acc == nullptr: zeros
        if (acc) {
            wave_sync();                                        // the reads of the previous tile are done
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 v = {acc[mb][4 * g], acc[mb][4 * g + 1], acc[mb][4 * g + 2], acc[mb][4 * g + 3]};
                    *reinterpret_cast<f32x4*>(&Wt[(lane & 31) * WP + mb * 32 + 8 * g + 4 * hh]) = v;
                }
            wave_sync();
        }
        const int key = kv0 + kcol;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int row = 4 * j + krow, qq = qw0 + row;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (acc) v = *reinterpret_cast<const f32x4*>(&Wt[row * WP + kcol]);
            if (qq >= a.T) continue;
            float* const wrow = wbase + (long)qq * m.ldw;
            if (m.vec4 && key + 4 <= a.S) {
                f32x4* p = reinterpret_cast<f32x4*>(wrow + key);
                if (m.accumulate) v += *p;
                *p = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (key + e < a.S) wrow[key + e] = m.accumulate ? wrow[key + e] + v[e] : v[e];
            }
        }
    };
    if (!m.accumulate) {                                        // tiles of the range that no row of the workgroup sees
        for (int kv0 = r_beg; kv0 < r_end; kv0 += BKV)
            if (kv0 < c_beg || kv0 >= c_end) put(kv0, nullptr);
    }
    const int ntile = c_beg < c_end ? (c_end - c_beg + BKV - 1) / BKV : 0, total = ntile * a.H;      // workgroup-uniform
    if (total == 0) return;

    // step `it` = (tile it / H, head it % H): its K rows, key bias, Q fragments and lse, loaded one step ahead
    RowTile<T, HD, BKV> kt;
    float bias_r = 0.f, lse_r = 0.f;
    F qraw[NKS];
    auto prefetch = [&](int it) {
        const int h = it % a.H, kv0 = c_beg + (it / a.H) * BKV;
        kt.load(K + h * HD, a.ldk, kv0, S, tid);
        if (tid < BKV) bias_r = a.key_bias ? a.key_bias[(long)b * a.S + min(kv0 + tid, S - 1)] * LOG2E : 0.f;      // keys >= S: masked
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
            qraw[ks] = q < a.T ? *reinterpret_cast<const F*>(Q + (long)q * a.ldq + h * HD + ks * KS + hh * VEC) : frag_zero<T>();
        lse_r = q < a.T ? a.lse[((long)b * a.H + h) * a.T + q] : 0.f;
    };
    if (tid == 0) Ka[BKV] = frag_zero<T>();
    prefetch(0);

    f32x16 wacc[2];
    for (int it = 0; it < total; ++it) {
        const int h = it % a.H, kv0 = c_beg + (it / a.H) * BKV;
        __syncthreads();
        kt.template store<PK>(Ks, tid);
        if (tid < BKV) Ka[tid] = Aug<T>::x(bias_r);
        F qf[NKS];                                              // Q * scale * log2 e, rounded to T as the forward rounds it
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int e = 0; e < VEC; ++e) qf[ks][e] = from_f32<T>(to_f32(qraw[ks][e]) * sc2);
        float lse2 = lse_r * LOG2E;
        const bool dead = !(lse2 > -INFINITY);                  // a row without a visible key (the forward's lse = -inf): zeros
        if (dead) lse2 = 0.f;
        __syncthreads();
        if (it + 1 < total) prefetch(it + 1);

        int lq = -1, lkv = 0;
        if (a.blk_lq) { const int bb = (b * a.H + h) % a.B; lq = a.blk_lq[bb]; lkv = a.blk_lkv[bb]; }
        int vis_lo; unsigned vis_span;
        visible_keys(a, q, S, lq, lkv, vis_lo, vis_span);
        if (dead) vis_span = 0;
        const F qa = hh ? frag_zero<T>() : Aug<T>::y(-lse2);    // query side of the score chain: minus the row's log-sum-exp

        // P^T = exp2(K Q~^T + bias - lse): keys on the register axis, lane = query
        f32x16 st[2];
        {
            F kfr[2][NKS + 1];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
                for (int r = 0; r < 16; ++r) st[mb][r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks)
                    kfr[mb][ks] = *reinterpret_cast<const F*>(&Ks[(mb * 32 + (lane & 31)) * PK + ks * KS + hh * VEC]);
                kfr[mb][NKS] = Ka[hh ? BKV : mb * 32 + (lane & 31)];
            }
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) mma32(st[mb], kfr[mb][ks], qf[ks]);
                mma32(st[mb], kfr[mb][NKS], qa);
            }
        }
        uint64_t w0[16], w1[16];
        if constexpr (DROP) {                                   // the words of this (head, 32 queries, 64 keys) tile, as the forward reads them
            const uint64_t* wp = dmask + drop_word_base(a, b * a.H + h, qw0 >> 5, kv0 >> 6);
#pragma unroll
            for (int r = 0; r < 16; ++r) { w0[r] = wp[r]; w1[r] = wp[16 + r]; }
        }
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[mb][r] = __builtin_amdgcn_exp2f(st[mb][r]);
        const bool full = (kv0 + BKV <= S) && (qw0 + 32 <= a.T) && lq < 0 &&
                          (!a.causal || (kv0 + BKV - 1 <= qw0 && (!win_on || kv0 >= qw0 + 31 - a.window)));
        if (!full || __builtin_amdgcn_ballot_w64(dead) != 0) {
            const int rel = kv0 + 4 * hh - vis_lo;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) st[mb][r] = (unsigned)(rel + mb * 32 + acc_row(r, 0)) < vis_span ? st[mb][r] : 0.f;
        }
        if constexpr (DROP) {                                   // the select feeds the VALU add below, never an MFMA
#pragma unroll
            for (int r = 0; r < 16; ++r) st[0][r] = keep_or_zero<true>(st[0][r], w0[r], lane);
#pragma unroll
            for (int r = 0; r < 16; ++r) st[1][r] = keep_or_zero<true>(st[1][r], w1[r], lane);
        }
        if (h == 0) { wacc[0] = st[0]; wacc[1] = st[1]; }
        else { wacc[0] += st[0]; wacc[1] += st[1]; }
        if (h == a.H - 1) {
            wacc[0] *= m.scale; wacc[1] *= m.scale;
            put(kv0, wacc);
        }
    }
}

// Keys per workgroup: whole 64-key tiles, as few as still give ~4 workgroups per CU -- a workgroup reuses nothing from one tile
// to the next (the Q fragments come back from cache), so shorter ranges only add parallelism.  OMR_ATTN_MAP_MIN_WG (experiment /
// test knob like OMR_ATTN_MIN_WG, default 1024; read at every call, nothing else plans with it): 1 = one workgroup walks all S keys
// of its query block.  The result does not depend on it (one owner per element either way).
int choose_range(int B, int T, int S) {
    const char* env = getenv("OMR_ATTN_MAP_MIN_WG");
    const long min_wg = env && atol(env) > 0 ? atol(env) : 1024;
    const long blocks = (long)B * ((T + 127) / 128);
    const int ntile = (S + 63) / 64;
    long want = (min_wg + blocks - 1) / blocks;
    if (want > ntile) want = ntile;
    if (want < 1) want = 1;
    return (int)((ntile + want - 1) / want) * 64;
}

template <typename T, int HD> int run_weights(const AttnArgs& a, const MapOut& m, const int* kv_len, hipStream_t s) {
    const long gx = (long)cdiv(a.T, 128) * cdiv(a.S, m.range_len);
    if (gx > 0x7fffffffL) return OMR_ERR_ARG;
    const dim3 grid((unsigned)gx, 1, (unsigned)a.B);
    if (a.drop_thresh) hipLaunchKernelGGL((attn_weights_kernel<T, HD, true>), grid, dim3(256), 0, s, a, m, a.dmask, kv_len);
    else hipLaunchKernelGGL((attn_weights_kernel<T, HD, false>), grid, dim3(256), 0, s, a, m, a.dmask, kv_len);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

}  // namespace

extern "C" long omr_attn_weights_range(int B, int T, int S) {
    if (B <= 0 || T <= 0 || S <= 0) return 0;
    return choose_range(B, T, S);
}

extern "C" int omr_attn_weights(int dtype, const void* q, const void* k, const float* lse, float* w, long ldq, long ldk, long ldw, long bsq, long bsk,
                                long bsw, int B, int H, int T, int S, int head_dim, int causal, int window, const float* key_bias,
                                const int* blk_lq, const int* blk_lkv, const int* kv_len, float dropout_p, const unsigned long long* drop_words,
                                float out_scale, int accumulate, void* stream) {
    if (dtype != OMR_F32 && dtype != OMR_BF16) return OMR_ERR_UNSUPPORTED;
    AttnArgs a = {};
    int rc = fill_common(a, B, H, T, S, head_dim, dropout_p, 0, causal, window, key_bias, blk_lq, blk_lkv, drop_words, true);
    if (rc) return rc;
    if (!q || !k || !lse || !w) return OMR_ERR_ARG;
    const int vec = dtype == OMR_BF16 ? 8 : 4;                  // q and k rows are read as 16-byte fragments
    if (ldq % vec || ldk % vec || bsq % vec || bsk % vec || ((uintptr_t)q | (uintptr_t)k) % 16 || (uintptr_t)w % 4 || (uintptr_t)lse % 4)
        return OMR_ERR_ARG;
    const long d = (long)H * head_dim;
    if (ldq < d || ldk < d || ldw < S) return OMR_ERR_ARG;
    // int indices in the kernel: rows of lse, the key_bias row, the dropout-word index; grid z
    if ((long)B * H * T > 0x7fffffffL || (long)B * S > 0x7fffffffL || B > 65535) return OMR_ERR_ARG;
    a.q = q; a.k = k; a.ldq = ldq; a.ldk = ldk; a.bsq = bsq; a.bsk = bsk;
    a.lse = const_cast<float*>(lse);                            // read only
    MapOut m;
    m.w = w; m.ldw = ldw; m.bsw = bsw;
    m.scale = a.drop_thresh ? out_scale * a.drop_scale : out_scale;
    m.accumulate = accumulate ? 1 : 0;
    m.vec4 = ((uintptr_t)w % 16 == 0 && ldw % 4 == 0 && bsw % 4 == 0) ? 1 : 0;
    m.range_len = choose_range(B, T, S);
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T(dtype, DISPATCH_HD(head_dim, return (run_weights<T, HD>(a, m, kv_len, s))))
}
