// Fused multi-head attention (flash style: scores never leave the chip) for gfx950: the forward.  Backward: attention_bwd.hip;
// the pieces both share: attn_common.h.
// Reference math: torch nn/functional.py multi_head_attention_forward as used by
//   nn.TransformerDecoderLayer self/cross attention (decoder.py:86-95) and CrossAttention (model.py:289-355):
//   P = softmax(Q K^T / sqrt(hd) + bias), O = dropout(P) V, heads = contiguous hd-wide channel slices.
// Mask semantics reproduced exactly:
//   * key_bias[b][key]  : ADDED to the score.  Float padding masks add +1.0 (quirk 1); bool masks arrive as -inf.
//   * causal / window   : key <= q, and key >= q - window when 0 < window < T (decoder.py:191-217).
//   * block mask        : score = -inf where q >= lq[b'] and key >= lkv[b'] with b' = (b*H + h) % B (quirk 2, model.py:349-354).
//
// Data flow per wave (32 query rows), keys on the MFMA M dimension so that each LANE owns one query row:
//   S^T = K . Q^T        (A = K tile from LDS, B = Q fragments held in registers)      -> softmax is lane-local
//   O^T += V^T . P^T     (A = V^T tile from LDS, B = P^T straight from the accumulator registers, permuted-k order)
// Backward: dQ kernel (same orientation) and dK/dV kernel (queries on the register axis, keys on the lanes).
#include "attn_common.h"

namespace {
using namespace attn;

// ------------------------------------------------------------------------------------------------
// Forward.  grid = (ceil(T/128), H, B); wave w owns query rows q0 + 32w .. +31; KV tiles of 64 keys.
// SPLITW (T <= 32: KV-cached greedy decode, one query row): the four waves would own the same 32 rows, so they split the KEYS
// instead -- 256 keys are staged per step, wave w takes keys [64w, 64w+64) of them -- and their (max, sum, O) partials are
// merged through LDS at the end.  Same arithmetic per score, a quarter of the serial tile walk.
// kv_len (SPLITW only, nullable): batch row b attends over keys [0, kv_len[b]) of its padded S (a ragged batch of decode
// memories).  Every key bound below is that row's; a key split or wave past it walks nothing and leaves (O 0, max -inf,
// sum 0), which both mergers weigh with 0.  The tile loads clamp to the row's last key, so nothing past it is ever read.
// kv_start (SPLITW only, nullable): row b's keys begin at row kv_start[b] of its K / V slot (per-row positions of a decode state
// with slots: the banded self-attention window [lo_b, t_b]); key j of the row, its key_bias entry included, is slot row
// kv_start[b] + j, and nothing before the start is read either.
template <typename T, int HD, bool SPLITW, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(AttnArgs a, const uint64_t* __restrict__ dmask, const int* __restrict__ kv_len,
                                                          const int* __restrict__ kv_start) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = ACfg<T>::VEC, NFR = ACfg<T>::NFR, KS = KStep<T>::value;
    constexpr int NKS = HD / KS, NDB = HD / 32, BKV = 64;
    constexpr int NTL = SPLITW ? 4 : 1, BST = BKV * NTL;        // keys staged per step
    constexpr int PK = HD + VEC;          // Ks pitch
    constexpr int PV = BST + 4;   // Vt pitch: 136 B (bf16) / 272 B (fp32) -> conflict-free permuted reads
    constexpr float THR = 8.f;            // the reference maximum of a row moves when a tile exceeds it by 2^THR
    constexpr bool TRD = std::is_same<T, bf16>::value;          // bf16: V is staged row-major and read with tr reads
    // bf16, query-per-wave form: the staged tiles are DOUBLE-BUFFERED -- tile t+1 is committed to the other buffer before the math on
    // tile t, so one workgroup barrier per tile orders both "t+1 is complete" and "everybody is done with t" (was two)
    constexpr int NBUF = (TRD && !SPLITW) ? 2 : 1;
    __shared__ __attribute__((aligned(16))) T Ks_[NBUF][BST * PK];
    __shared__ __attribute__((aligned(16))) T Vt[TRD ? 8 : HD * PV];
    __shared__ __attribute__((aligned(16))) T Vs_[NBUF][TRD ? BST * PK : 8];
    __shared__ __attribute__((aligned(16))) F Ka_[NBUF][BST + 1];      // augmented k-step, key side: the key bias; entry BST = zeros

    const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // blockIdx.x = key split (SPLITW: one query block) or query block + nqb * key split
    const int nqb = SPLITW ? 1 : (a.T + 127) / 128;
    const int ksplit = blockIdx.x / nqb, q0 = (blockIdx.x % nqb) * 128;
    const int b = blockIdx.z, h = blockIdx.y;
    const int qw0 = q0 + (SPLITW ? 0 : wave * 32);              // first query row of this wave
    const int q = qw0 + (lane & 31);
    const int kboff = SPLITW ? wave * BKV : 0;                  // this wave's keys inside the staged block
    const T* Q = (const T*)a.q + (long)b * a.bsq + h * HD;
    const int bk = SPLITW ? b / a.kv_group : b;                 // K|V slot of this row (beam search: the hypotheses of an input share one)
    const T* K = (const T*)a.k + (long)bk * a.bsk + h * HD;
    const T* V = (const T*)a.v + (long)bk * a.bsv + h * HD;
    int S = a.S;                                                // this row's key count (never past the padded S; <= 0: no keys)
    if constexpr (SPLITW) {
        const int bt = a.kv_row_tables ? b : bk;                // uniform: a grouped decode position keeps its tables per row
        if (kv_len) S = min(kv_len[bt], a.S);
        if (kv_start) { const long first = max(kv_start[bt], 0); K += first * a.ldk; V += first * a.ldv; }
    }

    const float sc2 = a.scale * LOG2E;
    F qf[NKS];                                                  // Q * scale * log2 e
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const F raw = q < a.T ? *reinterpret_cast<const F*>(Q + (long)q * a.ldq + ks * KS + hh * VEC) : frag_zero<T>();
#pragma unroll
        for (int e = 0; e < VEC; ++e) qf[ks][e] = from_f32<T>(to_f32(raw[e]) * sc2);
    }
    int lq = -1, lkv = 0;
    if (a.blk_lq) { const int bb = (b * a.H + h) % a.B; lq = a.blk_lq[bb]; lkv = a.blk_lkv[bb]; }
    int vis_lo; unsigned vis_span;
    visible_keys(a, q, S, lq, lkv, vis_lo, vis_span);

    f32x16 acc_o[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_o[d][r] = 0.f;
    // m_ref: the row's reference maximum (log2 domain; exactly representable in T, so that one slot of the augmented k-step
    // subtracts it without rounding); meaningless until m_set
    float m_ref = 0.f, l_run = 0.f;
    bool m_set = false;
    F qa = hh ? frag_zero<T>() : Aug<T>::y(0.f);
    const bool win_on = a.window > 0 && a.window < a.T;

    int kv_beg = 0, kv_end = S;
    if (a.causal) {
        kv_end = min(S, q0 + 128);
        if (a.window > 0 && a.window < a.T) kv_beg = max(0, q0 - a.window) / BKV * BKV;
    }
    if (a.nsplit > 1) { kv_beg = max(kv_beg, ksplit * a.split_len); kv_end = min(kv_end, (ksplit + 1) * a.split_len); }
    RowTile<T, HD, BST> kt, vt;
    float bias_r = 0.f;
    auto prefetch = [&](int kvb) {
        kt.load(K, a.ldk, kvb, S, tid);
        vt.load(V, a.ldv, kvb, S, tid);
        if (tid < BST) bias_r = a.key_bias ? a.key_bias[(long)b * a.S + min(kvb + tid, S - 1)] * LOG2E : 0.f;     // keys >= S: masked
    };
    if (tid < NBUF) Ka_[tid][BST] = frag_zero<T>();
    auto commit = [&](int buf) {
        kt.template store<PK>(Ks_[buf], tid);
        if constexpr (TRD) vt.template store<PK>(Vs_[buf], tid);
        else vt.template store_t<PV>(Vt, tid);
        if (tid < BST) Ka_[buf][tid] = Aug<T>::x(bias_r);
    };
    if (kv_beg < kv_end) prefetch(kv_beg);
    if constexpr (NBUF == 2) {
        if (kv_beg < kv_end) {
            commit(0);
            if (kv_beg + BST < kv_end) prefetch(kv_beg + BST);
        }
        __syncthreads();
    }
    int buf = 0;
    for (int kvb = kv_beg; kvb < kv_end; kvb += BST) {
        if constexpr (NBUF == 2) {
            // tile kvb sits complete in buffer `buf` (the barrier that ended the previous iteration); the next tile's registers go into
            // the other buffer, which everybody left at that barrier, and the loads of the tile after it start
            if (kvb + BST < kv_end) {
                commit(buf ^ 1);
                if (kvb + 2 * BST < kv_end) prefetch(kvb + 2 * BST);
            }
        } else {
            __syncthreads();
            commit(0);
            __syncthreads();
            if (kvb + BST < kv_end) prefetch(kvb + BST);
        }
        T* const Ks = Ks_[buf];
        T* const Vs = Vs_[buf];
        F* const Ka = Ka_[buf];
        const int kv0 = kvb + kboff;                            // first key of this wave's 64-key tile
        const uint64_t* wp = DROP ? dmask + drop_word_base(a, b * a.H + h, qw0 >> 5, min(kv0, a.S - 1) >> 6) : nullptr;

        // scores in the log2 domain, already relative to the row's reference:  s * scale * log2 e + bias - m_ref
        f32x16 st[2];
        {   // every LDS operand of the two score chains is requested before the first MFMA (one LDS latency, counted waits)
            F kfr[2][NKS + 1];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
                for (int r = 0; r < 16; ++r) st[mb][r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks)
                    kfr[mb][ks] = *reinterpret_cast<const F*>(&Ks[(kboff + mb * 32 + (lane & 31)) * PK + ks * KS + hh * VEC]);
                kfr[mb][NKS] = Ka[hh ? BST : kboff + mb * 32 + (lane & 31)];
            }
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * (NKS + 1), 0);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) mma32(st[mb], kfr[mb][ks], qf[ks]);
                mma32(st[mb], kfr[mb][NKS], qa);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * (NKS + 1) * ACfg<T>::MPI, 0);
        }
        // The tile's dropout words are requested HERE: scalar loads share lgkmcnt with the LDS reads and return out of order, so
        // the next wait on an LDS operand also waits for them -- behind the score chain the next LDS read is the first V
        // fragment, a whole softmax (~450 issue cycles) away, and the words land under the max / exp2 / sum code.
        uint64_t w0[16], w1[16];
        if constexpr (DROP) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) { w0[r] = wp[r]; w1[r] = wp[16 + r]; }
            __builtin_amdgcn_sched_barrier(0);
        }
        // Tiles that are entirely visible for this wave's 32 query rows (the common case) skip every per-element mask test.
        const bool full = (kv0 + BKV <= S) && (qw0 + 32 <= a.T) && lq < 0 &&
                          (!a.causal || (kv0 + BKV - 1 <= qw0 && (!win_on || kv0 >= qw0 + 31 - a.window)));
        if (!full) {
            const int rel = kv0 + 4 * hh - vis_lo;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    st[mb][r] = (unsigned)(rel + mb * 32 + acc_row(r, 0)) < vis_span ? st[mb][r] : -INFINITY;
        }
        float mx = fmaxf(st[0][0], st[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(fmaxf(mx, st[0][r]), st[1][r]);
        mx = max_halves(mx);
        const bool fix = m_set ? (mx > THR) : (mx > -INFINITY);   // the same for both lanes of a row
        if (__builtin_amdgcn_ballot_w64(fix) != 0) {              // rare: first tile of a row, or its maximum grew past the threshold
            const float m2 = fix ? to_f32(from_f32<T>(m_ref + mx)) : m_ref;
            const float delta = m2 - m_ref;
            const float alpha = (fix && m_set) ? __builtin_amdgcn_exp2f(-delta) : 1.f;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) st[mb][r] -= delta;
            l_run *= alpha;
#pragma unroll
            for (int d = 0; d < NDB; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc_o[d][r] *= alpha;
            m_ref = m2;
            m_set = m_set || fix;
            qa = hh ? frag_zero<T>() : Aug<T>::y(-m_ref);
        }
        float psum = 0.f;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(st[mb][r]);          // exp2(-inf) = 0 for masked keys
                psum += pv;
                st[mb][r] = pv;
            }
        l_run += psum;
        if constexpr (DROP) {
            constexpr bool P_IS_CONVERTED = std::is_same<T, bf16>::value;      // acc_to_frag below: a VALU conversion only for bf16
#pragma unroll
            for (int r = 0; r < 16; ++r) st[0][r] = keep_or_zero<P_IS_CONVERTED>(st[0][r], w0[r], lane);
#pragma unroll
            for (int r = 0; r < 16; ++r) st[1][r] = keep_or_zero<P_IS_CONVERTED>(st[1][r], w1[r], lane);
        }
        // O^T += V^T . P^T
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int s = 0; s < NFR; ++s) {
                const F pf = acc_to_frag<T>(st[mb], s);
#pragma unroll
                for (int d = 0; d < NDB; ++d) {
                    const F vf = kperm_frag<T>(Vs, PK, Vt, PV, kboff + mb * 32, s, d * 32, lane);
                    mma32(acc_o[d], vf, pf);
                }
            }
        if constexpr (NBUF == 2) { __syncthreads(); buf ^= 1; }
    }
    float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    float m_fin = l_tot > 0.f ? m_ref : -INFINITY;              // a row that saw no finite score has no reference
    if constexpr (SPLITW) {
        // merge the four waves' partial softmaxes of the same 32 query rows (log2 domain): the staging tiles are dead
        __syncthreads();
        float* o_s = reinterpret_cast<float*>(Ks_[0]);              // [4][HD][32]
        float* m_s = o_s + 4 * HD * 32;                         // [4][32]
        float* l_s = m_s + 4 * 32;
        static_assert((4 * HD * 32 + 8 * 32) * sizeof(float) <= sizeof(T) * BST * PK, "merge scratch fits in the K tile");
        const int qi = lane & 31;
#pragma unroll
        for (int d = 0; d < NDB; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) o_s[(wave * HD + d * 32 + acc_row(r, lane)) * 32 + qi] = acc_o[d][r];
        if (hh == 0) { m_s[wave * 32 + qi] = m_fin; l_s[wave * 32 + qi] = l_tot; }
        __syncthreads();
        if (wave != 0) return;
        float mm = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) mm = fmaxf(mm, m_s[w * 32 + qi]);
        float wsc[4];
        l_tot = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float mw = m_s[w * 32 + qi];
            wsc[w] = mw == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw - mm);
            l_tot += l_s[w * 32 + qi] * wsc[w];
        }
        m_fin = mm;
#pragma unroll
        for (int d = 0; d < NDB; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) v += o_s[(w * HD + d * 32 + acc_row(r, lane)) * 32 + qi] * wsc[w];
                acc_o[d][r] = v;
            }
    }
    if (a.nsplit > 1) {          // partial softmax of this key split: un-normalised O, reference maximum (log2 domain) and sum
        if (q < a.T) {
            float* P = a.part + ((((long)b * a.H + h) * a.nsplit + ksplit) * a.T + q) * (HD + 2);
#pragma unroll
            for (int d = 0; d < NDB; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) P[d * 32 + acc_row(r, lane)] = acc_o[d][r];
            if (hh == 0) { P[HD] = m_fin; P[HD + 1] = l_tot; }
        }
        return;
    }
    const float inv = l_tot > 0.f ? a.drop_scale / l_tot : 0.f;      // dropout rescale folded in (1 when p = 0)
    if (q < a.T) {
        T* O = (T*)a.o + (long)b * a.bso + (long)q * a.ldo + h * HD;
#pragma unroll
        for (int d = 0; d < NDB; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) O[d * 32 + acc_row(r, lane)] = from_f32<T>(acc_o[d][r] * inv);
        if (hh == 0 && a.lse) a.lse[((long)b * a.H + h) * a.T + q] = (l_tot > 0.f) ? (m_fin + log2f(l_tot)) * LN2 : -INFINITY;
    }
}

// Merge of the key-split partials (same arithmetic as the in-kernel merge of the four waves): one 64-thread block per
// (b, h, q), thread = output channel.
template <typename T, int HD>
__global__ __launch_bounds__(64) void attn_split_merge_kernel(AttnArgs a) {
    const int q = blockIdx.x % a.T, bh = blockIdx.x / a.T, h = bh % a.H, b = bh / a.H, dch = threadIdx.x;
    const float* P = a.part + (((long)bh * a.nsplit) * a.T + q) * (HD + 2);
    const long pstride = (long)a.T * (HD + 2);
    float mm = -INFINITY;
    for (int j = 0; j < a.nsplit; ++j) mm = fmaxf(mm, P[j * pstride + HD]);
    float l_tot = 0.f, o = 0.f;
    for (int j = 0; j < a.nsplit; ++j) {
        const float mj = P[j * pstride + HD];
        const float wj = mj == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mj - mm);
        l_tot += P[j * pstride + HD + 1] * wj;
        if (dch < HD) o += P[j * pstride + dch] * wj;
    }
    const float inv = l_tot > 0.f ? a.drop_scale / l_tot : 0.f;
    if (dch < HD) ((T*)a.o)[(long)b * a.bso + (long)q * a.ldo + h * HD + dch] = from_f32<T>(o * inv);
    if (dch == 0 && a.lse) a.lse[((long)b * a.H + h) * a.T + q] = (l_tot > 0.f) ? (mm + log2f(l_tot)) * LN2 : -INFINITY;
}

// Debug / test entry: materialise the keep-mask the three kernels above regenerate on the fly (1 = kept), one byte per score.
__global__ void attn_dropout_mask_kernel(unsigned char* __restrict__ out, AttnArgs a) {
    const long n = (long)a.B * a.H * a.T * a.S;
    const uint32_t s2 = (uint32_t)(a.S + 1) >> 1, thr32 = a.drop_thresh << 16;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int key = (int)(i % a.S); long r = i / a.S;
        const int q = (int)(r % a.T); r /= a.T;
        const int h = (int)(r % a.H), b = (int)(r / a.H);
        const uint32_t x = attn_rand2(attn_bh_key(a, b, h), (uint32_t)q * s2 + (uint32_t)(key >> 1));
        out[i] = (a.drop_thresh == 0 || ((key & 1) ? attn_keep_hi(x, thr32) : attn_keep_lo(x, thr32))) ? 1 : 0;
    }
}

// The keep bits in the kernels' word layout (drop_word_base): one wave per (b, h, 32-query block, 64-key tile) evaluates the
// pair hash in the forward kernel's lane layout (lane = query + 32 * k-half, register = key) and turns each register's
// comparison into its 64-bit lane mask -- v_cmp writes exactly that word.
__global__ __launch_bounds__(256) void attn_dropout_words_kernel(uint64_t* __restrict__ out, AttnArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5;
    const int nkt = (a.S + 63) >> 6, kt = blockIdx.x * 4 + wave;
    if (kt >= nkt) return;                                       // wave-uniform
    const int qb32 = blockIdx.y, bh = blockIdx.z;
    const uint32_t bh_key = hash32((uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)bh);
    const uint32_t s2 = (uint32_t)(a.S + 1) >> 1, thr32 = a.drop_thresh << 16;
    const uint32_t pbase = (uint32_t)(qb32 * 32 + (lane & 31)) * s2 + (uint32_t)((kt * 64 + 4 * hh) >> 1);
    uint64_t mine = 0;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int j = 0; j < 8; ++j) {     // registers 2j, 2j+1 of a block are adjacent keys: one hash per pair
            const uint32_t x = attn_rand2(bh_key, pbase + (uint32_t)((mb * 32 + acc_row(2 * j, 0)) >> 1));
            const uint64_t w0 = __builtin_amdgcn_ballot_w64(attn_keep_lo(x, thr32));
            const uint64_t w1 = __builtin_amdgcn_ballot_w64(attn_keep_hi(x, thr32));
            if (lane == mb * 16 + 2 * j) mine = w0;
            if (lane == mb * 16 + 2 * j + 1) mine = w1;
        }
    if (lane < 32) out[drop_word_base(a, bh, qb32, kt) + lane] = mine;
}

// A single 32-row query block with more keys than one tile (KV-cached decode) takes the SPLITW kernel: the keys go over the
// waves (and, with a workspace, over workgroups).  Inference only: a training forward with dropout and T <= 32 takes the
// query-per-wave kernel.
bool takes_decode_kernel(const AttnArgs& a) { return a.T <= 32 && a.S > 64 && !a.drop_thresh; }

// force_split: the key-split kernel whatever S is (omr_attn_fwd_split_rows: rows of at most 64 keys beside longer ones)
template <typename T, int HD> int run_fwd(const AttnArgs& a, hipStream_t s, bool merge, const int* kv_len, const int* kv_start, bool force_split) {
    const int nsplit = a.nsplit > 1 ? a.nsplit : 1;
    if (force_split || takes_decode_kernel(a)) {
        hipLaunchKernelGGL((attn_fwd_kernel<T, HD, true, false>), dim3(nsplit, a.H, a.B), dim3(256), 0, s, a, a.dmask, kv_len, kv_start);
    } else {
        if (kv_len) return OMR_ERR_UNSUPPORTED;                // per-row key counts: the key-split kernel above only
        const dim3 grid(cdiv(a.T, 128) * nsplit, a.H, a.B);
        if (a.drop_thresh) hipLaunchKernelGGL((attn_fwd_kernel<T, HD, false, true>), grid, dim3(256), 0, s, a, a.dmask, (const int*)nullptr, (const int*)nullptr);
        else hipLaunchKernelGGL((attn_fwd_kernel<T, HD, false, false>), grid, dim3(256), 0, s, a, a.dmask, (const int*)nullptr, (const int*)nullptr);
        merge = true;                                          // partials of this kernel are always merged here
    }
    if (a.nsplit > 1 && merge) hipLaunchKernelGGL((attn_split_merge_kernel<T, HD>), dim3(a.B * a.H * a.T), dim3(64), 0, s, a);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

// Every forward entry point.  nsplit_out: the caller merges the key-split partials itself (decode.hip) and is told how many
// there are; kv_len / kv_start / kv_group: see attn_fwd_kernel.  rows: the per-row-window form (omr_attn_fwd_split_rows), which takes
// the key-split kernel for every S.
int attn_fwd_impl(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv, long ldo,
                  long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim, int causal, int window,
                  const float* key_bias, const int* blk_lq, const int* blk_lkv, float dropout_p, unsigned long long seed,
                  const unsigned long long* drop_words, float* split_ws, long split_ws_floats, void* stream, int* nsplit_out = nullptr,
                  const int* kv_len = nullptr, int kv_group = 1, const int* kv_start = nullptr, bool rows = false, bool row_tables = false) {
    AttnArgs a = {};
    int rc = fill_common(a, B, H, T, S, head_dim, dropout_p, seed, causal, window, key_bias, blk_lq, blk_lkv, drop_words, true);
    if (rc) return rc;
    rc = fill_qkvo(a, dtype, q, k, v, o, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso);
    if (rc || ldo % 4) return OMR_ERR_ARG;
    a.lse = lse; a.kv_group = kv_group; a.kv_row_tables = row_tables;
    if (kv_group < 1 || B % kv_group) return OMR_ERR_ARG;
    if (row_tables && !(rows && kv_len && kv_start)) return OMR_ERR_ARG;
    rc = plan_split(a, head_dim, split_ws, split_ws_floats, fwd_split_floats);
    if (rc) return rc;
    // per-row key counts exist only in the key-split decode kernel: a shape that would not take it is refused, not run unmasked
    if (rows && (T > 32 || a.drop_thresh || causal || blk_lq)) return OMR_ERR_ARG;
    const bool split_kernel = rows || takes_decode_kernel(a);
    if ((kv_len || kv_start || kv_group != 1) && !(split_kernel && !causal && !blk_lq)) return OMR_ERR_UNSUPPORTED;
    const bool merge = nsplit_out == nullptr;           // a caller that asks for the split count merges the partials itself
    // only that kernel leaves partials (its rule also asks for "no dropout", which is immaterial here: no entry point passes both
    // nsplit_out and dropout)
    if (!merge && !split_kernel) { a.nsplit = 1; a.split_len = 0; a.part = nullptr; }
    if (nsplit_out) *nsplit_out = a.nsplit;
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T(dtype, DISPATCH_HD(head_dim, return (run_fwd<T, HD>(a, s, merge, kv_len, kv_start, rows))))
}

}  // namespace

int attn::min_workgroups() { static const int min_wg = getenv("OMR_ATTN_MIN_WG") ? atoi(getenv("OMR_ATTN_MIN_WG")) : 512; return min_wg; }

extern "C" int omr_attn_dropout_mask(unsigned char* mask, int B, int H, int T, int S, float dropout_p, unsigned long long seed, void* stream) {
    AttnArgs a = {};
    int rc = fill_common(a, B, H, T, S, 64, dropout_p, seed, 0, -1, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (!mask) return OMR_ERR_ARG;
    const long n = (long)B * H * T * S;
    long g = (n + 255) / 256; if (g > 4096) g = 4096;
    hipLaunchKernelGGL(attn_dropout_mask_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, mask, a);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" long omr_attn_dropout_words_count(int B, int H, int T, int S) {
    if (B <= 0 || H <= 0 || T <= 0 || S <= 0) return 0;
    return (long)B * H * ((T + 31) / 32) * ((S + 63) / 64) * 32;
}

extern "C" int omr_attn_dropout_words(unsigned long long* words, int B, int H, int T, int S, float dropout_p, unsigned long long seed, void* stream) {
    AttnArgs a = {};
    int rc = fill_common(a, B, H, T, S, 64, dropout_p, seed, 0, -1, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (!words || a.drop_thresh == 0) return OMR_ERR_ARG;
    const dim3 grid((unsigned)(((S + 63) / 64 + 3) / 4), (unsigned)((T + 31) / 32), (unsigned)(B * H));
    hipLaunchKernelGGL(attn_dropout_words_kernel, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<uint64_t*>(words), a);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

/* floats of scratch omr_attn_fwd_ws / omr_attn_bwd_ws want for a shape (0: the shape is not split) */
extern "C" long omr_attn_workspace_floats(int B, int H, int T, int S, int head_dim, int causal, int backward) {
    if (B <= 0 || H <= 0 || T <= 0 || S <= 0) return 0;
    int nsplit, len;
    choose_split(B, H, T, S, causal, &nsplit, &len);
    if (nsplit <= 1) return 0;
    return (backward ? dq_split_floats : fwd_split_floats)(B, H, T, head_dim, nsplit);
}

/* omr_attn_fwd with caller-provided scratch for the key split (omr_attn_workspace_floats(..., backward = 0) floats) */
extern "C" int omr_attn_fwd_ws(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv, long ldo,
                               long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim, int causal, int window,
                               const float* key_bias, const int* blk_lq, const int* blk_lkv, float dropout_p, unsigned long long seed,
                               const unsigned long long* drop_words, float* ws, long ws_floats, void* stream) {
    return attn_fwd_impl(dtype, q, k, v, o, lse, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, B, H, T, S, head_dim, causal, window, key_bias, blk_lq, blk_lkv,
                         dropout_p, seed, drop_words, ws, ws_floats, stream);
}

extern "C" int omr_attn_fwd(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv, long ldo,
                            long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim, int causal, int window,
                            const float* key_bias, const int* blk_lq, const int* blk_lkv, float dropout_p, unsigned long long seed,
                            const unsigned long long* drop_words, void* stream) {
    return attn_fwd_impl(dtype, q, k, v, o, lse, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, B, H, T, S, head_dim, causal, window, key_bias, blk_lq, blk_lkv,
                         dropout_p, seed, drop_words, nullptr, 0, stream);
}

/* floats of split workspace omr_attn_fwd_split wants for (B, H, T <= 32, S): partial softmaxes of the key splits */
extern "C" long omr_attn_split_workspace_floats(int B, int H, int T, int S, int head_dim) {
    if (T > 32) return 0;
    return omr_attn_workspace_floats(B, H, T, S, head_dim, 0, 0);
}

/* omr_attn_fwd for a single block of at most 32 query rows (KV-cached decode) with the KEYS split over workgroups of 256 keys
 * each (flash-decoding): one query row otherwise keeps a (batch, head) pair on ONE workgroup that walks all S keys. */
extern "C" int omr_attn_fwd_split(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv, long ldo,
                                  long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim, const float* key_bias,
                                  float* split_ws, long split_ws_floats, void* stream) {
    if (T > 32) return OMR_ERR_ARG;
    return attn_fwd_impl(dtype, q, k, v, o, lse, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, B, H, T, S, head_dim, 0, -1, key_bias, nullptr, nullptr, 0.f, 0,
                         nullptr, split_ws, split_ws_floats, stream);
}

/* omr_attn_fwd_split WITHOUT the merge pass: when the keys were split (*nsplit > 1) `o` is not written and split_ws holds, per
 * (b, h, split j), head_dim un-normalised outputs + running max (log2 domain) + sum at ((b*H + h)*nsplit + j)*T*(head_dim+2);
 * the consumer merges them (omr_decode_linear, prologue 3).  *nsplit = 1: `o` holds the finished rows. */
extern "C" int omr_attn_fwd_split_partials(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv,
                                           long ldo, long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim,
                                           float* split_ws, long split_ws_floats, int* nsplit, void* stream) {
    if (T > 32 || !nsplit) return OMR_ERR_ARG;
    return attn_fwd_impl(dtype, q, k, v, o, lse, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, B, H, T, S, head_dim, 0, -1, nullptr, nullptr, nullptr, 0.f, 0,
                         nullptr, split_ws, split_ws_floats, stream, nsplit);
}

/* omr_attn_fwd_split over a ragged batch: S is the padded key count, row b attends over keys [0, kv_len[b]) (device int32 [B],
 * 1 <= kv_len[b] <= S; NULL = every row sees S).  The split plan stays that of S. */
extern "C" int omr_attn_fwd_split_varlen(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv,
                                         long ldo, long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim,
                                         const float* key_bias, const int* kv_len, float* split_ws, long split_ws_floats, void* stream) {
    if (T > 32) return OMR_ERR_ARG;
    return attn_fwd_impl(dtype, q, k, v, o, lse, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, B, H, T, S, head_dim, 0, -1, key_bias, nullptr, nullptr, 0.f, 0,
                         nullptr, split_ws, split_ws_floats, stream, nullptr, kv_len);
}

/* omr_attn_fwd_split_partials with per-row key counts and shared K|V slots (omr_common.h), for the decode executors (decode.hip).
 * A C++ symbol, not part of the C ABI */
int attn_fwd_split_partials_varlen(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv,
                                   long ldo, long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim,
                                   const int* kv_len, float* split_ws, long split_ws_floats, int* nsplit, void* stream, int kv_group) {
    if (T > 32) return OMR_ERR_ARG;
    return attn_fwd_impl(dtype, q, k, v, o, lse, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, B, H, T, S, head_dim, 0, -1, nullptr, nullptr, nullptr, 0.f, 0,
                         nullptr, split_ws, split_ws_floats, stream, nsplit, kv_len, kv_group);
}

/* omr_attn_fwd_split_varlen with a per-row key START as well: the self-attention of a decode state whose rows sit at their own
 * positions (src/transformer/model.py:171-199 decodes one input at a time; here a finished row's slot goes to the next input).
 * Row b attends over rows [kv_start[b], kv_start[b] + kv_len[b]) of its K / V slot; S is the largest kv_len (the split plan's).
 * Always the key-split kernel, S <= 64 included. */
extern "C" int omr_attn_fwd_split_rows(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv,
                                       long ldo, long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim,
                                       const float* key_bias, const int* kv_len, const int* kv_start, float* split_ws, long split_ws_floats,
                                       void* stream) {
    if (T > 32) return OMR_ERR_ARG;
    return attn_fwd_impl(dtype, q, k, v, o, lse, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, B, H, T, S, head_dim, 0, -1, key_bias, nullptr, nullptr, 0.f, 0,
                         nullptr, split_ws, split_ws_floats, stream, nullptr, kv_len, 1, kv_start, true);
}

/* omr_attn_fwd_split_rows without the merge pass, for the per-row-position decode executor (decode.hip).  A C++ symbol, not part
 * of the C ABI */
int attn_fwd_split_partials_rows(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv,
                                 long ldo, long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim,
                                 const int* kv_len, const int* kv_start, float* split_ws, long split_ws_floats, int* nsplit, void* stream) {
    if (T > 32 || !nsplit) return OMR_ERR_ARG;
    return attn_fwd_impl(dtype, q, k, v, o, lse, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, B, H, T, S, head_dim, 0, -1, nullptr, nullptr, nullptr, 0.f, 0,
                         nullptr, split_ws, split_ws_floats, stream, nsplit, kv_len, 1, kv_start, true);
}

/* attn_fwd_split_partials_rows for a grouped decode position (omr_common.h): the slot from b / group, the key range from row b.  A
 * C++ symbol, not part of the C ABI */
int attn_fwd_split_partials_group(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv,
                                  long ldo, long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim,
                                  const int* kv_len, const int* kv_start, int group, float* split_ws, long split_ws_floats, int* nsplit,
                                  void* stream) {
    if (T > 32 || !nsplit || group < 1) return OMR_ERR_ARG;
    return attn_fwd_impl(dtype, q, k, v, o, lse, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, B, H, T, S, head_dim, 0, -1, nullptr, nullptr, nullptr, 0.f, 0,
                         nullptr, split_ws, split_ws_floats, stream, nsplit, kv_len, group, kv_start, true, true);
}
