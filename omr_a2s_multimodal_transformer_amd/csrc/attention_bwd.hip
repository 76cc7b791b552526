// Fused multi-head attention for gfx950: the backward kernels (dQ; dK and dV) and their entry points.  Forward, reference
// math and mask semantics: attention.hip; the pieces both share (staging, visibility, chains, dropout words): attn_common.h.
#include "attn_common.h"

namespace {
using namespace attn;

// ------------------------------------------------------------------------------------------------
// Backward, dQ.  Same orientation as the forward: lane = query row.  c = 1 / (1 - p_drop), M = keep mask:
//   S'^T = K Q~^T + bias - lse  (augmented k-step) ; P^T = exp2(S'^T) ; dP'^T = V dO^T - delta / c  (augmented k-step)
//   dS^T / c = P^T o (M ? dP'^T : -delta / c) ; dQ^T += K^T dS^T / c ; dQ = scale * c * dQ^T
template <typename T, int HD, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(AttnArgs a, const uint64_t* __restrict__ dmask) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = ACfg<T>::VEC, NFR = ACfg<T>::NFR, KS = KStep<T>::value;
    constexpr int NKS = HD / KS, NDB = HD / 32, BKV = 64;
    constexpr int PK = HD + VEC;
    constexpr int PV = BKV + 4;
    constexpr bool TRD = std::is_same<T, bf16>::value;          // bf16: K^T fragments are tr reads of the row-major Ks tile
    constexpr int NBUF = TRD ? 2 : 1;                           // bf16: double-buffered tiles, one workgroup barrier per tile (see the forward)
    __shared__ __attribute__((aligned(16))) T Ks_[NBUF][BKV * PK];
    __shared__ __attribute__((aligned(16))) T Vs_[NBUF][BKV * PK];
    __shared__ __attribute__((aligned(16))) T Kt[TRD ? 8 : HD * PV];
    __shared__ __attribute__((aligned(16))) F Ka_[NBUF][BKV + 1];      // augmented k-step, key side: the key bias; entry BKV = zeros

    const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nqb = (a.T + 127) / 128;                          // blockIdx.x = query block + nqb * key split
    const int ksplit = blockIdx.x / nqb, q0 = (blockIdx.x % nqb) * 128;
    const int b = blockIdx.z, h = blockIdx.y;
    const int qw0 = q0 + wave * 32;
    const int q = qw0 + (lane & 31);
    const T* Q = (const T*)a.q + (long)b * a.bsq + h * HD;
    const T* K = (const T*)a.k + (long)b * a.bsk + h * HD;
    const T* V = (const T*)a.v + (long)b * a.bsv + h * HD;
    const T* DO = (const T*)a.dout + (long)b * a.bsdo + h * HD;

    const float sc2 = a.scale * LOG2E;
    F qf[NKS], dof[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const F raw = q < a.T ? *reinterpret_cast<const F*>(Q + (long)q * a.ldq + ks * KS + hh * VEC) : frag_zero<T>();
#pragma unroll
        for (int e = 0; e < VEC; ++e) qf[ks][e] = from_f32<T>(to_f32(raw[e]) * sc2);
        dof[ks] = q < a.T ? *reinterpret_cast<const F*>(DO + (long)q * a.lddo + ks * KS + hh * VEC) : frag_zero<T>();
    }
    const long sidx = ((long)b * a.H + h) * a.T + q;
    float lse2 = q < a.T ? a.lse[sidx] * LOG2E : 0.f;
    if (!(lse2 > -INFINITY)) lse2 = 0.f;                        // a row without a visible key: every P is zeroed by its mask below
    // delta[q] = sum_d dO[q][d] * O[q][d] is formed HERE (the two lanes of a row hold the two halves of its d values) and stored for
    // the dK/dV kernel that follows on the stream -- a separate pass over O and dO was a launch of its own per layer
    float dlt = 0.f;
    {
        const T* O = (const T*)a.o + (long)b * a.bso + h * HD;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const F of = q < a.T ? *reinterpret_cast<const F*>(O + (long)q * a.ldo + ks * KS + hh * VEC) : frag_zero<T>();
#pragma unroll
            for (int e = 0; e < VEC; ++e) dlt += to_f32(of[e]) * to_f32(dof[ks][e]);
        }
        dlt += __shfl_xor(dlt, 32, 64);
        if (hh == 0 && q < a.T && ksplit == 0) const_cast<float*>(a.delta)[sidx] = dlt;
    }
    const float ndc = -dlt / a.drop_scale;                      // -delta / c
    const bool win_on = a.window > 0 && a.window < a.T;
    int lq = -1, lkv = 0;
    if (a.blk_lq) { const int bb = (b * a.H + h) % a.B; lq = a.blk_lq[bb]; lkv = a.blk_lkv[bb]; }
    int vis_lo; unsigned vis_span;
    visible_keys(a, q, a.S, lq, lkv, vis_lo, vis_span);
    const F qa = hh ? frag_zero<T>() : Aug<T>::y(-lse2);        // query side of the score chain: minus the row's log-sum-exp
    const F da = hh ? frag_zero<T>() : Aug<T>::y(ndc);          // dO side of the dP chain: minus delta / c
    const F va = hh ? frag_zero<T>() : Aug<T>::x(0.f);          // V side of the dP chain: the unit slots

    f32x16 acc_q[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_q[d][r] = 0.f;

    int kv_beg = 0, kv_end = a.S;
    if (a.causal) {
        kv_end = min(a.S, q0 + 128);
        if (a.window > 0 && a.window < a.T) kv_beg = max(0, q0 - a.window) / BKV * BKV;
    }
    if (a.nsplit > 1) { kv_beg = max(kv_beg, ksplit * a.split_len); kv_end = min(kv_end, (ksplit + 1) * a.split_len); }
    RowTile<T, HD, BKV> kt, vt;
    float bias_r = 0.f;
    auto prefetch = [&](int kv0) {
        kt.load(K, a.ldk, kv0, a.S, tid);
        vt.load(V, a.ldv, kv0, a.S, tid);
        if (tid < BKV) bias_r = a.key_bias ? a.key_bias[(long)b * a.S + min(kv0 + tid, a.S - 1)] * LOG2E : 0.f;     // keys >= S: masked
    };
    if (tid < NBUF) Ka_[tid][BKV] = frag_zero<T>();
    auto commit = [&](int bi) {
        kt.template store<PK>(Ks_[bi], tid);
        vt.template store<PK>(Vs_[bi], tid);
        if constexpr (!TRD) kt.template store_t<PV>(Kt, tid);
        if (tid < BKV) Ka_[bi][tid] = Aug<T>::x(bias_r);
    };
    if (kv_beg < kv_end) prefetch(kv_beg);
    if constexpr (NBUF == 2) {
        if (kv_beg < kv_end) {
            commit(0);
            if (kv_beg + BKV < kv_end) prefetch(kv_beg + BKV);
        }
        __syncthreads();
    }
    int buf = 0;
    for (int kv0 = kv_beg; kv0 < kv_end; kv0 += BKV) {
        if constexpr (NBUF == 2) {
            if (kv0 + BKV < kv_end) {
                commit(buf ^ 1);
                if (kv0 + 2 * BKV < kv_end) prefetch(kv0 + 2 * BKV);
            }
        } else {
            __syncthreads();
            commit(0);
            __syncthreads();
            if (kv0 + BKV < kv_end) prefetch(kv0 + BKV);
        }
        T* const Ks = Ks_[buf];
        T* const Vs = Vs_[buf];
        F* const Ka = Ka_[buf];
        const bool full = (kv0 + BKV <= a.S) && (qw0 + 32 <= a.T) && lq < 0 &&
                          (!a.causal || (kv0 + BKV - 1 <= qw0 && (!win_on || kv0 >= qw0 + 31 - a.window)));
        const uint64_t* wp = DROP ? dmask + drop_word_base(a, b * a.H + h, qw0 >> 5, kv0 >> 6) : nullptr;
        f32x16 st[2], dp[2];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { st[mb][r] = 0.f; dp[mb][r] = 0.f; }
            if constexpr (TRD) {   // the block's LDS operands first, then its two chains (one LDS latency per block, counted waits)
                F kfr[NKS + 1], vfr[NKS];
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    kfr[ks] = *reinterpret_cast<const F*>(&Ks[(mb * 32 + (lane & 31)) * PK + ks * KS + hh * VEC]);
                    vfr[ks] = *reinterpret_cast<const F*>(&Vs[(mb * 32 + (lane & 31)) * PK + ks * KS + hh * VEC]);
                }
                kfr[NKS] = Ka[hh ? BKV : mb * 32 + (lane & 31)];
                __builtin_amdgcn_sched_group_barrier(0x100, 2 * NKS + 1, 0);
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    mma32(st[mb], kfr[ks], qf[ks]);
                    mma32(dp[mb], vfr[ks], dof[ks]);
                }
                mma32(st[mb], kfr[NKS], qa);
                mma32(dp[mb], va, da);
                __builtin_amdgcn_sched_group_barrier(0x008, 2 * NKS + 2, 0);
            } else {               // fp32 (parity mode): the registers do not hold twice the fragments
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const F kf = *reinterpret_cast<const F*>(&Ks[(mb * 32 + (lane & 31)) * PK + ks * KS + hh * VEC]);
                    mma32(st[mb], kf, qf[ks]);
                    const F vf = *reinterpret_cast<const F*>(&Vs[(mb * 32 + (lane & 31)) * PK + ks * KS + hh * VEC]);
                    mma32(dp[mb], vf, dof[ks]);
                }
                mma32(st[mb], Ka[hh ? BKV : mb * 32 + (lane & 31)], qa);
                mma32(dp[mb], va, da);
            }
        }
        // dropout words: requested behind the last LDS operand of the score / dP chains (see the forward kernel), consumed
        // behind the 32 exp2
        uint64_t w0[16], w1[16];
        if constexpr (DROP) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) { w0[r] = wp[r]; w1[r] = wp[16 + r]; }
            __builtin_amdgcn_sched_barrier(0);
        }
        // P^T = exp2(score - lse) (0 where masked); wave-uniform branches keep the common tile free of mask tests
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[mb][r] = __builtin_amdgcn_exp2f(st[mb][r]);
        if (!full) {
            const int rel = kv0 + 4 * hh - vis_lo;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) st[mb][r] = (unsigned)(rel + mb * 32 + acc_row(r, 0)) < vis_span ? st[mb][r] : 0.f;
        }
        if constexpr (DROP) {
#pragma unroll
            for (int r = 0; r < 16; ++r) dp[0][r] = keep_or(dp[0][r], ndc, w0[r]);
#pragma unroll
            for (int r = 0; r < 16; ++r) dp[1][r] = keep_or(dp[1][r], ndc, w1[r]);
        }
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) st[mb][r] *= dp[mb][r];                 // dS^T / c
            if constexpr (TRD) {
                F ktf[NFR][NDB];
#pragma unroll
                for (int s = 0; s < NFR; ++s)
#pragma unroll
                    for (int d = 0; d < NDB; ++d) ktf[s][d] = kperm_frag<T>(Ks, PK, Kt, PV, mb * 32, s, d * 32, lane);
                __builtin_amdgcn_sched_group_barrier(0x100, NFR * NDB * ACfg<T>::RPF, 0);
#pragma unroll
                for (int s = 0; s < NFR; ++s) {
                    const F sf = acc_to_frag<T>(st[mb], s);
#pragma unroll
                    for (int d = 0; d < NDB; ++d) mma32(acc_q[d], ktf[s][d], sf);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, NFR * NDB, 0);
            } else {
#pragma unroll
                for (int s = 0; s < NFR; ++s) {
                    const F sf = acc_to_frag<T>(st[mb], s);
#pragma unroll
                    for (int d = 0; d < NDB; ++d) {
                        const F kf = kperm_frag<T>(Ks, PK, Kt, PV, mb * 32, s, d * 32, lane);
                        mma32(acc_q[d], kf, sf);
                    }
                }
            }
        }
        if constexpr (NBUF == 2) { __syncthreads(); buf ^= 1; }
    }
    const float osc = a.scale * a.drop_scale;
    if (q < a.T) {
        if (a.nsplit > 1) {          // partial dQ of this key split, fp32 [nsplit][B][T][H*HD]: summed by attn_dq_sum_kernel
            float* PQ = a.part + ((((long)ksplit * a.B + b) * a.T + q) * a.H + h) * HD;
#pragma unroll
            for (int d = 0; d < NDB; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) PQ[d * 32 + acc_row(r, lane)] = acc_q[d][r] * osc;
        } else {
            T* DQ = (T*)a.dq + (long)b * a.bsdq + (long)q * a.lddq + h * HD;
#pragma unroll
            for (int d = 0; d < NDB; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) DQ[d * 32 + acc_row(r, lane)] = from_f32<T>(acc_q[d][r] * osc);
        }
    }
}

// dq[b][q][c] = sum over key splits of the fp32 partials (fixed order), c over the H*HD channels
template <typename T>
__global__ void attn_dq_sum_kernel(AttnArgs a, int hd) {
    const long per = (long)a.B * a.T * a.H * hd, cols = (long)a.H * hd;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < per; i += (long)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int j = 0; j < a.nsplit; ++j) s += a.part[j * per + i];
        const long c = i % cols, bq = i / cols, qq = bq % a.T, bb = bq / a.T;
        ((T*)a.dq)[bb * a.bsdq + qq * a.lddq + c] = from_f32<T>(s);
    }
}

// ------------------------------------------------------------------------------------------------
// Backward, dK and dV.  grid = (ceil(S/128), H, B); wave w owns keys k0 + 32w .. +31 (lane = key), queries
// on the register axis:  S' = Q K~^T + bias - lse ; P = exp2(S') ; dP' = dO V^T - delta / c  (both by augmented k-steps)
//   dV += (M o P)^T dO      dK += (dS / c)^T Q,  dS / c = P o (M ? dP' : -delta / c)        (A operand straight from accumulator registers)
// K~ = K * scale * log2 e is rounded to T here while the forward rounds Q * scale * log2 e: in bf16 the recomputed P differs from
// the forward's by the two roundings (a few 1e-3 relative, the size of P's own bf16 rounding); exact in fp32.
template <typename T, int HD, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_kernel(AttnArgs a, const uint64_t* __restrict__ dmask) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = ACfg<T>::VEC, NFR = ACfg<T>::NFR, KS = KStep<T>::value;
    constexpr int NKS = HD / KS, NDB = HD / 32, BQ = 64;
    constexpr int PK = HD + VEC;
    constexpr int PT = BQ + 4;   // transposed tiles [d][q]
    constexpr bool TRD = std::is_same<T, bf16>::value;          // bf16: Q^T / dO^T fragments are tr reads of Qs / Ds
    constexpr int NBUF = TRD ? 2 : 1;                           // bf16: double-buffered tiles, one workgroup barrier per tile (see the forward)
    __shared__ __attribute__((aligned(16))) T Qs_[NBUF][BQ * PK];
    __shared__ __attribute__((aligned(16))) T Ds_[NBUF][BQ * PK];
    __shared__ __attribute__((aligned(16))) T Qt[TRD ? 8 : HD * PT];
    __shared__ __attribute__((aligned(16))) T Dt[TRD ? 8 : HD * PT];
    __shared__ __attribute__((aligned(16))) F Qa_[NBUF][BQ + 1];       // augmented k-step, query side of the score chain: -lse; entry BQ = zeros
    __shared__ __attribute__((aligned(16))) F Da_[NBUF][BQ + 1];       // ... of the dP chain: -delta / c
    __shared__ __attribute__((aligned(16))) float ndc_s_[NBUF][BQ];    // -delta / c per query row (the value a dropped score takes)

    const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.z, h = blockIdx.y, k0 = blockIdx.x * 128;
    const int kw0 = k0 + wave * 32;
    const int key = kw0 + (lane & 31);
    const T* Q = (const T*)a.q + (long)b * a.bsq + h * HD;
    const T* K = (const T*)a.k + (long)b * a.bsk + h * HD;
    const T* V = (const T*)a.v + (long)b * a.bsv + h * HD;
    const T* DO = (const T*)a.dout + (long)b * a.bsdo + h * HD;

    const float sc2 = a.scale * LOG2E;
    F kf[NKS], vf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const F raw = key < a.S ? *reinterpret_cast<const F*>(K + (long)key * a.ldk + ks * KS + hh * VEC) : frag_zero<T>();
#pragma unroll
        for (int e = 0; e < VEC; ++e) kf[ks][e] = from_f32<T>(to_f32(raw[e]) * sc2);
        vf[ks] = key < a.S ? *reinterpret_cast<const F*>(V + (long)key * a.ldv + ks * KS + hh * VEC) : frag_zero<T>();
    }
    const float kb2 = (a.key_bias && key < a.S) ? a.key_bias[(long)b * a.S + key] * LOG2E : 0.f;
    const F kya = hh ? frag_zero<T>() : Aug<T>::y(kb2);         // key side of the score chain: the key bias
    const F vya = hh ? frag_zero<T>() : Aug<T>::y(0.f);         // V side of the dP chain: the unit slots
    const bool win_on = a.window > 0 && a.window < a.T;
    int lq = -1, lkv = 0;
    if (a.blk_lq) { const int bb = (b * a.H + h) % a.B; lq = a.blk_lq[bb]; lkv = a.blk_lkv[bb]; }
    int vis_lo; unsigned vis_span;
    visible_queries(a, key, lq, lkv, vis_lo, vis_span);
    // dropout bits of this lane's key: one 32-bit column (bit = query & 31) of the (32-query, 64-key) tile's words
    const int ko = lane & 31, nqb32 = (a.T + 31) >> 5;
    const uint32_t* wcol = reinterpret_cast<const uint32_t*>(dmask) +
                           2 * (drop_word_base(a, b * a.H + h, 0, min(kw0, a.S - 1) >> 6) + ((kw0 >> 5) & 1) * 16 + (ko & 3) + 4 * (ko >> 3)) + ((ko >> 2) & 1);
    const long wq_stride = 2L * ((a.S + 63) >> 6) * 32;         // dwords between consecutive 32-query blocks

    f32x16 acc_k[NDB], acc_v[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc_k[d][r] = 0.f; acc_v[d][r] = 0.f; }

    int q_beg = 0, q_end = a.T;
    if (a.causal) {
        q_beg = k0 / BQ * BQ;                                   // rows q < k0 never see these keys
        if (a.window > 0 && a.window < a.T) q_end = min(a.T, k0 + 128 + a.window);
    }
    const long sbase = ((long)b * a.H + h) * a.T;
    RowTile<T, HD, BQ> qt, dt;
    float lse_r = 0.f, ndc_r = 0.f;
    auto prefetch = [&](int q0) {
        qt.load(Q, a.ldq, q0, a.T, tid);
        dt.load(DO, a.lddo, q0, a.T, tid);
        if (tid < BQ) {                                         // rows >= T: masked
            const int qq = min(q0 + tid, a.T - 1);
            lse_r = a.lse[sbase + qq] * LOG2E;
            if (!(lse_r > -INFINITY)) lse_r = 0.f;              // a row without a visible key: every P is zeroed by its mask below
            ndc_r = -a.delta[sbase + qq] / a.drop_scale;
        }
    };
    if (tid < NBUF) { Qa_[tid][BQ] = frag_zero<T>(); Da_[tid][BQ] = frag_zero<T>(); }
    auto commit = [&](int bi) {
        qt.template store<PK>(Qs_[bi], tid);
        dt.template store<PK>(Ds_[bi], tid);
        if constexpr (!TRD) {
            qt.template store_t<PT>(Qt, tid);
            dt.template store_t<PT>(Dt, tid);
        }
        if (tid < BQ) { Qa_[bi][tid] = Aug<T>::x(-lse_r); Da_[bi][tid] = Aug<T>::x(ndc_r); ndc_s_[bi][tid] = ndc_r; }
    };
    if (q_beg < q_end) prefetch(q_beg);
    if constexpr (NBUF == 2) {
        if (q_beg < q_end) {
            commit(0);
            if (q_beg + BQ < q_end) prefetch(q_beg + BQ);
        }
        __syncthreads();
    }
    int buf = 0;
    for (int q0 = q_beg; q0 < q_end; q0 += BQ) {
        uint32_t wbits[BQ / 32];
        auto load_bits = [&]() {
#pragma unroll
            for (int mb = 0; mb < BQ / 32; ++mb) {              // requested ahead of the next tile's rows: vmcnt is in order
                const int qb32 = min((q0 >> 5) + mb, nqb32 - 1);
                wbits[mb] = DROP ? wcol[qb32 * wq_stride] >> (4 * hh) : 0u;
            }
        };
        if constexpr (NBUF == 2) {
            if (q0 + BQ < q_end) commit(buf ^ 1);
            load_bits();
            if (q0 + 2 * BQ < q_end) prefetch(q0 + 2 * BQ);
        } else {
            __syncthreads();
            commit(0);
            __syncthreads();
            load_bits();
            if (q0 + BQ < q_end) prefetch(q0 + BQ);
        }
        T* const Qs = Qs_[buf];
        T* const Ds = Ds_[buf];
        F* const Qa = Qa_[buf];
        F* const Da = Da_[buf];
        float* const ndc_s = ndc_s_[buf];
#pragma unroll
        for (int mb = 0; mb < BQ / 32; ++mb) {
            const int qb = q0 + mb * 32;
            if (qb >= q_end) break;                                     // block-uniform
            f32x16 st, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
            if constexpr (TRD) {   // every LDS operand of the two chains is requested before the first MFMA: one LDS latency per block, not one per MFMA
                F qfr[NKS + 1], dfr[NKS + 1];
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    qfr[ks] = *reinterpret_cast<const F*>(&Qs[(mb * 32 + (lane & 31)) * PK + ks * KS + hh * VEC]);
                    dfr[ks] = *reinterpret_cast<const F*>(&Ds[(mb * 32 + (lane & 31)) * PK + ks * KS + hh * VEC]);
                }
                qfr[NKS] = Qa[hh ? BQ : mb * 32 + (lane & 31)];
                dfr[NKS] = Da[hh ? BQ : mb * 32 + (lane & 31)];
                __builtin_amdgcn_sched_group_barrier(0x100, 2 * NKS + 2, 0);      // the DS reads ...
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    mma32(st, qfr[ks], kf[ks]);
                    mma32(dp, dfr[ks], vf[ks]);
                }
                mma32(st, qfr[NKS], kya);
                mma32(dp, dfr[NKS], vya);
                __builtin_amdgcn_sched_group_barrier(0x008, 2 * NKS + 2, 0);      // ... then the MFMAs
            } else {               // fp32 (parity mode): twice the fragments; the registers do not hold them all
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const F qf = *reinterpret_cast<const F*>(&Qs[(mb * 32 + (lane & 31)) * PK + ks * KS + hh * VEC]);
                    mma32(st, qf, kf[ks]);
                    const F df = *reinterpret_cast<const F*>(&Ds[(mb * 32 + (lane & 31)) * PK + ks * KS + hh * VEC]);
                    mma32(dp, df, vf[ks]);
                }
                mma32(st, Qa[hh ? BQ : mb * 32 + (lane & 31)], kya);
                mma32(dp, Da[hh ? BQ : mb * 32 + (lane & 31)], vya);
            }
            f32x16 pd;  // dropped probabilities (for dV)
            const bool full = (kw0 + 32 <= a.S) && (qb + 32 <= a.T) && lq < 0 &&
                              (!a.causal || (kw0 + 31 <= qb && (!win_on || kw0 >= qb + 31 - a.window)));
#pragma unroll
            for (int r = 0; r < 16; ++r) st[r] = __builtin_amdgcn_exp2f(st[r]);            // P
            if (!full) {
                const int rel = qb + 4 * hh - vis_lo;
#pragma unroll
                for (int r = 0; r < 16; ++r) st[r] = (unsigned)(rel + acc_row(r, 0)) < vis_span ? st[r] : 0.f;
            }
            if constexpr (DROP) {
                const uint32_t wb = wbits[mb];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 n4 = *reinterpret_cast<const f32x4*>(&ndc_s[mb * 32 + 8 * g + 4 * hh]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = 4 * g + e;
                        // m = all ones where kept (v_bfe_i32); pd = P & m; t = kept ? dP' : -delta / c (v_bfi_b32); written as
                        // instructions: the compiler's own lowering of the same expressions took twice as many
                        const float pv = st[r], dv = dp[r], nv = n4[e];
                        uint32_t m;
                        asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(wb), "n"(8 * g + e));
                        pd[r] = __uint_as_float(__float_as_uint(pv) & m);
                        float t;
                        asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(t) : "v"(m), "v"(dv), "v"(nv));
                        st[r] *= t;                                                                      // dS / c
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) { pd[r] = st[r]; st[r] *= dp[r]; }
            }
            if constexpr (TRD) {
                F dtf[NFR][NDB], qtf[NFR][NDB];
#pragma unroll
                for (int s = 0; s < NFR; ++s)
#pragma unroll
                    for (int d = 0; d < NDB; ++d) {
                        dtf[s][d] = kperm_frag<T>(Ds, PK, Dt, PT, mb * 32, s, d * 32, lane);
                        qtf[s][d] = kperm_frag<T>(Qs, PK, Qt, PT, mb * 32, s, d * 32, lane);
                    }
                __builtin_amdgcn_sched_group_barrier(0x100, 2 * NFR * NDB * ACfg<T>::RPF, 0);
#pragma unroll
                for (int s = 0; s < NFR; ++s) {
                    const F pf = acc_to_frag<T>(pd, s);
                    const F sf = acc_to_frag<T>(st, s);
#pragma unroll
                    for (int d = 0; d < NDB; ++d) {
                        mma32(acc_v[d], pf, dtf[s][d]);
                        mma32(acc_k[d], sf, qtf[s][d]);
                    }
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 2 * NFR * NDB, 0);
            } else {
#pragma unroll
                for (int s = 0; s < NFR; ++s) {
                    const F pf = acc_to_frag<T>(pd, s);
                    const F sf = acc_to_frag<T>(st, s);
#pragma unroll
                    for (int d = 0; d < NDB; ++d) {
                        const F dtf = kperm_frag<T>(Ds, PK, Dt, PT, mb * 32, s, d * 32, lane);
                        mma32(acc_v[d], pf, dtf);
                        const F qtf = kperm_frag<T>(Qs, PK, Qt, PT, mb * 32, s, d * 32, lane);
                        mma32(acc_k[d], sf, qtf);
                    }
                }
            }
        }
        if constexpr (NBUF == 2) { __syncthreads(); buf ^= 1; }
    }
    // accumulators: column = d (lane & 31), row = key (register axis)
    const float ksc = a.scale * a.drop_scale;
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kk = k0 + wave * 32 + acc_row(r, lane);
            if (kk >= a.S) continue;
            const int col = h * HD + d * 32 + (lane & 31);
            ((T*)a.dk)[(long)b * a.bsdk + (long)kk * a.lddk + col] = from_f32<T>(acc_k[d][r] * ksc);
            ((T*)a.dv)[(long)b * a.bsdv + (long)kk * a.lddv + col] = from_f32<T>(acc_v[d][r] * a.drop_scale);
        }
}

template <typename T, int HD> int run_bwd(const AttnArgs& a, hipStream_t s) {
    const dim3 gq(cdiv(a.T, 128) * (a.nsplit > 1 ? a.nsplit : 1), a.H, a.B);
    if (a.drop_thresh) hipLaunchKernelGGL((attn_bwd_dq_kernel<T, HD, true>), gq, dim3(256), 0, s, a, a.dmask);
    else hipLaunchKernelGGL((attn_bwd_dq_kernel<T, HD, false>), gq, dim3(256), 0, s, a, a.dmask);
    if (a.nsplit > 1) {
        long nsum = (long)a.B * a.T * a.H * HD, gs = (nsum + 255) / 256;
        hipLaunchKernelGGL((attn_dq_sum_kernel<T>), dim3((unsigned)(gs > 4096 ? 4096 : gs)), dim3(256), 0, s, a, HD);
    }
    const dim3 gk(cdiv(a.S, 128), a.H, a.B);
    if (a.drop_thresh) hipLaunchKernelGGL((attn_bwd_dkv_kernel<T, HD, true>), gk, dim3(256), 0, s, a, a.dmask);
    else hipLaunchKernelGGL((attn_bwd_dkv_kernel<T, HD, false>), gk, dim3(256), 0, s, a, a.dmask);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

}  // namespace

extern "C" int omr_attn_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                            float* delta_ws, void* dq, void* dk, void* dv, long ldq, long ldk, long ldv, long ldo, long lddo, long lddq,
                            long lddk, long lddv, long bsq, long bsk, long bsv, long bso, long bsdo, long bsdq, long bsdk, long bsdv, int B,
                            int H, int T, int S, int head_dim, int causal, int window, const float* key_bias, const int* blk_lq,
                            const int* blk_lkv, float dropout_p, unsigned long long seed, const unsigned long long* drop_words, void* stream) {
    return omr_attn_bwd_ws(dtype, q, k, v, o, dout, lse, delta_ws, dq, dk, dv, ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv, bsq, bsk, bsv, bso, bsdo, bsdq,
                           bsdk, bsdv, B, H, T, S, head_dim, causal, window, key_bias, blk_lq, blk_lkv, dropout_p, seed, drop_words, nullptr, 0, stream);
}

/* omr_attn_bwd with caller-provided scratch for the key split of the dQ kernel (omr_attn_workspace_floats(..., backward = 1)) */
extern "C" int omr_attn_bwd_ws(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                               float* delta_ws, void* dq, void* dk, void* dv, long ldq, long ldk, long ldv, long ldo, long lddo, long lddq,
                               long lddk, long lddv, long bsq, long bsk, long bsv, long bso, long bsdo, long bsdq, long bsdk, long bsdv, int B,
                               int H, int T, int S, int head_dim, int causal, int window, const float* key_bias, const int* blk_lq,
                               const int* blk_lkv, float dropout_p, unsigned long long seed, const unsigned long long* drop_words, float* ws,
                               long ws_floats, void* stream) {
    AttnArgs a = {};
    int rc = fill_common(a, B, H, T, S, head_dim, dropout_p, seed, causal, window, key_bias, blk_lq, blk_lkv, drop_words, true);
    if (rc) return rc;
    rc = fill_qkvo(a, dtype, q, k, v, (void*)o, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso);
    if (rc || lddo % (dtype == OMR_BF16 ? 8 : 4)) return OMR_ERR_ARG;
    if (!delta_ws || !lse) return OMR_ERR_ARG;
    a.lse = (float*)lse; a.dout = dout; a.delta = delta_ws; a.dq = dq; a.dk = dk; a.dv = dv;
    a.lddo = lddo; a.lddq = lddq; a.lddk = lddk; a.lddv = lddv; a.bsdo = bsdo; a.bsdq = bsdq; a.bsdk = bsdk; a.bsdv = bsdv;
    rc = plan_split(a, head_dim, T > 32 ? ws : nullptr, ws_floats, dq_split_floats);      // the decode shapes (T <= 32) have no backward split
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T(dtype, DISPATCH_HD(head_dim, return (run_bwd<T, HD>(a, s))))
}
