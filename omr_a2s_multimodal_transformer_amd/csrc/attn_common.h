// Shared pieces of the fused attention kernels (attention.hip: forward; attention_bwd.hip: dQ, dK/dV): the argument block, the
// fragment / staging / visibility / augmented-k-step / dropout-word helpers every kernel uses, and the host-side split plan
// and argument filling.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "omr_common.h"
#include "omr_hip.h"

namespace attn {      // local to the translation unit that includes it (static host helpers), min_workgroups() excepted

constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

struct AttnArgs {
    const void* q; const void* k; const void* v; void* o;
    long ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso;      // row / batch strides in elements
    float* lse;                                        // [B][H][T]
    const float* key_bias;                             // [B][S] or null
    const int* blk_lq; const int* blk_lkv;             // [B] or null
    int B, H, T, S; float scale; int causal; int window;
    uint32_t drop_thresh; float drop_scale; uint64_t seed;
    const uint64_t* dmask;                             // dropout keep bits (attn_dropout_words_kernel); passed to the kernels as a
                                                       // separate __restrict__ parameter so that its loads become scalar loads
    // single-query-block forward split over the keys (decode): blockIdx.x = split, partials [B][H][nsplit][T][HD + 2] floats
    int nsplit, split_len; float* part;
    int kv_group;                                      // key-split forward: batch row b reads the K|V (and kv_len) of slot b / kv_group
    int kv_row_tables;                                 // key-split forward: kv_len / kv_start are indexed by the batch row b itself, the
                                                       // slot still by b / kv_group (a grouped decode position)
    // backward only
    const void* dout; long lddo, bsdo;
    const float* delta;                                // [B][H][T]
    void* dq; void* dk; void* dv; long lddq, lddk, lddv, bsdq, bsdk, bsdv;
};

template <typename T> struct ACfg {
    static constexpr int MPI = std::is_same<T, bf16>::value ? 1 : 4;      // MFMA instructions per mma32 (sched_group_barrier counts)
    static constexpr int RPF = std::is_same<T, bf16>::value ? 2 : 1;      // LDS reads per permuted-k fragment (kperm_frag)
    static constexpr int VEC = Frag<T>::N;
    static constexpr int NFR = 16 / VEC;   // operand fragments per 32-wide accumulator block (2 bf16 / 4 fp32)
};

// Fragment of a k-contiguous LDS row whose k order matches accumulator registers s*VEC .. s*VEC+VEC-1 of a
// 32-row block: element j  <->  k = kb + acc_row(s*VEC + j, lane).
template <typename T> __device__ __forceinline__ typename Frag<T>::type load_kperm_frag(const T* row, int kb, int s, int h);
template <> __device__ __forceinline__ bf16x8 load_kperm_frag<bf16>(const bf16* row, int kb, int s, int h) {
    const bf16x4 lo = *reinterpret_cast<const bf16x4*>(row + kb + 16 * s + 4 * h);
    const bf16x4 hi = *reinterpret_cast<const bf16x4*>(row + kb + 16 * s + 4 * h + 8);
    bf16x8 r;
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3]; r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
    return r;
}
template <> __device__ __forceinline__ f32x4 load_kperm_frag<float>(const float* row, int kb, int s, int h) {
    return *reinterpret_cast<const f32x4*>(row + kb + 8 * s + 4 * h);
}

// The same permuted-k fragment, dtype dispatched:
//   bf16: straight from the ROW-MAJOR tile [k][cols] with two ds_read_b64_tr_b16 (each returns 4 consecutive k rows of this
//         lane's column) -- no transposed copy of the tile is ever staged;
//   fp32: from a transposed tile [col][k] (staged with element-wise LDS stores; parity path only).
template <typename T>
__device__ __forceinline__ typename Frag<T>::type kperm_frag(const T* rowmajor, int prow, const T* transposed, int ptr_, int kb, int s,
                                                              int col0, int lane) {
    if constexpr (std::is_same<T, bf16>::value) {
        typedef __attribute__((address_space(3))) bf16x4 LdsV4;
        const int q = (lane & 15) >> 2, col = col0 + ((lane >> 4) & 1) * 16 + (lane & 3) * 4, k = kb + 16 * s + 4 * (lane >> 5) + q;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LdsV4*)(rowmajor + k * prow + col));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LdsV4*)(rowmajor + (k + 8) * prow + col));
        const bf16x8 f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return f;
    } else {
        return load_kperm_frag<T>(transposed + (col0 + (lane & 31)) * ptr_, kb, s, lane >> 5);
    }
}

template <typename T> __device__ __forceinline__ typename Frag<T>::type acc_to_frag(const f32x16& acc, int s) {
    typename Frag<T>::type f;
#pragma unroll
    for (int j = 0; j < Frag<T>::N; ++j) f[j] = from_f32<T>(acc[s * Frag<T>::N + j]);
    return f;
}

// Register-staged tile of NR rows x HD: load() issues the global reads, store() / store_t() commit them to LDS row-major /
// transposed.  The kernels load tile t+1 right after the barrier that publishes tile t, so the HBM latency of the next tile
// is hidden behind the MFMA / softmax work on the current one.  Rows at or beyond nrows read the LAST VALID row instead
// (finite data; every consumer masks those rows' scores): the loads carry no per-lane condition -- a conditional load
// compiles to an exec-masked branch per chunk and pessimistic waits behind it.
template <typename T, int HD, int NR> struct RowTile {
    typedef typename Frag<T>::type F;
    static constexpr int VEC = Frag<T>::N, CPR = HD / VEC, NCH = (NR * CPR) / 256;
    static_assert((NR * CPR) % 256 == 0, "every thread owns the same number of 16-byte chunks");
    F r[NCH];
    __device__ __forceinline__ void load(const T* src, long ld, int r0, int nrows, int tid) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = tid + i * 256, row = c / CPR, kc = (c % CPR) * VEC;
            r[i] = *reinterpret_cast<const F*>(src + (long)min(r0 + row, nrows - 1) * ld + kc);
        }
    }
    template <int P> __device__ __forceinline__ void store(T* lds, int tid) const {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = tid + i * 256, row = c / CPR, kc = (c % CPR) * VEC;
            *reinterpret_cast<F*>(lds + row * P + kc) = r[i];
        }
    }
    template <int P> __device__ __forceinline__ void store_t(T* lds, int tid) const {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = tid + i * 256, row = c / CPR, kc = (c % CPR) * VEC;
#pragma unroll
            for (int e = 0; e < VEC; ++e) lds[(kc + e) * P + row] = r[i][e];
        }
    }
};

// Visibility (length limits, causal / window band, CrossAttention's block mask) as a per-lane RANGE, computed once per kernel:
// the keys a query row sees are [lo, lo + span) (lane = query: forward, dQ); the queries that see a key are such a range too
// (lane = key: dK/dV).  A boundary tile then tests  (unsigned)(index - lo) < span  per score: no branches.
__device__ __forceinline__ void visible_keys(const AttnArgs& a, int q, int S, int lq, int lkv, int& lo, unsigned& span) {
    int hi = q < a.T ? S : 0;
    lo = 0;
    if (a.causal) {
        hi = min(hi, q + 1);
        if (a.window > 0 && a.window < a.T) lo = max(0, q - a.window);
    }
    if (lq >= 0 && q >= lq) hi = min(hi, lkv);
    span = (unsigned)max(hi - lo, 0);
}
__device__ __forceinline__ void visible_queries(const AttnArgs& a, int key, int lq, int lkv, int& lo, unsigned& span) {
    int hi = key < a.S ? a.T : 0;
    lo = 0;
    if (a.causal) {
        lo = key;
        if (a.window > 0 && a.window < a.T) hi = min(hi, key + a.window + 1);
    }
    if (lq >= 0 && key >= lkv) hi = min(hi, lq);
    span = (unsigned)max(hi - lo, 0);
}
// Attention-probability dropout mask (nn.MultiheadAttention dropout, decoder.py:91): ONE 7-op multiply-xorshift hash of the
// pair index (q, key >> 1), keyed per (seed, b, h), decides two adjacent keys with 16 bits each (keep iff bits >= p * 2^16).
// The bits are a pure function of (seed, b, h, q, key); attn_dropout_words_kernel evaluates it once per (layer, step) into
// the word layout the three kernels consume (1 bit per score).  The 1/(1-p) rescale is folded out of the per-score code
// (applied to O / dV / dQ / dK).
__device__ __forceinline__ uint32_t attn_bh_key(const AttnArgs& a, int b, int h) {
    return hash32((uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)(b * a.H + h));
}
// 32 random bits for the key pair (key & ~1, key | 1) of query q: low half = even key, high half = odd key
__device__ __forceinline__ uint32_t attn_rand2(uint32_t bh_key, uint32_t pair_idx) {
    uint32_t x = pair_idx ^ bh_key;
    x *= 0x9E3779B1u; x ^= x >> 15; x *= 0x85EBCA6Bu; x ^= x >> 16;
    return x;
}
// thr32 = threshold << 16.  High half: (x >> 16) >= t  <=>  x >= t << 16; low half: shift it up first.
__device__ __forceinline__ bool attn_keep_lo(uint32_t x, uint32_t thr32) { return (x << 16) >= thr32; }
__device__ __forceinline__ bool attn_keep_hi(uint32_t x, uint32_t thr32) { return x >= thr32; }

// ------------------------------------------------------------------------------------------------
// Vector-instruction budget.  The kernels below are bound by the VALU issue rate, not by the matrix pipe (hd = 64: a lane owns 2
// scores per MFMA), so everything that can leave the per-score vector code does:
//   * the softmax scale * log2(e) is folded into the Q (forward, dQ) / K (dK, dV) fragments once per kernel;
//   * the additive terms of a score -- key bias, minus the row's reference maximum (forward) or log-sum-exp (backward), minus
//     delta / c for dP -- ride on ONE extra k-step of the score's MFMA chain ("augmented k-step"): side X carries a value in
//     two bf16 slots (hi + lo = the fp32 value to 2^-17; fp32 mode: one exact slot) against unit slots of side Y and vice versa,
//     so the accumulator leaves the chain as  s * scale * log2 e + bias - reference  and the only vector work on a score is the exp2;
//   * forward: the reference maximum is LAGGED (it moves only when a tile's maximum exceeds it by more than 2^THR, a
//     wave-uniform rare branch), so no subtraction and no accumulator rescale in the common tile;
//   * attention-probability dropout: the keep bits are generated ONCE per (layer, step) by attn_dropout_words_kernel in the
//     accumulator's own lane layout -- one 64-bit word per (32 queries, register) -- and the kernels apply them with one
//     v_cndmask per score whose mask operand is that word in an SGPR pair (forward, dQ: scalar loads) or, in the key-per-lane
//     dK/dV kernel, from the same words read as one 32-bit column per lane (v_bfe + v_and / v_bfi).
template <typename T> struct Aug;
template <> struct Aug<bf16> {
    static __device__ __forceinline__ void split(float v, bf16& hi, bf16& lo) {
        hi = (bf16)v;
        const float r = v - (float)hi;
        lo = (r == r) ? (bf16)r : (bf16)0.f;                  // v = +-inf: hi carries it, inf - inf = NaN is dropped
    }
    static __device__ __forceinline__ bf16x8 x(float v) {
        bf16 hi, lo; split(v, hi, lo);
        const bf16 one = (bf16)1.f, z = (bf16)0.f;
        const bf16x8 f = {hi, lo, one, one, z, z, z, z};
        return f;
    }
    static __device__ __forceinline__ bf16x8 y(float v) {
        bf16 hi, lo; split(v, hi, lo);
        const bf16 one = (bf16)1.f, z = (bf16)0.f;
        const bf16x8 f = {one, one, hi, lo, z, z, z, z};
        return f;
    }
};
template <> struct Aug<float> {
    static __device__ __forceinline__ f32x4 x(float v) { const f32x4 f = {v, 1.f, 0.f, 0.f}; return f; }
    static __device__ __forceinline__ f32x4 y(float v) { const f32x4 f = {1.f, v, 0.f, 0.f}; return f; }
};
// x . y over the augmented k-step = x's value + y's value; only the lanes of the lower k half (lane < 32) carry the slots.

// Both halves of the wave (lanes i and i + 32 hold the two k-halves of one row): v_permlane32_swap instead of a ds_bpermute
// shuffle -- an LDS-pipe instruction would make the kernel wait on lgkmcnt, i.e. on the scalar dropout-word loads in flight.
__device__ __forceinline__ float max_halves(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const unsigned lo = r[0], hi = r[1];                        // the lower half's value / the upper half's value, in every lane
    return fmaxf(__uint_as_float(lo), __uint_as_float(hi));
}

// One score under its dropout bit: mask = the 64-bit word of this accumulator register (bit = lane).
// The compiler pads its own instructions with the wait states gfx950 wants (two between a VALU result and the MFMA that reads it)
// but does not look inside an asm statement.  RESULT_FEEDS_VALU: the caller passes the result through a VALU instruction of the
// compiler's before any MFMA reads it (the bf16 forward: the conversion to bf16), so the select may be the one v_cndmask_b32
// with the word in an SGPR pair, written as an instruction.  Otherwise (the fp32 forward hands the result to the PV MFMA as it
// is) the select is stated in C++ and every hazard is the compiler's.  DESIGN.md, "Attention error bounds", has the defect this
// settles.
template <bool RESULT_FEEDS_VALU>
__device__ __forceinline__ float keep_or_zero(float x, uint64_t mask, int lane) {
    if constexpr (RESULT_FEEDS_VALU) {
        float r;
        asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(x), "s"(mask));
        return r;
    } else {
        return ((mask >> lane) & 1) ? x : 0.f;
    }
}
__device__ __forceinline__ float keep_or(float x, float alt, uint64_t mask) {
    float r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(alt), "v"(x), "s"(mask));
    return r;
}
// Dropout words: [B*H][ceil(T/32)][ceil(S/64)][32] 64-bit words; word (mb, r) of a (32-query, 64-key) tile holds, at bit
// (query & 31) + 32 * hh, the keep bit of key  tile*64 + mb*32 + acc_row(r, hh).
// (indices are clamped to the last block: waves whose rows lie beyond T / S read valid words and discard the result)
__device__ __forceinline__ long drop_word_base(const AttnArgs& a, int bh, int qb32, int kt) {
    const int nqb = (a.T + 31) >> 5, nkt = (a.S + 63) >> 6;
    return (((long)bh * nqb + min(qb32, nqb - 1)) * nkt + min(kt, nkt - 1)) * 32;
}

// ------------------------------------------------------------------------------------------------ host side
// Key split of the lane-per-query kernels (forward, dQ).  They own 32 query rows per wave, so B*H*T/32 waves exist whatever
// the key count: 2 per SIMD at the benchmark's cross-attention (B 32, H 4, T 512, S 4096) -- too few to hide the LDS / barrier /
// load latencies of a 64-key tile (measured: 4 000 SIMD cycles per wave-tile against ~1 900 of issue).  Splitting the KEYS of
// a (batch, head, query block) over several workgroups multiplies the resident waves; the forward's partial softmaxes are
// merged by attn_split_merge_kernel, the partial dQ sums by attn_dq_sum_kernel (both fixed-order, no atomics).  Decode
// (T <= 32): one 256-key block per workgroup.  Causal attention is not split (its key range depends on the query block).
// OMR_ATTN_MIN_WG (experiment knob, default 512).  Defined in attention.hip, not here: one copy per library, read once, so the
// workspace size query, the forward and the backward always plan with the same value.
__attribute__((visibility("hidden"))) int min_workgroups();
static inline void choose_split(int B, int H, int T, int S, int causal, int* nsplit, int* split_len) {
    *nsplit = 1; *split_len = 0;
    if (causal || S <= 256) return;
    int want;
    if (T <= 32) { want = (S + 255) / 256; if (want > 64) want = 64; }      // the merge prologue of omr_decode_linear takes <= 64 splits
    else {
        const long blocks = (long)B * H * ((T + 127) / 128);
        const int min_wg = min_workgroups();
        want = (int)((min_wg + blocks - 1) / blocks);              // at least ~512 workgroups (2 per CU); more buys nothing: the
                                                                  // kernels are VALU-issue bound, not latency bound (measured)
        const int maxs = S / 512;                                 // at least 512 keys per split
        if (want > maxs) want = maxs;
    }
    if (want <= 1) return;
    const int len = ((S + want - 1) / want + 255) / 256 * 256;    // whole 256-key staging blocks
    *split_len = len; *nsplit = (S + len - 1) / len;
    if (*nsplit <= 1) { *nsplit = 1; *split_len = 0; }
}
// floats of scratch the split wants: the forward's partial softmaxes [B][H][nsplit][T][hd + 2], the partial dQ [nsplit][B][T][H*hd]
static inline long fwd_split_floats(int B, int H, int T, int hd, int nsplit) { return (long)B * H * nsplit * T * (hd + 2); }
static inline long dq_split_floats(int B, int H, int T, int hd, int nsplit) { return (long)nsplit * B * T * H * hd; }

// Adopt the split plan of the shape when the caller brought scratch `ws` for it (ws_floats: its size; need: the size function
// above).  Without scratch, or for a shape that is not split, the args stay at one split.
static inline int plan_split(AttnArgs& a, int hd, float* ws, long ws_floats, long (*need)(int, int, int, int, int)) {
    a.nsplit = 1; a.split_len = 0; a.part = nullptr;
    if (!ws) return OMR_OK;
    int nsplit, len;
    choose_split(a.B, a.H, a.T, a.S, a.causal, &nsplit, &len);
    if (nsplit <= 1) return OMR_OK;
    if (ws_floats < need(a.B, a.H, a.T, hd, nsplit)) return OMR_ERR_ARG;
    a.nsplit = nsplit; a.split_len = len; a.part = ws;
    return OMR_OK;
}

// Shape, masks and dropout of every entry point.  need_words: the entry launches kernels that READ the keep bits
static inline int fill_common(AttnArgs& a, int B, int H, int T, int S, int hd, float dropout_p, unsigned long long seed, int causal, int window,
                       const float* key_bias, const int* blk_lq, const int* blk_lkv, const unsigned long long* drop_words = nullptr,
                       bool need_words = false) {
    if (B <= 0 || H <= 0 || T <= 0 || S <= 0) return OMR_ERR_ARG;
    if (hd != 32 && hd != 64) return OMR_ERR_UNSUPPORTED;
    if (dropout_p < 0.f || dropout_p >= 1.f) return OMR_ERR_ARG;
    if ((blk_lq == nullptr) != (blk_lkv == nullptr)) return OMR_ERR_ARG;
    a.B = B; a.H = H; a.T = T; a.S = S; a.scale = 1.0f / sqrtf((float)hd); a.causal = causal; a.window = window;
    a.key_bias = key_bias; a.blk_lq = blk_lq; a.blk_lkv = blk_lkv;
    a.drop_thresh = (uint32_t)((double)dropout_p * 65536.0 + 0.5);      // 16-bit threshold (attn_rand2); 0 = dropout off
    a.drop_scale = 1.f / (1.f - dropout_p);
    a.seed = seed;
    a.dmask = reinterpret_cast<const uint64_t*>(drop_words);
    if (need_words && a.drop_thresh != 0 && !drop_words) return OMR_ERR_ARG;      // the kernels read the keep bits, they do not hash
    return OMR_OK;
}
// The q / k / v / o pointers and strides of the forward and the backward; q, k and v rows are read as 16-byte fragments
static inline int fill_qkvo(AttnArgs& a, int dtype, const void* q, const void* k, const void* v, void* o, long ldq, long ldk, long ldv, long ldo, long bsq,
                     long bsk, long bsv, long bso) {
    const int vec = dtype == OMR_BF16 ? 8 : 4;
    if (ldq % vec || ldk % vec || ldv % vec) return OMR_ERR_ARG;
    a.q = q; a.k = k; a.v = v; a.o = o;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.bsq = bsq; a.bsk = bsk; a.bsv = bsv; a.bso = bso;
    return OMR_OK;
}

// Run CALL with HD = the head dim as a compile-time constant (fill_common has refused everything but 32 and 64)
#define DISPATCH_HD(hd, CALL)                                  \
    do {                                                       \
        if ((hd) == 64) { constexpr int HD = 64; CALL; }       \
        else { constexpr int HD = 32; CALL; }                  \
    } while (0)

}  // namespace attn
