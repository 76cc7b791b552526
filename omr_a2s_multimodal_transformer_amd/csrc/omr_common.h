// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels of libomr_hip.so.
// Wave = 64 lanes.  All matrix work goes through 32x32 MFMA tiles:
//   bf16 : v_mfma_f32_32x32x16_bf16  (8 k-values per lane per operand)
//   fp32 : v_mfma_f32_32x32x2_f32 x4 (4 k-values per lane per operand; exact f32 fma chain)
// Both consume ONE 16-byte fragment per lane per operand, so every tile loop below is written
// once over Frag<T> and works for the fp32 parity path and the bf16 throughput path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define OMR_F32 0
#define OMR_BF16 1

#define OMR_OK 0
#define OMR_ERR_ARG (-1)
#define OMR_ERR_LAUNCH (-2)
#define OMR_ERR_UNSUPPORTED (-3)

#define OMR_CHECK_LAUNCH()                                    \
    do {                                                      \
        hipError_t e__ = hipGetLastError();                   \
        if (e__ != hipSuccess) return OMR_ERR_LAUNCH;         \
    } while (0)

// Run CALL with T = the element type of a C-ABI dtype code (inside a function that returns an OMR_* status).
#define DISPATCH_T(dtype, CALL)                         \
    if ((dtype) == OMR_F32) { typedef float T; CALL; }  \
    else if ((dtype) == OMR_BF16) { typedef bf16 T; CALL; } \
    else return OMR_ERR_UNSUPPORTED;

template <typename T> struct Frag;
template <> struct Frag<bf16> {
    typedef bf16x8 type;
    static constexpr int N = 8;      // elements per 16-byte fragment
};
template <> struct Frag<float> {
    typedef f32x4 type;
    static constexpr int N = 4;
};
// k-values consumed by one mma32 call: lanes 0-31 hold k = [0,N), lanes 32-63 hold k = [N,2N)
template <typename T> struct KStep { static constexpr int value = 2 * Frag<T>::N; };

__device__ __forceinline__ void mma32(f32x16& acc, bf16x8 a, bf16x8 b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma32(f32x16& acc, f32x4 a, f32x4 b) {
    // lane half h holds k = 4h+e (e=0..3); instruction e sums k in {e, 4+e}.  A and B use the
    // same (arbitrary) k order, so the result is the exact f32 dot product.
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b[3], acc, 0, 0, 0);
}

// 32x32 accumulator layout (dtype independent on gfx950): column = lane & 31,
// row(reg) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
__device__ __forceinline__ int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(bf16 x) { return (float)x; }
template <typename T> __device__ __forceinline__ T from_f32(float x);
template <> __device__ __forceinline__ float from_f32<float>(float x) { return x; }
template <> __device__ __forceinline__ bf16 from_f32<bf16>(float x) { return (bf16)x; }

template <typename T> __device__ __forceinline__ typename Frag<T>::type frag_zero() {
    typename Frag<T>::type z;
#pragma unroll
    for (int i = 0; i < Frag<T>::N; ++i) z[i] = from_f32<T>(0.f);
    return z;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// LayerNorm of one row held by a wave, lane = PER consecutive columns: v <- (v - mean) * rstd * gamma + beta.  One definition
// for add_ln_fwd_kernel (norm.hip) and the decode row kernel's prologue (decode_linear.hip): the KV-cached step has to build the rows
// the training forward builds, to the bit.
template <int PER>
__device__ __forceinline__ void ln_row(float (&v)[PER], const float* __restrict__ gamma, const float* __restrict__ beta, int lane, float eps, float& mu,
                                       float& rs) {
    constexpr int d = PER * 64;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) s += v[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    mu = s * (1.f / d);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) { const float t = v[i] - mu; q += t * t; }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    rs = rsqrtf(q * (1.f / d) + eps);
#pragma unroll
    for (int i = 0; i < PER; ++i) v[i] = (v[i] - mu) * rs * gamma[lane * PER + i] + beta[lane * PER + i];
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Counter-based RNG for dropout masks: one 32-bit hash per (seed, element index), so a mask is
// regenerated in backward instead of being stored (never materialised in HBM).
__device__ __forceinline__ uint32_t hash_u32(uint64_t seed, uint64_t idx) {
    uint64_t z = idx * 0x9E3779B97F4A7C15ull + seed;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (uint32_t)(z >> 32);
}
// 32-bit variant (two rounds of a multiply-xorshift mixer keyed by both seed halves) for indices < 2^32:
// ~10 VALU ops per element instead of ~30 for the 64-bit mixer.
__device__ __forceinline__ uint32_t hash32(uint32_t seed_lo, uint32_t seed_hi, uint32_t idx) {
    uint32_t h = idx * 0x9E3779B1u + seed_lo;
    h ^= h >> 16; h *= 0x85EBCA6Bu;
    h ^= h >> 13; h += seed_hi; h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
// Dropout keep decision of element `idx` under (seed, p): ONE 32-bit hash serves the element PAIR (idx & ~1, idx | 1) with 16
// random bits each (low half: even element), keep iff bits >= p * 2^16 (thresh16 = OMR_DROP_THRESH16(p); p is realised to
// 1.5e-5, 0.5 and 0.25 exactly).  Every dropout site of the library uses this convention (omr_dropout, the conv / GEMM /
// add+LayerNorm epilogues), so a mask can be regenerated anywhere from (seed, index); vector code hashes once per pair.
#define OMR_DROP_THRESH16(p) ((uint32_t)((double)(p) * 65536.0 + 0.5))
__device__ __forceinline__ uint32_t drop_pair_bits(uint64_t seed, uint64_t pair) {
    return hash32((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)pair ^ (uint32_t)(pair >> 32) * 0x27D4EB2Fu);
}
__device__ __forceinline__ bool drop_keep(uint64_t seed, uint64_t idx, uint32_t thresh16) {
    const uint32_t h = drop_pair_bits(seed, idx >> 1);
    return ((idx & 1) ? (h >> 16) : (h & 0xffffu)) >= thresh16;
}

__host__ __device__ static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// attention.hip -> decode.hip: omr_attn_fwd_split_partials with per-row key counts (omr_attn_fwd_split_varlen's rule).  nsplit == NULL:
// the partials are merged here (omr_attn_fwd_split_varlen).  kv_group (>= 1): batch row b reads the K|V of slot b / kv_group and
// kv_len[b / kv_group] -- the `beam` hypotheses of one input share that input's memory K|V (beam search over a batch).
int attn_fwd_split_partials_varlen(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv,
                                   long ldo, long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim,
                                   const int* kv_len, float* split_ws, long split_ws_floats, int* nsplit, void* stream, int kv_group = 1);

// The same with a per-row first key (omr_attn_fwd_split_rows' rule: the key-split kernel for every S).
int attn_fwd_split_partials_rows(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv,
                                 long ldo, long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim,
                                 const int* kv_len, const int* kv_start, float* split_ws, long split_ws_floats, int* nsplit, void* stream);

// The self-attention of a grouped decode position (omr_decode_verify_rows): `group` consecutive rows are consecutive positions of ONE
// K|V slot, so row b reads slot b / group while kv_len / kv_start stay PER ROW (device int32 [B]): row b sees slot rows
// [kv_start[b], kv_start[b] + kv_len[b]).  Otherwise attn_fwd_split_partials_rows.
int attn_fwd_split_partials_group(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv,
                                  long ldo, long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim,
                                  const int* kv_len, const int* kv_start, int group, float* split_ws, long split_ws_floats, int* nsplit,
                                  void* stream);

// How a row body reads x[i].  PlainLoad: the value.  MaskedLoad (grammar-constrained decoding, omr_grammar_desc of include/omr_hip.h): -inf where the
// token automaton forbids token i in the row's current state -- next_row[cls[i]] < 0, next_row being that state's row of the
// transition table (C <= 256 ints, staged in LDS once per row by stage_next_row) and cls the class of every vocabulary entry
// (V bytes of global memory, shared by all rows).  The value is replaced BEFORE any comparison or expf, so a NaN or +inf in a
// forbidden column cannot reach a maximum, a sum or a pick.
struct PlainLoad {
    __device__ __forceinline__ float operator()(const float* __restrict__ x, int i) const { return x[i]; }
};
struct MaskedLoad {
    const unsigned char* __restrict__ cls; const int* next_row;
    __device__ __forceinline__ float operator()(const float* __restrict__ x, int i) const { return next_row[cls[i]] < 0 ? -INFINITY : x[i]; }
};
// Row `state` (clamped into [0, S)) of next [S][C] into next_row[256] (LDS; entries >= C: forbidden) by the 256 threads tid of a
// group; the caller synchronises before the first masked load.  -> the clamped state.
__device__ __forceinline__ int stage_next_row(const int* __restrict__ next, int S, int C, int state, int tid, int* next_row) {
    const int s = min(max(state, 0), S - 1);
    next_row[tid] = tid < C ? next[(long)s * C + tid] : -1;
    return s;
}

// Arg-max of ONE row by a group of 256 threads (every thread of the WORKGROUP must call it): first index of the maximum
// (torch.argmax's tie rule).  On return sv[0] holds the maximum and si[0] its index (0x7fffffff when no comparison was won: a row
// of NaN or -inf), visible to every thread.  One definition for argmax_kernel and the constrained pick (elementwise.hip).
template <typename Load = PlainLoad>
__device__ __forceinline__ void argmax_row(const float* __restrict__ x, int n, int tid, float* sv, int* si, Load load = Load()) {
    float best = -INFINITY; int bi = 0x7fffffff;
    for (int i = tid; i < n; i += 256) {
        float v = load(x, i);
        if (v > best || (v == best && i < bi)) { best = v; bi = i; }
    }
    sv[tid] = best; si[tid] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            float v2 = sv[tid + o]; int i2 = si[tid + o];
            if (v2 > sv[tid] || (v2 == sv[tid] && i2 < si[tid])) { sv[tid] = v2; si[tid] = i2; }
        }
        __syncthreads();
    }
}

// elementwise.hip -> decode.hip, decode_beam.hip: non-NULL tables and state, 1 <= C <= 256, S >= 1
struct omr_grammar_desc;
bool grammar_desc_ok(const omr_grammar_desc* g);

// Top-k log-probabilities of ONE row by a group of 256 threads (tid 0..255; every thread of the WORKGROUP must call it: it
// synchronises with __syncthreads): emit(j, index, log_softmax(x)[index]) for the j-th largest, j < k, ties towards the smaller
// index, with the same values in every thread.  A max / sum-exp pass, then k selection passes over the candidates that come
// after the previous pick in (value descending, index ascending) order.  A pass in which no candidate wins a comparison emits
// index j, always inside [0, n): a row that is ALL NaN yields 0 .. k - 1 with NaN values, the indices a row of -inf gets by the
// tie rule.  (A row with f < k comparable entries and NaN elsewhere yields those f, then f .. k - 1, which may name one of them
// again; its values are NaN.)  sv / si: 256 entries of LDS each, the group's own.
// One definition for topk_logprob_kernel (elementwise.hip) and the beam selection (decode_beam.hip): the on-device beam search has
// to rank the very floats the host route reads back.
// load: how x[i] is read (PlainLoad; MaskedLoad renormalises over the allowed tokens).
template <typename Emit, typename Load = PlainLoad>
__device__ __forceinline__ void topk_logprob_row(const float* __restrict__ x, int n, int k, int tid, float* sv, int* si, Emit emit, Load load = Load()) {
    float mx = -INFINITY;
    for (int i = tid; i < n; i += 256) mx = fmaxf(mx, load(x, i));
    sv[tid] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) sv[tid] = fmaxf(sv[tid], sv[tid + o]); __syncthreads(); }
    mx = sv[0];
    __syncthreads();
    float se = 0.f;
    for (int i = tid; i < n; i += 256) se += expf(load(x, i) - mx);
    sv[tid] = se;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) sv[tid] += sv[tid + o]; __syncthreads(); }
    const float lse = mx + logf(sv[0]);
    __syncthreads();
    float last_v = INFINITY; int last_i = -1;
    for (int j = 0; j < k; ++j) {
        float best = -INFINITY; int bi = 0x7fffffff;
        for (int i = tid; i < n; i += 256) {
            const float v = load(x, i);
            const bool cand = v < last_v || (v == last_v && i > last_i);
            if (cand && (v > best || (v == best && i < bi))) { best = v; bi = i; }
        }
        sv[tid] = best; si[tid] = bi;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) {
                const float v2 = sv[tid + o]; const int i2 = si[tid + o];
                if (v2 > sv[tid] || (v2 == sv[tid] && i2 < si[tid])) { sv[tid] = v2; si[tid] = i2; }
            }
            __syncthreads();
        }
        last_v = sv[0]; last_i = si[0];
        emit(j, last_i < n ? last_i : (j < n ? j : 0), last_v - lse);      // no candidate (a row of NaN): pick j is index j, never past the row
        __syncthreads();
    }
}

// Weighted late fusion of ONE pair of logit rows by a group of 256 threads (every thread of the WORKGROUP must call these: they
// synchronise with __syncthreads).  weighted_mix_stats: the two rows' maxima and sums of exponentials over the 256-thread
// strided partition and the halving trees of weighted_argmax_kernel (elementwise.hip), which calls it.  sa / sb: 256 entries
// of LDS each, the group's own; free again on return.
struct MixStats { float ma, mb, za, zb; };
template <typename Load = PlainLoad>
__device__ __forceinline__ MixStats weighted_mix_stats(const float* __restrict__ la, const float* __restrict__ lb, int n, int tid, float* sa, float* sb,
                                                       Load load = Load()) {
    float ma = -INFINITY, mb = -INFINITY;
    for (int i = tid; i < n; i += 256) { ma = fmaxf(ma, load(la, i)); mb = fmaxf(mb, load(lb, i)); }
    sa[tid] = ma; sb[tid] = mb;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) { sa[tid] = fmaxf(sa[tid], sa[tid + o]); sb[tid] = fmaxf(sb[tid], sb[tid + o]); } __syncthreads(); }
    ma = sa[0]; mb = sb[0];
    __syncthreads();
    float ea = 0.f, eb = 0.f;
    for (int i = tid; i < n; i += 256) { ea += expf(load(la, i) - ma); eb += expf(load(lb, i) - mb); }
    sa[tid] = ea; sb[tid] = eb;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) { sa[tid] += sa[tid + o]; sb[tid] += sb[tid + o]; } __syncthreads(); }
    const MixStats st = {ma, mb, sa[0], sb[0]};
    __syncthreads();
    return st;
}
// wa * softmax(la)[i] + wb * softmax(lb)[i]: two rounded products and one add like torch's `alpha * p + (1 - alpha) * q`
// (no fma contraction), so ties break the way they do there
__device__ __forceinline__ float weighted_mix(float la_i, float lb_i, const MixStats& st, float wa, float wb) {
    return __fadd_rn(__fmul_rn(wa, expf(la_i - st.ma) / st.za), __fmul_rn(wb, expf(lb_i - st.mb) / st.zb));
}

// Arg-max of the mixed distribution of ONE pair of rows by a group of 256 threads (every thread of the WORKGROUP must call it):
// on return sa[0] holds the largest weighted_mix and si[0] its first index (0x7fffffff: no comparison won).  One definition for
// weighted_argmax_kernel and the constrained weighted pick (elementwise.hip); sa / sb / si: 256 entries of LDS each.
template <typename Load = PlainLoad>
__device__ __forceinline__ void weighted_argmax_row(const float* __restrict__ la, const float* __restrict__ lb, int n, float wa, float wb, int tid,
                                                    float* sa, float* sb, int* si, Load load = Load()) {
    const MixStats st = weighted_mix_stats(la, lb, n, tid, sa, sb, load);
    float best = -INFINITY; int bi = 0x7fffffff;
    for (int i = tid; i < n; i += 256) {
        const float v = weighted_mix(load(la, i), load(lb, i), st, wa, wb);
        if (v > best || (v == best && i < bi)) { best = v; bi = i; }
    }
    sa[tid] = best; si[tid] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const float v2 = sa[tid + o]; const int i2 = si[tid + o];
            if (v2 > sa[tid] || (v2 == sa[tid] && i2 < si[tid])) { sa[tid] = v2; si[tid] = i2; }
        }
        __syncthreads();
    }
}

// topk_logprob_row for the mixed distribution p = weighted_mix(la, lb) (beam search over the weighted late fusion; an
// extension: the reference decodes greedily, weighted_multimodal/test.py:50-61): emit(j, index, logf(p[index])) for the j-th
// largest p, j < k, ties towards the smaller index, the same values in every thread.  Every selection pass recomputes p by the
// one expression above, so k = 1 is weighted_argmax_kernel's pick and a row's result does not depend on the grid.  p = 0
// (both exponentials underflowed) is a candidate like any other and emits -inf.  One definition for weighted_topk_logprob_kernel
// (elementwise.hip) and the weighted beam selection (decode_beam.hip).
template <typename Emit, typename Load = PlainLoad>
__device__ __forceinline__ void weighted_topk_logprob_row(const float* __restrict__ la, const float* __restrict__ lb, int n, float wa, float wb, int k,
                                                          int tid, float* sa, float* sb, int* si, Emit emit, Load load = Load()) {
    const MixStats st = weighted_mix_stats(la, lb, n, tid, sa, sb, load);
    float last_v = INFINITY; int last_i = -1;
    for (int j = 0; j < k; ++j) {
        float best = -INFINITY; int bi = 0x7fffffff;
        for (int i = tid; i < n; i += 256) {
            const float v = weighted_mix(load(la, i), load(lb, i), st, wa, wb);
            const bool cand = v < last_v || (v == last_v && i > last_i);
            if (cand && (v > best || (v == best && i < bi))) { best = v; bi = i; }
        }
        sa[tid] = best; si[tid] = bi;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) {
                const float v2 = sa[tid + o]; const int i2 = si[tid + o];
                if (v2 > sa[tid] || (v2 == sa[tid] && i2 < si[tid])) { sa[tid] = v2; si[tid] = i2; }
            }
            __syncthreads();
        }
        last_v = sa[0]; last_i = si[0];
        emit(j, last_i < n ? last_i : (j < n ? j : 0), logf(last_v));      // no candidate (a row of NaN): pick j is index j, never past the row
        __syncthreads();
    }
}
