// Device steps shared by the GEMM kernels (gemm.hip, gemm_panel.hip, gemm_tall.hip): each is written here once.
#pragma once
#include "omr_common.h"
#include "gemm_args.h"

// Row-group view (GemmArgs): physical - logical row offset of the tile that starts at logical row i of `operand`; 0 when the
// view is on another operand or off.  A tile never straddles a group (host-checked: grp is a multiple of every tile extent).
__device__ __forceinline__ long grp_delta(const GemmArgs& g, int operand, int i) {
    return g.grp_operand == operand ? (long)(i / g.grp) * (g.grp_stride - g.grp) + g.grp_base : 0;
}

// bf16 MFMA fragment of an operand staged reduction-major in LDS: two ds_read_tr16_b64 reads four reduction rows apart
// (`rows4_bytes` = the byte distance of four reduction rows), glued into the eight k values a lane feeds to one k-step.
typedef __attribute__((address_space(3))) bf16x4 LdsV4;
__device__ __forceinline__ bf16x8 tr_frag_bf16(const void* p, int rows4_bytes) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LdsV4*)b);
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((LdsV4*)(b + rows4_bytes));
    const bf16x8 f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return f;
}

// Zero an array (of arrays) of 32 x 32 accumulators.
template <typename A> __device__ __forceinline__ void acc_clear(A& acc) {
    f32x16* a = reinterpret_cast<f32x16*>(&acc);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(A) / sizeof(f32x16)); ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) a[i][r] = 0.f;
}

// C^T pack step.  With the product taken as C^T a lane owns one output row and, per accumulator group q, the four consecutive
// columns in registers 4q .. 4q + 3: they leave as one bf16x4 (an 8-byte store into the kernel's LDS image of the tile), each
// converted from f(value, e), e = the column inside the run (bias, activation).  The plain form converts the value as it is: it
// must not be spelled "+ 0.f", which costs a v_add per element and turns -0.f into +0.f.
template <typename F> __device__ __forceinline__ bf16x4 pack_ct4(const f32x16& acc, int q, F f) {
    bf16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (bf16)f(acc[4 * q + e], e);
    return o;
}
__device__ __forceinline__ bf16x4 pack_ct4(const f32x16& acc, int q) { return pack_ct4(acc, q, [](float v, int) { return v; }); }
