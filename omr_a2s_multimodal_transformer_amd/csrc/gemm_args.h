// Arguments of the GEMM kernels (gemm.hip, gemm_panel.hip, gemm_tall.hip) and the call as the specialised routes see it.
#pragma once
#include <hip/hip_runtime.h>

// Everything is off by default: a caller sets what it means, and a new field needs no visit to the callers that do not use it.
struct GemmArgs {
    const void* A = nullptr; const void* B = nullptr; void* C = nullptr; const float* bias = nullptr;
    int M = 0, N = 0, K = 0; long lda = 0, ldb = 0, ldc = 0;
    int relu = 0, accum = 0, atomic = 0, ksplit_len = 0;
    float* colsum_a = nullptr;   // transA only: colsum_a[m] += sum_k A[k][m] (bias gradient of a linear layer), fused into the dW GEMM
    int mt = 0, nt = 0, chunk = 0, total = 0;   // tile grid and XCD chunking (filled by the launchers)
    unsigned drop_thresh = 0; float drop_scale = 1.f; unsigned long long drop_seed = 0;   // fused dropout on the bf16/f32 output (0 = off)
    // Row-group view of the weight-side operand (0 = off): logical row i lives at physical row (i / grp) * grp_stride +
    // grp_base + i % grp.  grp_operand: 1 = rows of B / entries of bias (index n), 2 = reduction rows of a transposed B
    // (index k), 3 = rows of C / entries of colsum_a (index m).  Lets ONE GEMM run over the K|V rows of all decoder layers'
    // packed in_proj matrices where they lie in the flat parameter buffer ([Wq;Wk;Wv] blocks back to back).
    int grp = 0, grp_stride = 0, grp_base = 0, grp_operand = 0;
    // fp8 operands (omr_gemm_fp8): C = (A8 . B8^T) * scale_a[m] * scale_b[n] + bias -- per-row quantisation scales of both operands
    const float* scale_a = nullptr; const float* scale_b = nullptr;
};
static_assert(sizeof(GemmArgs) == 160, "GemmArgs travels as kernel arguments");

// What omr_gemm was asked for beyond GemmArgs.  omr_gemm hands the call to each specialised route in turn (panel, tall); a route
// states its WHOLE acceptance condition in its own file and answers OMR_ERR_UNSUPPORTED ("not my shape") otherwise, and what none
// of them takes is the tile kernel's.
struct GemmCall { int dtype, c_dtype, trans_a, trans_b, splits; float drop_p; };
int omr_gemm_panel_bf16(const GemmCall& call, const GemmArgs& g, hipStream_t s);      // gemm_panel.hip
int omr_gemm_tall_bf16(const GemmCall& call, const GemmArgs& g, hipStream_t s);       // gemm_tall.hip
