// KV-cached decoding as ONE host call per run of tokens (SURVEY.md section 8b `decode_step`, section 8f rank 1).
// Reference loop: Transformer.validation_step / get_pred_seq_and_pred_prob_seq (src/transformer/model.py:182-193,247-260)
// re-runs the whole decoder over the prefix for every token and reads the argmax back to the host each time.  Here
// run_position issues the kernels of ONE new position of ONE model back to back from C++ (no Python, no per-kernel argument
// marshalling): it appends that position's self-attention K|V to the cache by letting the K|V projection write straight into
// its cache row and reads the cross-attention K|V that were projected once per input.  A driver loops it over the positions of
// a call and chains the chosen token to the next position THROUGH DEVICE MEMORY, so n_steps tokens are produced without a single
// host synchronisation: greedy_steps (the head's fused pick), weighted_steps (two models, one mixed pick) here, beam_steps (one
// or two models, selection and cache reorder) in decode_beam.hip.  Every extern "C" entry is argument checks and one driver
// call.  Same kernels and the same per-row arithmetic as the training forward pass: the tokens equal the full re-run's
// (tests/test_model_gpu.py).
#include <utility>

#include "decode_common.h"

namespace omr_dec {

size_t carve(const omr_decode_desc& d, int rows, char* base, Ws* w) {
    const size_t es = d.dtype == OMR_BF16 ? 2 : 4, B = (size_t)rows;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
    char* x = take(B * d.d * es); char* x2 = take(B * d.d * es); char* q = take(B * d.d * es); char* o = take(B * d.d * es); char* proj = take(B * d.d * es);
    char* h = take(B * (size_t)d.ff * es); char* logits = take(B * (size_t)d.ldv * es);
    float* l32 = (float*)take(B * (size_t)d.ldv * 4); float* lse = (float*)take(B * (size_t)d.nhead * 4);
    float* mean = (float*)take(B * 4); float* rstd = (float*)take(B * 4);
    const int smax = d.S > d.max_len ? d.S : d.max_len;                // key-split partials of the longer of the two attentions
    const long sf = omr_attn_split_workspace_floats(rows, d.nhead, 1, smax, d.d / d.nhead);
    float* split = (float*)take((size_t)sf * 4);
    float* apart = (float*)take(2 * B * (size_t)((d.V + 15) / 16) * 4);      // greedy pick: the head kernel's per-workgroup candidates
    const size_t kmax = (size_t)(d.d > d.ff ? d.d : d.ff);
    unsigned char* a8 = (unsigned char*)take(d.fp8 ? B * ((kmax + 15) / 16 * 16) : 0);
    float* sa8 = (float*)take(d.fp8 ? B * 4 : 0);
    int* rows_tab = (int*)take(3 * B * (size_t)(d.max_len > 0 ? d.max_len : 0) * 4);
    if (w) *w = Ws{x, x2, q, o, proj, h, logits, l32, lse, mean, rstd, split, sf, apart, a8, sa8, rows_tab};
    return off;
}

int check_desc(const omr_decode_desc& d) {
    if (d.B <= 0 || d.L <= 0 || d.d <= 0 || d.d % d.nhead || d.V <= 0 || d.ldv < d.V || d.ldv % 8) return OMR_ERR_ARG;
    if (!d.emb || !d.pe || !d.layer_w || !d.head_w || !d.self_kv || !d.cross_kv) return OMR_ERR_ARG;
    if (d.fp8 && (!d.layer_w8 || !d.layer_s8 || !d.head_w8 || !d.head_s8 || d.d % 16 || d.ff % 16)) return OMR_ERR_ARG;
    return OMR_OK;
}

int check_model(const omr_decode_desc& d) {
    OMR_TRY(check_desc(d));
    if (!d.ws || d.ws_bytes < (long)carve(d, d.B, nullptr, nullptr)) return OMR_ERR_ARG;
    return OMR_OK;
}

// the positional-encoding table / cache must hold every position of the call (decoder.py:31): refused before the first launch,
// not at the position that runs out
int check_steps(int t0, int n_steps, int max_len) {
    return (n_steps < 1 || t0 < 0 || t0 + n_steps > max_len) ? OMR_ERR_ARG : OMR_OK;
}

Model make_model(const omr_decode_desc* d, const int* mem_len, int kv_group) {
    Model m = {d, Ws{}, mem_len, kv_group, d->B, 1};
    carve(*d, d->B, (char*)d->ws, &m.w);
    return m;
}

Model make_group_model(const omr_decode_desc* d, const int* mem_len, int group, void* ws) {
    Model m = {d, Ws{}, mem_len, group, d->B * group, group};      // the rows of a slot share its memory K|V: kv_group = group
    carve(*d, m.rows, (char*)ws, &m.w);
    return m;
}

int copy_logits(const Model& m, float* dst, const float* logits32, void* stream) {
    const size_t bytes = (size_t)m.rows * m.d->ldv * sizeof(float);
    return hipMemcpyAsync(dst, logits32, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess ? OMR_OK : OMR_ERR_LAUNCH;
}

}  // namespace omr_dec

using namespace omr_dec;

namespace {

// ------------------------------------------------------------------------------------------------
// The weights of a layer by name.  layer_w holds 18 pointers per layer (include/omr_hip.h): each of the six matrices followed by
// its bias, and norm k's gamma | beta after every second pair; layer_w8 / layer_s8 hold the six matrices in the enum's order.
enum LayerMatrix { SELF_IN, SELF_OUT, CROSS_Q, CROSS_OUT, FF1, FF2 };
struct Matrix { const void* w; const float* bias; const unsigned char* w8; const float* s8; int N, K, relu; };      // w8 / s8: fp8 mode only
struct Norm { const float* gamma; const float* beta; };

// SELF_IN: the packed q | k | v rows.  CROSS_Q: the q rows of the packed in_proj (the memory's K|V were projected once, at init).
// The one place that looks the fp8 pointers up.
Matrix layer_matrix(const omr_decode_desc& d, int l, LayerMatrix which) {
    static const int widx[6] = {0, 2, 6, 8, 12, 14};
    const void* const* W = d.layer_w + (size_t)l * OMR_DECODE_LAYER_PTRS;
    const int N = which == SELF_IN ? 3 * d.d : which == FF1 ? d.ff : d.d, K = which == FF2 ? d.ff : d.d;
    Matrix mx = {W[widx[which]], (const float*)W[widx[which] + 1], nullptr, nullptr, N, K, which == FF1};
    if (d.fp8) {
        mx.w8 = d.layer_w8[(size_t)l * OMR_DECODE_LAYER_FP8 + which];
        mx.s8 = d.layer_s8[(size_t)l * OMR_DECODE_LAYER_FP8 + which];
    }
    return mx;
}
// vocabulary head (Conv1d k=1, decoder.py:145-146)
Matrix head_matrix(const omr_decode_desc& d) {
    return Matrix{d.head_w, d.head_b, d.fp8 ? d.head_w8 : nullptr, d.fp8 ? d.head_s8 : nullptr, d.V, d.d, 0};
}
// output rows row0 .. row0 + N of a matrix
Matrix rows_of(Matrix mx, int row0, int N, size_t es) {
    mx.w = (const char*)mx.w + (size_t)row0 * mx.K * es; mx.bias += row0; mx.N = N;
    if (mx.w8) { mx.w8 += (size_t)row0 * mx.K; mx.s8 += row0; }
    return mx;
}
Norm layer_norm(const omr_decode_desc& d, int l, int k) {       // k = 0, 1, 2: norm1, norm2, norm3
    const void* const* W = d.layer_w + (size_t)l * OMR_DECODE_LAYER_PTRS;
    return Norm{(const float*)W[4 + 6 * k], (const float*)W[5 + 6 * k]};
}
char* self_cache(const omr_decode_desc& d, int l, size_t es) { return (char*)d.self_kv + ((size_t)l * d.B * d.max_len) * 2 * d.d * es; }
// banded causal mask = a key range (decoder.py:213-214): the first key position t sees
int band_start(const omr_decode_desc& d, int t) { return (d.window > 0 && t - d.window > 0) ? t - d.window : 0; }

// ------------------------------------------------------------------------------------------------
// Row path: 8 launches per layer (bf16 / fp32 weights, or e4m3 weights dequantised on load by the row kernel).  Every
// element-wise step between two linears (embedding + positional row, the three add + LayerNorm, the merge of the key-split
// attention) is folded into the loading of the NEXT linear's input rows (omr_decode_linear prologues), so a linear is a prologue,
// a matrix and a destination: one of the four helpers below fills the first two, the call site names the destination fields.
typedef omr_decode_linear_args Lin;

// what every row linear of the position shares
Lin shared_fields(const Model& m, const Position& p, const long* tok_in) {
    const omr_decode_desc& d = *m.d;
    Lin a = {};
    a.dtype = d.dtype; a.M = m.rows; a.H = d.nhead; a.hd = d.d / d.nhead; a.vocab = d.V; a.eps = 1e-5f; a.ld32 = d.ldv;
    a.tokens = tok_in; a.emb = d.emb; a.pe_row = d.pe + (size_t)p.t * d.d;
    return a;
}
void set_matrix(Lin& a, const Matrix& mx) {          // every column to out0 unless the call site sets n0
    a.w = mx.w; a.bias = mx.bias; a.w8 = mx.w8; a.w8_scale = mx.s8;
    a.N = mx.N; a.K = mx.K; a.relu = mx.relu; a.n0 = mx.N; a.ldx = mx.K; a.ldres = mx.K;
}
// input = the rows of x
Lin plain_linear(const Lin& shared, const Matrix& mx, const void* x) {
    Lin a = shared;
    a.pro = 0; a.x = x;
    set_matrix(a, mx);
    return a;
}
// input = LayerNorm(y + res), also stored to xn_out
Lin ln_linear(const Lin& shared, const Matrix& mx, const void* y, const void* res, Norm norm, void* xn_out) {
    Lin a = shared;
    a.pro = 1; a.x = y; a.res = res; a.gamma = norm.gamma; a.beta = norm.beta; a.xn_out = xn_out;
    set_matrix(a, mx);
    return a;
}
// input = embedding[token] + positional row, also stored to xn_out
Lin embed_linear(const Lin& shared, const Matrix& mx, void* xn_out) {
    Lin a = shared;
    a.pro = 2; a.xn_out = xn_out;
    set_matrix(a, mx);
    return a;
}
// input = the attention output: the ns key-split partials merged on load, or the rows of o where the attention did not split
Lin merged_linear(const Lin& shared, const Matrix& mx, const Ws& w, int ns) {
    Lin a = shared;
    a.pro = ns > 1 ? 3 : 0; a.x = w.o; a.part = w.split; a.nsplit = ns;
    set_matrix(a, mx);
    return a;
}

int row_position(const Model& m, const Position& p, const long* tok_in, Pick pick, void* stream) {
    const omr_decode_desc& d = *m.d;
    const Ws& w = m.w;
    const int dt = d.dtype, B = m.rows, dm = d.d, hd = dm / d.nhead, t = p.t, lo = band_start(d, t);
    const size_t es = dt == OMR_BF16 ? 2 : 4;
    const long kv_ld = (long)d.max_len * 2 * dm;
    const Lin shared = shared_fields(m, p, tok_in);
    if (m.group > 1 && !p.row_pos) return OMR_ERR_ARG;                           // a grouped position has its rows' tables
    // the residual stream alternates between two buffers because the workgroup that stores a freshly normalised row runs beside
    // workgroups still reading the previous one.  xa: the stream entering the sub-layer
    char* xa = w.x; char* xb = w.x2;
    Norm norm3 = {};                                                            // of the previous layer, still to be applied
    for (int l = 0; l < d.L; ++l) {
        char* cache_l = self_cache(d, l, es);
        // q | k|v projection of the position: q -> w.q, k|v straight into the rows' cache row.  Its input is the embedding (layer 0)
        // or norm3(x + ffn) of the previous layer; either way the rows land in xb
        const Matrix in = layer_matrix(d, l, SELF_IN);
        Lin qkv = l == 0 ? embed_linear(shared, in, xb) : ln_linear(shared, in, w.proj, xa, norm3, xb);
        qkv.out0 = w.q; qkv.ld0 = dm; qkv.n0 = dm; qkv.ld1 = kv_ld;
        if (p.row_pos) {                    // per-row positions: the kernel adds each row's own positional and cache row
            qkv.pe_row = d.pe; qkv.out1 = cache_l;
            OMR_TRY(decode_linear_impl(qkv, p.row_pos, 2L * dm, stream, m.group));
        } else {
            qkv.out1 = cache_l + (size_t)t * 2 * dm * es;
            OMR_TRY(decode_linear_impl(qkv, nullptr, 0, stream));
        }
        std::swap(xa, xb);
        int ns = 1;
        if (m.group > 1) {      // row b over keys [lo_b, t_b] of slot b / group: those of the rows before it in its group were written
                                // by the launch above
            OMR_TRY(attn_fwd_split_partials_group(dt, w.q, cache_l, cache_l + (size_t)dm * es, w.o, w.lse, dm, 2 * dm, 2 * dm, dm, dm, kv_ld, kv_ld, dm, B,
                                              d.nhead, 1, t + 1 - lo, hd, p.kv_count, p.kv_start, m.group, w.split, w.split_floats, &ns, stream));
        } else if (p.row_pos) { // row b over its own keys [lo_b, t_b]; the split plan is that of the furthest row's count
            OMR_TRY(attn_fwd_split_partials_rows(dt, w.q, cache_l, cache_l + (size_t)dm * es, w.o, w.lse, dm, 2 * dm, 2 * dm, dm, dm, kv_ld, kv_ld, dm, B,
                                             d.nhead, 1, t + 1 - lo, hd, p.kv_count, p.kv_start, w.split, w.split_floats, &ns, stream));
        } else {
            const char* k0 = cache_l + (size_t)lo * 2 * dm * es;
            OMR_TRY(omr_attn_fwd_split_partials(dt, w.q, k0, k0 + (size_t)dm * es, w.o, w.lse, dm, 2 * dm, 2 * dm, dm, dm, kv_ld, kv_ld, dm, B, d.nhead, 1,
                                            t + 1 - lo, hd, w.split, w.split_floats, &ns, stream));
        }
        Lin out = merged_linear(shared, layer_matrix(d, l, SELF_OUT), w, ns);
        out.out0 = w.proj; out.ld0 = dm;
        OMR_TRY(decode_linear_impl(out, nullptr, 0, stream));
        // cross-attention query from norm1(x + self-attention)
        Lin cq = ln_linear(shared, layer_matrix(d, l, CROSS_Q), w.proj, xa, layer_norm(d, l, 0), xb);
        cq.out0 = w.q; cq.ld0 = dm;
        OMR_TRY(decode_linear_impl(cq, nullptr, 0, stream));
        std::swap(xa, xb);
        const char* ck = (const char*)d.cross_kv + (size_t)l * 2 * dm * es;
        OMR_TRY(attn_fwd_split_partials_varlen(dt, w.q, ck, ck + (size_t)dm * es, w.o, w.lse, dm, d.cross_ld, d.cross_ld, dm, dm, d.cross_bs, d.cross_bs,
                                           dm, B, d.nhead, 1, d.S, hd, m.mem_len, w.split, w.split_floats, &ns, stream, m.kv_group));
        Lin co = merged_linear(shared, layer_matrix(d, l, CROSS_OUT), w, ns);
        co.out0 = w.proj; co.ld0 = dm;
        OMR_TRY(decode_linear_impl(co, nullptr, 0, stream));
        // feed-forward from norm2(x + cross-attention)
        Lin f1 = ln_linear(shared, layer_matrix(d, l, FF1), w.proj, xa, layer_norm(d, l, 1), xb);
        f1.out0 = w.h; f1.ld0 = d.ff;
        OMR_TRY(decode_linear_impl(f1, nullptr, 0, stream));
        std::swap(xa, xb);
        Lin f2 = plain_linear(shared, layer_matrix(d, l, FF2), w.h);
        f2.out0 = w.proj; f2.ld0 = dm;
        OMR_TRY(decode_linear_impl(f2, nullptr, 0, stream));
        norm3 = layer_norm(d, l, 2);
    }
    // vocabulary head on norm3 of the last layer: logits rounded to the compute dtype like the training forward, kept as fp32
    // rows ... and the greedy pick (model.py:187,253): candidates from the head's workgroups, one small launch to reduce them
    Lin head = ln_linear(shared, head_matrix(d), w.proj, xa, norm3, xb);
    head.out0 = w.logits; head.ld0 = d.ldv; head.out32 = w.logits32;
    head.amax_idx = pick.idx; head.amax_val = pick.val; head.amax_part = pick.idx ? w.apart : nullptr;
    return decode_linear_impl(head, nullptr, 0, stream);
}

// ------------------------------------------------------------------------------------------------
// Generic path, for the model widths the row kernel does not take: one GEMM / element-wise kernel per step of the layer.
// One linear: bf16 / fp32 GEMM on the matrix, or (fp8 mode) quantise the B input rows per token and run the fp8 MFMA GEMM on the
// pre-quantised rows and their scales.
int gemm(const Model& m, const Matrix& mx, const void* a, void* c, long ldc, void* stream) {
    const omr_decode_desc& d = *m.d;
    const int dt = d.dtype;
    if (!d.fp8) return omr_gemm(dt, dt, 0, 0, d.B, mx.N, mx.K, a, mx.K, mx.w, mx.K, c, ldc, mx.bias, mx.relu, 0, 1, nullptr, 0.f, 0, 0, 0, 0, 0, stream);
    const long lda8 = (mx.K + 15) / 16 * 16;
    OMR_TRY(omr_quantize_rows_fp8(dt, a, mx.K, m.w.a8, lda8, m.w.sa8, d.B, mx.K, stream));
    return omr_gemm_fp8(dt, d.B, mx.N, mx.K, m.w.a8, lda8, m.w.sa8, mx.w8, mx.K, mx.s8, c, ldc, mx.bias, mx.relu, stream);
}

int add_norm(const Model& m, Norm norm, void* stream) {      // x <- LayerNorm(proj + x)
    const Ws& w = m.w;
    return omr_add_layernorm_fwd(m.d->dtype, w.proj, w.x, norm.gamma, norm.beta, w.x, w.mean, w.rstd, m.d->B, m.d->d, 1e-5f, 0.f, 0, stream);
}

int gemm_position(const Model& m, int t, const long* tok_in, Pick pick, float** logits32, void* stream) {
    const omr_decode_desc& d = *m.d;
    const Ws& w = m.w;
    const int dt = d.dtype, B = d.B, dm = d.d, hd = dm / d.nhead, lo = band_start(d, t);
    const size_t es = dt == OMR_BF16 ? 2 : 4;
    const long kv_ld = (long)d.max_len * 2 * dm;
    // embedding(tgt) + pe[t]  (decoder.py:124; T_len = 1 so every row of the batch takes the table row given)
    OMR_TRY(omr_embed_pe_fwd(dt, tok_in, d.emb, d.pe + (size_t)t * dm, w.x, B, 1, dm, d.V, stream));
    for (int l = 0; l < d.L; ++l) {
        char* cache_l = self_cache(d, l, es);
        // self-attention: q rows of the packed in_proj; the k|v rows go straight into position t of the cache
        const Matrix in = layer_matrix(d, l, SELF_IN);
        OMR_TRY(gemm(m, rows_of(in, 0, dm, es), w.x, w.q, dm, stream));
        OMR_TRY(gemm(m, rows_of(in, dm, 2 * dm, es), w.x, cache_l + (size_t)t * 2 * dm * es, kv_ld, stream));
        const char* k0 = cache_l + (size_t)lo * 2 * dm * es;
        OMR_TRY(omr_attn_fwd_split(dt, w.q, k0, k0 + (size_t)dm * es, w.o, w.lse, dm, 2 * dm, 2 * dm, dm, dm, kv_ld, kv_ld, dm, B, d.nhead, 1, t + 1 - lo, hd,
                               nullptr, w.split, w.split_floats, stream));
        OMR_TRY(gemm(m, layer_matrix(d, l, SELF_OUT), w.o, w.proj, dm, stream));
        OMR_TRY(add_norm(m, layer_norm(d, l, 0), stream));
        // cross-attention over the memory K|V projected once (init): layer l's block of the [B][S][L*2d] buffer
        OMR_TRY(gemm(m, layer_matrix(d, l, CROSS_Q), w.x, w.q, dm, stream));
        const char* ck = (const char*)d.cross_kv + (size_t)l * 2 * dm * es;
        if (m.kv_group == 1)
            OMR_TRY(omr_attn_fwd_split_varlen(dt, w.q, ck, ck + (size_t)dm * es, w.o, w.lse, dm, d.cross_ld, d.cross_ld, dm, dm, d.cross_bs, d.cross_bs, dm,
                                          B, d.nhead, 1, d.S, hd, nullptr, m.mem_len, w.split, w.split_floats, stream));
        else        // shared K|V slots exist in the key-split kernel only (S > 64); the partials are merged there
            OMR_TRY(attn_fwd_split_partials_varlen(dt, w.q, ck, ck + (size_t)dm * es, w.o, w.lse, dm, d.cross_ld, d.cross_ld, dm, dm, d.cross_bs, d.cross_bs,
                                               dm, B, d.nhead, 1, d.S, hd, m.mem_len, w.split, w.split_floats, nullptr, stream, m.kv_group));
        OMR_TRY(gemm(m, layer_matrix(d, l, CROSS_OUT), w.o, w.proj, dm, stream));
        OMR_TRY(add_norm(m, layer_norm(d, l, 1), stream));
        // feed-forward
        OMR_TRY(gemm(m, layer_matrix(d, l, FF1), w.x, w.h, d.ff, stream));
        OMR_TRY(gemm(m, layer_matrix(d, l, FF2), w.h, w.proj, dm, stream));
        OMR_TRY(add_norm(m, layer_norm(d, l, 2), stream));
    }
    // vocabulary head in the compute dtype like the training forward, then fp32 rows
    OMR_TRY(gemm(m, head_matrix(d), w.x, w.logits, d.ldv, stream));
    float* l32 = w.logits32;
    if (dt == OMR_F32) l32 = (float*)w.logits;
    else OMR_TRY(omr_cast(w.logits, dt, w.logits32, OMR_F32, (long)B * d.ldv, stream));
    if (pick.idx) OMR_TRY(omr_argmax(l32, B, d.V, d.ldv, pick.idx, pick.val, stream));      // greedy pick (model.py:187,253)
    *logits32 = l32;
    return OMR_OK;
}

}  // namespace

int omr_dec::run_position(const Model& m, const Position& p, const long* tok_in, Pick pick, float** logits32, void* stream) {
    if (takes_row_kernel(*m.d)) {
        *logits32 = m.w.logits32;
        return row_position(m, p, tok_in, pick, stream);
    }
    if (p.row_pos) return OMR_ERR_UNSUPPORTED;          // per-row positions exist in the row kernel only
    return gemm_position(m, p.t, tok_in, pick, logits32, stream);
}

extern "C" long omr_decode_workspace_bytes(const omr_decode_desc* d) {
    if (!d || d->B <= 0 || d->d <= 0 || d->ff <= 0 || d->ldv < d->V) return OMR_ERR_ARG;
    return (long)carve(*d, d->B, nullptr, nullptr);
}

extern "C" long omr_decode_group_workspace_bytes(const omr_decode_desc* d, int R) {
    if (!d || d->B <= 0 || d->d <= 0 || d->ff <= 0 || d->ldv < d->V || R < 2 || R > OMR_MAX_VERIFY_ROWS) return OMR_ERR_ARG;
    return (long)carve(*d, d->B * R, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------------
// A grouped position: R consecutive positions of every slot as the rows of ONE pass of the row path (row_position with a group
// model).  Row b * R + r feeds tokens[b][r] to position pos[b] + r; within a layer the q|k|v launch of all rows completes before
// the attention launch, so row r reads the K|V rows r' < r of its group wrote.  Nothing is advanced.
int omr_dec::verify_rows(const omr_decode_desc* dp, const int* mem_len, const int* pos, int t_max, int R, const long* tokens, long* out_tokens,
                         float* out_top1, void* ws, long ws_bytes, void* stream) {
    if (!dp) return OMR_ERR_ARG;
    if (!takes_row_kernel(*dp)) return OMR_ERR_UNSUPPORTED;
    if (!pos || !tokens || !out_tokens || !ws) return OMR_ERR_ARG;
    if (R < 2 || R > OMR_MAX_VERIFY_ROWS || t_max < 0 || t_max + R > dp->max_len) return OMR_ERR_ARG;
    if (dp->S <= 64) return OMR_ERR_UNSUPPORTED;          // the rows of a slot share its memory K|V: the key-split kernel only (S > 64)
    OMR_TRY(check_desc(*dp));
    if (ws_bytes < (long)carve(*dp, dp->B * R, nullptr, nullptr)) return OMR_ERR_ARG;
    const Model m = make_group_model(dp, mem_len, R, ws);
    const Position p = launch_group_tables(m, pos, t_max, stream);
    return row_position(m, p, tokens, Pick{out_tokens, out_top1}, stream);
}

extern "C" int omr_decode_verify_rows(const omr_decode_desc* dp, const int* mem_len, const int* pos, int t_max, int R, const long* tokens,
                                      long* out_tokens, float* out_top1, void* ws, long ws_bytes, void* stream) {
    return verify_rows(dp, mem_len, pos, t_max, R, tokens, out_tokens, out_top1, ws, ws_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// Greedy driver.  Positions t0 .. t0 + n_steps - 1; pos (nullable, device int32 [B]): the per-row-position form
// (omr_decode_steps_rows) -- row b runs positions pos[b] + s and t0 is the LARGEST of those first positions.
// g (nullable; the *_grammar entries, checked there): the constrained pick -- the position runs without a pick (the head without
// its pick halves, or no omr_argmax) and ONE omr_grammar_pick launch over its fp32 logits writes the same outputs and advances
// g->state, so the launches per position are the unconstrained count.
namespace {

struct Run { int t0, n_steps; const int* pos; };

int greedy_steps(const omr_decode_desc* dp, const int* mem_len, Run run, const omr_grammar_desc* g, long* tokens, long* out_tokens, float* out_top1,
                 float* last_logits, void* stream) {
    if (!dp || !tokens || (g && !out_tokens)) return OMR_ERR_ARG;
    OMR_TRY(check_model(*dp));
    OMR_TRY(check_steps(run.t0, run.n_steps, dp->max_len));
    if (run.n_steps > 1 && !out_tokens) return OMR_ERR_ARG;             // several steps need the token feedback
    const bool row_kernel = takes_row_kernel(*dp);
    const Model m = make_model(dp, mem_len, 1);
    const size_t B = (size_t)dp->B;
    if (run.pos) launch_rows_tables(m, run.pos, 0, run.n_steps, stream);
    // The picked token reaches the next position through device memory.  Row path: the next position reads it where the pick
    // wrote it, and `tokens` is brought up to date once, after the run.  Generic path: `tokens` is, after every position.
    const long* tok_in = tokens;
    float* l32 = nullptr;
    for (int s = 0; s < run.n_steps; ++s) {
        const Pick pick = {out_tokens ? out_tokens + s * B : nullptr, (out_tokens && out_top1) ? out_top1 + s * B : nullptr};
        OMR_TRY(run_position(m, position_at(m, run.pos, run.t0 + s, s), tok_in, g ? Pick{nullptr, nullptr} : pick, &l32, stream));
        if (g) OMR_TRY(omr_grammar_pick(l32, dp->ldv, dp->B, dp->V, g, pick.idx, pick.val, nullptr, stream));
        if (!out_tokens) break;                                         // one position without a pick
        if (row_kernel) tok_in = pick.idx;
        if (!row_kernel || s == run.n_steps - 1)
            if (hipMemcpyAsync(tokens, pick.idx, B * sizeof(long), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return OMR_ERR_LAUNCH;
    }
    if (last_logits) OMR_TRY(copy_logits(m, last_logits, l32, stream));
    return OMR_OK;
}

}  // namespace

extern "C" int omr_decode_steps(const omr_decode_desc* dp, long* tokens, int t0, int n_steps, long* out_tokens, float* out_top1,
                                float* last_logits, void* stream) {
    return greedy_steps(dp, nullptr, Run{t0, n_steps, nullptr}, nullptr, tokens, out_tokens, out_top1, last_logits, stream);
}

/* omr_decode_steps over a ragged batch of memories: desc->S is the padded memory length, row b attends over mem_len[b] of it */
extern "C" int omr_decode_steps_varlen(const omr_decode_desc* dp, const int* mem_len, long* tokens, int t0, int n_steps, long* out_tokens,
                                       float* out_top1, float* last_logits, void* stream) {
    if (!mem_len) return OMR_ERR_ARG;
    return greedy_steps(dp, mem_len, Run{t0, n_steps, nullptr}, nullptr, tokens, out_tokens, out_top1, last_logits, stream);
}

/* omr_decode_steps_varlen for a state whose rows each sit at their own position (continuous batching of the reference's greedy
 * loop, src/transformer/model.py:171-199): row b runs positions pos[b] .. pos[b] + n_steps - 1.  Whether the descriptor takes
 * this entry is answered first, so that a caller can ask with NULL pointers. */
extern "C" int omr_decode_steps_rows(const omr_decode_desc* dp, const int* mem_len, const int* pos, int t_max, long* tokens, int n_steps,
                                     long* out_tokens, float* out_top1, float* last_logits, void* stream) {
    if (!dp) return OMR_ERR_ARG;
    if (!takes_row_kernel(*dp)) return OMR_ERR_UNSUPPORTED;
    if (!pos) return OMR_ERR_ARG;
    return greedy_steps(dp, mem_len, Run{t_max, n_steps, pos}, nullptr, tokens, out_tokens, out_top1, last_logits, stream);
}

/* The three greedy entries under a token automaton (include/omr_hip.h "grammar-constrained decoding"; an extension of the loop of
 * src/transformer/model.py:182-193): the same driver with the constrained pick; the descriptor is checked here. */
extern "C" int omr_decode_steps_grammar(const omr_decode_desc* dp, const omr_grammar_desc* g, long* tokens, int t0, int n_steps, long* out_tokens,
                                        float* out_top1, float* last_logits, void* stream) {
    if (!grammar_desc_ok(g)) return OMR_ERR_ARG;
    return greedy_steps(dp, nullptr, Run{t0, n_steps, nullptr}, g, tokens, out_tokens, out_top1, last_logits, stream);
}

extern "C" int omr_decode_steps_varlen_grammar(const omr_decode_desc* dp, const int* mem_len, const omr_grammar_desc* g, long* tokens, int t0,
                                               int n_steps, long* out_tokens, float* out_top1, float* last_logits, void* stream) {
    if (!mem_len || !grammar_desc_ok(g)) return OMR_ERR_ARG;
    return greedy_steps(dp, mem_len, Run{t0, n_steps, nullptr}, g, tokens, out_tokens, out_top1, last_logits, stream);
}

extern "C" int omr_decode_steps_rows_grammar(const omr_decode_desc* dp, const int* mem_len, const int* pos, int t_max, const omr_grammar_desc* g,
                                             long* tokens, int n_steps, long* out_tokens, float* out_top1, float* last_logits, void* stream) {
    if (!dp) return OMR_ERR_ARG;
    if (!takes_row_kernel(*dp)) return OMR_ERR_UNSUPPORTED;
    if (!pos || !grammar_desc_ok(g)) return OMR_ERR_ARG;
    return greedy_steps(dp, mem_len, Run{t_max, n_steps, pos}, g, tokens, out_tokens, out_top1, last_logits, stream);
}

// ------------------------------------------------------------------------------------------------
/* Weighted late fusion (src/multimodal/weighted_multimodal/test.py:21-70) as ONE host call per run of tokens: two unimodal
 * models with their own KV caches decode the same prefixes in lock-step; per position both models run their position for all
 * B rows without a pick (fp32 logits only, copied to that side's `logits`), ONE omr_weighted_argmax_rows launch mixes the two
 * softmaxes of every row and picks, and the tokens reach BOTH models' next position through device memory (`tokens`, written by
 * the same launch).  mem_len (nullable, independently per side): ragged memories of that model.  Rows never interact, so a row
 * equals the pair decoded alone (omr_weighted_decode_steps) whenever both of its memories take the key-split attention (> 64
 * tokens).  run.pos: one pos / t0 for both models (the two models of a pair are always at the same position); each model's
 * tables are filled per position, for that position alone.  g (nullable; the *_grammar entries): omr_weighted_grammar_pick stands
 * where omr_weighted_argmax_rows stood, one state per row for both models. */
namespace {

struct Side { const omr_decode_desc* d; const int* mem_len; float* logits; };

int weighted_steps(const Side (&side)[2], Run run, const omr_grammar_desc* g, float alpha, long* tokens, long* out_tokens, float* out_prob, void* stream) {
    const omr_decode_desc *da = side[0].d, *db = side[1].d;
    if (!tokens || !out_tokens || !side[0].logits || !side[1].logits) return OMR_ERR_ARG;
    if (da->B < 1 || da->B != db->B || da->V != db->V) return OMR_ERR_ARG;
    for (const Side& sd : side) OMR_TRY(check_steps(run.t0, run.n_steps, sd.d->max_len));
    Model m[2];
    const size_t B = (size_t)da->B;
    for (int s = 0; s < run.n_steps; ++s) {
        for (int k = 0; k < 2; ++k) {
            float* l32 = nullptr;
            if (s == 0) {               // a descriptor is looked into when its model's first position comes up, as it always was
                OMR_TRY(check_model(*side[k].d));
                m[k] = make_model(side[k].d, side[k].mem_len, 1);
            }
            if (run.pos) launch_rows_tables(m[k], run.pos, s, 1, stream);
            OMR_TRY(run_position(m[k], position_at(m[k], run.pos, run.t0 + s, 0), tokens, Pick{nullptr, nullptr}, &l32, stream));
            OMR_TRY(copy_logits(m[k], side[k].logits, l32, stream));
        }
        if (g)
            OMR_TRY(omr_weighted_grammar_pick(side[0].logits, da->ldv, side[1].logits, db->ldv, (int)B, da->V, alpha, g, out_tokens + s * B,
                                          out_prob ? out_prob + s * B : nullptr, tokens, stream));
        else
            OMR_TRY(omr_weighted_argmax_rows(side[0].logits, da->ldv, side[1].logits, db->ldv, (int)B, da->V, alpha, out_tokens + s * B,
                                         out_prob ? out_prob + s * B : nullptr, tokens, stream));
    }
    return OMR_OK;
}

}  // namespace

extern "C" int omr_weighted_decode_steps_varlen(const omr_decode_desc* da, const int* mem_len_a, const omr_decode_desc* db, const int* mem_len_b,
                                                float alpha, long* tokens, int t0, int n_steps, long* out_tokens, float* out_prob, float* logits_a,
                                                float* logits_b, void* stream) {
    if (!da || !db) return OMR_ERR_ARG;
    const Side side[2] = {{da, mem_len_a, logits_a}, {db, mem_len_b, logits_b}};
    return weighted_steps(side, Run{t0, n_steps, nullptr}, nullptr, alpha, tokens, out_tokens, out_prob, stream);
}

/* omr_weighted_decode_steps_varlen over rows at their own positions.  As in omr_decode_steps_rows, whether both descriptors
 * take this entry is answered before any other argument is looked at. */
extern "C" int omr_weighted_decode_steps_rows(const omr_decode_desc* da, const int* mem_len_a, const omr_decode_desc* db, const int* mem_len_b,
                                              const int* pos, int t_max, float alpha, long* tokens, int n_steps, long* out_tokens,
                                              float* out_prob, float* logits_a, float* logits_b, void* stream) {
    if (!da || !db) return OMR_ERR_ARG;
    if (!takes_row_kernel(*da) || !takes_row_kernel(*db)) return OMR_ERR_UNSUPPORTED;
    if (!pos) return OMR_ERR_ARG;
    const Side side[2] = {{da, mem_len_a, logits_a}, {db, mem_len_b, logits_b}};
    return weighted_steps(side, Run{t_max, n_steps, pos}, nullptr, alpha, tokens, out_tokens, out_prob, stream);
}

/* The two batched fusion entries under a token automaton (include/omr_hip.h "grammar-constrained decoding"; an extension of
 * weighted_multimodal/test.py:21-70). */
extern "C" int omr_weighted_decode_steps_varlen_grammar(const omr_decode_desc* da, const int* mem_len_a, const omr_decode_desc* db, const int* mem_len_b,
                                                        const omr_grammar_desc* g, float alpha, long* tokens, int t0, int n_steps, long* out_tokens,
                                                        float* out_prob, float* logits_a, float* logits_b, void* stream) {
    if (!da || !db || !grammar_desc_ok(g)) return OMR_ERR_ARG;
    const Side side[2] = {{da, mem_len_a, logits_a}, {db, mem_len_b, logits_b}};
    return weighted_steps(side, Run{t0, n_steps, nullptr}, g, alpha, tokens, out_tokens, out_prob, stream);
}

extern "C" int omr_weighted_decode_steps_rows_grammar(const omr_decode_desc* da, const int* mem_len_a, const omr_decode_desc* db, const int* mem_len_b,
                                                      const int* pos, int t_max, const omr_grammar_desc* g, float alpha, long* tokens, int n_steps,
                                                      long* out_tokens, float* out_prob, float* logits_a, float* logits_b, void* stream) {
    if (!da || !db) return OMR_ERR_ARG;
    if (!takes_row_kernel(*da) || !takes_row_kernel(*db)) return OMR_ERR_UNSUPPORTED;
    if (!pos || !grammar_desc_ok(g)) return OMR_ERR_ARG;
    const Side side[2] = {{da, mem_len_a, logits_a}, {db, mem_len_b, logits_b}};
    return weighted_steps(side, Run{t_max, n_steps, pos}, g, alpha, tokens, out_tokens, out_prob, stream);
}

/* bs = 1 like the reference (test.py:27): the one-row, full-memory case */
extern "C" int omr_weighted_decode_steps(const omr_decode_desc* da, const omr_decode_desc* db, float alpha, long* tokens, int t0, int n_steps,
                                         long* out_tokens, float* out_prob, float* logits_a, float* logits_b, void* stream) {
    if (!da || !db || da->B != 1 || db->B != 1) return OMR_ERR_ARG;
    return omr_weighted_decode_steps_varlen(da, nullptr, db, nullptr, alpha, tokens, t0, n_steps, out_tokens, out_prob, logits_a, logits_b, stream);
}
