// Batched beam search on the device (include/omr_hip.h "batched beam search").  The host loop it reproduces is
// _Base.beam_search of this package's model.py; the three pieces per position are a model's position without a pick
// (run_position, decode.hip), the selection kernel and the cache reorder below.
#include "decode_common.h"

using namespace omr_dec;

namespace {

constexpr int BEAM_GROUPS = 4;         // rows of an input ranked side by side: one 256-thread group each

// Phase 2 of a selection kernel, one workgroup per input n (every thread calls it): the beam * beam (<= 64) candidates
// (c_tok, c_val)[parent * beam + j] that phase 1 left in LDS get fp64 scores from the live rows, wave 0 ranks them by all-pairs
// comparison, one candidate per lane, and walks them in order as ballots -- the host loop's walk (_Base.beam_search): finished
// record, stop rule, survivors and dead padding (`put`).  One definition for the selection kernels.
// g (absent in the unconstrained kernels; omr_grammar_desc of the constrained ones): a candidate is live only if its parent is
// live AND the table allows its token in the parent's state -- decided by next[state[parent]][cls[token]], not by the value, so
// a forbidden token (phase 1 emits them, at -inf, where a state allows fewer than `beam` tokens) is never a survivor, a finished
// hypothesis or a history entry.  Every candidate's successor state is looked up from the input's OLD states here, before the
// barriers that precede the first `put`; a survivor's slot gets its own, dead padding rows the first survivor's.
__device__ __forceinline__ void beam_rank_and_put(const omr_beam_desc& bd, int n, int t, const float* c_val, const int* c_tok,
                                                  const omr_grammar_desc* g = nullptr) {
    __shared__ double u_sc[64], o_sc[64];          // candidates as found / in order
    __shared__ int u_live[64], o_tok[64], o_par[64], o_ok[64];
    __shared__ int old_state[OMR_MAX_BEAM], o_ns[64];
    const int beam = bd.beam, row0 = n * beam, lane = threadIdx.x;
    if (g && lane < beam) old_state[lane] = min(max(g->state[row0 + lane], 0), g->S - 1);
    __syncthreads();
    const int nc = beam * beam;
    double sc = 0.0; int par = 0, tok = 0, ns = 0; bool live = false;
    if (lane < 64) {
        o_ok[lane] = 0;
        if (lane < nc) {
            par = lane / beam; tok = c_tok[lane];
            const double ps = bd.scores[row0 + par];
            live = ps > -INFINITY;                  // dead rows contribute no candidates
            sc = ps + (double)c_val[lane];
            if (g) {
                const int c = g->cls[tok];            // a class the table does not hold is forbidden, never an index past its row
                ns = c < g->C ? g->next[(long)old_state[par] * g->C + c] : -1;
                live = live && ns >= 0 && ns < g->S;
            }
        }
        u_sc[lane] = sc; u_live[lane] = live;
    }
    __syncthreads();
    if (lane < 64 && live) {                        // (score descending, parent ascending, token ascending); lane = parent * beam + j
        int rank = 0;
        for (int c = 0; c < nc; ++c) {
            if (!u_live[c] || c == lane) continue;
            const double s2 = u_sc[c]; const int p2 = c / beam, t2 = c_tok[c];
            if (s2 > sc || (s2 == sc && (p2 < par || (p2 == par && t2 < tok)))) ++rank;
        }
        o_sc[rank] = sc; o_tok[rank] = tok; o_par[rank] = par; o_ok[rank] = 1;
        if (g) o_ns[rank] = ns;
    }
    __syncthreads();
    if (lane >= 64) return;
    const bool ok = o_ok[lane] != 0;
    sc = o_sc[lane]; tok = o_tok[lane]; par = o_par[lane];
    const bool is_eos = ok && tok == bd.eos, alive = ok && !is_eos;
    const unsigned long long live_mask = __ballot(alive);
    const int before = __popcll(live_mask & ((1ull << lane) - 1ull));       // non-<eos> candidates ahead of this one
    const bool surv = alive && before < beam;
    const unsigned long long eos_mask = __ballot(is_eos && before < beam);    // the host loop breaks after the beam-th survivor
    double best = bd.best_score[n];
    if (eos_mask) {                                 // the first <eos> in the order has the largest score of them
        const int fl = __ffsll(eos_mask) - 1;
        const double es = o_sc[fl];
        if (es > best) {
            best = es;
            if (lane == 0) { bd.best_score[n] = es; bd.best_row[n] = o_par[fl]; bd.best_pos[n] = t; }
        }
    }
    const int first = live_mask ? __ffsll(live_mask) - 1 : 0;
    if (!live_mask || o_sc[first] <= best) {        // nothing survives, or no survivor can overtake the best finished hypothesis
        if (lane == 0) { bd.done[n] = 1; bd.exhausted[n] = 0; }
        return;
    }
    const int nsurv = min(__popcll(live_mask), beam);
    const long hrow = (long)t * bd.N * beam;
    auto put = [&](int slot, int p_out, int t_out, double s_out, int rank) {
        const int r = row0 + slot;
        bd.parents[r] = p_out; bd.tokens[r] = t_out; bd.scores[r] = s_out;
        bd.hist_parent[hrow + r] = p_out; bd.hist_token[hrow + r] = t_out;
        if (g) g->state[r] = o_ns[rank];
    };
    if (surv) put(before, par, tok, sc, lane);
    if (lane >= nsurv && lane < beam) put(lane, o_par[first], o_tok[first], -INFINITY, first);      // dead padding rows: copies of the first survivor
}

// One workgroup per input.  Phase 1: the top `beam` log-probabilities of each of its rows (topk_logprob_row, the row body of
// omr_topk_logprob), BEAM_GROUPS rows side by side.  Phase 2: beam_rank_and_put.
__global__ __launch_bounds__(256 * BEAM_GROUPS) void beam_select_kernel(const float* __restrict__ logits, long ld, int V, omr_beam_desc bd, int t) {
    __shared__ float sv[BEAM_GROUPS][256];
    __shared__ int si[BEAM_GROUPS][256];
    __shared__ float c_val[64];
    __shared__ int c_tok[64];
    const int n = blockIdx.x, beam = bd.beam, row0 = n * beam;
    if (bd.done[n]) return;                         // frozen (uniform over the workgroup)
    const int g = threadIdx.x >> 8, tid = threadIdx.x & 255;
    for (int k0 = 0; k0 < beam; k0 += BEAM_GROUPS) {
        const int k = k0 + g;
        const bool real = k < beam;                 // a group without a row walks an empty one: the barriers stay uniform
        topk_logprob_row(logits + (long)(row0 + (real ? k : 0)) * ld, real ? V : 0, beam, tid, sv[g], si[g], [&](int j, int idx, float val) {
            if (tid == 0 && real) { c_tok[k * beam + j] = idx; c_val[k * beam + j] = val; }
        });
    }
    beam_rank_and_put(bd, n, t, c_val, c_tok);
}

// beam_select_kernel as two launches, for a selection that re-scores the candidates in between (omr_beam_select_ctc: the CTC prefix
// scores of ctc_prefix.hip scan thousands of frames with one wave per input).  Phase 1 alone: input n's candidates (token, value) go to
// g_tok / g_val [N][beam * beam] in the order c_tok / c_val have in LDS above.
__global__ __launch_bounds__(256 * BEAM_GROUPS) void beam_topk_kernel(const float* __restrict__ logits, long ld, int V, omr_beam_desc bd,
                                                                      long* __restrict__ g_tok, float* __restrict__ g_val) {
    __shared__ float sv[BEAM_GROUPS][256];
    __shared__ int si[BEAM_GROUPS][256];
    const int n = blockIdx.x, beam = bd.beam, row0 = n * beam;
    if (bd.done[n]) return;                         // frozen (uniform over the workgroup)
    const int g = threadIdx.x >> 8, tid = threadIdx.x & 255;
    const long c0 = (long)row0 * beam;
    for (int k0 = 0; k0 < beam; k0 += BEAM_GROUPS) {
        const int k = k0 + g;
        const bool real = k < beam;                 // a group without a row walks an empty one: the barriers stay uniform
        topk_logprob_row(logits + (long)(row0 + (real ? k : 0)) * ld, real ? V : 0, beam, tid, sv[g], si[g], [&](int j, int idx, float val) {
            if (tid == 0 && real) { g_tok[c0 + k * beam + j] = idx; g_val[c0 + k * beam + j] = val; }
        });
    }
}

// Phase 2 alone, one wave per input: the candidates come back from g_tok / g_val and go through beam_rank_and_put.
__global__ __launch_bounds__(64) void beam_rank_kernel(const long* __restrict__ g_tok, const float* __restrict__ g_val, omr_beam_desc bd, int t) {
    __shared__ float c_val[64];
    __shared__ int c_tok[64];
    const int n = blockIdx.x, nc = bd.beam * bd.beam, lane = threadIdx.x;
    if (bd.done[n]) return;                         // frozen (uniform over the workgroup)
    if (lane < nc) { c_tok[lane] = (int)g_tok[(long)n * nc + lane]; c_val[lane] = g_val[(long)n * nc + lane]; }
    beam_rank_and_put(bd, n, t, c_val, c_tok);      // its first barrier orders the two arrays
}

// beam_select_kernel over the weighted late fusion of two models (an extension: the reference decodes greedily,
// weighted_multimodal/test.py:50-61): phase 1 ranks wa * softmax(la) + wb * softmax(lb) of each row pair
// (weighted_topk_logprob_row, the row body of omr_weighted_topk_logprob); phase 2 is the same.
__global__ __launch_bounds__(256 * BEAM_GROUPS) void weighted_beam_select_kernel(const float* __restrict__ la, long lda, const float* __restrict__ lb, long ldb,
                                                                                 int V, float wa, float wb, omr_beam_desc bd, int t) {
    __shared__ float sa[BEAM_GROUPS][256], sb[BEAM_GROUPS][256];
    __shared__ int si[BEAM_GROUPS][256];
    __shared__ float c_val[64];
    __shared__ int c_tok[64];
    const int n = blockIdx.x, beam = bd.beam, row0 = n * beam;
    if (bd.done[n]) return;                         // frozen (uniform over the workgroup)
    const int g = threadIdx.x >> 8, tid = threadIdx.x & 255;
    for (int k0 = 0; k0 < beam; k0 += BEAM_GROUPS) {
        const int k = k0 + g;
        const bool real = k < beam;                 // a group without a row walks an empty one: the barriers stay uniform
        const long r = row0 + (real ? k : 0);
        weighted_topk_logprob_row(la + r * lda, lb + r * ldb, real ? V : 0, wa, wb, beam, tid, sa[g], sb[g], si[g], [&](int j, int idx, float val) {
            if (tid == 0 && real) { c_tok[k * beam + j] = idx; c_val[k * beam + j] = val; }
        });
    }
    beam_rank_and_put(bd, n, t, c_val, c_tok);
}

// The two selection kernels under a token automaton (include/omr_hip.h "grammar-constrained decoding").  Phase 1: each group
// stages the `next` row of ITS row's state in LDS and ranks through the masked load, so the log-probabilities are renormalised
// over the allowed tokens.  Phase 2: beam_rank_and_put with the descriptor.
__global__ __launch_bounds__(256 * BEAM_GROUPS) void beam_select_grammar_kernel(const float* __restrict__ logits, long ld, int V, omr_beam_desc bd,
                                                                                omr_grammar_desc gd, int t) {
    __shared__ float sv[BEAM_GROUPS][256];
    __shared__ int si[BEAM_GROUPS][256];
    __shared__ int next_row[BEAM_GROUPS][256];
    __shared__ float c_val[64];
    __shared__ int c_tok[64];
    const int n = blockIdx.x, beam = bd.beam, row0 = n * beam;
    if (bd.done[n]) return;                         // frozen (uniform over the workgroup)
    const int g = threadIdx.x >> 8, tid = threadIdx.x & 255;
    for (int k0 = 0; k0 < beam; k0 += BEAM_GROUPS) {
        const int k = k0 + g;
        const bool real = k < beam;                 // a group without a row walks an empty one: the barriers stay uniform
        const long r = row0 + (real ? k : 0);
        __syncthreads();                            // the previous round's loads of next_row are over
        stage_next_row(gd.next, gd.S, gd.C, gd.state[r], tid, next_row[g]);
        __syncthreads();
        topk_logprob_row(logits + r * ld, real ? V : 0, beam, tid, sv[g], si[g], [&](int j, int idx, float val) {
            if (tid == 0 && real) { c_tok[k * beam + j] = idx; c_val[k * beam + j] = val; }
        }, MaskedLoad{gd.cls, next_row[g]});
    }
    beam_rank_and_put(bd, n, t, c_val, c_tok, &gd);
}

__global__ __launch_bounds__(256 * BEAM_GROUPS) void weighted_beam_select_grammar_kernel(const float* __restrict__ la, long lda, const float* __restrict__ lb,
                                                                                         long ldb, int V, float wa, float wb, omr_beam_desc bd,
                                                                                         omr_grammar_desc gd, int t) {
    __shared__ float sa[BEAM_GROUPS][256], sb[BEAM_GROUPS][256];
    __shared__ int si[BEAM_GROUPS][256];
    __shared__ int next_row[BEAM_GROUPS][256];
    __shared__ float c_val[64];
    __shared__ int c_tok[64];
    const int n = blockIdx.x, beam = bd.beam, row0 = n * beam;
    if (bd.done[n]) return;                         // frozen (uniform over the workgroup)
    const int g = threadIdx.x >> 8, tid = threadIdx.x & 255;
    for (int k0 = 0; k0 < beam; k0 += BEAM_GROUPS) {
        const int k = k0 + g;
        const bool real = k < beam;                 // a group without a row walks an empty one: the barriers stay uniform
        const long r = row0 + (real ? k : 0);
        __syncthreads();                            // the previous round's loads of next_row are over
        stage_next_row(gd.next, gd.S, gd.C, gd.state[r], tid, next_row[g]);
        __syncthreads();
        weighted_topk_logprob_row(la + r * lda, lb + r * ldb, real ? V : 0, wa, wb, beam, tid, sa[g], sb[g], si[g], [&](int j, int idx, float val) {
            if (tid == 0 && real) { c_tok[k * beam + j] = idx; c_val[k * beam + j] = val; }
        }, MaskedLoad{gd.cls, next_row[g]});
    }
    beam_rank_and_put(bd, n, t, c_val, c_tok, &gd);
}

// Cache reorder: new row i of an input continues row parents[i] of it.  Positions [lo, t] of every layer and row move from the
// cache that holds position t to the one position t + 1 will be written into, 16 bytes per lane and access; nothing beyond t is
// touched.  grid = (chunks of 1024 vectors, rows, L).  Inputs that are done are left where they are: their rows keep running on
// stale cache contents, and nothing they produce is read.
__global__ __launch_bounds__(256) void beam_reorder_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, const int* __restrict__ parents,
                                                           const int* __restrict__ done, int beam, int rows, long row_vecs, long off_vecs, long nvec) {
    const int r = blockIdx.y, n = r / beam;
    if (done[n]) return;
    const int p = min(max(parents[r], 0), beam - 1);
    const uint4* s = src + ((long)blockIdx.z * rows + n * beam + p) * row_vecs + off_vecs;
    uint4* d = dst + ((long)blockIdx.z * rows + r) * row_vecs + off_vecs;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long i = (long)blockIdx.x * 1024 + u * 256 + threadIdx.x;
        if (i < nvec) d[i] = s[i];
    }
}

size_t beam_carve(omr_beam_desc* b) {
    const size_t rows = (size_t)b->N * b->beam, N = (size_t)b->N, hist = (size_t)b->max_len * rows;
    char* base = (char*)b->state;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base + off; off += align256(bytes); return p; };
    b->scores = (double*)take(rows * 8); b->best_score = (double*)take(N * 8); b->tokens = (long*)take(rows * 8);
    b->best_row = (int*)take(N * 4); b->best_pos = (int*)take(N * 4); b->done = (int*)take(N * 4); b->exhausted = (int*)take(N * 4);
    b->parents = (int*)take(rows * 4); b->hist_parent = (int*)take(hist * 4); b->hist_token = (int*)take(hist * 4);
    return off;
}

bool beam_desc_ok(const omr_beam_desc& b) {
    if (b.beam < 1 || b.beam > OMR_MAX_BEAM || b.N < 1 || b.max_len < 1 || !b.state) return false;
    omr_beam_desc c = b;
    if ((long)beam_carve(&c) > b.state_bytes) return false;
    return c.scores == b.scores && c.best_score == b.best_score && c.tokens == b.tokens && c.best_row == b.best_row && c.best_pos == b.best_pos &&
           c.done == b.done && c.exhausted == b.exhausted && c.parents == b.parents && c.hist_parent == b.hist_parent && c.hist_token == b.hist_token;
}


// ---- the checks the entries share
// a descriptor beam_desc_ok took against a vocabulary of V entries
bool beam_fits_vocab(const omr_beam_desc& b, int V) { return V >= b.beam && b.eos >= 0 && b.eos < V; }

// One model of a beam search: its descriptor, its memory lengths (nullable, device int32 [N]) and its second self-attention
// cache.  Position t lives in d->self_kv for even t and in kv2 for odd t.
struct BeamModel { const omr_decode_desc* d; const int* mem_len; void* kv2; };

// K|V bytes of one (layer, row, position) of the model
size_t kv_pos_bytes(const omr_decode_desc& d) { return (size_t)2 * d.d * (d.dtype == OMR_BF16 ? 2 : 4); }

// B rows = N inputs x beam hypotheses, the vocabulary holds the beam and <eos>, and both caches take the reorder's 16-byte moves
bool beam_model_ok(const BeamModel& bm, const omr_beam_desc& b) {
    const omr_decode_desc& d = *bm.d;
    if ((long)d.B != (long)b.N * b.beam || !beam_fits_vocab(b, d.V) || !d.self_kv || !bm.kv2) return false;
    return kv_pos_bytes(d) % 16 == 0 && (((uintptr_t)d.self_kv | (uintptr_t)bm.kv2) & 15) == 0;
}

// ---- launches
// g (nullable): the constrained kernel of each pair
void launch_select(const float* logits, long ld, int V, const omr_beam_desc& b, const omr_grammar_desc* g, int t, void* stream) {
    if (g) hipLaunchKernelGGL(beam_select_grammar_kernel, dim3((unsigned)b.N), dim3(256 * BEAM_GROUPS), 0, (hipStream_t)stream, logits, ld, V, b, *g, t);
    else hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)b.N), dim3(256 * BEAM_GROUPS), 0, (hipStream_t)stream, logits, ld, V, b, t);
}

// The selection with the CTC prefix score (include/omr_hip.h, omr_beam_select_ctc): top-k, score + mix over the parity t & 1 state, rank.
void launch_select_ctc(const float* logits, long ld, int V, const omr_beam_desc& b, const omr_ctc_beam_desc& c, int t, void* stream) {
    hipLaunchKernelGGL(beam_topk_kernel, dim3((unsigned)b.N), dim3(256 * BEAM_GROUPS), 0, (hipStream_t)stream, logits, ld, V, b, c.cand_tok, c.cand_val);
    launch_prefix_scores(c, t & 1, c.cand_tok, b.scores, b.done, c.cand_val, c.cand_val, stream);
    hipLaunchKernelGGL(beam_rank_kernel, dim3((unsigned)b.N), dim3(64), 0, (hipStream_t)stream, (const long*)c.cand_tok, (const float*)c.cand_val, b, t);
}

// a CTC descriptor ctc_beam_desc_check took against the search it scores for
bool ctc_fits_beam(const omr_ctc_beam_desc& c, const omr_beam_desc& b, int V) { return c.V == V && c.N == b.N && c.beam == b.beam && c.eos == b.eos; }

struct LogitRows { const float* logits; long ld; };
void launch_weighted_select(LogitRows a, LogitRows b, int V, float alpha, const omr_beam_desc& bd, const omr_grammar_desc* g, int t, void* stream) {
    const float wb = (float)(1.0 - (double)alpha);                           // the weights as omr_weighted_argmax_rows rounds them
    if (g) hipLaunchKernelGGL(weighted_beam_select_grammar_kernel, dim3((unsigned)bd.N), dim3(256 * BEAM_GROUPS), 0, (hipStream_t)stream, a.logits, a.ld,
                              b.logits, b.ld, V, alpha, wb, bd, *g, t);
    else hipLaunchKernelGGL(weighted_beam_select_kernel, dim3((unsigned)bd.N), dim3(256 * BEAM_GROUPS), 0, (hipStream_t)stream, a.logits, a.ld, b.logits, b.ld,
                            V, alpha, wb, bd, t);
}

// The reorder launch after position t of one model: position t + 1 reads keys [lo, t + 1] (the position's band), so positions
// [lo, t] move from `cur` to `nxt`.
void launch_beam_reorder(const omr_decode_desc& d, const omr_beam_desc& b, const void* cur, void* nxt, int t, void* stream) {
    if (t + 1 >= d.max_len) return;
    const long pos_vecs = (long)(kv_pos_bytes(d) / 16);
    const int lo = (d.window > 0 && t + 1 - d.window > 0) ? t + 1 - d.window : 0;
    const long nvec = (long)(t + 1 - lo) * pos_vecs;
    const dim3 grid((unsigned)cdiv(nvec, 1024), (unsigned)d.B, (unsigned)d.L);
    hipLaunchKernelGGL(beam_reorder_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const uint4*)cur, (uint4*)nxt, b.parents, b.done, b.beam, d.B,
                       (long)d.max_len * pos_vecs, (long)lo * pos_vecs, nvec);
}

// Beam driver: positions t0 .. t0 + n_steps - 1 of ONE search state over nm (1 or 2) models.  Per position every model's
// position without a pick (all read b.tokens; kv_group = beam: the hypotheses of an input share its cross-attention K|V),
// select(logits32 of each model, t), then the cache reorder once per model with that model's own L, d, dtype and window.
// b.last_logits (nullable) gets the first model's logits of the last position.
template <typename Select>
int beam_steps(const BeamModel* bm, int nm, const omr_beam_desc& b, int t0, int n_steps, Select select, void* stream) {
    if (!beam_desc_ok(b)) return OMR_ERR_ARG;
    OMR_TRY(check_steps(t0, n_steps, b.max_len));
    omr_decode_desc desc[2];                        // own copies: the cache pointer alternates per position
    Model m[2];
    for (int k = 0; k < nm; ++k) {
        if (!beam_model_ok(bm[k], b)) return OMR_ERR_ARG;
        OMR_TRY(check_steps(t0, n_steps, bm[k].d->max_len));
        desc[k] = *bm[k].d;
    }
    for (int s = 0; s < n_steps; ++s) {
        const int t = t0 + s;
        float* l32[2] = {nullptr, nullptr};
        void *cur[2], *nxt[2];
        for (int k = 0; k < nm; ++k) {
            cur[k] = (t & 1) ? bm[k].kv2 : bm[k].d->self_kv;
            nxt[k] = (t & 1) ? bm[k].d->self_kv : bm[k].kv2;
            desc[k].self_kv = cur[k];
            if (s == 0) {               // a descriptor is looked into when its model's first position comes up, as it always was
                OMR_TRY(check_model(desc[k]));
                m[k] = make_model(&desc[k], bm[k].mem_len, b.beam);
            }
            OMR_TRY(run_position(m[k], Position{t, nullptr, nullptr, nullptr}, b.tokens, Pick{nullptr, nullptr}, &l32[k], stream));
            if (k == 0 && s == n_steps - 1 && b.last_logits) OMR_TRY(copy_logits(m[0], b.last_logits, l32[0], stream));
        }
        select(l32, t);
        for (int k = 0; k < nm; ++k) launch_beam_reorder(desc[k], b, cur[k], nxt[k], t, stream);
        OMR_CHECK_LAUNCH();
    }
    return OMR_OK;
}

}  // namespace

extern "C" long omr_beam_workspace_bytes(omr_beam_desc* b) {
    if (!b || b->beam < 1 || b->beam > OMR_MAX_BEAM || b->N < 1 || b->max_len < 1) return OMR_ERR_ARG;
    return (long)beam_carve(b);
}

// ---- the four select / four decode entries: each pair (plain, grammar) is one definition with a nullable descriptor
namespace {

int beam_select(const float* logits, long ld, int V, const omr_beam_desc* bp, const omr_grammar_desc* g, int t, void* stream) {
    if (!logits || !bp || !beam_desc_ok(*bp)) return OMR_ERR_ARG;
    if (!beam_fits_vocab(*bp, V) || ld < V || t < 0 || t >= bp->max_len) return OMR_ERR_ARG;
    launch_select(logits, ld, V, *bp, g, t, stream);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

int weighted_beam_select(const float* logits_a, long lda, const float* logits_b, long ldb, int V, float alpha, const omr_beam_desc* bp,
                         const omr_grammar_desc* g, int t, void* stream) {
    if (!logits_a || !logits_b || !bp || !beam_desc_ok(*bp)) return OMR_ERR_ARG;
    if (!beam_fits_vocab(*bp, V) || lda < V || ldb < V || t < 0 || t >= bp->max_len) return OMR_ERR_ARG;
    launch_weighted_select(LogitRows{logits_a, lda}, LogitRows{logits_b, ldb}, V, alpha, *bp, g, t, stream);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

/* This entry wants the history exactly as long as the cache (the weighted one below: long enough for the run). */
int beam_decode(const omr_decode_desc* dp, const omr_beam_desc* bp, const int* mem_len, const omr_grammar_desc* g, int t0, int n_steps, void* stream) {
    if (!dp || !bp || bp->max_len != dp->max_len) return OMR_ERR_ARG;
    const BeamModel bm = {dp, mem_len, bp->self_kv2};
    auto select = [&](float* const* l32, int t) { launch_select(l32[0], (long)dp->ldv, dp->V, *bp, g, t, stream); };
    return beam_steps(&bm, 1, *bp, t0, n_steps, select, stream);
}

/* omr_beam_decode_steps over the weighted late fusion: ONE search state drives two models, and one weighted selection launch
 * ranks both models' logits.  bp->self_kv2 is model A's second cache, self_kv2_b model B's. */
int weighted_beam_decode(const omr_decode_desc* da, const int* mem_len_a, const omr_decode_desc* db, const int* mem_len_b, const omr_beam_desc* bp,
                         void* self_kv2_b, const omr_grammar_desc* g, float alpha, int t0, int n_steps, void* stream) {
    if (!da || !db || !bp || da->V != db->V) return OMR_ERR_ARG;
    const BeamModel bm[2] = {{da, mem_len_a, bp->self_kv2}, {db, mem_len_b, self_kv2_b}};
    auto select = [&](float* const* l32, int t) {
        launch_weighted_select(LogitRows{l32[0], (long)da->ldv}, LogitRows{l32[1], (long)db->ldv}, da->V, alpha, *bp, g, t, stream);
    };
    return beam_steps(bm, 2, *bp, t0, n_steps, select, stream);
}

}  // namespace

extern "C" int omr_beam_select(const float* logits, long ld, int V, const omr_beam_desc* bp, int t, void* stream) {
    return beam_select(logits, ld, V, bp, nullptr, t, stream);
}

extern "C" int omr_weighted_beam_select(const float* logits_a, long lda, const float* logits_b, long ldb, int V, float alpha, const omr_beam_desc* bp, int t,
                                        void* stream) {
    return weighted_beam_select(logits_a, lda, logits_b, ldb, V, alpha, bp, nullptr, t, stream);
}

extern "C" int omr_beam_decode_steps(const omr_decode_desc* dp, const omr_beam_desc* bp, const int* mem_len, int t0, int n_steps, void* stream) {
    return beam_decode(dp, bp, mem_len, nullptr, t0, n_steps, stream);
}

extern "C" int omr_weighted_beam_decode_steps(const omr_decode_desc* da, const int* mem_len_a, const omr_decode_desc* db, const int* mem_len_b,
                                              const omr_beam_desc* bp, void* self_kv2_b, float alpha, int t0, int n_steps, void* stream) {
    return weighted_beam_decode(da, mem_len_a, db, mem_len_b, bp, self_kv2_b, nullptr, alpha, t0, n_steps, stream);
}

/* The selection and the decode with the CTC prefix score (include/omr_hip.h "joint CTC / attention beam search"; extensions of the host
 * loop _Base.beam_search of this package's model.py).  The state advances behind the selection of a position: survivors read their parents'
 * rows of parity t & 1 and write their own of the other. */
extern "C" int omr_beam_select_ctc(const float* logits, long ld, int V, const omr_beam_desc* bp, const omr_ctc_beam_desc* cp, int t, void* stream) {
    OMR_TRY(ctc_beam_desc_check(cp));
    if (!logits || !bp || !beam_desc_ok(*bp)) return OMR_ERR_ARG;
    if (!beam_fits_vocab(*bp, V) || !ctc_fits_beam(*cp, *bp, V) || ld < V || t < 0 || t >= bp->max_len) return OMR_ERR_ARG;
    launch_select_ctc(logits, ld, V, *bp, *cp, t, stream);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_beam_decode_steps_ctc(const omr_decode_desc* dp, const omr_beam_desc* bp, const omr_ctc_beam_desc* cp, const int* mem_len, int t0,
                                         int n_steps, void* stream) {
    OMR_TRY(ctc_beam_desc_check(cp));
    if (!dp || !bp || bp->max_len != dp->max_len || !ctc_fits_beam(*cp, *bp, dp->V)) return OMR_ERR_ARG;
    const BeamModel bm = {dp, mem_len, bp->self_kv2};
    auto select = [&](float* const* l32, int t) {
        launch_select_ctc(l32[0], (long)dp->ldv, dp->V, *bp, *cp, t, stream);
        launch_prefix_advance(*cp, t & 1, bp->parents, bp->tokens, bp->scores, bp->done, stream);
    };
    return beam_steps(&bm, 1, *bp, t0, n_steps, select, stream);
}

/* The same four under a token automaton (include/omr_hip.h "grammar-constrained decoding"; extensions of the host loop
 * _Base.beam_search of this package's model.py): the descriptor is checked here, then the shared definition runs. */
extern "C" int omr_beam_select_grammar(const float* logits, long ld, int V, const omr_beam_desc* bp, const omr_grammar_desc* g, int t, void* stream) {
    if (!grammar_desc_ok(g)) return OMR_ERR_ARG;
    return beam_select(logits, ld, V, bp, g, t, stream);
}

extern "C" int omr_weighted_beam_select_grammar(const float* logits_a, long lda, const float* logits_b, long ldb, int V, float alpha,
                                                const omr_beam_desc* bp, const omr_grammar_desc* g, int t, void* stream) {
    if (!grammar_desc_ok(g)) return OMR_ERR_ARG;
    return weighted_beam_select(logits_a, lda, logits_b, ldb, V, alpha, bp, g, t, stream);
}

extern "C" int omr_beam_decode_steps_grammar(const omr_decode_desc* dp, const omr_beam_desc* bp, const int* mem_len, const omr_grammar_desc* g, int t0,
                                             int n_steps, void* stream) {
    if (!grammar_desc_ok(g)) return OMR_ERR_ARG;
    return beam_decode(dp, bp, mem_len, g, t0, n_steps, stream);
}

extern "C" int omr_weighted_beam_decode_steps_grammar(const omr_decode_desc* da, const int* mem_len_a, const omr_decode_desc* db, const int* mem_len_b,
                                                      const omr_beam_desc* bp, void* self_kv2_b, const omr_grammar_desc* g, float alpha, int t0,
                                                      int n_steps, void* stream) {
    if (!grammar_desc_ok(g)) return OMR_ERR_ARG;
    return weighted_beam_decode(da, mem_len_a, db, mem_len_b, bp, self_kv2_b, g, alpha, t0, n_steps, stream);
}
