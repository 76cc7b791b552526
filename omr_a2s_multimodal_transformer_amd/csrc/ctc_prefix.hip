// CTC prefix scores for the joint CTC / attention beam search (gfx950; include/omr_hip.h "joint CTC / attention beam search" states the
// definition and every entry).  An extension: the reference decodes greedily from the attention decoder alone.
//
// One kernel, ctc_prefix_kernel<T, STORE>, is the score (STORE = false: lane = candidate parent * beam + j, delta out) and the advance
// (STORE = true: lane = new row, gn / gb rows, logpsi and last out).  Both run prefix_scan, the ONE row body, on the same LDS tiles, so the
// logpsi a survivor stores has the bits its candidate's had; this file is built with -ffp-contract=off (Makefile), so no product is fused
// into an add in one instantiation and not in the other, and the mix fl(fl(wa * value) + fl(wc * delta)) is the three roundings it says.
//
// Structure.  One workgroup of 4 waves per input.  The recursion is sequential in the frame, its operands are not: a tile of PFX_CH = 32
// frames holds y_f(c) for the 64 lanes' tokens, y_f(blank), and phi[f - 1] of the input's `beam` parent hypotheses in both forms (with and
// without the repeat rule) -- phi is computed once per (parent, frame) here, not once per candidate.  All four waves fetch tile k + 1 into
// registers (scattered 2- / 4-byte gathers of one logits row per frame, 8 per thread, plus one parent pair per thread), wave 0 scans tile k
// out of LDS while those loads are in flight, then everyone commits the registers to the other LDS buffer: one barrier per 32 frames, and
// the scanning wave never waits for memory it asked for in the same tile.  The sweep of ctc.hip prefetches into a register ring instead;
// that needs every lane to load its own operands, which here would compute phi beam times over and leave three waves without work.
// logpsi is a sum over frames, not a chain: it is accumulated around a running maximum 8 frames at a time (8 independent expf), so the
// score's only per-frame chain is one fmaxf.  The advance carries gn / gb through two log-adds per frame (independent of each other):
// that chain, expf + log1pf per frame, is what bounds it.
#include "ctc_rows.h"
#include "decode_common.h"

namespace {

constexpr int PFX_CH = 32;             // frames per LDS tile
constexpr int PFX_SUB = 8;             // frames per step of the logpsi accumulation
constexpr int PFX_Y = PFX_CH / 4;      // gathered emissions per thread and tile (4 waves x 64 lanes)
static_assert(PFX_CH * OMR_MAX_BEAM == 256 && PFX_CH % PFX_SUB == 0, "one (frame, parent) pair per thread");

enum { LANE_NONE = 0, LANE_LABEL = 1, LANE_EOS = 2 };

struct PfxArgs {
    omr_ctc_beam_desc c;
    int parity;
    const long* tok;            // score: cand [rows][beam]; advance: tokens [rows]
    const int* parents;         // advance only
    const double* scores;       // nullable: rows at -inf are dead
    const int* done;            // nullable
    const float* att_val;       // score only, nullable: the values to mix delta into
    float* out;                 // score only: delta, or the mixed value
    float wa, wc;
};

struct PfxTile {
    float y[2][PFX_CH][64];
    float yb[2][PFX_CH];
    float phi[2][PFX_CH][OMR_MAX_BEAM][2];
};

// The row body: lane's hypothesis h = g c over the nf frames of tile buffer b.  (m, s): logpsi's running maximum and sum; (gn, gb): the
// rows' last values.  par / rep pick phi's parent and form.  STORE: the frames' gn / gb go to on / ob (the lane's rows, at the tile's
// first frame) where put is set.
template <bool STORE>
__device__ __forceinline__ void prefix_scan(const PfxTile& tl, int b, int nf, int lane, int par, int rep, float& m, float& s, float& gn, float& gb,
                                            bool put, float* on, float* ob) {
    for (int k0 = 0; k0 < nf; k0 += PFX_SUB) {
        float term[PFX_SUB];
        float cm = m;
#pragma unroll
        for (int k = 0; k < PFX_SUB; ++k) {
            const int fr = k0 + k;
            const float y = tl.y[b][fr][lane], ph = tl.phi[b][fr][par][rep];
            term[k] = fr < nf ? ph + y : -INFINITY;
            cm = fmaxf(cm, term[k]);
            if constexpr (STORE) {
                if (fr < nf) {
                    const float ngn = lse2(gn, ph) + y;
                    const float ngb = lse2(gb, gn) + tl.yb[b][fr];
                    gn = ngn;
                    gb = ngb;
                    if (put) { on[fr] = gn; ob[fr] = gb; }
                }
            }
        }
        if (cm > -INFINITY) {
            s = s * expf(m - cm);
#pragma unroll
            for (int k = 0; k < PFX_SUB; ++k) s = s + expf(term[k] - cm);
            m = cm;
        }
    }
}

template <typename T, bool STORE>
__global__ __launch_bounds__(256) void ctc_prefix_kernel(PfxArgs a) {
    __shared__ PfxTile tl;
    __shared__ int s_tok[64], s_last[OMR_MAX_BEAM];
    const omr_ctc_beam_desc& c = a.c;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, beam = c.beam, row0 = n * beam;
    if (a.done && a.done[n]) return;                // uniform over the workgroup
    const int Fmax = c.Fmax, F = clamp_len(c.frame_len[n], Fmax);
    const long ldv = c.ldv;
    const T* X = (const T*)c.logits + (long)n * Fmax * ldv;
    const float* Z = c.lse + (long)n * Fmax;
    const float* SI = c.state[a.parity] + (long)row0 * 2 * Fmax;
    float* SO = c.state[a.parity ^ 1] + (long)row0 * 2 * Fmax;
    const int* last_in = c.last[a.parity] + row0;

    // the lane's role: its parent row, its token, what it computes
    const int nl = STORE ? beam : beam * beam;
    int par = 0, tok = c.blank, kind = LANE_NONE;
    if (lane < nl) {
        par = STORE ? min(max(a.parents[row0 + lane], 0), beam - 1) : lane / beam;
        const long tk = STORE ? a.tok[row0 + lane] : a.tok[(long)row0 * beam + lane];
        const bool live = !a.scores || a.scores[row0 + (STORE ? lane : par)] > -INFINITY;
        if (live && tk == c.eos) kind = LANE_EOS;
        else if (live && tk >= 0 && tk < c.V && tk != c.blank && tk != c.sos) { kind = LANE_LABEL; tok = (int)tk; }
    }
    if (STORE && kind == LANE_EOS) kind = LANE_NONE;
    if (wv == 0) s_tok[lane] = tok;
    if (tid < beam) s_last[tid] = last_in[tid];
    __syncthreads();
    const int mytok = s_tok[lane];                  // the column this thread gathers (waves 1-3: lane's, as wave 0's)
    const int pf = tid >> 3, pp = tid & 7;          // the (frame of the tile, parent) pair this thread prepares
    const bool p_empty = pp < beam && s_last[pp] == c.sos;

    T ry[PFX_Y], rb = from_f32<T>(0.f);
    float rz[PFX_Y], rgn = -INFINITY, rgb = -INFINITY, rbz = 0.f;
    auto fetch = [&](int f0) {                      // loads only: nothing here waits for them
#pragma unroll
        for (int i = 0; i < PFX_Y; ++i) {
            const int f = f0 + i * 4 + wv;
            const bool ok = f < F;
            ry[i] = ok ? X[(long)f * ldv + mytok] : from_f32<T>(0.f);
            rz[i] = ok ? Z[f] : 0.f;
        }
        const int f = f0 + pf;
        rgn = rgb = -INFINITY;
        if (pp < beam && f < F && f >= 1) {
            rgn = SI[((long)pp * 2 + 0) * Fmax + f - 1];
            rgb = SI[((long)pp * 2 + 1) * Fmax + f - 1];
        }
        if (STORE && tid < PFX_CH && f0 + tid < F) { rb = X[(long)(f0 + tid) * ldv + c.blank]; rbz = Z[f0 + tid]; }
    };
    auto commit = [&](int b, int f0) {
#pragma unroll
        for (int i = 0; i < PFX_Y; ++i) tl.y[b][i * 4 + wv][lane] = to_f32(ry[i]) - rz[i];
        float full = lse2(rgb, rgn), rep = rgb;
        if (f0 + pf == 0) full = rep = p_empty ? 0.f : -INFINITY;      // phi[-1]
        tl.phi[b][pf][pp][0] = full;
        tl.phi[b][pf][pp][1] = rep;
        if (STORE && tid < PFX_CH) tl.yb[b][tid] = to_f32(rb) - rbz;
    };

    const int rep = (kind == LANE_LABEL && mytok == s_last[par]) ? 1 : 0;
    float m = -INFINITY, s = 0.f, gn = -INFINITY, gb = -INFINITY;
    const bool put = STORE && kind == LANE_LABEL;
    float* on = SO + ((long)lane * 2 + 0) * Fmax;   // dereferenced where put is set only (lane < beam there)
    float* ob = SO + ((long)lane * 2 + 1) * Fmax;
    if (F > 0) {
        fetch(0);
        commit(0, 0);
    }
    __syncthreads();
    for (int f0 = 0, b = 0; f0 < F; f0 += PFX_CH, b ^= 1) {
        const bool more = f0 + PFX_CH < F;
        if (more) fetch(f0 + PFX_CH);
        if (wv == 0) prefix_scan<STORE>(tl, b, min(PFX_CH, F - f0), lane, par, rep, m, s, gn, gb, put, on + f0, ob + f0);
        if (more) commit(b ^ 1, f0 + PFX_CH);
        __syncthreads();
    }
    if (wv != 0 || lane >= nl) return;
    if (STORE && lane == 0) c.advanced[n] = c.advanced[n] + 1;      // one writer per input
    float psi = -INFINITY;
    if (kind == LANE_LABEL) psi = m == -INFINITY ? -INFINITY : m + logf(s);
    else if (kind == LANE_EOS)
        psi = F > 0 ? lse2(SI[((long)par * 2 + 0) * Fmax + F - 1], SI[((long)par * 2 + 1) * Fmax + F - 1]) : (s_last[par] == c.sos ? 0.f : -INFINITY);
    if constexpr (STORE) {
        if (put) {
            c.logpsi[row0 + lane] = psi;
            c.last[a.parity ^ 1][row0 + lane] = mytok;
        }
    } else {
        const float delta = psi == -INFINITY ? -INFINITY : fminf(psi - c.logpsi[row0 + par], 0.f);
        const long o = (long)row0 * beam + lane;
        a.out[o] = a.att_val ? a.wa * a.att_val[o] + a.wc * delta : delta;
    }
}

// The empty hypothesis into every row's parity-0 state: lane k < beam writes row n * beam + k (the same values in each).
template <typename T>
__global__ __launch_bounds__(64) void ctc_prefix_init_kernel(omr_ctc_beam_desc c) {
    const int n = blockIdx.x, k = threadIdx.x;
    if (k >= c.beam) return;
    if (k == 0) c.advanced[n] = 0;
    const int Fmax = c.Fmax, F = clamp_len(c.frame_len[n], Fmax), row = n * c.beam + k;
    const T* X = (const T*)c.logits + (long)n * Fmax * c.ldv;
    const float* Z = c.lse + (long)n * Fmax;
    float* gn = c.state[0] + (long)row * 2 * Fmax;
    float* gb = gn + Fmax;
    float acc = 0.f;
#pragma unroll 8
    for (int f = 0; f < F; ++f) {
        acc = acc + (to_f32(X[(long)f * c.ldv + c.blank]) - Z[f]);
        gn[f] = -INFINITY;
        gb[f] = acc;
    }
    c.logpsi[row] = 0.f;
    c.last[0][row] = c.sos;
}

size_t ctc_beam_carve(omr_ctc_beam_desc* c) {
    const size_t rows = (size_t)c->N * c->beam, N = (size_t)c->N, F = (size_t)c->Fmax, nc = N * c->beam * c->beam;
    char* base = (char*)c->ws;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base + off; off += omr_dec::align256(bytes); return p; };
    c->lse = (float*)take(N * F * 4);
    c->state[0] = (float*)take(rows * 2 * F * 4); c->state[1] = (float*)take(rows * 2 * F * 4);
    c->last[0] = (int*)take(rows * 4); c->last[1] = (int*)take(rows * 4);
    c->logpsi = (float*)take(rows * 4);
    c->cand_tok = (long*)take(nc * 8); c->cand_val = (float*)take(nc * 4);
    c->advanced = (int*)take(N * 4);
    return off;
}

bool ctc_beam_sizes_ok(const omr_ctc_beam_desc& c) { return c.N >= 1 && c.N <= 65535 && c.Fmax >= 1 && c.beam >= 1 && c.beam <= OMR_MAX_BEAM; }

template <bool STORE>
void launch_prefix(const PfxArgs& a, void* stream) {
    if (a.c.dtype == OMR_F32) hipLaunchKernelGGL((ctc_prefix_kernel<float, STORE>), dim3((unsigned)a.c.N), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((ctc_prefix_kernel<bf16, STORE>), dim3((unsigned)a.c.N), dim3(256), 0, (hipStream_t)stream, a);
}

}  // namespace

namespace omr_dec {

int ctc_beam_desc_check(const omr_ctc_beam_desc* cp) {
    if (!cp || !ctc_beam_sizes_ok(*cp) || !cp->logits || !cp->frame_len || !cp->ws) return OMR_ERR_ARG;
    const omr_ctc_beam_desc& c = *cp;
    if (!(c.lambda > 0.f && c.lambda < 1.f) || c.V < 1 || c.ldv < c.V) return OMR_ERR_ARG;
    if (c.blank < 0 || c.blank >= c.V || c.sos < 0 || c.sos >= c.V || c.eos < 0 || c.eos >= c.V) return OMR_ERR_ARG;
    if (c.blank == c.sos || c.blank == c.eos || c.sos == c.eos) return OMR_ERR_ARG;
    omr_ctc_beam_desc k = c;
    if ((long)ctc_beam_carve(&k) > c.ws_bytes) return OMR_ERR_ARG;
    if (k.lse != c.lse || k.state[0] != c.state[0] || k.state[1] != c.state[1] || k.last[0] != c.last[0] || k.last[1] != c.last[1] ||
        k.logpsi != c.logpsi || k.cand_tok != c.cand_tok || k.cand_val != c.cand_val || k.advanced != c.advanced)
        return OMR_ERR_ARG;
    return c.dtype == OMR_F32 || c.dtype == OMR_BF16 ? OMR_OK : OMR_ERR_UNSUPPORTED;
}

void launch_prefix_scores(const omr_ctc_beam_desc& c, int parity, const long* cand, const double* scores, const int* done, const float* att_val,
                          float* out, void* stream) {
    PfxArgs a = {c, parity, cand, nullptr, scores, done, att_val, out, (float)(1.0 - (double)c.lambda), c.lambda};
    launch_prefix<false>(a, stream);
}

void launch_prefix_advance(const omr_ctc_beam_desc& c, int parity, const int* parents, const long* tokens, const double* scores, const int* done,
                           void* stream) {
    PfxArgs a = {c, parity, tokens, parents, scores, done, nullptr, nullptr, 0.f, 0.f};
    launch_prefix<true>(a, stream);
}

}  // namespace omr_dec

extern "C" long omr_ctc_beam_workspace_bytes(omr_ctc_beam_desc* c) {
    if (!c || !ctc_beam_sizes_ok(*c)) return OMR_ERR_ARG;
    return (long)ctc_beam_carve(c);
}

extern "C" int omr_ctc_prefix_init(const omr_ctc_beam_desc* c, void* stream) {
    OMR_TRY(omr_dec::ctc_beam_desc_check(c));
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T(c->dtype, {
        hipLaunchKernelGGL((ctc_lse_kernel<T>), dim3(c->Fmax, c->N), 256, 0, s, (const T*)c->logits, c->frame_len, c->lse, c->Fmax, c->V, c->ldv);
        hipLaunchKernelGGL((ctc_prefix_init_kernel<T>), dim3(c->N), 64, 0, s, *c);
    })
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_ctc_prefix_scores(const omr_ctc_beam_desc* c, int parity, const long* cand, float* delta, void* stream) {
    OMR_TRY(omr_dec::ctc_beam_desc_check(c));
    if (!cand || !delta || (parity != 0 && parity != 1)) return OMR_ERR_ARG;
    omr_dec::launch_prefix_scores(*c, parity, cand, nullptr, nullptr, nullptr, delta, stream);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_ctc_prefix_advance(const omr_ctc_beam_desc* c, int parity, const int* parents, const long* tokens, const double* scores,
                                      const int* done, void* stream) {
    OMR_TRY(omr_dec::ctc_beam_desc_check(c));
    if (!parents || !tokens || (parity != 0 && parity != 1)) return OMR_ERR_ARG;
    omr_dec::launch_prefix_advance(*c, parity, parents, tokens, scores, done, stream);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}
