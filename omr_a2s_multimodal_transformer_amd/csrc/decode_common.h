// What crosses the three decode translation units: decode_linear.hip (the row kernel and its launch), decode.hip (workspace,
// the position executor, the greedy and weighted-greedy entries) and decode_beam.hip (selection, reorder, the beam entries).
// ctc_prefix.hip (the CTC prefix score of the joint beam search) hands decode_beam.hip its two launches through here too.
#pragma once
#include "omr_common.h"
#include "omr_hip.h"

#define OMR_TRY(call) do { int rc__ = (call); if (rc__ != OMR_OK) return rc__; } while (0)

namespace omr_dec {

struct Ws {          // activation scratch of one step, carved out of the caller's workspace
    char* x; char* x2; char* q; char* o; char* proj; char* h; char* logits; float* logits32; float* lse; float* mean; float* rstd;
    float* split; long split_floats; float* apart;
    unsigned char* a8; float* sa8;          // fp8 mode: the quantised input rows of the current GEMM and their scales
    int* rows_tab;                          // per-row positions: [3][max_len][B] tables of position | first key | key count
};

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// decode.hip; base == NULL: the size only.  rows: the rows of a position (d.B, or d.B * group for a grouped position)
size_t carve(const omr_decode_desc& d, int rows, char* base, Ws* w);

// ---- decode_linear.hip
// the model widths the row kernel takes (8 launches per layer); any other takes one kernel per step of the layer
bool takes_row_kernel(const omr_decode_desc& d);
// The row-linear launch (omr_decode_linear).  row_pos != NULL: the per-row-position form -- row m sits at position row_pos[m],
// takes the positional row pe_row + row_pos[m] * K and stores its out1 part out1_pos_ld elements further per position.
// group > 1 (needs row_pos): the grouped form -- `group` consecutive rows are consecutive positions of ONE slot, so the out1 part of
// row m lands in slot m / group: out1 + (m / group) * ld1 + row_pos[m] * out1_pos_ld.
int decode_linear_impl(const omr_decode_linear_args& a, const int* row_pos, long out1_pos_ld, void* stream, int group = 1);

// ---- decode.hip: one position of one model
// One decoder with its scratch.  mem_len (nullable, device int32 [B / kv_group]): row b's cross-attention sees the first
// mem_len[b / kv_group] of the d->S memory rows (ragged batch).  kv_group: that many consecutive rows share one cross-attention
// K|V slot (the hypotheses of one input of a batched beam search); 1 everywhere else.  d is read at every position: a beam
// search points it at its own copy and alternates self_kv there.
// rows / group: a grouped position (omr_decode_verify_rows) runs rows = d->B * group rows, row m being position pos[m / group] +
// m % group of slot m / group -- the caches hold d->B slots, the scratch `rows` rows; everywhere else rows = d->B and group = 1.
struct Model { const omr_decode_desc* d; Ws w; const int* mem_len; int kv_group; int rows; int group; };
// Where the rows are.  Tables NULL: every row at position t.  Otherwise (omr_decode_steps_rows; device int32 [B] each, one
// position's rows of Ws::rows_tab) row b sits at row_pos[b] and sees the kv_count[b] cache keys from kv_start[b] on, and t is the
// LARGEST of the rows' positions (the key-split plan is the furthest row's).
struct Position { int t; const int* row_pos; const int* kv_start; const int* kv_count; };
// The greedy pick of the position: token (and its fp32 logit, nullable) per row.  NULL idx: logits only.
struct Pick { long* idx; float* val; };

int check_model(const omr_decode_desc& d);                              // every descriptor check, once
int check_desc(const omr_decode_desc& d);                               // check_model without the workspace (a grouped position brings its own)
int check_steps(int t0, int n_steps, int max_len);                      // positions t0 .. t0 + n_steps - 1 against a table / cache length
Model make_model(const omr_decode_desc* d, const int* mem_len, int kv_group);      // of a descriptor check_model took
// Fills the tables of positions pos[b] + off + s, s < n_steps (clamped into the cache), one launch; position_at picks those of s.
void launch_rows_tables(const Model& m, const int* pos, int off, int n_steps, void* stream);
Position position_at(const Model& m, const int* pos, int t, int s);
// The model of a grouped position over the caller's scratch `ws` (carve(d, d.B * group) bytes), and its tables (one launch): t_max is
// the largest entry of pos, the Position's t the furthest row's.
Model make_group_model(const omr_decode_desc* d, const int* mem_len, int group, void* ws);
Position launch_group_tables(const Model& m, const int* pos, int t_max, void* stream);
// One grouped position of the row path: argument checks, tables, launches (decode.hip; the body of omr_decode_verify_rows)
int verify_rows(const omr_decode_desc* d, const int* mem_len, const int* pos, int t_max, int R, const long* tokens, long* out_tokens, float* out_top1,
                void* ws, long ws_bytes, void* stream);
// Issues the launches of ONE position for all rows: row kernel path or generic-width path by takes_row_kernel.  tok_in: the
// token each row feeds in (device int64 [B]).  *logits32: where the position's fp32 logits [B][ldv] lie in the workspace.
int run_position(const Model& m, const Position& p, const long* tok_in, Pick pick, float** logits32, void* stream);
int copy_logits(const Model& m, float* dst, const float* logits32, void* stream);      // [B][ldv] fp32, device to device, async


// ---- ctc_prefix.hip: the CTC prefix score of the joint beam search (decode_beam.hip launches it between its own two phases)
int ctc_beam_desc_check(const omr_ctc_beam_desc* c);                    // every descriptor check, once
// out[r][j] over cand [rows][beam] against the parity state: delta, or with att_val the mix fl(fl(wa * att_val) + fl(wc * delta));
// scores / done (nullable): dead rows' candidates get -inf, done inputs nothing
void launch_prefix_scores(const omr_ctc_beam_desc& c, int parity, const long* cand, const double* scores, const int* done, const float* att_val,
                          float* out, void* stream);
void launch_prefix_advance(const omr_ctc_beam_desc& c, int parity, const int* parents, const long* tokens, const double* scores, const int* done,
                           void* stream);

}  // namespace omr_dec
