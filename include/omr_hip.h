/* libomr_hip.so -- C ABI of the MI355X (gfx950) encoder/decoder hot path.
 *
 * The reference (mariaalfaroc/omr_a2s_multimodal_transformer) has no FFI: its hot path is the set of ATen ops that
 * src/transformer/{encoder,decoder,model}.py reach through torch.nn.  Each entry point below
 * replaces one of those op families; the reference call site it stands in for is cited per function.
 *
 * Conventions: every function returns 0 (OMR_OK) or a negative error code and never throws; the caller owns
 * all buffers (device pointers); `stream` is a hipStream_t passed as void*; dtype is OMR_F32 (0) or OMR_BF16 (1)
 * and names the activation/weight element type (accumulation is always fp32); "small vectors" (bias, LayerNorm
 * gamma/beta, statistics) are always fp32.  Encoder activations are NHWC; token matrices are row-major [rows][ld].
 * No hidden state: every call is re-entrant across streams and host threads (the only process-wide data are per-kernel
 * launch constants -- resident blocks per CU, dynamic-LDS opt-in -- cached in atomics on first use; one process drives one GPU).
 */
#ifndef OMR_HIP_H
#define OMR_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define OMR_DTYPE_F32 0
#define OMR_DTYPE_BF16 1
/* a SOURCE type of omr_gather_ragged_batch only (8-bit grays); no other entry takes it */
#define OMR_DTYPE_U8 2

int omr_abi_version(void);

/* ---- elementwise / gather ------------------------------------------------------------------------------ */
int omr_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, void* stream);
/* residual adds: encoder.py:289 (x + xt) */
int omr_add(int dtype, const void* a, const void* b, void* out, long n, void* stream);
/* ReLU(+dropout) backward: dx = dy * (y > 0) * scale   (aten::threshold_backward; encoder.py:163-176) */
int omr_relu_bwd(int dtype, const void* dy, const void* y, void* dx, long n, float scale, void* stream);
/* nn.Dropout / nn.Dropout2d (encoder.py:98-104, decoder.py:19, model.py:31): counter-based mask, regenerated not stored.
 * channel_mode=1: one decision per (sample, channel) of an NHWC tensor with `per_sample` = H*W*C elements per sample. */
int omr_dropout(int dtype, const void* x, void* out, long n, float p, unsigned long long seed, int channel_mode, long per_sample, int C,
                void* stream);
/* nn.Embedding + PositionalEncoding1D: out[m] = table[tok[m]] + pe[m % T]   (decoder.py:124) */
int omr_embed_pe_fwd(int dtype, const long* tokens, const void* table, const float* pe, void* out, long M, int T_len, int d, int vocab,
                     void* stream);
/* embedding backward: dtable[tok[m]] += dout[m], PAD row skipped (nn.Embedding padding_idx, decoder.py:73-77) */
int omr_embed_bwd(int dtype, const long* tokens, const void* dout, float* dtable, long M, int d, int pad_idx, int vocab, void* stream);
/* PositionalEncoding2D on NHWC maps: out[b,i,j,c] = x[b,i,j,c] + pe[i,j,c], pe laid out [maxh][maxw][C]   (model.py:45-47) */
int omr_add_pe2d(int dtype, const void* x, const float* pe_hwc, void* out, int B, int h, int w, int C, int maxh, int maxw, void* stream);
/* bias gradients: db[n] += sum_m dy[m][n] */
int omr_colsum(int dtype, const void* dy, float* db, long M, int N, long ld, void* stream);
/* torch.optim.Adam step over one flat fp32 buffer (model.py:134-139; torch optim/adam.py:347); step is 1-based.
 * p_bf16 (nullable) receives the bf16 compute copy of the updated parameters in the same pass.
 * omr_adamw_ema (below) with weight_decay = 0 and ema = decay_blocks = ctl = NULL, and its contract: any n >= 1, but p, g, m, v
 * non-NULL and, like p_bf16, 16-byte aligned; anything else, or step < 1, is refused with OMR_ERR_ARG before any launch. */
int omr_adam(float* p, const float* g, float* m, float* v, void* p_bf16, long n, int step, float lr, float b1, float b2, float eps,
             float grad_scale, void* stream);
/* greedy token pick: argmax(dim=-1) / topk(1) of the last-step logits (model.py:187,253), one row per decoded sample
 * (x [rows][ld], first n columns); first-index tie rule */
int omr_argmax(const float* x, int rows, int n, long ld, long* idx_out, float* val_out, void* stream);
/* weighted late fusion (src/multimodal/weighted_multimodal/test.py:50-61): the token of one decoding step of two unimodal models
 * run in lock-step, argmax(alpha * softmax(logits_a) + (1 - alpha) * softmax(logits_b)) over fp32 rows of n logits, first-index
 * tie rule; prob_out (nullable) receives the winning mixed probability.  alpha is rounded like the reference's Python float. */
int omr_weighted_argmax(const float* logits_a, const float* logits_b, int n, float alpha, long* idx_out, float* prob_out, void* stream);
/* omr_weighted_argmax for a batch of row pairs (one decoding step of `rows` samples, test.py:50-61 per sample): row r reads
 * logits_a + r * lda and logits_b + r * ldb (lda, ldb >= n); idx_out[r] / prob_out[r] (nullable) are bit for bit what
 * omr_weighted_argmax gives for that pair alone (one kernel serves both).  tokens_out (nullable, [rows]) receives the picked
 * tokens as well: where the next decoding position reads its input. */
int omr_weighted_argmax_rows(const float* logits_a, long lda, const float* logits_b, long ldb, int rows, int n, float alpha,
                             long* idx_out, float* prob_out, long* tokens_out, void* stream);
/* audio front end (preprocessing.py:17-30): after the windowed DFT -- ONE omr_gemm of the centred,
 * hop-strided frames (lda = hop) against the Hann-weighted [cos | -sin] basis of the kept bins -- spec [frames][2*bins] holds
 * (re | im); this turns it into the reference's normalised log-spectrogram out [bins][frames] =
 * amplitude_to_db(|S|, ref=max, top_db=80) / 80 + 1.  spec is overwritten (magnitudes); max_ws: 4 bytes of device scratch,
 * cleared by the call.  As with numpy's maxima, one NaN magnitude makes every output NaN; the element that holds the maximum is
 * exactly 1.0, also when the maximum is +inf (every finite element is 0.0 then). */
int omr_log_stft_post(float* spec, long frames, int bins, unsigned* max_ws, float* out, void* stream);
/* score-image front end (preprocessing.py:44-52: PIL convert("L") -> Image.resize (Pillow's default BICUBIC, antialiased,
 * 8-bit fixed point) -> ToTensor).  Bit-exact with Pillow.
 *   omr_resample_ksize / omr_resample_coeffs: HOST functions (no GPU work): taps per output pixel, and the tables
 *     bounds [out_size][2] = (first input index, count), coefs [out_size][ksize] (22 fractional bits); coeffs returns ksize.
 *   omr_image_gray_hpass: interleaved 8-bit pixels (channels 1 = L, 3 = RGB, 4 = RGBA, alpha ignored) -> luma ->
 *     horizontal pass -> dst [h][out_w] uint8, packed.  Strides of src: the bytes of a pixel are adjacent, pixels are
 *     `channels` bytes apart, rows row_stride BYTES apart with row_stride >= w * channels (any alignment; the bytes between
 *     rows are not read).  No other pixel or channel pitch is expressible: such views are packed by the caller.
 *     bounds = coefs = NULL (out_w == w): conversion only (channels == 1: a row-packing copy).
 *   omr_image_vpass_to_float: vertical pass over src [h][w] uint8, PACKED (rows w bytes apart) -> value / 255 as out_dtype
 *     (OMR_F32 / OMR_BF16) into dst rows dst_row_stride ELEMENTS apart, dst_row_stride >= w, unit stride inside a row (a
 *     sample's slot inside the padded batch tensor, preprocessing.py:55-75); only the out_h x w elements are written.
 *     bounds = coefs = NULL (out_h == h): conversion only.
 *   Both: a null src / dst, a size <= 0, channels outside {1, 3, 4}, one of bounds / coefs without the other, no tables with
 *     another output size, tables with ksize <= 0, a stride below the row length: OMR_ERR_ARG; another out_dtype:
 *     OMR_ERR_UNSUPPORTED; nothing is written then. */
int omr_resample_ksize(int in_size, int out_size);
int omr_resample_coeffs(int in_size, int out_size, int* bounds, int* coefs);
int omr_image_gray_hpass(const unsigned char* src, int h, int w, int channels, long row_stride, const int* bounds, const int* coefs,
                         int ksize, int out_w, unsigned char* dst, void* stream);
int omr_image_vpass_to_float(const unsigned char* src, int h, int w, const int* bounds, const int* coefs, int ksize, int out_h,
                             int out_dtype, void* dst, long dst_row_stride, void* stream);
/* late (prediction-level) fusion, src/multimodal/smith_waterman/test.py:136-150: Smith-Waterman local alignment of the
 * image model's and the audio model's token sequences.  HOST function (no GPU work).  Restates swalign 0.3.x's
 * LocalAlignment (package absent here: PARITY UNPINNED).  ref / query: token ids; ops receives one of 'm' 'i' 'd' per
 * alignment column (capacity nr + nq), r_pos / q_pos the 0-based start of the aligned region in ref / query; returns the
 * number of columns. */
/* Token noise of Transformer.apply_teacher_forcing (model.py:152-160) in one HOST call, continuing Python's own Mersenne
 * Twister: for each of `count` tokens (row-major B x T) draw random.random(); if it is < prob and the token is not pad_idx,
 * replace it by random.randint(0, vocab - 1).  mt_state[624] / *mt_index = random.getstate()[1] (words, position); both are
 * advanced exactly as the interpreter's calls would advance them, for random.setstate().  Host memory only. */
int omr_teacher_forcing_noise(long* tokens, long count, double prob, long pad_idx, long vocab, unsigned int* mt_state, int* mt_index);
int omr_sw_align(const int* ref, int nr, const int* query, int nq, int match, int mismatch, int gap_penalty,
                 int gap_extension_penalty, char* ops, int* r_pos, int* q_pos, int* score);
/* Sym-ER / Seq-ER edit distances (src/utils/metrics.py:59-88, levenshtein over token lists): unit-cost Levenshtein distance
 * of n pairs of int32 id sequences.  Pair i is a[a_off[i] .. a_off[i+1]) against b[b_off[i] .. b_off[i+1]) (offsets: n + 1
 * entries, non-decreasing); dist[i] receives its distance.  HOST function (no GPU work), two-row dynamic programme. */
int omr_edit_distance_batch(const int* a, const long* a_off, const int* b, const long* b_off, long n, long* dist);
/* beam-search expansion (BASELINE config C5; an extension: the reference decodes greedily): per row the k largest
 * log_softmax values and their token ids, same tie rule as omr_argmax, idx_out / val_out [rows][k] */
int omr_topk_logprob(const float* x, int rows, int n, long ld, int k, long* idx_out, float* val_out, void* stream);

/* ---- normalisation ------------------------------------------------------------------------------------- */
/* nn.InstanceNorm2d(eps=1e-3, affine=False) on x[B][HW][C] (encoder.py:151-156,174,232); the apply is fused into the consumer
 * conv (in_mean / in_rstd arguments below).  Statistics are reduced DETERMINISTICALLY (bit-identical from run to run, like
 * the reference's CPU path): every producer block stores fp64 partials into its own slot of workspace[B][slots][C][2] and
 * the consumer adds an image's slots in index order -- no atomics.  workspace_bytes covers the slots plus the compact
 * [B][C][2] sums the backward apply reads; slots = omr_instnorm_slots(B, HW) for the stand-alone passes
 * (omr_instnorm_stats / omr_instnorm_bwd) or omr_conv3x3_stat_slots(B, Ho, Wo) when a conv epilogue is the producer
 * (a conv launch that uses fewer blocks per image than there are slots writes zeros into the rest: no clearing needed). */
int omr_instnorm_slots(int B, long HW);
long omr_instnorm_workspace_bytes(int B, int C, int slots);
int omr_instnorm_stats(int dtype, const void* x, float* mean, float* rstd, int B, long HW, int C, float eps, void* workspace, void* stream);
int omr_instnorm_finalize(const void* workspace, int slots, float* mean, float* rstd, int B, long HW, int C, float eps, void* stream);
int omr_instnorm_bwd_apply(int dtype, const void* dxhat, const void* x, const float* mean, const float* rstd, void* dx, int B, long HW, int C,
                           int relu_mask, float relu_scale, void* workspace, int slots, void* stream);
int omr_instnorm_bwd(int dtype, const void* dxhat, const void* x, const float* mean, const float* rstd, void* dx, int B, long HW, int C,
                     int relu_mask, float relu_scale, void* workspace, void* stream);
/* post-norm residual with the sublayer dropout fused: out = LayerNorm(dropout(x) + res) (eps 1e-5), torch
 * nn/modules/transformer.py:1146-1154 (x = dropout1/2/3(sublayer), res = the residual stream).  drop_p = 0: plain add.
 * The mask is omr_dropout's counter-based mask (same seed / element-index convention) and is regenerated in backward.
 * Backward: ds = gradient of res (and of x when drop_p = 0); with drop_p > 0, dx receives the gradient of x. */
int omr_add_layernorm_fwd(int dtype, const void* x, const void* res, const float* gamma, const float* beta, void* out, float* mean,
                          float* rstd, long M, int d, float eps, float drop_p, unsigned long long drop_seed, void* stream);
int omr_add_layernorm_bwd(int dtype, const void* dy, const void* x, const void* res, const float* gamma, const float* mean,
                          const float* rstd, void* ds, float* dgamma, float* dbeta, long M, int d, float drop_p,
                          unsigned long long drop_seed, void* dx, void* stream);

/* ---- ragged batches: samples of different sizes in one padded plane ----------------------------------------- */
/* The reference trains on inputs of different sizes at batch size 1 (its encoder, encoder.py:241-291, pads nothing: zero padding
 * would move every conv's border and enter every InstanceNorm).  Here B samples share one NHWC plane x[B][H][W][C], sample b's
 * content in the top-left corner, extents [B][2] int32 ON THE DEVICE = (h_b, w_b) at this layer's resolution (ceil(h / stride)
 * per strided conv, the rule of omr_conv3x3_fwd's output size); every activation is kept zero outside its extent, which makes
 * sample b's features and gradients those of b run alone (DESIGN.md "Ragged training").  No function below reads a value that
 * lies outside an extent.  16-byte accesses when C is a multiple of 4 (fp32) / 8 (bf16), element-wise otherwise.  Limits: B <= 65535;
 * H * W * C <= 2^31 - 1 per sample (and Smax * C for the pack pair), else OMR_ERR_ARG; the two InstanceNorm entries keep one channel
 * group (4 / 8 channels, or 1 on the element-wise path) per thread of a 256-thread workgroup and return OMR_ERR_UNSUPPORTED beyond
 * that: C <= 1024 (fp32) / 2048 (bf16) when C is a multiple of 4 / 8, C <= 256 otherwise.  omr_extent_zero and the pack pair take any C.
 * A thread of the statistics passes adds its pixels in fp32 before the fp64 slot sum (omr_instnorm_stats' convention): 2048 pixels per
 * workgroup over 256 / (channel groups) threads per group, i.e. up to 512 pixels per thread at the encoder's widest map (C = 256 fp32)
 * and all 2048 at the widest C the entries take.
 *   omr_extent_zero: x[b,i,j,:] = 0 for i >= h_b or j >= w_b, in place, after the bias + ReLU of encoder.py:163-176,222-236 made the
 *     outside non-zero; its own adjoint, so the same call serves the gradient.  Stores to the outside only.
 *   omr_instnorm_extent_fwd: nn.InstanceNorm2d(eps, affine=False) of encoder.py:151-156,174,232 with sums over the extent (count
 *     h_b * w_b, biased variance, fp64 slots, omr_instnorm_finalize's arithmetic): y = (x - mean) * rstd inside, 0 outside; mean /
 *     rstd [B][C] fp32.  workspace: omr_instnorm_workspace_bytes(B, C, omr_instnorm_extent_slots(B, H * W)), no clearing needed.
 *   omr_instnorm_extent_bwd: dx = rstd * (g - sum g / n - xhat * sum(g * xhat) / n) [* (x > 0) * relu_scale] inside, 0 outside
 *     (omr_instnorm_bwd over the extent); same workspace.
 *   omr_pack_memory_fwd / _bwd: x.flatten(2).permute(0, 2, 1) of model.py:147 per sample: out[b][i * w_b + j][:] = x[b][i][j][:],
 *     rows h_b * w_b <= r < Smax of out[B][Smax][C] zero; the backward scatters dout back (zeros outside, rows >= h_b * w_b ignored).
 *   omr_concat_memory_fwd / _bwd: torch.cat([xi, xa], dim=1) of mixer_concat, model.py:644-675, per sample.  a [B][La][C] and
 *     b [B][Lb][C] are packed memories, len_a / len_b int32 [B] ON THE DEVICE, la = clamp(len_a[b], 0, La), lb likewise:
 *     out[b][r] = a[b][r] for r < la, b[b][r - la] for la <= r < la + lb, 0 for la + lb <= r < Smax (out [B][Smax][C]; rows the
 *     concatenation has beyond Smax are dropped).  Backward: da[b][r] = dout[b][r] for r < la and r < Smax, db[b][r] = dout[b][la + r]
 *     for r < lb and la + r < Smax, 0 elsewhere, both in one launch.  Tail-zeroing form: b (db) = NULL with Lb = 0 (len_b is not
 *     read) copies the first la rows and zeroes the rest.  Rows of a / b at or past their length and rows of dout at or past
 *     la + lb are never read.  La * C, Lb * C and Smax * C <= 2^31 - 1, else OMR_ERR_ARG; any C. */
int omr_extent_zero(int dtype, void* x, const int* extents, int B, int H, int W, int C, void* stream);
int omr_instnorm_extent_slots(int B, long HW);
int omr_instnorm_extent_fwd(int dtype, const void* x, const int* extents, void* y, float* mean, float* rstd, int B, int H, int W, int C,
                            float eps, void* workspace, void* stream);
int omr_instnorm_extent_bwd(int dtype, const void* dxhat, const void* x, const float* mean, const float* rstd, const int* extents, void* dx,
                            int B, int H, int W, int C, int relu_mask, float relu_scale, void* workspace, void* stream);
int omr_pack_memory_fwd(int dtype, const void* x, const int* extents, void* out, int B, int H, int W, int C, int Smax, void* stream);
int omr_pack_memory_bwd(int dtype, const void* dout, const int* extents, void* dx, int B, int H, int W, int C, int Smax, void* stream);
int omr_concat_memory_fwd(int dtype, const void* a, const int* len_a, int La, const void* b, const int* len_b, int Lb, void* out, int B, int C,
                          int Smax, void* stream);
int omr_concat_memory_bwd(int dtype, const void* dout, const int* len_a, int La, const int* len_b, int Lb, void* da, void* db, int B, int C,
                          int Smax, void* stream);
/* A padded batch out [B][1][H][W] from a device-resident data set in ONE launch: pad_batch_inputs (src/data/preprocessing.py:55-75)
 * plus the / 255 of preprocess_image (:44-52).  src is one packed device buffer of src_dtype elements (OMR_DTYPE_U8: grays before the
 * / 255; OMR_F32: spectrograms); sample n is a row-major h_n x w_n plane that starts at ELEMENT offsets[n] (int64 [N] on the device),
 * sizes int32 [N][2] on the device = (h_n, w_n) clamped to [0, H] x [0, W], idx int32 [B] on the device (clamped to [0, N)), the
 * same index may occur twice.  out[b][0][i][j] = conv(src[offsets[n] + i * w_n + j]) for i < h_n, j < w_n, n = idx[b], pad_value
 * everywhere else (0: the ragged route; 1.0: the white background of preprocessing.py:104-109; a NaN pad stays a NaN: fp32 keeps its bits,
 * bf16 gets 0xFFFF, what torch's host fp32 -> bf16 conversion writes for any NaN).  conv(uint8 v)
 * = v / 255 by a correctly rounded fp32 DIVISION (omr_image_vpass_to_float's expression: the floats of preprocess_image, to the
 * bit); an fp32 source is copied.  dst_dtype OMR_F32 or OMR_BF16 (the rounded fp32 value: omr_cast's).  Of src exactly the h_n * w_n
 * elements of each listed sample are read.  16-byte stores when W is a multiple of 4 (fp32) / 8 (bf16) and out is 16-byte aligned.
 * B < 1, B > 65535, N < 1, H * W > 2^31 - 1 or a null pointer: OMR_ERR_ARG; any other dtype code: OMR_ERR_UNSUPPORTED. */
int omr_gather_ragged_batch(int src_dtype, const void* src, const long* offsets, const int* sizes, int N, const int* idx, int dst_dtype,
                            void* out, int B, int H, int W, float pad_value, void* stream);
/* omr_gather_ragged_batch with a fresh distortion of every sample inside the same launch: what the reference can only offer as a second,
 * pre-rendered copy of every score (`image_distorted`, src/data/ar_dataset.py:258-265,377) on the way into pad_batch_inputs
 * (src/data/preprocessing.py:55-75).  aug: B records on the device, record b for batch row b (the same sample may occur twice with
 * different records).  With n = idx[b], (h, w) = sizes[n] (the SOURCE plane: not clamped to H, W; h * w <= 2^31 - 1) and
 * (oh, ow) = (out_h, out_w) clamped to [0, H] x [0, W], destination pixel (i, j) of row b is
 *   pad_value (omr_gather_ragged_batch's rule, NaN included)               for i >= oh or j >= ow;
 *   conv(fill)                                                             for i in a row band or j in a column band
 *                                                                          (start <= . < start + length; length <= 0: no band);
 *   otherwise, every step ONE rounded fp32 operation, no product fused into an add:
 *   1. y = (m0 * i + m1 * j) + m2, x = (m3 * i + m4 * j) + m5; y = fminf(fmaxf(y, -1), h), x = fminf(fmaxf(x, -1), w) (a NaN becomes -1);
 *   2. y0 = floorf(y), fy = y - y0, x0 = floorf(x), fx = x - x0;
 *   3. lerp(v0, v1, f) = f == 0 ? v0 : v0 * (1 - f) + v1 * f (v1 is not read for f == 0);
 *      g = lerp(lerp(tap(y0, x0), tap(y0, x0 + 1), fx), lerp(tap(y0 + 1, x0), tap(y0 + 1, x0 + 1), fx), fy); a tap is the source element
 *      as a float (a gray 0 .. 255 for OMR_DTYPE_U8), `fill` outside the plane: only elements of listed samples are read;
 *   4. g = gain * g + bias unless gain == 1 and bias == 0;
 *   5. noise != 0: g = g + noise * ((float)(hash32(seed_lo, seed_hi, i * ow + j) >> 8) * 2^-23 - 1), hash32 of csrc/omr_common.h, the
 *      index in 32-bit unsigned arithmetic;
 *   6. OMR_DTYPE_U8: g = fminf(fmaxf(g, 0), 255);   7. conv(g): g / 255 by the correctly rounded division (u8), g itself (fp32);
 *   8. the output type's rounding (omr_cast's).
 * The identity record (m = 1,0,0, 0,1,0; gain 1, bias 0, noise 0, no bands, out_h, out_w = h, w) gives omr_gather_ragged_batch's bits.
 * Arguments are checked like omr_gather_ragged_batch's; aug == NULL: OMR_ERR_ARG. */
typedef struct OmrAugment {
    float m[6];                 /* source (y, x) of destination pixel (i, j): y = m0*i + m1*j + m2, x = m3*i + m4*j + m5 */
    float gain, bias;           /* in source units (grays 0..255 for a u8 store, the value itself for f32) */
    float noise;                /* amplitude in source units, 0 = off */
    float fill;                 /* value of every tap outside the source plane, and of masked bands (255 = paper, 0 = silence) */
    int out_h, out_w;           /* extent of the augmented sample in the output plane (clamped to H, W) */
    unsigned seed_lo, seed_hi;  /* noise stream */
    int rows[2][2], cols[2][2]; /* up to two row bands and two column bands (start, length); length <= 0 = none */
} OmrAugment;
int omr_gather_augmented_batch(int src_dtype, const void* src, const long* offsets, const int* sizes, int N, const int* idx,
                               const OmrAugment* aug, int dst_dtype, void* out, int B, int H, int W, float pad_value, void* stream);

/* ---- GEMM: C[M,N] (+)= act(opA(A) . opB(B)^T + bias) ------------------------------------------------------ */
/* aten::linear/addmm/mm of the decoder layers (torch nn/modules/transformer.py:1158-1199), 1x1 point_conv
 * (encoder.py:65-70), Conv1d(k=1) head (decoder.py:98-102,146).  transA/transB: operand stored reduction-major.
 * split_k > 1 accumulates into fp32 C with atomics (C must hold the running sum / zeros).
 * colsum_a (nullable, transA only): colsum_a[m] += sum_k A[k][m] -- the bias gradient of a linear layer comes out of the
 * same pass that computes its weight gradient dW = dY^T . X.
 * drop_p > 0: nn.Dropout on the (activated) output, omr_dropout's mask over the flat [M][ldc] element index (FFN dropout,
 * torch nn/modules/transformer.py:1197-1199).
 * row_group_operand != 0: the weight-side operand is a row-group view -- logical row i is physical row
 * (i / row_group) * row_group_stride + row_group_base + i % row_group (row_group a multiple of 128); operand 1 = rows of B and
 * bias entries, 2 = reduction rows of a transposed B, 3 = rows of C and colsum_a entries.  One call then covers the K|V rows
 * of all decoder layers' packed in_proj_weight ([Wq;Wk;Wv], torch nn/modules/activation.py) laid back to back. */
int omr_gemm(int dtype, int c_dtype, int transA, int transB, int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C,
             long ldc, const float* bias, int relu, int accumulate, int split_k, float* colsum_a, float drop_p,
             unsigned long long drop_seed, int row_group, int row_group_stride, int row_group_base, int row_group_operand, void* stream);

/* fp8 path (BASELINE config 5 "fp8 MFMA weights"; an extension -- the reference has no fp8; inference only).  Operands are
 * OCP e4m3 with one fp32 scale per ROW: weights [N][K] quantised once (scale per output feature), activations [M][K] per
 * token on the fly.  omr_quantize_rows_fp8: scale[m] = absmax(row) / 448, q = round_to_fp8(x / scale) (x in `dtype`).
 * omr_gemm_fp8: C[M][N] = (A8 . W8^T) * scale_a[m] * scale_w[n] + bias[n] [-> ReLU], products on the fp8 MFMA
 * (v_mfma_f32_32x32x16_fp8_fp8), fp32 accumulation, C in c_dtype; K and both row strides multiples of 16. */
int omr_quantize_rows_fp8(int dtype, const void* x, long ldx, unsigned char* q, long ldq, float* scale, int M, int K, void* stream);
int omr_gemm_fp8(int c_dtype, int M, int N, int K, const unsigned char* A8, long lda, const float* scale_a, const unsigned char* W8, long ldb,
                 const float* scale_w, void* C, long ldc, const float* bias, int relu, void* stream);

/* Weight (and bias) gradients of SEVERAL linear layers in one launch: for each problem dw[n_out][n_in] += dy^T . x and
 * db[n_out] += column sums of dy (db nullable), reducing over `rows`; dy [rows][ld_dy], x [rows][ld_x] in `dtype`, dw / db fp32
 * accumulators (fp32 atomics: the buffers hold the running sums).  A linear's dW at d_model = 256 is too small to fill the
 * chip on its own (aten::mm of the decoder layers / 1x1 point_convs, torch nn/modules/transformer.py:1158-1199,
 * encoder.py:65-70): the backward pass collects them and launches them together.  row_group* (0 = off): dw rows / db
 * entries are a row-group view as in omr_gemm (operand 3).  `problems` is a HOST array. */
typedef struct omr_dw_problem {
    const void* dy; const void* x; float* dw; float* db;
    int rows, n_out, n_in, row_group; long ld_dy, ld_x, ld_dw; int row_group_stride, row_group_base;
} omr_dw_problem;
int omr_linear_wgrad_grouped(int dtype, int nprob, const omr_dw_problem* problems, void* stream);

/* ---- convolutions (NHWC) --------------------------------------------------------------------------------- */
/* nn.Conv2d 3x3 pad 1 (encoder.py:132-150) with fused bias + ReLU, optional fused InstanceNorm apply on the input
 * (in_mean/in_rstd [B][CIN]) and optional epilogue mask (y = mask>0 ? y*mask_scale : 0).  Weights [COUT][3][3][CIN].
 * dil_* > 1 reads the input as if zero-dilated: with flipped weights (omr_conv3x3_weight_flip) this is the data
 * gradient of a strided conv.  CIN == 1 takes the direct (non-MFMA) first-layer path. */
/* Fused on the output: MixDropout after the ReLU (drop_p > 0; encoder.py:165-179; elementwise mask keyed by the flat NHWC
 * index, or per (image, channel) when drop_channel_mode) and a per-(image, channel) reduction over the stored tile into
 * the fp64 slots stat_ws[B][stat_slots][COUT][2] (every slot is written; stat_slots = omr_conv3x3_stat_slots(B, Ho, Wo), an
 * upper bound on the persistent grid's blocks per image; deterministic, see "normalisation"): stat_mode 1 = {sum y, sum y^2}
 * (InstanceNorm statistics of this output, finalised by omr_instnorm_finalize), stat_mode 2 = {sum g, sum g*xhat} with
 * xhat = (stat_x - mean)*rstd (InstanceNorm backward sums when this call is the data gradient that produces g = dL/dxhat;
 * consumed by omr_instnorm_bwd_apply).
 * stat_mode 4 / 5 -- the data gradient through a normalise-on-load conv without ever storing g: mode 4 takes the sums of
 * mode 2 and stores nothing (y may be NULL); omr_instnorm_reduce_sums adds the slots of each image; mode 5 recomputes the
 * data gradient and applies the InstanceNorm backward in its epilogue, y = rstd * (g - mean(g) - xhat * mean(g * xhat)),
 * times (stat_x > 0) * mask_scale when `relu` is set (the ReLU / dropout backward of the layer that produced stat_x).  In
 * these two modes bias and out_mask must be NULL.  (The stand-alone form is omr_instnorm_bwd_apply on a stored g.) */
int omr_conv3x3_stat_slots(int B, int Ho, int Wo);
int omr_instnorm_reduce_sums(void* workspace, int slots, int B, int C, void* stream);
int omr_conv3x3_fwd(int dtype, const void* x, const void* w, const float* bias, void* y, const float* in_mean, const float* in_rstd,
                    const void* out_mask, float mask_scale, int B, int H, int W, int CIN, int COUT, int stride_h, int stride_w, int dil_h,
                    int dil_w, int Ho, int Wo, int relu, float drop_p, unsigned long long drop_seed, int drop_channel_mode,
                    int stat_mode, double* stat_ws, int stat_slots, const void* stat_x, const float* stat_mean, const float* stat_rstd,
                    void* stream);
int omr_conv3x3_weight_flip(int dtype, const void* w, void* wd, int COUT, int CIN, void* stream);
/* The same re-layout for n convs in ONE launch (descs is a HOST array): the data-gradient weights of every 3x3 conv are
 * refreshed once per optimizer step, behind omr_adam, so the backward pass (aten::convolution_backward of encoder.py:132-150)
 * carries no re-layout launches. */
typedef struct omr_flip_desc { const void* w; void* wd; int cout, cin; } omr_flip_desc;
int omr_conv3x3_weight_flip_grouped(int dtype, int n, const omr_flip_desc* descs, void* stream);
/* dw[COUT][3][3][CIN] (fp32) += dy^T * im2col(x);  db[COUT] (nullable, fp32) += column sums of dy (bias gradient) */
int omr_conv3x3_wgrad(int dtype, const void* x, const void* dy, float* dw, float* db, const float* in_mean, const float* in_rstd, int B, int H, int W,
                      int CIN, int COUT, int stride_h, int stride_w, int Ho, int Wo, void* stream);
/* The whole backward of a stride-1 3x3 conv with CIN, COUT in {16, 32} (bf16; (COUT, CIN) = (32,32), (32,16), (16,16)) in one pass
 * over its operands (aten::convolution_backward of nn.Conv2d, encoder.py:132-150): dx = conv^T(g) [* (x > 0) * mask_scale],
 * dw[COUT][3][3][CIN] += g^T im2col(x), db[COUT] (nullable) += column sums of g.  w_flipped = omr_conv3x3_weight_flip(w).
 * norm_y != NULL: g is dL/d(InstanceNorm output) of the layer above and norm_y that layer's input (= this conv's stored output);
 * the InstanceNorm backward (omr_instnorm_bwd_apply's arithmetic, sums from norm_workspace after omr_instnorm_reduce_sums)
 * and the ReLU / dropout mask of norm_y are applied while the tile is loaded, so the gradient w.r.t. this conv's output never
 * exists in memory.  x_mean / x_rstd != NULL (CIN = COUT = 16): the conv normalised its input on load; xhat = (x - mean) * rstd is
 * formed in LDS for the weight gradient and dx = dL/dxhat leaves with {sum dx, sum dx * xhat} reduced into the slots of
 * stat_workspace (omr_conv3x3_fwd stat_mode 2's layout: omr_instnorm_bwd_apply or the norm_y form above consumes them).
 * OMR_ERR_UNSUPPORTED for other shapes (callers then use omr_conv3x3_fwd + omr_conv3x3_wgrad). */
int omr_conv3x3_bwd_fused(const void* g, const void* x, const void* w_flipped, void* dx, float* dw, float* db, int B, int H, int W, int CIN,
                          int COUT, int mask_input, float mask_scale, const void* norm_y, const float* norm_mean, const float* norm_rstd,
                          const void* norm_workspace, int norm_slots, int relu_mask, float relu_scale, const float* x_mean, const float* x_rstd,
                          void* stat_workspace, int stat_slots, void* stream);
/* The same for the stride-(2,2) normalise-on-load conv with 32 -> 32 channels (ConvBlock 1's conv3, encoder.py:132-156): g is the
 * gradient of the [ceil(H/2)][ceil(W/2)] output, x the [H][W] input, dx = dL/dxhat with the InstanceNorm-backward sums in the slots. */
int omr_conv3x3_bwd_fused_s2(const void* g, const void* x, const void* w_flipped, void* dx, float* dw, float* db, int B, int H, int W,
                             const float* x_mean, const float* x_rstd, void* stat_workspace, int stat_slots, void* stream);
/* depthwise 3x3, stride 1, pad 1 (DepthSepConv2D.depth_conv, encoder.py:56-64); flip=1 mirrors the taps (data gradient) */
int omr_dwconv3x3(int dtype, const void* x, const void* w, const float* bias, void* y, const float* in_mean, const float* in_rstd,
                  const void* out_mask, float mask_scale, int B, int H, int W, int C, int flip, void* stream);
int omr_dwconv3x3_wgrad(int dtype, const void* x, const void* dy, float* dw, float* db, const float* in_mean, const float* in_rstd, int B,
                        int H, int W, int C, void* stream);

/* ---- attention ------------------------------------------------------------------------------------------ */
/* softmax(Q K^T / sqrt(hd) + masks) V per head (torch nn/functional.py multi_head_attention_forward; decoder.py:86-95,
 * model.py:292-297,323).  q/k/v/o are [B][rows][ld*] with head h at columns [h*hd, (h+1)*hd).  key_bias [B][S] is
 * ADDED (float +1.0 padding masks, -inf for bool masks); causal/window per decoder.py:191-217; blk_lq/blk_lkv [B]
 * reproduce CrossAttention.create_attention_mask incl. its (b*H+h)%B tiling (model.py:343-354). */
int omr_attn_fwd(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv, long ldo,
                 long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim, int causal, int window,
                 const float* key_bias, const int* blk_lq, const int* blk_lkv, float dropout_p, unsigned long long seed,
                 const unsigned long long* drop_words, void* stream);
/* Attention-probability dropout (nn.MultiheadAttention dropout, decoder.py:91; model.py:292-297).  The keep bits are a pure
 * function of (seed, b, h, query, key).  With dropout_p > 0 the attention kernels do not hash: they READ the bits, 1 per score,
 * from `drop_words` -- omr_attn_dropout_words_count(B, H, T, S) 64-bit words that omr_attn_dropout_words fills for
 * (dropout_p, seed), once per (layer, step), in the accumulator layout of the kernels (word = one register of a 32-query x
 * 64-key tile, bit = lane): forward and dQ take a word as the SGPR mask of one v_cndmask per score, dK/dV reads a 32-bit
 * column of the same words per key.  Forward and backward of a layer get the same buffer.  drop_words may be NULL when
 * dropout_p == 0. */
long omr_attn_dropout_words_count(int B, int H, int T, int S);
int omr_attn_dropout_words(unsigned long long* words, int B, int H, int T, int S, float dropout_p, unsigned long long seed, void* stream);
/* omr_attn_fwd / omr_attn_bwd with caller-provided scratch that lets the library split the KEYS of a (batch, head, query block)
 * over several workgroups where that fills the chip better (the query-per-lane kernels have B*H*T/32 waves whatever S is:
 * 2 per SIMD at B 32, T 512): partial softmaxes / partial dQ sums are merged by fixed-order kernels, results are
 * deterministic.  ws: omr_attn_workspace_floats(B, H, T, S, head_dim, causal, backward) floats (0 = this shape is not split;
 * NULL / 0 is then fine).  Same arguments and semantics as omr_attn_fwd / omr_attn_bwd otherwise. */
long omr_attn_workspace_floats(int B, int H, int T, int S, int head_dim, int causal, int backward);
int omr_attn_fwd_ws(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv, long ldo,
                    long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim, int causal, int window,
                    const float* key_bias, const int* blk_lq, const int* blk_lkv, float dropout_p, unsigned long long seed,
                    const unsigned long long* drop_words, float* ws, long ws_floats, void* stream);
int omr_attn_bwd_ws(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, float* delta_ws,
                    void* dq, void* dk, void* dv, long ldq, long ldk, long ldv, long ldo, long lddo, long lddq, long lddk, long lddv, long bsq,
                    long bsk, long bsv, long bso, long bsdo, long bsdq, long bsdk, long bsdv, int B, int H, int T, int S, int head_dim,
                    int causal, int window, const float* key_bias, const int* blk_lq, const int* blk_lkv, float dropout_p,
                    unsigned long long seed, const unsigned long long* drop_words, float* ws, long ws_floats, void* stream);
/* Attention map: the head-averaged attention weights of CrossAttention (model.py:323, `attn_output, attn_weights = ...`), which
 * torch's multi_head_attention_forward returns with need_weights = True, average_attn_weights = True -- recomputed from the `lse`
 * omr_attn_fwd* wrote for the same operands (same layout [B][H][T], natural log):
 *   w[b][t][s] (+)= out_scale * sum_h c * m_bhts * exp(score_bhts - lse_bht),      w fp32 [B][T][ldw], batch stride bsw
 * score is what omr_attn_fwd scores (q.k / sqrt(hd) + key_bias, -inf under causal / window / the block mask / s >= kv_len[b]);
 * m is the keep bit of drop_words (omr_attn_dropout_words) and c = 1 / (1 - p) when dropout_p > 0 -- torch returns the
 * post-dropout weights in train mode -- else m = c = 1.  out_scale = 1 / H is torch's head average; 1 / (H L) with accumulate = 1
 * on all but the first call averages L layers into one buffer.  Every s < S of every row is written (hidden keys: exactly 0; a
 * row whose lse is -inf: zeros), columns S .. ldw - 1 are not touched.  kv_len: device int32 [B] or NULL.  No atomics: two runs
 * give the same bits.  fp32 / bf16 operands, head_dim 32 or 64 (else OMR_ERR_UNSUPPORTED); q, k 16-byte aligned with row and
 * batch strides that are multiples of 16 bytes. */
int omr_attn_weights(int dtype, const void* q, const void* k, const float* lse, float* w, long ldq, long ldk, long ldw, long bsq, long bsk,
                     long bsw, int B, int H, int T, int S, int head_dim, int causal, int window, const float* key_bias, const int* blk_lq,
                     const int* blk_lkv, const int* kv_len, float dropout_p, const unsigned long long* drop_words, float out_scale,
                     int accumulate, void* stream);
/* keys one workgroup of omr_attn_weights walks for (B, T, S): a multiple of 64, the launcher's own plan (tests assert that their
 * shapes give a workgroup more than one 64-key tile); 0 for a non-positive size */
long omr_attn_weights_range(int B, int T, int S);
/* omr_attn_fwd for ONE block of at most 32 query rows (KV-cached decode: T = 1) with the keys split over workgroups of 256 keys
 * (partial softmaxes merged by a second small kernel): a single query row would otherwise keep each (batch, head) on one
 * workgroup walking all S keys.  No causal / block masks (a decode step sees every cached key), no dropout.
 * split_ws: omr_attn_split_workspace_floats(...) floats of device scratch (0 = the shape needs no split). */
long omr_attn_split_workspace_floats(int B, int H, int T, int S, int head_dim);
int omr_attn_fwd_split(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv, long ldo,
                       long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim, const float* key_bias,
                       float* split_ws, long split_ws_floats, void* stream);
/* omr_attn_fwd_split without its merge pass (decode: the out-projection merges while it loads its input rows).  *nsplit > 1:
 * `o` is not written and split_ws holds, for (b, h, split j), head_dim un-normalised outputs + the running max (log2 domain)
 * + the sum at ((b*H + h)*nsplit + j)*T*(head_dim + 2); *nsplit = 1: `o` holds the finished rows. */
int omr_attn_fwd_split_partials(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv,
                                long ldo, long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim, float* split_ws,
                                long split_ws_floats, int* nsplit, void* stream);
/* omr_attn_fwd_split over a ragged batch (the cross-attention of batched greedy decoding over memories of different lengths;
 * the reference decodes one memory at a time, src/transformer/model.py:171-199): S is the padded key count and batch row b
 * attends over keys [0, kv_len[b]) (device int32 [B], 1 <= kv_len[b] <= S; NULL = every row sees S).  The key split is the
 * plan of S; a split past a row's end contributes nothing.  Rows with kv_len[b] > 64 are bit-equal to omr_attn_fwd_split of
 * that row alone with S = kv_len[b].  S <= 64 with a non-NULL kv_len returns OMR_ERR_UNSUPPORTED (that shape does not take
 * the key-split kernel, which alone reads kv_len). */
int omr_attn_fwd_split_varlen(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv,
                              long ldo, long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim,
                              const float* key_bias, const int* kv_len, float* split_ws, long split_ws_floats, void* stream);
/* omr_attn_fwd_split_varlen with a per-row first key as well (continuous batching of greedy evaluation: the reference decodes
 * one input at a time, src/transformer/model.py:171-199; here the rows of a decode state each sit at their own position, so
 * the banded self-attention window [lo_b, t_b] of decoder.py:213-214 differs per row).  Row b attends over rows
 * [kv_start[b], kv_start[b] + kv_len[b]) of its K / V slot (kv_start: device int32 [B], in keys, NULL = 0; key_bias[b][j]
 * belongs to key kv_start[b] + j); nothing outside that range is read.  S = the largest kv_len, any value >= 1: this entry
 * always takes the key-split kernel, so output and lse of every row are bit-equal to omr_attn_fwd_split of that row alone
 * (K / V advanced by kv_start[b], S = kv_len[b]) for every kv_len[b] >= 1, 64 keys and fewer included. */
int omr_attn_fwd_split_rows(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, long ldq, long ldk, long ldv,
                            long ldo, long bsq, long bsk, long bsv, long bso, int B, int H, int T, int S, int head_dim,
                            const float* key_bias, const int* kv_len, const int* kv_start, float* split_ws, long split_ws_floats,
                            void* stream);
/* Test / debug entry: the attention-probability dropout keep-mask (1 = kept) for (seed, dropout_p) -- the function
 * omr_attn_dropout_words packs -- one byte per score, mask[B][H][T][S].  Lets a checker inject the very same mask into a CPU
 * restatement of nn.MultiheadAttention's dropout (tests/test_dropout_parity_gpu.py). */
int omr_attn_dropout_mask(unsigned char* mask, int B, int H, int T, int S, float dropout_p, unsigned long long seed, void* stream);
int omr_attn_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, float* delta_ws,
                 void* dq, void* dk, void* dv, long ldq, long ldk, long ldv, long ldo, long lddo, long lddq, long lddk, long lddv, long bsq,
                 long bsk, long bsv, long bso, long bsdo, long bsdq, long bsdk, long bsdv, int B, int H, int T, int S, int head_dim,
                 int causal, int window, const float* key_bias, const int* blk_lq, const int* blk_lkv, float dropout_p,
                 unsigned long long seed, const unsigned long long* drop_words, void* stream);

/* ---- KV-cached greedy decoding: one host call per run of tokens ------------------------------------------------------ */
/* Reference: the autoregressive loop of Transformer.validation_step / get_pred_seq_and_pred_prob_seq (model.py:182-193,
 * 247-260) -- embed the last token, run every decoder layer, project to the vocabulary, argmax, repeat.  omr_decode_steps
 * runs n_steps positions t0 .. t0+n_steps-1 for B independent rows without returning to the caller in between: per position
 * it appends the self-attention K|V to the cache, attends over the cached keys (banded by `window`, decoder.py:213-214) and
 * over the cross-attention K|V projected once per input, and (out_tokens != NULL) writes the argmax token [step][B] (and its
 * fp32 logit, out_top1, nullable) and feeds it to the next position through `tokens` (device int64 [B], updated in place).
 * out_tokens == NULL: one position only, no token pick (beam search / late fusion choose the token themselves).
 * last_logits (nullable): fp32 [B][ldv] logits of the last position.  All pointers are device pointers except `layer_w`.
 * layer_w: HOST array [L][OMR_DECODE_LAYER_PTRS] of device pointers, per layer in this order (torch parameter names):
 *   self_attn.in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, norm1.weight, norm1.bias,
 *   multihead_attn.in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, norm2.weight, norm2.bias,
 *   linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm3.weight, norm3.bias
 * (matrices in `dtype`, biases / LayerNorm vectors fp32).  self_kv [L][B][max_len][2d]; cross_kv: layer l's K|V rows of
 * sample b, key s at cross_kv + b*cross_bs + s*cross_ld + l*2d (elements; cross_bs = 0 shares one memory between rows). */
#define OMR_DECODE_LAYER_PTRS 18
/* fp8 != 0 (BASELINE config 5 "fp8 MFMA weights", an extension): the linears run as omr_quantize_rows_fp8 + omr_gemm_fp8 on
 * weights quantised once per output row.  layer_w8 / layer_s8: HOST arrays [L][OMR_DECODE_LAYER_FP8] of device pointers to the
 * e4m3 codes [rows][in] and fp32 row scales of, in order: self_attn.in_proj_weight, self_attn.out_proj.weight,
 * multihead_attn.in_proj_weight, multihead_attn.out_proj.weight, linear1.weight, linear2.weight; head_w8 / head_s8: the head.
 * Biases, LayerNorm, embedding, attention and the cross-attention K|V (projected once at init) stay in `dtype`. */
#define OMR_DECODE_LAYER_FP8 6
typedef struct omr_decode_desc {
    int dtype, B, L, d, nhead, ff, V, ldv, max_len, S, window, fp8;
    const void* emb; const float* pe; const void* const* layer_w; const void* head_w; const float* head_b;
    void* self_kv; const void* cross_kv; long cross_ld, cross_bs; void* ws; long ws_bytes;
    const unsigned char* const* layer_w8; const float* const* layer_s8; const unsigned char* head_w8; const float* head_s8;
} omr_decode_desc;
long omr_decode_workspace_bytes(const omr_decode_desc* desc);
/* One linear layer of a decode position, y[m][n] = act(sum_k x[m][k] * w[n][k] + bias[n]) for a handful of rows (M = batch rows
 * of ONE position), with the element-wise kernel that would precede it folded into the loading of x (`pro`):
 *   0  x = rows of `x` (ld ldx)
 *   1  x = LayerNorm(y_prev + res) * gamma + beta   (nn.TransformerDecoderLayer norm1/2/3, decoder.py:86-95; y_prev = `x`)
 *   2  x = embedding[tokens[m]] + pe_row            (decoder.py:124 at one position)
 *   3  x = the merged key-split attention partials of omr_attn_fwd_split_partials (part, nsplit, H, hd; K = H * hd)
 * Prologues 1 and 2 also store the rows they build to xn_out [M][K] (the residual input of the next sub-layer).  Columns
 * [0, n0) go to out0 (ld0), the rest to out1 (ld1) -- a q | k|v projection writes its k|v part straight into the cache row;
 * out32 (nullable, ld32): fp32 copy of the value rounded to `dtype` (the vocabulary head's logits).  Each (row, column) is
 * a fixed-order fp32 sum that does not depend on M: a batched step reproduces the single-row step to the bit.
 * amax_idx (nullable): also return, per row, the first index of the largest rounded output and its value (the greedy pick of
 * model.py:187,253): every workgroup leaves its 16-column candidate in amax_part (>= 2 * M * ceil(N/16) floats of scratch) and
 * a second, one-wave-per-row launch reduces them -- cheaper than a pass over the N logits.
 * w8 (nullable; BASELINE config 5 "fp8 MFMA weights", an extension): the weight rows as OCP e4m3 codes [N][K] with one fp32
 * scale per output row (omr_quantize_rows_fp8 of the matrix); the codes are dequantised as they are loaded -- half the weight
 * bytes of a bf16 row, the dominant traffic of a decode position -- the products are summed in fp32 against the same input
 * rows and the row scale multiplies the finished sum.  `w` is then unused.
 * Requires K a multiple of 128 (bf16 / fp8 weights) / 64 (fp32) columns, K <= 2048, 16-byte aligned weight rows. */
typedef struct omr_decode_linear_args {
    int dtype, pro, M, N, K, relu, n0, nsplit, H, hd, vocab, pad_;
    float eps, pad2_;
    const void* x; long ldx; const void* res; long ldres; const float* gamma; const float* beta; void* xn_out;
    const long* tokens; const void* emb; const float* pe_row; const float* part;
    const void* w; const float* bias; void* out0; long ld0; void* out1; long ld1; float* out32; long ld32;
    long* amax_idx; float* amax_val; float* amax_part;
    const unsigned char* w8; const float* w8_scale;
} omr_decode_linear_args;
int omr_decode_linear(const omr_decode_linear_args* args, void* stream);
/* omr_decode_linear for rows that each sit at their OWN position (the linears omr_decode_steps_rows issues; continuous
 * batching has no counterpart in the reference's one-input loop, src/transformer/model.py:171-199): row m is at position
 * row_pos[m] (device int32 [M], must not be NULL).  Prologue 2 then adds the positional row pe_row + row_pos[m] * K, so pe_row
 * is the whole table, and the out1 part of row m (the K|V projection's cache row) lands at
 * out1 + m * ld1 + row_pos[m] * out1_pos_ld.  Everything else as in omr_decode_linear, to the bit.  The contents of row_pos
 * are NOT range-checked here: the caller keeps them inside its table and cache, as omr_decode_steps_rows does by clamping them
 * on the device before its first linear. */
int omr_decode_linear_rows(const omr_decode_linear_args* args, const int* row_pos, long out1_pos_ld, void* stream);
int omr_decode_steps(const omr_decode_desc* desc, long* tokens, int t0, int n_steps, long* out_tokens, float* out_top1, float* last_logits,
                     void* stream);
/* omr_decode_steps over memories of different lengths in one batch (validation at batch size > 1; the reference's greedy loop,
 * src/transformer/model.py:171-199, runs one memory at a time): desc->S is the padded memory length (cross_kv rows past a
 * row's own length are never read) and row b's cross-attention sees mem_len[b] keys (device int32 [B], 1 <= mem_len[b] <=
 * S).  A row with mem_len[b] > 64 gets, token for token, what omr_decode_steps gives for that memory alone. */
int omr_decode_steps_varlen(const omr_decode_desc* desc, const int* mem_len, long* tokens, int t0, int n_steps, long* out_tokens,
                            float* out_top1, float* last_logits, void* stream);
/* omr_decode_steps_varlen for rows that each sit at their OWN position (continuous batching: a row that took <eos> hands its
 * slot to the next input while its neighbours go on; the reference's loop, src/transformer/model.py:171-199, has one input).
 * pos: device int32 [B], row b's position when the call starts; row b runs positions pos[b] .. pos[b] + n_steps - 1: it adds
 * pe[pos[b] + s], writes its K|V into cache row pos[b] + s of its own slot, attends over cache rows [lo_b, pos[b] + s]
 * (omr_attn_fwd_split_rows) and over its mem_len[b] memory keys (mem_len nullable).  Nothing beyond a row's own position or
 * memory length is read: a slot may still hold its previous occupant's cache.  t_max: the largest entry of pos, given by the
 * host; t_max + n_steps > max_len is refused before the first launch (and positions are clamped on the device to the cache).
 * `pos` is read once per call and not advanced.  Everything else as in omr_decode_steps_varlen.  Only descriptors of the row
 * kernel (d in {128, 256, 512}, ff <= 2048) are taken; any other returns OMR_ERR_UNSUPPORTED -- that answer comes before
 * every other argument check, so a caller may ask with NULL pointers. */
int omr_decode_steps_rows(const omr_decode_desc* desc, const int* mem_len, const int* pos, int t_max, long* tokens, int n_steps,
                          long* out_tokens, float* out_top1, float* last_logits, void* stream);
/* Weighted late fusion (src/multimodal/weighted_multimodal/test.py:21-70) without a host round trip per token: positions
 * t0 .. t0+n_steps-1 of TWO models (descriptors with B = 1 and the same vocabulary) in lock-step; per position
 * argmax(alpha * softmax(logits_a) + (1 - alpha) * softmax(logits_b)) (omr_weighted_argmax) is written to out_tokens[s]
 * (and its mixed probability to out_prob[s], nullable) and fed to both models' next position through `tokens` (device,
 * 1 entry: in = the token of position t0).  logits_a / logits_b: fp32 scratch of ldv entries each. */
int omr_weighted_decode_steps(const omr_decode_desc* desc_a, const omr_decode_desc* desc_b, float alpha, long* tokens, int t0, int n_steps,
                              long* out_tokens, float* out_prob, float* logits_a, float* logits_b, void* stream);
/* omr_weighted_decode_steps for B pairs at once (the reference loops over its test set one pair at a time,
 * src/multimodal/weighted_multimodal/test.py:21-70,154-172): desc_a->B == desc_b->B == B >= 1, same V.  mem_len_a / mem_len_b:
 * device int32 [B] as in omr_decode_steps_varlen, or NULL (every row of that model sees its S), independently per model.
 * Per position both models run their step for all rows, then ONE omr_weighted_argmax_rows launch writes out_tokens[s][B],
 * out_prob[s][B] (nullable) and `tokens` (device, B entries: in = the tokens of position t0, out = those of the last
 * position).  logits_a / logits_b: fp32 scratch [B][ldv] of the respective model.  A row whose memories BOTH have more than
 * 64 tokens gets, token for token and probability bit for bit, what omr_weighted_decode_steps gives for that pair alone. */
int omr_weighted_decode_steps_varlen(const omr_decode_desc* desc_a, const int* mem_len_a, const omr_decode_desc* desc_b,
                                     const int* mem_len_b, float alpha, long* tokens, int t0, int n_steps, long* out_tokens,
                                     float* out_prob, float* logits_a, float* logits_b, void* stream);
/* omr_weighted_decode_steps_varlen over rows at their own positions (src/multimodal/weighted_multimodal/test.py:21-70,154-172
 * with continuous batching): ONE pos / t_max for both models -- the two models of a pair are always at the same position --
 * as in omr_decode_steps_rows; `tokens` in = the token each row feeds to its position pos[b]. */
int omr_weighted_decode_steps_rows(const omr_decode_desc* desc_a, const int* mem_len_a, const omr_decode_desc* desc_b, const int* mem_len_b,
                                   const int* pos, int t_max, float alpha, long* tokens, int n_steps, long* out_tokens, float* out_prob,
                                   float* logits_a, float* logits_b, void* stream);

/* ---- batched beam search on the device ------------------------------------------------------------------------------- */
/* Beam search (BASELINE config 5 "beam-search decode"; an extension -- the reference only decodes greedily, model.py:182-193)
 * for N inputs at once without a host round trip between positions.  The yardstick is the host loop of _Base.beam_search
 * (model.py of this package): every input gets exactly its result.  Row r = n * beam + k of the decode descriptor
 * (desc->B == N * beam) is hypothesis k of input n; the rows of an input share its cross-attention K|V (desc->cross_kv holds
 * N slots, cross_bs apart) and its mem_len[n].  Row and parent indices below are LOCAL to the input (0 .. beam-1).
 * State, all device memory, carved out of ONE block `state` of omr_beam_workspace_bytes bytes so that one copy brings the
 * results to the host:
 *   scores      fp64 [rows]   sum of log-probabilities of the hypothesis (-inf: dead row); before position 0: 0, -inf, ...
 *   best_score  fp64 [N]      best finished hypothesis: its score (-inf: none yet), the row it extended (best_row) and the
 *   best_row / best_pos [N]   position at which it took <eos>; its tokens are the history walked back from there, + <eos>
 *   done [N]                  1: the input stopped (no survivor, or its best survivor cannot overtake best_score); frozen
 *   exhausted [N]             1 until the input stops by that rule (it then did not run out of positions)
 *   parents int32 [rows]      the row each row of the NEXT position continues (written by the selection, read by the reorder)
 *   tokens int64 [rows]       the token each row feeds to the next position; before position 0: <sos>
 *   hist_parent / hist_token int32 [max_len][rows]   (parent, token) of every row at every position run
 * Scores are fp64 because the host route adds Python floats to the fp32 log-probabilities it reads back.
 * self_kv2: a second self-attention cache, the size of desc->self_kv; position t lives in desc->self_kv for even t and in
 * self_kv2 for odd t (a run starts at position 0).  last_logits (nullable): fp32 [rows][ldv] logits of the last position run. */
#define OMR_MAX_BEAM 8
typedef struct omr_beam_desc {
    int beam, N, eos, max_len;
    void* state; long state_bytes;
    double* scores; double* best_score; long* tokens; int* best_row; int* best_pos; int* done; int* exhausted; int* parents;
    int* hist_parent; int* hist_token;
    void* self_kv2; float* last_logits;
} omr_beam_desc;
/* Bytes of the state block for desc->{beam, N, max_len}; also points the ten state fields into desc->state (NULL: offsets). */
long omr_beam_workspace_bytes(omr_beam_desc* desc);
/* The selection of ONE position `t` for all inputs in one launch (the loop body of _Base.beam_search, model.py of this package):
 * per row the `beam` largest log_softmax values of logits [rows][ld] (omr_topk_logprob's arithmetic and tie rule); candidates
 * scores[parent] + value in fp64 from live rows, ordered by (score descending, parent ascending, token ascending); walked in
 * that order: the first `beam` non-<eos> candidates survive, an <eos> candidate before the beam-th survivor replaces the best
 * finished record if its score is strictly greater; the input stops when nothing survives or its best survivor's score is
 * <= the best finished one, else parents / tokens / scores / history row t are written (padded with dead copies of the first
 * survivor).  Inputs already done are not touched. */
int omr_beam_select(const float* logits, long ld, int V, const omr_beam_desc* beam_desc, int t, void* stream);
/* Positions t0 .. t0+n_steps-1 for all rows from one host call: per position the decode step without a pick
 * (omr_decode_steps' position, fp32 logits), omr_beam_select, and one launch that moves the still readable cache positions
 * [max(0, t+1-window), t] of every layer and row from its parent's row into the other cache buffer.  mem_len (nullable): device
 * int32 [N] as in omr_decode_steps_varlen.  Refused before the first launch: beam outside 1..OMR_MAX_BEAM, desc->B != N * beam,
 * t0 + n_steps > max_len. */
int omr_beam_decode_steps(const omr_decode_desc* desc, const omr_beam_desc* beam_desc, const int* mem_len, int t0, int n_steps, void* stream);

/* ---- beam search over the weighted late fusion ------------------------------------------------------------------------ */
/* The k best tokens of one decoding step of the weighted late fusion (src/multimodal/weighted_multimodal/test.py:50-61; an
 * extension: the reference decodes greedily, k = 1).  Per row pair r of logits_a [rows][lda] / logits_b [rows][ldb] (fp32, n
 * entries read): p[i] = alpha * softmax(a)[i] + (1 - alpha) * softmax(b)[i] in omr_weighted_argmax_rows' arithmetic (the
 * same maxima, sums and weight roundings; two rounded products and one add); idx_out [rows][k] are the indices of the k
 * largest p, ordered by p descending, then index ascending; val_out [rows][k] = logf(p) in fp32 (-inf where p underflowed to
 * 0).  k = 1 gives omr_weighted_argmax_rows' index, ties included.  One workgroup per row; a row's result does not depend on
 * `rows`.  Refused: rows < 1, k outside 1..OMR_MAX_BEAM, n < k, lda < n, ldb < n. */
int omr_weighted_topk_logprob(const float* logits_a, long lda, const float* logits_b, long ldb, int rows, int n, float alpha, int k,
                              long* idx_out, float* val_out, void* stream);
/* omr_beam_select for the weighted late fusion (weighted_multimodal/test.py:50-61; an extension: the reference decodes
 * greedily): the candidates of row r are omr_weighted_topk_logprob's `beam` (index, logf(p)) of rows r of logits_a / logits_b
 * [N * beam][ld] -- ranked by p descending, then index ascending -- and everything after that (fp64 scores, order, finished
 * record, stop rule, padding) is omr_beam_select's, by the same code.  A candidate of value -inf gets no special case. */
int omr_weighted_beam_select(const float* logits_a, long lda, const float* logits_b, long ldb, int V, float alpha,
                             const omr_beam_desc* beam_desc, int t, void* stream);
/* omr_beam_decode_steps for the weighted late fusion (weighted_multimodal/test.py:21-70; an extension: the reference decodes
 * greedily): ONE search state drives two models.  Per position: model A's step, model B's step (no pick; both read
 * beam_desc->tokens, the hypotheses of an input share its cross-attention K|V slot in either model), one
 * omr_weighted_beam_select launch over the two models' fp32 logits (candidates: the `beam` largest
 * alpha * softmax(a) + (1 - alpha) * softmax(b) per row, p descending then index ascending, value logf(p)), then the cache
 * reorder once per model with that model's own L, d, dtype and window.  beam_desc->self_kv2 is model A's second cache,
 * self_kv2_b model B's; both models' caches alternate by the parity of the position.  beam_desc->last_logits (nullable) gets
 * model A's logits of the last position.  mem_len_a / mem_len_b: device int32 [N] of that model.  Refused before the first
 * launch: desc_a->V != desc_b->V, desc_x->B != N * beam, beam outside 1..OMR_MAX_BEAM, t0 + n_steps greater than either
 * model's max_len or beam_desc->max_len, a cache that is not 16-byte aligned. */
int omr_weighted_beam_decode_steps(const omr_decode_desc* desc_a, const int* mem_len_a, const omr_decode_desc* desc_b, const int* mem_len_b,
                                   const omr_beam_desc* beam_desc, void* self_kv2_b, float alpha, int t0, int n_steps, void* stream);

/* ---- speculative greedy decoding ----------------------------------------------------------------------------------------- */
/* An extension of the greedy loop of Transformer.validation_step / get_pred_seq_and_pred_prob_seq (src/transformer/model.py:171-199,
 * 226-262), which runs one position per pass: a cheap DRAFT model with the same vocabulary proposes k tokens, ONE pass of the
 * target model runs the R = k + 1 positions they would occupy, and the longest prefix of proposals the target itself would have
 * picked is kept.  Tokens and top-1 values are those of the one-position loop, to the bit.
 *
 * A GROUPED position: rows = B * R, row m is position pos[m / R] + m % R of slot m / R (desc->B = B slots: the caches hold B
 * slots, the scratch B * R rows).  Row path only (omr_decode_steps_rows' descriptors; any other: OMR_ERR_UNSUPPORTED before any
 * pointer is read).  Per layer the q|k|v linear of all rows writes row m's K|V into cache row pos + m % R of slot m / R and
 * completes before the attention launch, in which row m attends over cache rows [lo_m, pos + m % R] of its slot -- those of the
 * rows before it in its group included -- and over the slot's memory keys.  Nothing past a row's own position is read. */
#define OMR_MAX_VERIFY_ROWS 32
/* Bytes of scratch a grouped position of R rows per slot wants (2 <= R <= OMR_MAX_VERIFY_ROWS; desc->ws is not looked at). */
long omr_decode_group_workspace_bytes(const omr_decode_desc* desc, int R);
/* R consecutive positions of every slot in one pass (the loop body of model.py:182-193,247-260, R times).  pos: device int32 [B];
 * t_max: its largest entry, given by the host.  tokens: device int64 [B][R], column 0 the token slot b feeds to pos[b], columns
 * 1..R-1 the proposed continuations.  out_tokens [B][R] / out_top1 [B][R] (nullable): the greedy pick of every row and its fp32
 * logit -- out_tokens[b][r] is what omr_decode_steps_rows picks at position pos[b] + r after the prefix tokens[b][0..r].  ws /
 * ws_bytes: omr_decode_group_workspace_bytes(desc, R) bytes of device scratch (desc->ws is not used).  Nothing is advanced;
 * self_kv rows pos[b] .. pos[b] + R - 1 of every slot are overwritten.  Refused before the first launch: R outside
 * 2..OMR_MAX_VERIFY_ROWS, t_max < 0, t_max + R > max_len, a NULL pos / tokens / out_tokens / ws, too small a ws, and (with
 * OMR_ERR_UNSUPPORTED) desc->S <= 64 -- the rows of a slot share its memory K|V, which only the key-split kernel does; on the device
 * positions are clamped into the cache as in omr_decode_steps_rows. */
int omr_decode_verify_rows(const omr_decode_desc* desc, const int* mem_len, const int* pos, int t_max, int R, const long* tokens,
                           long* out_tokens, float* out_top1, void* ws, long ws_bytes, void* stream);
/* The state of a speculative decode of B slots with k proposals per cycle, all device memory carved out of ONE block `state` of
 * omr_spec_workspace_bytes bytes, so that one copy brings the results to the host (the pattern of omr_beam_desc):
 *   pos int32 [B]          the next position of each slot = the tokens it has produced (>= 1: position 0 is run by the caller)
 *   out_len int32 [B]      tokens in the slot's output run
 *   done int32 [B]         1: the slot took <eos> or filled its run; frozen from then on
 *   accepted int32 [B]     j of the last cycle
 *   totals int64 [2]       proposals made / proposals accepted, over all cycles and live slots
 *   first / prev int64 [B] the token the slot feeds to pos[b] / fed to pos[b] - 1
 *   tokens / picks int64 [B][k+1], top1 fp32 [B][k+1]      omr_decode_verify_rows' tokens, out_tokens and out_top1
 *   dpicks int64 [k+1][B]  the draft's picks of the cycle
 *   out_tokens int64 [B][max_out], out_top1 fp32 [B][max_out]      the output runs
 * ws_t / ws_t_bytes: omr_decode_group_workspace_bytes(target, k + 1) bytes of scratch, not part of the block.  t_max: the host's
 * upper bound of pos[] when omr_spec_decode_cycles is called. */
typedef struct omr_spec_desc {
    int B, k, eos, max_out, t_max, pad_;
    void* state; long state_bytes;
    int* pos; int* out_len; int* done; int* accepted; long* totals; long* first; long* prev;
    long* tokens; long* picks; float* top1; long* dpicks; long* out_tokens; float* out_top1;
    void* ws_t; long ws_t_bytes;
} omr_spec_desc;
/* Bytes of the state block for desc->{B, k, max_out}; also points the thirteen state fields into desc->state (NULL: offsets). */
long omr_spec_workspace_bytes(omr_spec_desc* desc);
/* The acceptance of ONE cycle for all slots in one launch (no counterpart in the reference's loop, model.py:182-193, which keeps
 * every token it computes): per live slot j = the number of leading proposals with tokens[b][i] == picks[b][i - 1]; picks[b][0..j]
 * and their top-1 values are appended to the slot's run, cut after the first <eos> and at max_out (either sets done); pos[b] and
 * out_len[b] grow by the tokens appended, first[b] becomes the last of them and prev[b] the one before it; accepted[b] = j, and
 * totals grow by (k, j).  Plain loads and stores, one workgroup, no atomics. */
int omr_spec_accept(const omr_spec_desc* spec, void* stream);
/* n_cycles cycles without a host round trip (an extension of model.py:171-199; all positions come from spec->pos).  Per cycle: the
 * DRAFT runs k + 1 single positions pos - 1 .. pos + k - 1 of every slot through omr_decode_steps_rows' path on its own caches --
 * the first one feeds prev[b] and closes the gap a fully accepted cycle leaves (its last proposal was never consumed), the
 * second feeds first[b], the others the draft's own previous pick --, one launch builds tokens[B][k+1], the TARGET runs
 * omr_decode_verify_rows, then omr_spec_accept.  Both descriptors: B slots, the same V, the row path.  Refused before the first
 * launch: k outside 1..OMR_MAX_VERIFY_ROWS - 1, n_cycles < 1, spec->t_max < 1, spec->t_max + n_cycles * (k + 1) beyond either
 * model's max_len, NULL state fields, too small a block or ws_t, and (OMR_ERR_UNSUPPORTED) target->S <= 64, or draft->S <= 64 with
 * mem_len_d. */
int omr_spec_decode_cycles(const omr_decode_desc* target, const omr_decode_desc* draft, const int* mem_len_t, const int* mem_len_d,
                           const omr_spec_desc* spec, int k, int n_cycles, void* stream);

/* ---- grammar-constrained decoding -------------------------------------------------------------------------------------- */
/* An extension: the reference picks over the whole vocabulary at every position (argmax in Transformer.validation_step,
 * src/transformer/model.py:182-193; the mixed argmax of src/multimodal/weighted_multimodal/test.py:50-61), so nothing keeps a
 * transcript inside the token stream src/data/encoding.py `encode` produces.  Here a deterministic automaton over token ids
 * (grammar.py of this package), compressed by token class, restricts every pick and every beam candidate ON THE DEVICE:
 *   cls    uint8 [V]      class of every vocabulary entry, < C
 *   next   int32 [S][C]   next[s][c] = the state after a token of class c in state s, or -1: forbidden there
 *   state  int32 [rows]   each row's current state, advanced by the kernels below (rows = B; N * beam for a beam search)
 * All three are device memory.  A forbidden token's logit is read as -inf BEFORE any comparison or expf (NaN / +inf there cannot
 * reach a maximum, a sum or a pick), so log-probabilities are renormalised over the allowed tokens.  The host builder
 * guarantees that every reachable state allows a token and that state values stay inside [0, S); the kernels clamp a state into
 * that range and never write a value outside it.  Every entry below refuses (OMR_ERR_ARG) a NULL descriptor, a NULL cls / next /
 * state, C outside 1..OMR_GRAMMAR_MAX_CLASSES and S < 1. */
#define OMR_GRAMMAR_MAX_CLASSES 256
typedef struct omr_grammar_desc {
    const unsigned char* cls; const int* next; int S, C; int* state;
} omr_grammar_desc;
/* omr_argmax (model.py:187,253) over the allowed tokens of each row's state: idx_out[r] = first index of the largest allowed
 * logit of logits [rows][ld] (n entries read), val_out[r] (nullable) that logit, tokens_out[r] (nullable) a second copy of
 * the index, and state[r] <- next[state[r]][cls[idx]].  Equal, bit for bit, to omr_argmax on logits the host masked with -inf. */
int omr_grammar_pick(const float* logits, long ld, int rows, int n, const omr_grammar_desc* grammar, long* idx_out, float* val_out,
                     long* tokens_out, void* stream);
/* omr_weighted_argmax_rows (weighted_multimodal/test.py:50-61) the same way: both logit rows are masked before their softmax
 * statistics; ONE state per row drives both models. */
int omr_weighted_grammar_pick(const float* logits_a, long lda, const float* logits_b, long ldb, int rows, int n, float alpha,
                              const omr_grammar_desc* grammar, long* idx_out, float* prob_out, long* tokens_out, void* stream);
/* omr_beam_select (the loop body of _Base.beam_search, model.py of this package) under the automaton; state: int32 [N * beam].
 * Phase 1 ranks log_softmax over the allowed tokens of each row's state.  Phase 2: a candidate (parent, token) is live only if
 * its parent is live AND next[state[parent]][cls[token]] >= 0 -- decided by the table, not by the value, so a forbidden token
 * never becomes a survivor, a finished hypothesis or a history entry, also where fewer than `beam` tokens are allowed.  The
 * input's `beam` old states are read before anything is written; survivor slot i gets next[old_state[parent_i]][cls[token_i]],
 * dead padding rows the first survivor's.  The states of inputs that are done (before or by this launch) are left alone. */
int omr_beam_select_grammar(const float* logits, long ld, int V, const omr_beam_desc* beam_desc, const omr_grammar_desc* grammar, int t,
                            void* stream);
/* omr_weighted_beam_select the same way (both rows masked before the mix's statistics). */
int omr_weighted_beam_select_grammar(const float* logits_a, long lda, const float* logits_b, long ldb, int V, float alpha,
                                     const omr_beam_desc* beam_desc, const omr_grammar_desc* grammar, int t, void* stream);
/* omr_decode_steps (model.py:182-193) with the constrained pick, as do the two entries after it: per position the head runs without its fused
 * pick and ONE omr_grammar_pick launch over the position's fp32 logits stands where the unconstrained pick's reduction (row
 * kernel) or omr_argmax (generic widths) stood -- the launches per position are the unconstrained count.  grammar->state (B
 * entries) advances across all n_steps without the host; out_top1 is the top-1 ALLOWED logit.  out_tokens must not be NULL. */
int omr_decode_steps_grammar(const omr_decode_desc* desc, const omr_grammar_desc* grammar, long* tokens, int t0, int n_steps, long* out_tokens,
                             float* out_top1, float* last_logits, void* stream);
/* omr_decode_steps_varlen (ragged memories; the loop of model.py:171-199 at batch size > 1) with the constrained pick; mem_len must
 * not be NULL. */
int omr_decode_steps_varlen_grammar(const omr_decode_desc* desc, const int* mem_len, const omr_grammar_desc* grammar, long* tokens, int t0,
                                    int n_steps, long* out_tokens, float* out_top1, float* last_logits, void* stream);
/* omr_decode_steps_rows (rows at their own positions: continuous batching of the loop of model.py:171-199) with the constrained
 * pick.  The host puts a refilled row's state to the start state, where it sets its token.  OMR_ERR_UNSUPPORTED (widths the
 * row kernel does not take) is answered before the descriptor is looked at, as in omr_decode_steps_rows. */
int omr_decode_steps_rows_grammar(const omr_decode_desc* desc, const int* mem_len, const int* pos, int t_max, const omr_grammar_desc* grammar,
                                  long* tokens, int n_steps, long* out_tokens, float* out_top1, float* last_logits, void* stream);
/* omr_weighted_decode_steps_varlen (weighted_multimodal/test.py:21-70 for B pairs) with omr_weighted_grammar_pick in place of
 * omr_weighted_argmax_rows: same launches per position; grammar->state holds B entries. */
int omr_weighted_decode_steps_varlen_grammar(const omr_decode_desc* desc_a, const int* mem_len_a, const omr_decode_desc* desc_b,
                                             const int* mem_len_b, const omr_grammar_desc* grammar, float alpha, long* tokens, int t0, int n_steps,
                                             long* out_tokens, float* out_prob, float* logits_a, float* logits_b, void* stream);
/* omr_weighted_decode_steps_rows (weighted_multimodal/test.py:21-70,154-172 with continuous batching) with
 * omr_weighted_grammar_pick; one pos / t_max and one state per row for both models. */
int omr_weighted_decode_steps_rows_grammar(const omr_decode_desc* desc_a, const int* mem_len_a, const omr_decode_desc* desc_b,
                                           const int* mem_len_b, const int* pos, int t_max, const omr_grammar_desc* grammar, float alpha,
                                           long* tokens, int n_steps, long* out_tokens, float* out_prob, float* logits_a, float* logits_b,
                                           void* stream);
/* omr_beam_decode_steps (an extension of the greedy loop of model.py:182-193) with omr_beam_select_grammar as the selection;
 * grammar->state: int32 [N * beam], every entry the start state before position 0. */
int omr_beam_decode_steps_grammar(const omr_decode_desc* desc, const omr_beam_desc* beam_desc, const int* mem_len,
                                  const omr_grammar_desc* grammar, int t0, int n_steps, void* stream);
/* omr_weighted_beam_decode_steps (an extension of weighted_multimodal/test.py:21-70) with omr_weighted_beam_select_grammar; one
 * state per row drives both models. */
int omr_weighted_beam_decode_steps_grammar(const omr_decode_desc* desc_a, const int* mem_len_a, const omr_decode_desc* desc_b,
                                           const int* mem_len_b, const omr_beam_desc* beam_desc, void* self_kv2_b,
                                           const omr_grammar_desc* grammar, float alpha, int t0, int n_steps, void* stream);

/* ---- loss ------------------------------------------------------------------------------------------------ */
/* CrossEntropyLoss(ignore_index=pad) (model.py:109,166) on row-major logits [M][ldv]; acc2 = {sum, count} (fp64). */
int omr_ce_fwd(int dtype, const void* logits, const long* target, float* lse, double* acc2, float* loss_out, long M, int V, long ldv,
               int pad_idx, void* stream);
/* grad_out (nullable): device pointer to the upstream scalar gradient dL/dloss (multiplies grad_scale). */
int omr_ce_bwd(int dtype, const void* logits, const long* target, const float* lse, const double* acc2, void* dlogits, long M, int V,
               long ldv, int pad_idx, float grad_scale, const float* grad_out, void* stream);
/* The same loss (model.py:109,166) with torch's label_smoothing = eps in [0, 1] (an extension: the reference trains with 0).  A row is
 * live when its target is not pad and lies in [0, V).  Per live row, with S = sum of the row's logits over the columns < V:
 *   objective = lse - (1 - eps) * logit[target] - (eps / V) * S,      nll = lse - logit[target].
 * loss_out = mean objective, nll_out = mean nll (both fp32 [1]), acc3 = {objective sum, live rows, nll sum} (fp64), rowsum = S (fp32 [M],
 * summed in a fixed order in the pass that computes lse).  A live row that holds -inf has objective +inf, as in torch.
 * eps == 0 runs the kernels of omr_ce_fwd: loss_out, lse and acc3[0..1] have its bits, nll_out = loss_out, rowsum is not written (may be
 * NULL).  eps outside [0, 1] (NaN included): OMR_ERR_ARG before any launch. */
int omr_ce_smooth_fwd(int dtype, const void* logits, const long* target, float* lse, float* rowsum, double* acc3, float* loss_out,
                      float* nll_out, long M, int V, long ldv, int pad_idx, float eps, void* stream);
/* dlogits = (softmax - (1 - eps) * onehot - eps / V) * grad_scale * grad_out / acc3[1] on live rows, +0 on the others and in the columns
 * >= V (model.py:109,166).  eps == 0 runs the kernel of omr_ce_bwd.  acc3: only the live-row count acc3[1] is read. */
int omr_ce_smooth_bwd(int dtype, const void* logits, const long* target, const float* lse, const double* acc3, void* dlogits, long M, int V,
                      long ldv, int pad_idx, float eps, float grad_scale, const float* grad_out, void* stream);

/* Knowledge distillation (an extension: the reference trains from hard labels alone): the loss above on student logits [M][ldv] plus the
 * KL divergence to one or two teachers' logits [M][ldt] (teacher_b nullable; both of dtype tdtype, which may differ from the student's), at
 * temperature tau > 0, distillation weight lam in [0, 1] and teacher mix alpha in [0, 1] (alpha on teacher_a; without teacher_b alpha must be 1).
 * Per live row over the columns < V:  q = alpha softmax(a / tau) + (1 - alpha) softmax(b / tau),  pt = softmax(x / tau),
 *   nll = lse - logit[target],   kd = tau^2 sum_v q_v (log q_v - log pt_v)  (terms with q_v = 0 are 0),   objective = (1 - lam) nll + lam kd.
 * lse4 = fp32 [4][M]: lse(x), lse(x / tau), lse(a / tau), lse(b / tau) (zeros on ignored rows and for an absent teacher_b); rowkd = fp32 [M];
 * acc4 = {objective sum, live rows, nll sum, kd sum} (fp64); means3 = {loss, nll, kd} (fp32).  No atomics: two calls give the same bits.
 * lam == 0 runs the kernels of omr_ce_fwd and never reads the teachers: means3[0], lse4[0][.] and acc4[0..1] have its bits, rowkd and
 * lse4[1..3] are not written.  OMR_ERR_ARG before any launch: tau <= 0 or not finite, lam or alpha outside [0, 1] (NaN included),
 * teacher_b == NULL with alpha != 1, ldt < V, ldv < V. */
int omr_ce_distill_fwd(int dtype, const void* logits, long ldv, int tdtype, const void* teacher_a, const void* teacher_b, long ldt,
                       const long* target, float* lse4, float* rowkd, double* acc4, float* means3, long M, int V, int pad_idx, float alpha,
                       float tau, float lam, void* stream);
/* dlogits = ((1 - lam) (softmax(x) - onehot) + lam tau (pt - q)) * grad_scale * grad_out / acc4[1] on live rows, +0 on the others and in the
 * columns >= V; the teachers get no gradient.  lam == 0 runs the kernel of omr_ce_bwd.  The same refusals as the forward. */
int omr_ce_distill_bwd(int dtype, const void* logits, long ldv, int tdtype, const void* teacher_a, const void* teacher_b, long ldt,
                       const long* target, const float* lse4, const double* acc4, void* dlogits, long M, int V, int pad_idx, float alpha,
                       float tau, float lam, float grad_scale, const float* grad_out, void* stream);

/* ---- CTC auxiliary head (csrc/ctc.hip; an extension: joint CTC / attention training, and a transcript from the encoder alone) ---- */
/* Memory -> time-ordered frames.  mem [B][S][d] holds sample b's own gh_b x gw_b feature grid row-major with pitch gw_b (cell (i, j) is
 * row i * gw_b + j), zeros behind: the packed memory of the ragged route with grid = int32 [B][2] = (gh_b, gw_b) on the device, or the dense
 * memory with grid == NULL, where every sample has the grid gh x gw (gh * gw <= S).  frames [B][Fmax][d]:
 *   G_b = ceil(gh_b / pool),  F_b = G_b * gw_b,  frame f = j * G_b + q  (column j, left to right; group q, top to bottom inside the column)
 *   frames[b][f][c] = (((x_r0 + x_r0+1) + x_r0+2) + ... + x_r1-1) / (float)(r1 - r0)     x_i = (float)mem[b][i * gw_b + j][c],
 *   r0 = q * pool, r1 = min(r0 + pool, gh_b): fp32 additions top to bottom, ONE IEEE fp32 division by the count, one rounding to dtype.
 *   A group of one row (always so with pool = 1) is a copy of the input's bits.  Rows f >= F_b are +0.  frame_len[b] = F_b (int32 [B]).
 * A sample whose grid is not positive, does not fit S, or has F_b > Fmax counts as empty: F_b = 0.
 * _bwd is the adjoint: dmem[b][i * gw_b + j][c] = dframes[b][f][c] / (float)count of the frame f that row i of column j went into (a copy
 * where count = 1), rounded once to dtype; rows outside the grid are +0.
 * OMR_ERR_ARG before any launch: a NULL mem / frames / frame_len, B < 1 or > 65535, S, d, pool or Fmax < 1, grid == NULL with gh or gw < 1 or
 * gh * gw > S. */
int omr_ctc_frames_fwd(int dtype, const void* mem, const int* grid, void* frames, int* frame_len, int B, int S, int d, int gh, int gw,
                       int pool, int Fmax, void* stream);
int omr_ctc_frames_bwd(int dtype, const void* dframes, const int* grid, void* dmem, int B, int S, int d, int gh, int gw, int pool, int Fmax,
                       void* stream);
/* bytes of the workspace of omr_ctc_fwd / omr_ctc_bwd (16-byte aligned): the frames' log-sum-exp, the stored log alpha / log beta
 * [2][B][Fmax][2 Tmax + 2] fp32, their fp64 offsets [2][B][Fmax], log P [2][B], and the per-sample label tables.  -1 for sizes the entries refuse. */
long omr_ctc_workspace_bytes(int B, int Fmax, int Tmax, int V);
/* F.ctc_loss(log_softmax(logits), targets, frame_len, L, blank=blank_idx, reduction="mean", zero_infinity=True) on logits [B][Fmax][ldv >= V]
 * (fp32 or bf16), frame_len int32 [B] (clamped into [0, Fmax]), targets int64 [B][T].  Sample b's label sequence is the prefix of
 * targets[b] before the first element that equals blank_idx or eos_idx (or lies outside [0, V)); its length L_b is found on the device.
 *   rows[b] = -log P_b (fp32; 0 where infeasible),  loss = (1 / B) sum_b rows_b / max(L_b, 1),  acc2 = {that sum, B} (fp64),
 *   infeasible[0] = the number of samples with P_b = 0 (F_b < L_b + repeats_b, F_b = 0, or -inf logits): they add 0 and get +0 gradients.
 * log alpha and log beta are kept relative to an fp64 offset that is advanced every 8 frames, so their precision does not fall with
 * Fmax; log P, the division and the mean are one fp64 fixed-order pass.  No atomics on floats: two calls give the same bits.
 * ws: omr_ctc_workspace_bytes(B, Fmax, T, V) bytes, handed unchanged to omr_ctc_bwd.
 * OMR_ERR_ARG before any launch: a NULL pointer, B < 1 or > 32767, Fmax < 1, T < 1 or > 1023, V < 1, ldv < V, blank_idx outside [0, V),
 * eos_idx outside [-1, V) (-1: no such token). */
int omr_ctc_fwd(int dtype, const void* logits, long ldv, const int* frame_len, const long* targets, void* ws, double* acc2, float* loss,
                float* rows, int* infeasible, int B, int Fmax, int T, int V, int blank_idx, int eos_idx, void* stream);
/* dlogits[b][f][v] = s_b (softmax(logits[b][f])[v] - post[b][f][v]), s_b = grad_scale * grad_out / (B max(L_b, 1)), post = the sum over the
 * lattice states that carry label v of exp(log alpha + log beta - log P - emission), summed in state order; written in the logits' dtype.
 * +0: the columns [V, ldv), the frames >= F_b, every frame of an infeasible sample.  The same refusals as the forward. */
int omr_ctc_bwd(int dtype, const void* logits, long ldv, const int* frame_len, const long* targets, const void* ws, void* dlogits, int B,
                int Fmax, int T, int V, int blank_idx, float grad_scale, const float* grad_out, void* stream);
/* The encoder-only transcript.  frame_arg / frame_val [B][Fmax]: each frame's arg-max column (ties to the lowest index) and its value as
 * fp32 (frames >= F_b: blank_idx and 0).  tokens int32 [B][Fmax]: the arg-max path with repeats collapsed and blanks dropped, blank_idx
 * behind; lengths int32 [B].  The same refusals as omr_ctc_fwd (no T). */
int omr_ctc_greedy(int dtype, const void* logits, long ldv, const int* frame_len, int* frame_arg, float* frame_val, int* tokens, int* lengths,
                   int B, int Fmax, int V, int blank_idx, void* stream);

/* ---- joint CTC / attention beam search (csrc/ctc_prefix.hip; an extension: Watanabe et al.'s decoding half of the CTC head) ---- */
/* The CTC prefix score.  Per input n with F_n frames (frame_len[n] clamped into [0, Fmax]), y_f(v) = (float)logits[n][f][v] - lse[n][f] (fp32,
 * one subtraction; lse from the row pass of omr_ctc_fwd, run once by omr_ctc_prefix_init).  A hypothesis g (the tokens behind <sos>) of row
 * r = n * beam + k holds two fp32 log-space rows of F_n entries and two scalars:
 *   gn[f] / gb[f]   log P(frames 0..f emit exactly g, the last frame a label / a blank);  empty g: gn = -inf, gb[f] = y_0(blank) + .. + y_f(blank)
 *   logpsi          log P(the frames emit something that starts with g): 0 for the empty g;     last: g's last token (sos: g is empty)
 * A label c (not blank, sos, eos; 0 <= c < V) extends g to h = g c -- log-add la(a, b) = max + log1pf(expf(min - max)), -inf for two -inf:
 *   phi[f]  = la(gb^g[f], c == last(g) ? -inf : gn^g[f]),   phi[-1] = g empty ? 0 : -inf
 *   gn^h[f] = la(gn^h[f-1], phi[f-1]) + y_f(c),   gb^h[f] = la(gb^h[f-1], gn^h[f-1]) + y_f(blank),   gn^h[-1] = gb^h[-1] = -inf
 *   logpsi(h) = log sum_f exp(phi[f-1] + y_f(c)), summed 8 frames at a time in frame order around a running maximum (m, s):
 *               cm = max(m, the 8 terms); s = s * expf(m - cm) + expf(term_0 - cm) + .. + expf(term_7 - cm); m = cm; logpsi = m + logf(s)
 * c == eos: logpsi = la(gn^g[F-1], gb^g[F-1]) (F_n = 0: 0 for the empty g, else -inf).  Any other c (blank, sos, outside [0, V)): -inf.
 *   delta(g, c) = logpsi(g c) == -inf ? -inf : min(logpsi(g c) - logpsi(g), 0)
 * Plain fp32 log space, every operation rounded on its own (the file is built without contraction); the score, the advance and the selection
 * run ONE row body, so a survivor's stored logpsi has the bits its candidate's had, and the batched and the per-input route agree to the bit.
 * No atomics: two runs give the same bits.
 * omr_ctc_beam_desc: N inputs x beam rows.  logits [N][Fmax][ldv >= V] (dtype fp32 / bf16), frame_len int32 [N], lambda the CTC weight.
 * Everything from `ws` on is carved out of ONE block `ws` of omr_ctc_beam_workspace_bytes bytes:
 *   lse fp32 [N][Fmax];  state[p] fp32 [rows][2][Fmax] (gn row, gb row) for the two parities p;  last[p] int32 [rows];  logpsi fp32 [rows];
 *   cand_tok int64 / cand_val fp32 [N][beam * beam]: scratch of omr_beam_select_ctc (each row's top-`beam` tokens, their mixed values);
 *   advanced int32 [N]: the omr_ctc_prefix_advance launches that took input n since omr_ctc_prefix_init.  In a search that is the position at
 *   which the input stopped; the host needs it where an input stops with nothing finished (every candidate at -inf: no label fits the frames
 *   left and <eos> is not among the attention's candidates) -- its result is then row 0 of the last position it survived.
 * Position t reads parity t & 1 and omr_ctc_prefix_advance writes the other one. */
typedef struct omr_ctc_beam_desc {
    int dtype, N, beam, V, Fmax, blank, sos, eos;
    long ldv;
    float lambda;
    const void* logits; const int* frame_len;
    void* ws; long ws_bytes;
    float* lse; float* state[2]; int* last[2]; float* logpsi; long* cand_tok; float* cand_val; int* advanced;
} omr_ctc_beam_desc;
/* Bytes of the block for desc->{N, beam, Fmax}; also points the fields behind ws_bytes into desc->ws (NULL: offsets).  OMR_ERR_ARG: N or
 * Fmax < 1, beam outside 1..OMR_MAX_BEAM. */
long omr_ctc_beam_workspace_bytes(omr_ctc_beam_desc* desc);
/* Once per search, before position 0: the frames' lse, then every row's parity-0 state = the empty hypothesis (gb by fp32 additions in frame
 * order, logpsi = 0, last = sos).  Refused with OMR_ERR_ARG before the first launch, like every entry below that takes the descriptor: a NULL
 * pointer, fields that are not the ones omr_ctc_beam_workspace_bytes set, lambda outside (0, 1), beam outside 1..OMR_MAX_BEAM, V < 1, ldv < V,
 * blank / sos / eos outside [0, V) or two of them equal; OMR_ERR_UNSUPPORTED: a dtype other than fp32 / bf16. */
int omr_ctc_prefix_init(const omr_ctc_beam_desc* desc, void* stream);
/* delta[r][j] (fp32 [rows][beam]) of candidate cand[r][j] (int64 [rows][beam]) against the hypothesis of row r in the parity `parity` state.
 * One workgroup per input, one candidate per lane of the scanning wave; nothing is written but delta.  Also refused: parity outside {0, 1}. */
int omr_ctc_prefix_scores(const omr_ctc_beam_desc* desc, int parity, const long* cand, float* delta, void* stream);
/* New row i of input n continues row parents[n * beam + i] (int32, LOCAL, clamped into 0..beam-1) of the parity `parity` state by the label
 * tokens[n * beam + i] (int64): its gn / gb rows, logpsi and last go into the OTHER parity (logpsi is shared: the advance does not read it).
 * scores (nullable, fp64 [rows]): rows of -inf (the dead padding of a selection) are skipped; done (nullable, int32 [N]): inputs that are done
 * are skipped.  A token that is no label leaves its row untouched.  The row body is the score's, with stores. */
int omr_ctc_prefix_advance(const omr_ctc_beam_desc* desc, int parity, const int* parents, const long* tokens, const double* scores,
                           const int* done, void* stream);
/* omr_beam_select with the CTC prefix score (the loop body of _Base.beam_search with ctc_decode, model.py of this package), three launches:
 * (1) phase 1 of omr_beam_select: each live input's beam * beam candidates (token, fp32 log-softmax value) -> cand_tok / cand_val;
 * (2) the score kernel over the parity t & 1 state: cand_val = fl(fl(wa * value) + fl(wc * delta)), wc = lambda, wa = (float)(1 - (double)lambda);
 * (3) omr_beam_select's phase 2 on those values, by the same code: fp64 scores, order, walk, finished record, stop rule, padding.
 * The CTC re-ranks inside the attention's candidate list; it does not widen it.  The state is not advanced (omr_ctc_prefix_advance).
 * Also refused: V != ctc->V, N or beam differing between the descriptors, eos differing. */
int omr_beam_select_ctc(const float* logits, long ld, int V, const omr_beam_desc* beam_desc, const omr_ctc_beam_desc* ctc, int t, void* stream);
/* omr_beam_decode_steps with omr_beam_select_ctc as the selection and, behind it, omr_ctc_prefix_advance over beam_desc's parents / tokens /
 * scores / done; then the cache reorder.  A run starts at position 0 behind omr_ctc_prefix_init.  Also refused: desc->V != ctc->V. */
int omr_beam_decode_steps_ctc(const omr_decode_desc* desc, const omr_beam_desc* beam_desc, const omr_ctc_beam_desc* ctc, const int* mem_len,
                              int t0, int n_steps, void* stream);

/* ---- guarded optimizer step ------------------------------------------------------------------------------- */
/* What the reference gets from Lightning: Trainer(precision="16-mixed") (src/train.py:153) puts every step behind GradScaler,
 * which skips optimizer.step() when a gradient holds inf / NaN (torch/amp/grad_scaler.py, _maybe_opt_step), and
 * Trainer(gradient_clip_val=..) clips by the global norm (torch.nn.utils.clip_grad_norm_).  Here the norm, the clip factor and the
 * apply / skip decision are computed ON THE DEVICE into one small record that the guarded Adam launch reads: the host never waits
 * for them (it reads a copy of the record one step late).
 *
 * omr_step_ctl: the record, device resident, 152 bytes.
 *   sumsq            sum of g[i]^2 over all ranges (UNscaled gradient), fp64
 *   norm             (float)(sqrt(sumsq) * grad_scale): the global L2 norm of the gradient the update would see
 *   clip             1.0f when max_norm <= 0 or max_norm is not finite, else min(1.0f, max_norm / (norm + 1e-6f)) in fp32 -- the
 *                    order of clip_grad_norm_ (torch/nn/utils/clip_grad.py)
 *   apply            nonfinite == 0 && isfinite(sumsq)
 *   nonfinite        number of inf / NaN ELEMENTS in the ranges, saturating at INT_MAX
 *   range_sumsq[r]   range r's share of sumsq (entries >= n_ranges are 0); sumsq is their sum in index order
 * Finite elements whose squares overflow fp32 (|g| > ~1.8e19) make the fp32 partial sum infinite: apply = 0 with nonfinite = 0.
 * A gradient that large cannot be used by an fp32 Adam step either (its second moment overflows), so the step is skipped. */
typedef struct omr_step_ctl {
    double sumsq;
    float norm, clip;
    int apply, nonfinite;
    double range_sumsq[16];
} omr_step_ctl;
#define OMR_GRAD_NORM_MAX_RANGES 16
/* The reduction's fixed shape: every thread sums the squares of OMR_GRAD_NORM_K elements in fp32, in a fixed order; everything
 * above that is fp64 in a fixed order.  Slot j of a range covers elements [j * CHUNK, (j + 1) * CHUNK) of that range, whatever
 * the device: the result does not depend on the CU count and two runs give identical bits (no atomics).
 * Error: all terms are >= 0, so |sumsq - exact| <= K 2^-24 sumsq and |norm - exact| <= (K / 2 + 2) 2^-24 norm. */
#define OMR_GRAD_NORM_K 64
#define OMR_GRAD_NORM_CHUNK 16384
/* bytes of workspace for omr_grad_norm over n elements in n_ranges ranges (non-decreasing in n); OMR_ERR_ARG for n < 1 or
 * n_ranges outside 1..16 */
long omr_grad_norm_workspace_bytes(long n, int n_ranges);
/* Two launches: (1) one workgroup per slot writes (sum of squares, non-finite count) of its chunk to ws; (2) one workgroup adds
 * each range's slots in index order, the ranges in index order, and fills *ctl.  g: 16-byte aligned fp32 [n].  range_begin /
 * range_end: HOST arrays [n_ranges] of element ranges [begin, end): sorted, disjoint, non-empty, inside [0, n), every begin a
 * multiple of 4; 1 <= n_ranges <= 16.  Elements outside every range are not read.  Anything else, or a NULL g / ws / ctl, is
 * refused with OMR_ERR_ARG before any launch.  ws: omr_grad_norm_workspace_bytes(n, n_ranges) bytes, 16-byte aligned. */
int omr_grad_norm(const float* g, long n, const long* range_begin, const long* range_end, int n_ranges, float grad_scale,
                  float max_norm, void* ws, omr_step_ctl* ctl, void* stream);
/* omr_adam behind the record (torch optim/adam.py:347 after clip_grad_norm_; GradScaler's skip): when ctl->apply == 0 the
 * launch writes NOTHING (p, m, v, p_bf16 keep their bits); otherwise g_i = (g[i] * grad_scale) * ctl->clip goes through the very
 * update omr_adam applies (one kernel), so with clip == 1.0f the results are omr_adam's bit for bit.  ctl is read on
 * the device, in stream order behind omr_grad_norm.  omr_adamw_ema (below) with weight_decay = 0, ema = decay_blocks = NULL and
 * this ctl, and its contract: p, g, m, v non-NULL and, like p_bf16, 16-byte aligned, ctl 8-byte aligned; anything else, step < 1
 * or a NULL ctl is refused with OMR_ERR_ARG before any launch. */
int omr_adam_guarded(float* p, const float* g, float* m, float* v, void* p_bf16, long n, int step, float lr, float b1, float b2,
                     float eps, float grad_scale, const omr_step_ctl* ctl, void* stream);

/* ---- optimizer recipe in the step kernel (csrc/optim.hip): decoupled weight decay, EMA weights ----
 * An extension: the reference trains with torch.optim.Adam(lr=1e-4) alone (model.py:134-139).  The definitions are torch's:
 * optim/adamw.py single-tensor math (param.mul_(1 - lr * weight_decay) in front of the Adam update) and optim/swa_utils.py
 * get_ema_multi_avg_fn (ema = d ema + (1 - d) p after the update).  ONE launch over n elements, per element, every rounded fp32
 * operation named:
 *   gi    = (g[i] * grad_scale) * clip            clip = ctl->clip, or 1.0f when ctl == NULL
 *   p'    = p[i] * f                              f = (float)(1.0 - (double)lr * (double)weight_decay), formed on the host; ONLY
 *                                                 where weight_decay != 0 and the element's block decays -- elsewhere p' = p[i]
 *                                                 and no multiply touches it
 *   m, v, denom, p_new = fma(-lr/bc1, m / denom, p')   omr_adam's four roundings (adam_update in csrc/optim.hip)
 *   ema_new = fma(d, ema[i], omd * p_new)         only when ema != NULL; d = ema_decay, omd = (float)(1.0 - (double)ema_decay).
 *                                                 d = 0 leaves p_new's bits in ema, d = 1 leaves ema's bits (signed zeros aside)
 *   p_bf16[i] = (bf16)p_new                       only when p_bf16 != NULL
 * decay_blocks (nullable: every element decays): one byte per OMR_ADAM_DECAY_BLOCK = 64 elements, byte k for elements
 * [64 k, 64 k + 64) counted from p; non-zero = decays; ceil(n / 64) bytes are read.  With ctl != NULL and ctl->apply == 0 the launch writes NOTHING: p, m, v,
 * p_bf16 and ema keep their bits.  With weight_decay == 0, ema == NULL this IS omr_adam (ctl == NULL) or
 * omr_adam_guarded: the three entries share one kernel.  16-byte loads and stores with a scalar tail: any n >= 1, but p, g, m, v, p_bf16 and ema
 * must be 16-byte aligned (ctl: 8); anything else, step < 1 or an ema_decay outside [0, 1] is refused with OMR_ERR_ARG.
 * Error against exact arithmetic on the same inputs, u = 2^-24: omr_adam's bound plus one rounding of p for the decay;
 * |ema_new - exact| <= 2 u max(|ema|, |p_new|) per step on top of what p_new carries. */
#define OMR_ADAM_DECAY_BLOCK 64
int omr_adamw_ema(float* p, const float* g, float* m, float* v, void* p_bf16, float* ema, const unsigned char* decay_blocks, long n,
                  int step, float lr, float b1, float b2, float eps, float weight_decay, float ema_decay, float grad_scale,
                  const omr_step_ctl* ctl, void* stream);
/* Exchange two fp32 buffers in place (16-byte vectors, scalar tail): the EMA weights go in for evaluation and come out again
 * without a third buffer.  a, b: 16-byte aligned; ranges that overlap (a == b included) are refused with OMR_ERR_ARG. */
int omr_swap_f32(float* a, float* b, long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
