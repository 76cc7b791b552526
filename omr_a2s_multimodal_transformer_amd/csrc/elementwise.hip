// HBM-bound elementwise / gather / reduction kernels (gfx950): 16-byte vector access per lane,
// grid-stride loops capped at 2048 blocks (256 CUs x 8).
#include "omr_common.h"
#include "omr_hip.h"

namespace {

constexpr int EW_BLOCK = 256;
inline int ew_grid(long nvec) { long g = (nvec + EW_BLOCK - 1) / EW_BLOCK; return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g)); }

template <typename T> struct Vec {
    typedef typename Frag<T>::type type;
    static constexpr int N = Frag<T>::N;
};

// ---------------------------------------------------------------- cast
template <typename TS, typename TD> __global__ void cast_kernel(const TS* __restrict__ s, TD* __restrict__ d, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        d[i] = from_f32<TD>(to_f32(s[i]));
}

// ---------------------------------------------------------------- out = a + b
template <typename T> __global__ void add_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ o, long n) {
    typedef typename Vec<T>::type V;
    constexpr int N = Vec<T>::N;
    long nv = n / N;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        V x = reinterpret_cast<const V*>(a)[i], y = reinterpret_cast<const V*>(b)[i], z;
#pragma unroll
        for (int e = 0; e < N; ++e) z[e] = from_f32<T>(to_f32(x[e]) + to_f32(y[e]));
        reinterpret_cast<V*>(o)[i] = z;
    }
    if (blockIdx.x == 0)
        for (long i = nv * N + threadIdx.x; i < n; i += blockDim.x) o[i] = from_f32<T>(to_f32(a[i]) + to_f32(b[i]));
}

// ---------------------------------------------------------------- dx = dy * (y > 0) * scale   (ReLU [+dropout] backward)
template <typename T> __global__ void relu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y, T* __restrict__ dx, long n, float scale) {
    typedef typename Vec<T>::type V;
    constexpr int N = Vec<T>::N;
    long nv = n / N;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        V g = reinterpret_cast<const V*>(dy)[i], yy = reinterpret_cast<const V*>(y)[i], z;
#pragma unroll
        for (int e = 0; e < N; ++e) z[e] = from_f32<T>(to_f32(yy[e]) > 0.f ? to_f32(g[e]) * scale : 0.f);
        reinterpret_cast<V*>(dx)[i] = z;
    }
    if (blockIdx.x == 0)
        for (long i = nv * N + threadIdx.x; i < n; i += blockDim.x)
            dx[i] = from_f32<T>(to_f32(y[i]) > 0.f ? to_f32(dy[i]) * scale : 0.f);
}

// ---------------------------------------------------------------- dropout (elementwise, or per (b, channel) for Dropout2d on NHWC)
// out = keep ? x / (1-p) : 0.   channel_mode: the mask index is b*C + c (nn.Dropout2d zeroes whole
// channels, encoder.py:99); otherwise the flat element index.
template <typename T, bool CH> __global__ void dropout_kernel(const T* __restrict__ x, T* __restrict__ o, long n, uint32_t thresh, float scale,
                                                              uint64_t seed, long per_sample, int C) {
    typedef typename Vec<T>::type V;
    constexpr int N = Vec<T>::N;
    if (CH) {
        // one keep/drop decision per (sample, channel): blockIdx.y = sample, 32-bit index math inside the sample
        const long sbase = (long)blockIdx.y * per_sample;
        const uint32_t nv = (uint32_t)(per_sample / N);
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += gridDim.x * blockDim.x) {
            const uint32_t c0 = (i * N) % (uint32_t)C;
            const V v = reinterpret_cast<const V*>(x + sbase)[i];
            V r;
#pragma unroll
            for (int e = 0; e < N; ++e)
                r[e] = drop_keep(seed, (uint64_t)blockIdx.y * C + c0 + e, thresh) ? from_f32<T>(to_f32(v[e]) * scale) : from_f32<T>(0.f);
            reinterpret_cast<V*>(o + sbase)[i] = r;
        }
        return;
    }
    const long nv = n / N;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        const V v = reinterpret_cast<const V*>(x)[i];
        V r;
#pragma unroll
        for (int e = 0; e < N; ++e) r[e] = drop_keep(seed, (uint64_t)(i * N + e), thresh) ? from_f32<T>(to_f32(v[e]) * scale) : from_f32<T>(0.f);
        reinterpret_cast<V*>(o)[i] = r;
    }
    if (blockIdx.x == 0)
        for (long k = nv * N + threadIdx.x; k < n; k += blockDim.x)
            o[k] = drop_keep(seed, (uint64_t)k, thresh) ? from_f32<T>(to_f32(x[k]) * scale) : from_f32<T>(0.f);
}

// ---------------------------------------------------------------- embedding gather + 1-D positional encoding
// out[m, :] = table[tok[m], :] + pe[m % T, :]      (decoder.py:124; no sqrt(d) scaling)
template <typename T> __global__ void embed_pe_kernel(const long* __restrict__ tok, const T* __restrict__ table, const float* __restrict__ pe,
                                                      T* __restrict__ out, long M, int Tlen, int d, int vocab) {
    long total = M * d;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long m = i / d; int c = (int)(i % d);
        long t = tok[m];
        float e = (t >= 0 && t < vocab) ? to_f32(table[t * d + c]) : 0.f;
        out[i] = from_f32<T>(e + pe[(m % Tlen) * d + c]);
    }
}
// dTable[tok[m], :] += dOut[m, :]   (fp32 atomics; the PAD row gets no gradient: nn.Embedding padding_idx)
template <typename T> __global__ void embed_bwd_kernel(const long* __restrict__ tok, const T* __restrict__ dout, float* __restrict__ dtable,
                                                       long M, int d, int pad_idx, int vocab) {
    long total = M * d;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long m = i / d; int c = (int)(i % d);
        long t = tok[m];
        if (t == pad_idx || t < 0 || t >= vocab) continue;
        atomicAdd(&dtable[t * d + c], to_f32(dout[i]));
    }
}

// ---------------------------------------------------------------- 2-D positional encoding on NHWC feature maps
// out[b,i,j,c] = x[b,i,j,c] + pe[i,j,c]  with pe stored [maxh][maxw][C]   (model.py:45-47 then flatten :147)
template <typename T> __global__ void add_pe2d_kernel(const T* __restrict__ x, const float* __restrict__ pe, T* __restrict__ out,
                                                      int B, int h, int w, int C, int maxw) {
    long total = (long)B * h * w * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int c = (int)(i % C); long p = i / C; int j = (int)(p % w); long q = p / w; int ii = (int)(q % h);
        out[i] = from_f32<T>(to_f32(x[i]) + pe[((long)ii * maxw + j) * C + c]);
    }
}
// the same with 16-byte fragments (C a multiple of the fragment width, 16-byte aligned tensors): one index decode per fragment
template <typename T> __global__ void add_pe2d_vec_kernel(const T* __restrict__ x, const float* __restrict__ pe, T* __restrict__ out,
                                                          int B, int h, int w, int C, int maxw) {
    typedef typename Frag<T>::type F;
    constexpr int VEC = Frag<T>::N;
    const int cv = C / VEC;
    const long total = (long)B * h * w * cv;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % cv) * VEC; const long p = i / cv; const int j = (int)(p % w); const long q = p / w; const int ii = (int)(q % h);
        const F xv = *reinterpret_cast<const F*>(x + p * C + c);
        const float* pp = pe + ((long)ii * maxw + j) * C + c;
        F o;
#pragma unroll
        for (int e = 0; e < VEC; e += 4) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(pp + e);
#pragma unroll
            for (int k = 0; k < 4; ++k) o[e + k] = from_f32<T>(to_f32(xv[e + k]) + pv[k]);
        }
        *reinterpret_cast<F*>(out + p * C + c) = o;
    }
}

// ---------------------------------------------------------------- column sums:  db[n] += sum_m dY[m, n]   (bias gradients)
// Block = 64 columns x 4 row phases over a slab of rows; LDS combine, one fp32 atomic per column per block.
template <typename T> __global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ dy, float* __restrict__ db, long M, int N, long ld, int rows_per_block) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + cl;
    const long r0 = (long)blockIdx.y * rows_per_block;
    const long r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
    float s = 0.f;
    if (col < N)
        for (long r = r0 + ph; r < r1; r += 4) s += to_f32(dy[r * ld + col]);
    red[ph][cl] = s;
    __syncthreads();
    if (ph == 0 && col < N) atomicAdd(&db[col], red[0][cl] + red[1][cl] + red[2][cl] + red[3][cl]);
}

// ---------------------------------------------------------------- argmax over fp32 rows (greedy decode, model.py:187)
// First-max-index tie rule (torch.argmax).  Also returns top-1 value (model.py:253 topk(1)).  One workgroup per row.
__global__ void argmax_kernel(const float* __restrict__ x0, int n, long ld, long* __restrict__ idx_out0, float* __restrict__ val_out0) {
    __shared__ float sv[256];
    __shared__ int si[256];
    long* idx_out = idx_out0 + blockIdx.x;
    float* val_out = val_out0 ? val_out0 + blockIdx.x : nullptr;
    argmax_row(x0 + (long)blockIdx.x * ld, n, threadIdx.x, sv, si);
    if (threadIdx.x == 0) { idx_out[0] = si[0] < n ? si[0] : 0; if (val_out) val_out[0] = sv[0]; }      // no comparison won (all NaN): index 0, as torch.argmax
}

// ---------------------------------------------------------------- grammar-constrained picks (omr_grammar_desc, include/omr_hip.h)
// argmax_kernel over the tokens the automaton allows in the row's state: the row's `next` row is staged in LDS, every load is
// masked (MaskedLoad), and the state advances by the picked token's class.  A pick the table forbids -- possible only where no
// allowed logit compares greater than -inf, which the Grammar constructor's guarantee (every state allows a token) leaves to
// rows of -inf / NaN -- leaves the state as it is: an invalid state is never written.
__global__ __launch_bounds__(256) void grammar_pick_kernel(const float* __restrict__ x0, int n, long ld, omr_grammar_desc g, long* __restrict__ idx_out,
                                                           float* __restrict__ val_out, long* __restrict__ tokens_out) {
    __shared__ float sv[256];
    __shared__ int si[256];
    __shared__ int next_row[256];
    const int tid = threadIdx.x, row = blockIdx.x;
    const int s = stage_next_row(g.next, g.S, g.C, g.state[row], tid, next_row);
    __syncthreads();
    argmax_row(x0 + (long)row * ld, n, tid, sv, si, MaskedLoad{g.cls, next_row});
    if (tid == 0) {
        const int pick = si[0] < n ? si[0] : 0;
        idx_out[row] = pick;
        if (val_out) val_out[row] = sv[0];
        if (tokens_out) tokens_out[row] = pick;
        const int ns = next_row[g.cls[pick]];
        g.state[row] = ns >= 0 && ns < g.S ? ns : s;
    }
}

// weighted_argmax_kernel the same way: BOTH logit rows are masked before their softmax statistics, one state per row drives both
// models.
__global__ __launch_bounds__(256) void weighted_grammar_pick_kernel(const float* __restrict__ la0, long lda, const float* __restrict__ lb0, long ldb, int n,
                                                                    float wa, float wb, omr_grammar_desc g, long* __restrict__ idx_out,
                                                                    float* __restrict__ prob_out, long* __restrict__ tokens_out) {
    __shared__ float sa[256], sb[256];
    __shared__ int si[256];
    __shared__ int next_row[256];
    const int tid = threadIdx.x, row = blockIdx.x;
    const int s = stage_next_row(g.next, g.S, g.C, g.state[row], tid, next_row);
    __syncthreads();
    weighted_argmax_row(la0 + (long)row * lda, lb0 + (long)row * ldb, n, wa, wb, tid, sa, sb, si, MaskedLoad{g.cls, next_row});
    if (tid == 0) {
        const int pick = si[0] < n ? si[0] : 0;
        idx_out[row] = pick;
        if (prob_out) prob_out[row] = sa[0];
        if (tokens_out) tokens_out[row] = pick;
        const int ns = next_row[g.cls[pick]];
        g.state[row] = ns >= 0 && ns < g.S ? ns : s;
    }
}

// ---------------------------------------------------------------- weighted late fusion (weighted_multimodal/test.py:50-61)
// token = argmax(alpha * softmax(la) + (1 - alpha) * softmax(lb)), first-index tie rule; also returns the mixed probability.
// One workgroup per row pair, three passes over the two logit rows (V <= a few thousand: L2-resident).  The mix is two roundings
// of products plus one add like torch's `alpha * p + (1 - alpha) * q` (no fma contraction), so ties break the same way.
// A row's arithmetic does not depend on how many rows the grid has: row r of a batch equals the same pair launched alone.
// tokens_out (nullable): a second copy of the picked index, where the next decoding position reads its input token.
__global__ void weighted_argmax_kernel(const float* __restrict__ la0, long lda, const float* __restrict__ lb0, long ldb, int n, float wa, float wb,
                                       long* __restrict__ idx_out, float* __restrict__ prob_out, long* __restrict__ tokens_out) {
    __shared__ float sa[256], sb[256];
    __shared__ int si[256];
    const int tid = threadIdx.x, row = blockIdx.x;
    weighted_argmax_row(la0 + (long)row * lda, lb0 + (long)row * ldb, n, wa, wb, tid, sa, sb, si);
    if (tid == 0) {
        const int pick = si[0] < n ? si[0] : 0;      // no comparison won (all NaN): index 0, never past the row
        idx_out[row] = pick;
        if (prob_out) prob_out[row] = sa[0];
        if (tokens_out) tokens_out[row] = pick;
    }
}

// ---------------------------------------------------------------- top-k log-probabilities per row (beam search)
// out_val[row][j] = log_softmax(x[row])[out_idx[row][j]], j-th largest, ties broken towards the smaller index (so k = 1 is
// argmax_kernel's pick).  One workgroup per row: a max / sum-exp pass, then k selection passes over the candidates that
// come after the previous pick in (value descending, index ascending) order.
__global__ void topk_logprob_kernel(const float* __restrict__ x0, int n, long ld, int k, long* __restrict__ idx_out, float* __restrict__ val_out) {
    __shared__ float sv[256];
    __shared__ int si[256];
    const int tid = threadIdx.x;
    long* io = idx_out + (long)blockIdx.x * k;
    float* vo = val_out + (long)blockIdx.x * k;
    topk_logprob_row(x0 + (long)blockIdx.x * ld, n, k, tid, sv, si, [&](int j, int idx, float val) {
        if (tid == 0) { io[j] = idx; vo[j] = val; }
    });
}

// ---------------------------------------------------------------- top-k log-probabilities of the weighted mix (beam search)
// out_val[row][j] = logf(alpha * softmax(la[row]) + (1 - alpha) * softmax(lb[row]))[out_idx[row][j]], j-th largest, ties towards
// the smaller index (k = 1 is weighted_argmax_kernel's pick).  One workgroup per row pair (weighted_topk_logprob_row).
__global__ void weighted_topk_logprob_kernel(const float* __restrict__ la0, long lda, const float* __restrict__ lb0, long ldb, int n, float wa, float wb,
                                             int k, long* __restrict__ idx_out, float* __restrict__ val_out) {
    __shared__ float sa[256], sb[256];
    __shared__ int si[256];
    const int tid = threadIdx.x;
    long* io = idx_out + (long)blockIdx.x * k;
    float* vo = val_out + (long)blockIdx.x * k;
    weighted_topk_logprob_row(la0 + (long)blockIdx.x * lda, lb0 + (long)blockIdx.x * ldb, n, wa, wb, k, tid, sa, sb, si, [&](int j, int idx, float val) {
        if (tid == 0) { io[j] = idx; vo[j] = val; }
    });
}

// ---------------------------------------------------------------- log-STFT post-processing (audio front end)
// spec [frames][2*bins] = (re | im) halves of the windowed DFT (one fp32 GEMM against the Hann-weighted cos / -sin basis).
// Pass 1: magnitude in place of `re` and the global maximum, carried as its bit pattern: non-negative floats order like their
// bits, and a NaN (either sign) sorts above +inf, so one non-finite magnitude reaches pass 2 instead of being dropped by fmaxf.
__global__ void stft_mag_max_kernel(float* __restrict__ spec, long frames, int bins, unsigned* __restrict__ maxbits) {
    const long n = frames * bins;
    unsigned mx = 0u;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long f = i / bins; const int k = (int)(i % bins);
        const float re = spec[f * 2 * bins + k], im = spec[f * 2 * bins + bins + k];
        const float m = sqrtf(re * re + im * im);
        spec[f * 2 * bins + k] = m;
        const unsigned b = __float_as_uint(m);
        mx = b > mx ? b : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)mx, o, 64); mx = t > mx ? t : mx; }
    if ((threadIdx.x & 63) == 0) atomicMax(maxbits, mx);
}
// Pass 2: out[bin][frame] = max(20 log10(max(amin, m)) - 20 log10(max(amin, max)), -top_db) / top_db + 1
// (librosa.amplitude_to_db(ref=np.max) with its default top_db = 80, then the reference's /80 + 1; preprocessing.py:27-28).
// The maxima are written as comparisons that keep a NaN, as numpy's do: a NaN magnitude makes the whole output NaN.  A
// magnitude equal to the maximum after the amin clamp is 0 dB by definition: the contracted 20 * log - ref_db leaves the
// product's rounding error there (up to 1 ulp of the output under 1.0), and a maximum of +inf would give inf - inf.
__global__ void stft_db_kernel(const float* __restrict__ spec, long frames, int bins, const unsigned* __restrict__ maxbits, float* __restrict__ out) {
    const float amin = 1e-5f, top_db = 80.f;
    const float mx_raw = __uint_as_float(*maxbits);
    const float mx = mx_raw < amin ? amin : mx_raw;
    const float ref_db = 20.f * log10f(mx);
    const long n = frames * bins;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i / frames); const long f = i % frames;       // output-major: coalesced stores
        const float m_raw = spec[f * 2 * bins + k];
        const float m = m_raw < amin ? amin : m_raw;
        float db = 20.f * log10f(m) - ref_db;
        if (m == mx) db = 0.f;
        db = db < -top_db ? -top_db : db;
        out[i] = db / top_db + 1.f;
    }
}

}  // namespace

extern "C" int omr_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, void* stream) {
    if (n <= 0) return OMR_OK;
    hipStream_t s = (hipStream_t)stream;
    int grid = ew_grid(n);
    if (src_dtype == OMR_F32 && dst_dtype == OMR_BF16) hipLaunchKernelGGL((cast_kernel<float, bf16>), grid, EW_BLOCK, 0, s, (const float*)src, (bf16*)dst, n);
    else if (src_dtype == OMR_BF16 && dst_dtype == OMR_F32) hipLaunchKernelGGL((cast_kernel<bf16, float>), grid, EW_BLOCK, 0, s, (const bf16*)src, (float*)dst, n);
    else if (src_dtype == OMR_F32 && dst_dtype == OMR_F32) hipLaunchKernelGGL((cast_kernel<float, float>), grid, EW_BLOCK, 0, s, (const float*)src, (float*)dst, n);
    else if (src_dtype == OMR_BF16 && dst_dtype == OMR_BF16) hipLaunchKernelGGL((cast_kernel<bf16, bf16>), grid, EW_BLOCK, 0, s, (const bf16*)src, (bf16*)dst, n);
    else return OMR_ERR_UNSUPPORTED;
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_add(int dtype, const void* a, const void* b, void* out, long n, void* stream) {
    if (n <= 0) return OMR_OK;
    DISPATCH_T(dtype, hipLaunchKernelGGL((add_kernel<T>), ew_grid(n / Frag<T>::N + 1), EW_BLOCK, 0, (hipStream_t)stream, (const T*)a, (const T*)b, (T*)out, n));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_relu_bwd(int dtype, const void* dy, const void* y, void* dx, long n, float scale, void* stream) {
    if (n <= 0) return OMR_OK;
    DISPATCH_T(dtype, hipLaunchKernelGGL((relu_bwd_kernel<T>), ew_grid(n / Frag<T>::N + 1), EW_BLOCK, 0, (hipStream_t)stream, (const T*)dy, (const T*)y, (T*)dx, n, scale));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_dropout(int dtype, const void* x, void* out, long n, float p, unsigned long long seed, int channel_mode,
                           long per_sample, int C, void* stream) {
    if (n <= 0) return OMR_OK;
    if (p < 0.f || p >= 1.f) return OMR_ERR_ARG;
    uint32_t thresh = OMR_DROP_THRESH16(p);
    float scale = 1.f / (1.f - p);
    hipStream_t s = (hipStream_t)stream;
    if (channel_mode) {
        const int vec = dtype == OMR_BF16 ? 8 : 4;
        if (per_sample <= 0 || n % per_sample || C % vec || per_sample % C || per_sample > 0x7fffffffL) return OMR_ERR_ARG;
        const int B = (int)(n / per_sample);
        dim3 grid(ew_grid(per_sample / vec) > 256 ? 256 : ew_grid(per_sample / vec), B);
        DISPATCH_T(dtype, hipLaunchKernelGGL((dropout_kernel<T, true>), grid, EW_BLOCK, 0, s, (const T*)x, (T*)out, n, thresh, scale, (uint64_t)seed, per_sample, C));
    } else {
        DISPATCH_T(dtype, hipLaunchKernelGGL((dropout_kernel<T, false>), ew_grid(n / Frag<T>::N + 1), EW_BLOCK, 0, s, (const T*)x, (T*)out, n, thresh, scale,
                                             (uint64_t)seed, per_sample, C));
    }
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_embed_pe_fwd(int dtype, const long* tokens, const void* table, const float* pe, void* out, long M, int T_len, int d,
                                int vocab, void* stream) {
    if (M <= 0 || d <= 0 || T_len <= 0) return OMR_ERR_ARG;
    DISPATCH_T(dtype, hipLaunchKernelGGL((embed_pe_kernel<T>), ew_grid(M * d), EW_BLOCK, 0, (hipStream_t)stream, tokens, (const T*)table, pe, (T*)out, M, T_len, d, vocab));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_embed_bwd(int dtype, const long* tokens, const void* dout, float* dtable, long M, int d, int pad_idx, int vocab,
                             void* stream) {
    if (M <= 0 || d <= 0) return OMR_ERR_ARG;
    DISPATCH_T(dtype, hipLaunchKernelGGL((embed_bwd_kernel<T>), ew_grid(M * d), EW_BLOCK, 0, (hipStream_t)stream, tokens, (const T*)dout, dtable, M, d, pad_idx, vocab));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_add_pe2d(int dtype, const void* x, const float* pe_hwc, void* out, int B, int h, int w, int C, int maxh, int maxw,
                            void* stream) {
    if (B <= 0 || h <= 0 || w <= 0 || C <= 0) return OMR_ERR_ARG;
    if (h > maxh || w > maxw) return OMR_ERR_ARG;  // feature map larger than the PE table
    const int vec = dtype == OMR_BF16 ? 8 : 4;
    if (C % vec == 0 && !(((uintptr_t)x | (uintptr_t)out | (uintptr_t)pe_hwc) & 15)) {
        DISPATCH_T(dtype, hipLaunchKernelGGL((add_pe2d_vec_kernel<T>), ew_grid((long)B * h * w * (C / vec)), EW_BLOCK, 0, (hipStream_t)stream, (const T*)x, pe_hwc, (T*)out, B, h, w, C, maxw));
        OMR_CHECK_LAUNCH();
        return OMR_OK;
    }
    DISPATCH_T(dtype, hipLaunchKernelGGL((add_pe2d_kernel<T>), ew_grid((long)B * h * w * C), EW_BLOCK, 0, (hipStream_t)stream, (const T*)x, pe_hwc, (T*)out, B, h, w, C, maxw));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_colsum(int dtype, const void* dy, float* db, long M, int N, long ld, void* stream) {
    if (M <= 0 || N <= 0) return OMR_ERR_ARG;
    int rpb = 128;
    dim3 grid(cdiv(N, 64), cdiv(M, rpb));
    DISPATCH_T(dtype, hipLaunchKernelGGL((colsum_kernel<T>), grid, 256, 0, (hipStream_t)stream, (const T*)dy, db, M, N, ld, rpb));
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_log_stft_post(float* spec, long frames, int bins, unsigned* max_ws, float* out, void* stream) {
    if (frames <= 0 || bins <= 0 || !spec || !max_ws || !out) return OMR_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(max_ws, 0, sizeof(unsigned), s) != hipSuccess) return OMR_ERR_LAUNCH;
    hipLaunchKernelGGL(stft_mag_max_kernel, ew_grid(frames * bins), EW_BLOCK, 0, s, spec, frames, bins, max_ws);
    hipLaunchKernelGGL(stft_db_kernel, ew_grid(frames * bins), EW_BLOCK, 0, s, (const float*)spec, frames, bins, (const unsigned*)max_ws, out);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_topk_logprob(const float* x, int rows, int n, long ld, int k, long* idx_out, float* val_out, void* stream) {
    if (n <= 0 || rows <= 0 || ld < n || k <= 0 || k > n || !idx_out || !val_out) return OMR_ERR_ARG;
    hipLaunchKernelGGL(topk_logprob_kernel, rows, 256, 0, (hipStream_t)stream, x, n, ld, k, idx_out, val_out);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_weighted_argmax_rows(const float* logits_a, long lda, const float* logits_b, long ldb, int rows, int n, float alpha,
                                        long* idx_out, float* prob_out, long* tokens_out, void* stream) {
    if (rows < 1 || n < 1 || lda < n || ldb < n || !logits_a || !logits_b || !idx_out) return OMR_ERR_ARG;
    // the reference multiplies fp32 tensors by the Python floats alpha and (1 - alpha): each is rounded to fp32 once
    hipLaunchKernelGGL(weighted_argmax_kernel, rows, 256, 0, (hipStream_t)stream, logits_a, lda, logits_b, ldb, n, alpha, (float)(1.0 - (double)alpha),
                       idx_out, prob_out, tokens_out);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_weighted_topk_logprob(const float* logits_a, long lda, const float* logits_b, long ldb, int rows, int n, float alpha, int k,
                                         long* idx_out, float* val_out, void* stream) {
    if (rows < 1 || k < 1 || k > OMR_MAX_BEAM || n < k || lda < n || ldb < n || !logits_a || !logits_b || !idx_out || !val_out) return OMR_ERR_ARG;
    hipLaunchKernelGGL(weighted_topk_logprob_kernel, rows, 256, 0, (hipStream_t)stream, logits_a, lda, logits_b, ldb, n, alpha, (float)(1.0 - (double)alpha),
                       k, idx_out, val_out);      // the weights as omr_weighted_argmax_rows rounds them
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_weighted_argmax(const float* logits_a, const float* logits_b, int n, float alpha, long* idx_out, float* prob_out, void* stream) {
    return omr_weighted_argmax_rows(logits_a, n, logits_b, n, 1, n, alpha, idx_out, prob_out, nullptr, stream);
}

extern "C" int omr_argmax(const float* x, int rows, int n, long ld, long* idx_out, float* val_out, void* stream) {
    if (n <= 0 || rows <= 0 || ld < n) return OMR_ERR_ARG;
    hipLaunchKernelGGL(argmax_kernel, rows, 256, 0, (hipStream_t)stream, x, n, ld, idx_out, val_out);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

// the descriptor check every grammar entry shares (declared in omr_common.h)
bool grammar_desc_ok(const omr_grammar_desc* g) {
    return g && g->cls && g->next && g->state && g->C >= 1 && g->C <= OMR_GRAMMAR_MAX_CLASSES && g->S >= 1;
}

extern "C" int omr_grammar_pick(const float* logits, long ld, int rows, int n, const omr_grammar_desc* g, long* idx_out, float* val_out,
                                long* tokens_out, void* stream) {
    if (!grammar_desc_ok(g)) return OMR_ERR_ARG;
    if (n <= 0 || rows <= 0 || ld < n || !logits || !idx_out) return OMR_ERR_ARG;
    hipLaunchKernelGGL(grammar_pick_kernel, rows, 256, 0, (hipStream_t)stream, logits, n, ld, *g, idx_out, val_out, tokens_out);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_weighted_grammar_pick(const float* logits_a, long lda, const float* logits_b, long ldb, int rows, int n, float alpha,
                                         const omr_grammar_desc* g, long* idx_out, float* prob_out, long* tokens_out, void* stream) {
    if (!grammar_desc_ok(g)) return OMR_ERR_ARG;
    if (rows < 1 || n < 1 || lda < n || ldb < n || !logits_a || !logits_b || !idx_out) return OMR_ERR_ARG;
    hipLaunchKernelGGL(weighted_grammar_pick_kernel, rows, 256, 0, (hipStream_t)stream, logits_a, lda, logits_b, ldb, n, alpha,
                       (float)(1.0 - (double)alpha), *g, idx_out, prob_out, tokens_out);      // the weights as omr_weighted_argmax_rows rounds them
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}
