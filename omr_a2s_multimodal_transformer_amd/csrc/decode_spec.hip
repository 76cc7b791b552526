// Speculative greedy decoding (include/omr_hip.h "speculative greedy decoding"): the state block, the acceptance kernel and the
// cycle driver.  A cycle is draft (k + 1 single positions of the per-row-position path on the draft's own caches), one launch that
// lays the proposals out, verify (ONE grouped position of the target: decode.hip verify_rows) and accept -- all positions come
// from device memory, so n_cycles cycles are one host call.
#include "decode_common.h"

using namespace omr_dec;

namespace {

size_t spec_carve(omr_spec_desc* s) {
    const size_t B = (size_t)s->B, R = (size_t)s->k + 1, out = B * (size_t)s->max_out;
    char* base = (char*)s->state;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base + off; off += align256(bytes); return p; };
    s->pos = (int*)take(B * 4); s->out_len = (int*)take(B * 4); s->done = (int*)take(B * 4); s->accepted = (int*)take(B * 4);
    s->totals = (long*)take(2 * 8); s->first = (long*)take(B * 8); s->prev = (long*)take(B * 8);
    s->tokens = (long*)take(B * R * 8); s->picks = (long*)take(B * R * 8); s->top1 = (float*)take(B * R * 4); s->dpicks = (long*)take(R * B * 8);
    s->out_tokens = (long*)take(out * 8); s->out_top1 = (float*)take(out * 4);
    return off;
}

bool spec_shape_ok(const omr_spec_desc& s) { return s.B >= 1 && s.k >= 1 && s.k < OMR_MAX_VERIFY_ROWS && s.max_out >= 1; }

bool spec_desc_ok(const omr_spec_desc& s) {
    if (!spec_shape_ok(s) || !s.state) return false;
    omr_spec_desc c = s;
    if ((long)spec_carve(&c) > s.state_bytes) return false;
    return c.pos == s.pos && c.out_len == s.out_len && c.done == s.done && c.accepted == s.accepted && c.totals == s.totals && c.first == s.first &&
           c.prev == s.prev && c.tokens == s.tokens && c.picks == s.picks && c.top1 == s.top1 && c.dpicks == s.dpicks && c.out_tokens == s.out_tokens &&
           c.out_top1 == s.out_top1;
}

// tokens[b][0] = the token slot b feeds to pos[b]; tokens[b][i] = the draft's pick of its position pos[b] + i - 1 (step i of the cycle)
__global__ __launch_bounds__(256) void spec_propose_kernel(omr_spec_desc s) {
    const int R = s.k + 1, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= s.B * R) return;
    const int b = i / R, r = i % R;
    s.tokens[i] = r == 0 ? s.first[b] : s.dpicks[(long)r * s.B + b];
}

// One workgroup; thread = slot (strided).  The two totals are summed through LDS in a fixed order by thread 0: no atomics.
__global__ __launch_bounds__(256) void spec_accept_kernel(omr_spec_desc s) {
    __shared__ int drafted_s[256], accepted_s[256];
    const int R = s.k + 1;
    int drafted = 0, accepted = 0;
    for (int b = threadIdx.x; b < s.B; b += 256) {
        if (s.done[b]) { s.accepted[b] = 0; continue; }
        const long* tok = s.tokens + (long)b * R;
        const long* pick = s.picks + (long)b * R;
        const float* val = s.top1 + (long)b * R;
        int j = 0;
        while (j < s.k && tok[j + 1] == pick[j]) ++j;
        int n = j + 1, done = 0;
        for (int i = 0; i < n; ++i)
            if (pick[i] == s.eos) { n = i + 1; done = 1; break; }
        const int len = s.out_len[b], room = s.max_out - len;
        if (n >= room) { n = room; done = 1; }
        for (int i = 0; i < n; ++i) {
            s.out_tokens[(long)b * s.max_out + len + i] = pick[i];
            s.out_top1[(long)b * s.max_out + len + i] = val[i];
        }
        if (n > 0) {
            s.prev[b] = n >= 2 ? pick[n - 2] : s.first[b];
            s.first[b] = pick[n - 1];
            s.out_len[b] = len + n;
            s.pos[b] += n;
        }
        s.done[b] = done;
        s.accepted[b] = j;
        drafted += s.k; accepted += j;
    }
    drafted_s[threadIdx.x] = drafted; accepted_s[threadIdx.x] = accepted;
    __syncthreads();
    if (threadIdx.x == 0) {
        long d = 0, a = 0;
        for (int i = 0; i < 256; ++i) { d += drafted_s[i]; a += accepted_s[i]; }
        s.totals[0] += d; s.totals[1] += a;
    }
}

}  // namespace

extern "C" long omr_spec_workspace_bytes(omr_spec_desc* s) {
    if (!s || !spec_shape_ok(*s)) return OMR_ERR_ARG;
    return (long)spec_carve(s);
}

extern "C" int omr_spec_accept(const omr_spec_desc* s, void* stream) {
    if (!s || !spec_desc_ok(*s)) return OMR_ERR_ARG;
    hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *s);
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

extern "C" int omr_spec_decode_cycles(const omr_decode_desc* target, const omr_decode_desc* draft, const int* mem_len_t, const int* mem_len_d,
                                      const omr_spec_desc* sp, int k, int n_cycles, void* stream) {
    if (!target || !draft) return OMR_ERR_ARG;
    if (!takes_row_kernel(*target) || !takes_row_kernel(*draft)) return OMR_ERR_UNSUPPORTED;
    if (!sp || !spec_desc_ok(*sp) || k != sp->k || n_cycles < 1) return OMR_ERR_ARG;
    const omr_spec_desc& s = *sp;
    const int R = k + 1;
    const long last = (long)s.t_max + (long)n_cycles * R;                 // one past the furthest position the last cycle may touch
    if (s.t_max < 1 || last > target->max_len || last > draft->max_len) return OMR_ERR_ARG;
    // the target's grouped cross-attention and the draft's per-row memory lengths exist in the key-split kernel only (S > 64)
    if (target->S <= 64 || (mem_len_d && draft->S <= 64)) return OMR_ERR_UNSUPPORTED;
    if (target->B != s.B || draft->B != s.B || target->V != draft->V || s.eos < 0 || s.eos >= target->V) return OMR_ERR_ARG;
    OMR_TRY(check_desc(*target));
    OMR_TRY(check_model(*draft));
    if (!s.ws_t || s.ws_t_bytes < omr_decode_group_workspace_bytes(target, R)) return OMR_ERR_ARG;
    const Model md = make_model(draft, mem_len_d, 1);
    const size_t B = (size_t)s.B;
    for (int c = 0; c < n_cycles; ++c) {
        const int t_max = s.t_max + c * R;                                // no slot is further: a cycle advances a slot by at most R
        // draft: positions pos - 1 .. pos + k - 1.  The first closes the gap of a fully accepted cycle and needs no pick
        launch_rows_tables(md, s.pos, -1, R, stream);
        for (int i = 0; i < R; ++i) {
            const long* tok_in = i == 0 ? s.prev : i == 1 ? s.first : s.dpicks + (size_t)(i - 1) * B;
            const Pick pick = {i == 0 ? nullptr : s.dpicks + (size_t)i * B, nullptr};
            float* l32 = nullptr;
            OMR_TRY(run_position(md, position_at(md, s.pos, t_max - 1 + i, i), tok_in, pick, &l32, stream));
        }
        hipLaunchKernelGGL(spec_propose_kernel, dim3((unsigned)cdiv((long)s.B * R, 256)), dim3(256), 0, (hipStream_t)stream, s);
        OMR_TRY(verify_rows(target, mem_len_t, s.pos, t_max, R, s.tokens, s.picks, s.top1, s.ws_t, s.ws_t_bytes, stream));
        hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, s);
        OMR_CHECK_LAUNCH();
    }
    return OMR_OK;
}
