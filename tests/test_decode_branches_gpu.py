"""The decode path's kernels, branch by branch, against the fp64 references of oracle/decode_refs.py: the row linear
(decode_linear_kernel<T, W8, ROWS> + decode_pick_kernel), every refusal of its entry, the selection rows of the beam search and
the fp8 GEMM at ragged shapes.  Every case is the smallest that reaches its branch ("Decode branch coverage", maps
branch to test id); operands are views into NaN-filled buffers, outputs views into sentinel-filled ones, and every test ends
with the check that nothing outside the logical outputs was written (inside `lin_check`).
tests/test_decode_refs_cpu.py runs the same table with torch CPU arithmetic in the kernels' place."""
import ctypes

import pytest
import torch

from oracle import decode_refs as R
from oracle.kernel_refs import BF16, DTYPES, F32, SENTINEL, TAG, assert_bit_equal, bits

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(case: R.LinCase, rows=None, want_argmax: bool = True):
    """The case through kernels.decode_linear.  rows: launch only these rows of the case (a list of row numbers), into fresh
    buffers of the same layout.  -> the buffers after the call, on the CPU (keys of R.lin_standin)."""
    from omr_a2s_multimodal_transformer_amd import kernels as K
    inp = R.lin_inputs(case)
    M, N, Kd, n0 = case.M, case.N, case.K, case.n_0
    sel = list(range(M)) if rows is None else rows
    m = len(sel)
    dev = {k: v.to(DEV) for k, v in inp.items() if isinstance(v, torch.Tensor)}
    kw = {}
    if case.pro in (0, 1):
        xb = dev["x_buf"]
        if rows is not None:
            xb = xb.clone(); xb[:m] = dev["x_buf"][sel]
        kw["x"] = xb[:m, :Kd]
        if case.pro == 1:
            rb = dev["res_buf"]
            if rows is not None:
                rb = rb.clone(); rb[:m] = dev["res_buf"][sel]
            kw.update(res=rb[:m, :Kd], ln=(dev["gamma"], dev["beta"], inp["eps"]))
    elif case.pro == 2:
        kw.update(tokens=dev["tokens"][sel].contiguous(), emb=dev["emb"], pe_row=dev["pe"])
        if case.rows:
            kw.update(row_pos=dev["row_pos"][sel].contiguous(), out1_pos_ld=dev["out1_buf"].stride(1))
    else:
        H = case.merge[0]
        kw.update(part=dev["part"].view(M, H, *dev["part"].shape[1:])[sel].reshape(m * H, *dev["part"].shape[1:]).contiguous(), heads=H)
    if case.w8:
        kw.update(w8=dev["w8"], w8_scale=dev["w8_scale"], dtype=case.dtype)
    out1 = dev["out1_buf"][:m, 0, :N - n0] if case.rows else dev["out1_buf"][:m, :N - n0]
    res = K.decode_linear(None if case.w8 else dev["w"], dev.get("bias") if inp["bias"] is not None else None, relu=case.relu, n0=n0,
                          out0=dev["out0_buf"][:m, :n0], out1=out1, out32=dev["out32_buf"][:m, :N],
                          built=dev["built_buf"][:m] if case.pro in (1, 2) else None, want_argmax=want_argmax, **kw)
    torch.cuda.synchronize()
    out = {k: dev[k].cpu() for k in ("out0_buf", "out1_buf", "out32_buf", "built_buf")}
    out["idx"], out["val"] = (res[4][0].cpu(), res[4][1].cpu()) if want_argmax else (None, None)
    return out


def _is_sentinel(t) -> bool:
    t = t.cpu()
    return bool((t == torch.full((), SENTINEL, dtype=t.dtype)).all())


def _check(case, out):
    r = R.lin_check(case, out, who="gpu ")
    assert r <= 1.0
    return r


# ---- decode_linear_kernel<T, W8, false>: every instantiation, three workgroups (the last with 5 real columns), M = 11 (rm = 3 on
#      the second row group), bias + ReLU and no bias; the pick over G = 3 candidates
@pytest.mark.parametrize("case", R.INST_CASES, ids=R.case_id)
def test_instantiations(case):
    _check(case, _run(case))


# ---- the K loop: cpt = 8 (the loop past the prefetched chunks is empty) and cpt = 9 (it runs once), all four instantiations
@pytest.mark.parametrize("case", R.CHUNK_CASES, ids=R.case_id)
def test_chunk_loops(case):
    assert case.cpt in (8, 9)
    _check(case, _run(case))


# ---- K = 2048, M = 9: 64 KiB of dynamic LDS on top of the static 16.5 KiB, the largest launch the entry accepts
@pytest.mark.parametrize("case", R.BIG_CASES, ids=R.case_id)
def test_largest_k(case):
    _check(case, _run(case))


# ---- row groups: M = 1 (lean body), 8 (one full group), 9 (second blockIdx.y with rm = 1: the lean body again), 11 (rm = 3:
#      arithmetic on stale LDS rows that is never stored); every row bit-equal to the same row launched alone
@pytest.mark.parametrize("case", R.GROUP_CASES, ids=R.case_id)
def test_row_groups(case):
    out = _run(case)
    _check(case, out)
    full = R.stored(case, out)
    for i in range(case.M):
        one = _run(case, rows=[i])
        got = one["out0_buf"][:1, :case.N]
        assert_bit_equal(got, full[i:i + 1], f"{case.name}: row {i} launched alone")
        assert one["idx"].tolist() == out["idx"][i:i + 1].tolist()
        rest = bits(one["out0_buf"]).clone()
        rest[:1, :case.N] = bits(torch.full((1,), SENTINEL, dtype=case.dtype))[0]
        assert bool((rest == bits(R.lin_inputs(case)["out0_buf"])).all()), f"{case.name}: the single-row launch wrote outside its row"


# ---- strides: ldx = K + 8, ldres = K + 16, ld0 = n0 + 8, ld1 = (N - n0) + 24, ld32 = N + 8, n0 in {0, 16, N}; pro 1
@pytest.mark.parametrize("case", R.STRIDE_CASES, ids=R.case_id)
def test_strides(case):
    from omr_a2s_multimodal_transformer_amd import kernels as K
    inp = R.lin_inputs(case)
    ln_rows, _, _ = K.add_layernorm_fwd(inp["x_buf"][:case.M, :case.K].contiguous().to(DEV), inp["res_buf"][:case.M, :case.K].contiguous().to(DEV),
                                        inp["gamma"].to(DEV), inp["beta"].to(DEV), inp["eps"])
    r = R.lin_check(case, _run(case), ln_rows=ln_rows, who="gpu ")
    assert r <= 1.0


# ---- prologues 1 and 2 at per = 2, 4, 8: identity weight, so out0 is the rows the product saw; xn_out equals them
@pytest.mark.parametrize("case", R.PRO_CASES, ids=R.case_id)
def test_prologues(case):
    from omr_a2s_multimodal_transformer_amd import kernels as K
    inp = R.lin_inputs(case)
    ln_rows = None
    if case.pro == 1:
        ln_rows, _, _ = K.add_layernorm_fwd(inp["x_buf"][:case.M, :case.K].contiguous().to(DEV), inp["res_buf"][:case.M, :case.K].contiguous().to(DEV),
                                            inp["gamma"].to(DEV), inp["beta"].to(DEV), inp["eps"])
    r = R.lin_check(case, _run(case), ln_rows=ln_rows, who="gpu ")
    assert r <= 1.0


# ---- prologue 3 on hand-made partials: strip loop once / twice / eight times (H nsplit = 8, 20, 66, 512 = MAXHS), nsplit odd and
#      no multiple of 4, an empty split with garbage, a row of empty splits, weights that underflow to 0
@pytest.mark.parametrize("case", R.MERGE_CASES, ids=R.case_id)
def test_merge_prologue(case):
    _check(case, _run(case))


@pytest.mark.parametrize("dtype", DTYPES, ids=[TAG[d] for d in DTYPES])
def test_merge_prologue_equals_the_attention_merge_kernel(dtype):
    """Prologue 3 builds, to the bit, the rows attn_split_merge_kernel writes from the same partials: a decode attention at
    S = 257, the smallest that splits (2 splits of 256 + 1 keys), merged once by the attention itself and once by the row kernel
    under an identity weight."""
    from omr_a2s_multimodal_transformer_amd import kernels as K
    H, hd, B, S = 4, 32, 3, 257
    d = H * hd
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, 1, d, generator=g).to(dtype).to(DEV)
    kv = torch.randn(B, S, 2 * d, generator=g).to(dtype).to(DEV)
    from omr_a2s_multimodal_transformer_amd._lib import cur_stream, dtype_code, lib
    k, v = kv[..., :d], kv[..., d:]
    o_ref = torch.empty((B, 1, d), dtype=dtype, device=DEV)
    lse = torch.empty((B, H, 1), dtype=torch.float32, device=DEV)
    n = lib().query("omr_attn_split_workspace_floats", B, H, 1, S, hd)
    assert n == B * H * 2 * (hd + 2)
    ws = torch.empty(n, dtype=torch.float32, device=DEV)
    lib().call("omr_attn_fwd_split", dtype_code(dtype), q.data_ptr(), k.data_ptr(), v.data_ptr(), o_ref.data_ptr(), lse.data_ptr(), d, 2 * d, 2 * d, d,
               d, S * 2 * d, S * 2 * d, d, B, H, 1, S, hd, None, ws.data_ptr(), n, cur_stream())
    part, ns = K.attn_fwd_split_partials(q, k, v, H)
    assert ns == 2
    o, _, _, _ = K.decode_linear(torch.eye(d, dtype=dtype, device=DEV), None, part=part, heads=H)
    assert_bit_equal(o.cpu(), o_ref.view(B, d).cpu(), "merge prologue vs attn_split_merge_kernel")


# ---- the greedy pick: G = 65 candidates, ties in three placements, the last real column, rows on which no comparison succeeds
@pytest.mark.parametrize("case", R.PICK_CASES, ids=R.case_id)
def test_pick(case):
    _check(case, _run(case))


# ---- decode_linear_kernel<T, false, true>: per-row positions
@pytest.mark.parametrize("case", R.ROWS_CASES, ids=R.case_id)
def test_per_row_positions(case):
    from omr_a2s_multimodal_transformer_amd import kernels as K
    out = _run(case)
    _check(case, out)
    # row m equals the plain entry given row_pos[m]'s positional row
    inp = R.lin_inputs(case)
    full = R.stored(case, out)
    for m in (1, 3, case.M - 1):
        o0, o1, built, _ = K.decode_linear(inp["w"].to(DEV), inp["bias"].to(DEV), tokens=inp["tokens"][m:m + 1].to(DEV), emb=inp["emb"].to(DEV),
                                           pe_row=inp["pe"][R.ROWS_POS[m]].contiguous().to(DEV), n0=case.n_0)
        assert_bit_equal(torch.cat([o0, o1], 1).cpu(), full[m:m + 1], f"{case.name}: row {m} vs omr_decode_linear at its position")
        assert_bit_equal(built.cpu(), out["built_buf"][m:m + 1], f"{case.name}: built row {m}")


@pytest.mark.parametrize("dtype", DTYPES, ids=[TAG[d] for d in DTYPES])
def test_per_row_positions_e4m3(dtype):
    """decode_linear_kernel<T, true, true>: the e4m3 weights under per-row positions equal, row by row, the plain e4m3 entry."""
    from omr_a2s_multimodal_transformer_amd import kernels as K
    case = R.CASE[f"rows-{TAG[dtype]}"]
    inp = R.lin_inputs(case)
    M, N, Kd, n0 = case.M, case.N, case.K, case.n_0
    w8, sc = R.e4m3_codes((N, Kd), 77).to(DEV), ((0.5 + torch.rand(N, generator=torch.Generator().manual_seed(78))) / 8.0).to(DEV)
    cache = inp["out1_buf"].to(DEV)
    o0, _, built, _ = K.decode_linear(None, inp["bias"].to(DEV), tokens=inp["tokens"].to(DEV), emb=inp["emb"].to(DEV), pe_row=inp["pe"].to(DEV), n0=n0,
                                      w8=w8, w8_scale=sc, dtype=dtype, out1=cache[:M, 0, :N - n0], row_pos=inp["row_pos"].to(DEV),
                                      out1_pos_ld=cache.stride(1))
    got1 = cache.cpu()[torch.arange(M), inp["row_pos"].long(), :N - n0]
    after = bits(cache.cpu()).clone()
    after[torch.arange(M), inp["row_pos"].long(), :N - n0] = bits(inp["out1_buf"])[0, 0, 0]
    assert bool((after == bits(inp["out1_buf"])).all()), "cache elements outside the rows' own positions were written"
    for m in range(M):
        a0, a1, b, _ = K.decode_linear(None, inp["bias"].to(DEV), tokens=inp["tokens"][m:m + 1].to(DEV), emb=inp["emb"].to(DEV),
                                       pe_row=inp["pe"][R.ROWS_POS[m]].contiguous().to(DEV), n0=n0, w8=w8, w8_scale=sc, dtype=dtype)
        assert_bit_equal(o0[m:m + 1].cpu(), a0.cpu(), f"row {m} out0")
        assert_bit_equal(got1[m:m + 1], a1.cpu(), f"row {m} out1")
        assert_bit_equal(built[m:m + 1].cpu(), b.cpu(), f"row {m} built")


# ---- every `return OMR_ERR_*` of decode_linear_impl: nothing is launched, the outputs keep their sentinel
ARG, UNSUPPORTED = -1, -3


def _valid_args(pro: int, dtype=F32, K_: int = 128, w8: bool = False):
    """A valid argument block (M = 2, N = 20, n0 = 16) and the tensors that back it."""
    from omr_a2s_multimodal_transformer_amd import kernels as K
    from omr_a2s_multimodal_transformer_amd._lib import dtype_code
    M, N, n0 = 2, 20, 16
    t = dict(x=torch.zeros(M, K_, dtype=dtype), res=torch.zeros(M, K_, dtype=dtype), gamma=torch.ones(K_), beta=torch.zeros(K_),
             tokens=torch.zeros(M, dtype=torch.int64), emb=torch.zeros(3, K_, dtype=dtype), pe=torch.zeros(K_), part=torch.zeros(M * 4, 2, K_ // 4 + 2),
             w=torch.zeros(N, K_, dtype=dtype), w8=torch.zeros(N * K_ + 16, dtype=torch.uint8), w8_scale=torch.ones(N), bias=torch.zeros(N),
             out0=torch.full((M, n0), SENTINEL, dtype=dtype), out1=torch.full((M, N - n0), SENTINEL, dtype=dtype),
             out32=torch.full((M, N), SENTINEL), xn=torch.full((M, K_), SENTINEL, dtype=dtype),
             idx=torch.full((M,), -7, dtype=torch.int64), val=torch.full((M,), SENTINEL), ap=torch.full((2 * M * 2,), SENTINEL),
             row_pos=torch.zeros(M, dtype=torch.int32))
    t = {k: v.to(DEV) for k, v in t.items()}
    a = K._DecodeLinearArgs()
    a.dtype, a.pro, a.M, a.N, a.K, a.n0, a.eps = dtype_code(dtype), pro, M, N, K_, n0, 1e-5
    a.x, a.ldx, a.res, a.ldres, a.gamma, a.beta, a.xn_out = t["x"].data_ptr(), K_, t["res"].data_ptr(), K_, t["gamma"].data_ptr(), t["beta"].data_ptr(), t["xn"].data_ptr()
    a.tokens, a.emb, a.pe_row, a.vocab = t["tokens"].data_ptr(), t["emb"].data_ptr(), t["pe"].data_ptr(), 3
    a.part, a.nsplit, a.H, a.hd = t["part"].data_ptr(), 2, 4, K_ // 4
    a.bias, a.out0, a.ld0, a.out1, a.ld1, a.out32, a.ld32 = t["bias"].data_ptr(), t["out0"].data_ptr(), n0, t["out1"].data_ptr(), N - n0, t["out32"].data_ptr(), N
    a.amax_idx, a.amax_val, a.amax_part = t["idx"].data_ptr(), t["val"].data_ptr(), t["ap"].data_ptr()
    if w8:
        a.w8, a.w8_scale = t["w8"].data_ptr(), t["w8_scale"].data_ptr()
    else:
        a.w = t["w"].data_ptr()
    return a, t


def _set(**kw):
    return lambda a, t: [setattr(a, k, v) for k, v in kw.items()]


REFUSALS = [
    # (id, pro, dtype, K, w8, change, expected code)
    ("M0", 0, F32, 128, False, _set(M=0), ARG), ("N0", 0, F32, 128, False, _set(N=0), ARG), ("K0", 0, F32, 128, False, _set(K=0), ARG),
    ("K-not-vec-f32", 0, F32, 128, False, _set(K=130), ARG), ("K-not-vec-bf16", 0, BF16, 128, False, _set(K=132), ARG),
    ("K-not-vec-e4m3", 0, F32, 128, True, _set(K=132), ARG), ("K-above-2048", 0, F32, 128, False, _set(K=2112), ARG),
    ("no-weights", 0, F32, 128, False, _set(w=None), ARG), ("no-out0", 0, F32, 128, False, _set(out0=None), ARG),
    ("n0-negative", 0, F32, 128, False, _set(n0=-1), ARG),
    ("w8-no-scale", 0, F32, 128, True, _set(w8_scale=None), ARG),
    ("w8-not-8-byte-aligned", 0, BF16, 128, True, lambda a, t: setattr(a, "w8", t["w8"].data_ptr() + 4), ARG),
    ("w-not-16-byte-aligned", 0, F32, 128, False, lambda a, t: setattr(a, "w", t["w"].data_ptr() + 8), ARG),
    ("no-out1", 0, F32, 128, False, _set(out1=None), ARG),
    ("pro-negative", 0, F32, 128, False, _set(pro=-1), ARG), ("pro-4", 0, F32, 128, False, _set(pro=4), ARG),
    ("K-not-16-chunks-f32", 0, F32, 128, False, _set(K=96), UNSUPPORTED), ("K-not-16-chunks-bf16", 0, BF16, 128, False, _set(K=64), UNSUPPORTED),
    ("K-not-16-chunks-e4m3", 0, F32, 128, True, _set(K=192), UNSUPPORTED),
    ("amax-idx-without-part", 0, F32, 128, False, _set(amax_part=None), ARG),
    ("pro-K-above-1024", 2, F32, 128, False, _set(K=1088), ARG),
    ("pro1-K-384", 1, F32, 128, False, _set(K=384), UNSUPPORTED),
    ("pro0-no-x", 0, F32, 128, False, _set(x=None), ARG), ("pro1-no-x", 1, F32, 128, False, _set(x=None), ARG),
    ("pro1-no-res", 1, F32, 128, False, _set(res=None), ARG), ("pro1-no-gamma", 1, F32, 128, False, _set(gamma=None), ARG),
    ("pro1-no-beta", 1, F32, 128, False, _set(beta=None), ARG), ("pro1-no-xn_out", 1, F32, 128, False, _set(xn_out=None), ARG),
    ("pro2-no-tokens", 2, F32, 128, False, _set(tokens=None), ARG), ("pro2-no-emb", 2, F32, 128, False, _set(emb=None), ARG),
    ("pro2-no-pe_row", 2, F32, 128, False, _set(pe_row=None), ARG), ("pro2-no-xn_out", 2, F32, 128, False, _set(xn_out=None), ARG),
    ("pro3-no-part", 3, F32, 128, False, _set(part=None), ARG), ("pro3-nsplit-0", 3, F32, 128, False, _set(nsplit=0), ARG),
    ("pro3-nsplit-65", 3, F32, 128, False, _set(nsplit=65), ARG), ("pro3-H-0", 3, F32, 128, False, _set(H=0), ARG),
    ("pro3-hd-0", 3, F32, 128, False, _set(hd=0), ARG), ("pro3-H-hd-not-K", 3, F32, 128, False, _set(H=2), ARG),
    ("pro3-H-nsplit-528", 3, F32, 128, False, _set(H=16, hd=8, nsplit=33), ARG),       # K = 128, per = 2, hd % 2 == 0, nsplit <= 64: MAXHS alone
    ("pro3-hd-not-multiple-of-per", 3, F32, 128, False, _set(H=128, hd=1, nsplit=1), ARG),
    ("dtype-2", 0, F32, 128, False, _set(dtype=2), UNSUPPORTED),
]


@pytest.mark.parametrize("rid,pro,dtype,K_,w8,change,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(rid, pro, dtype, K_, w8, change, code):
    from omr_a2s_multimodal_transformer_amd._lib import lib
    a, t = _valid_args(pro, dtype, K_, w8)
    change(a, t)
    for entry, extra in (("omr_decode_linear", ()), ("omr_decode_linear_rows", (t["row_pos"].data_ptr(), 0))):
        assert lib().query(entry, ctypes.byref(a), *extra, None) == code, (rid, entry)
    torch.cuda.synchronize()
    for k in ("out0", "out1", "out32", "xn", "val", "ap"):
        assert _is_sentinel(t[k]), f"{rid}: {k} was written"
    assert t["idx"].cpu().tolist() == [-7, -7]


def test_refusals_of_null_arguments_and_the_valid_block():
    """NULL argument block, NULL row_pos, negative out1_pos_ld; and the block the refusal cases start from is itself accepted by
    both entries for every prologue (so each refusal above is due to the one field it changes)."""
    from omr_a2s_multimodal_transformer_amd._lib import lib
    a, t = _valid_args(0)
    assert lib().query("omr_decode_linear", None, None) == ARG
    assert lib().query("omr_decode_linear_rows", None, t["row_pos"].data_ptr(), 0, None) == ARG
    assert lib().query("omr_decode_linear_rows", ctypes.byref(a), None, 0, None) == ARG
    assert lib().query("omr_decode_linear_rows", ctypes.byref(a), t["row_pos"].data_ptr(), -1, None) == ARG
    torch.cuda.synchronize()
    assert _is_sentinel(t["out0"])
    for pro in (0, 1, 2, 3):
        for w8 in (False, True):
            a, t = _valid_args(pro, BF16 if w8 else F32, 128, w8)
            assert lib().query("omr_decode_linear", ctypes.byref(a), None) == 0
            assert lib().query("omr_decode_linear_rows", ctypes.byref(a), t["row_pos"].data_ptr(), 0, None) == 0
            torch.cuda.synchronize()
            assert bool((t["out0"].cpu() == 0).all()) and t["idx"].cpu().tolist() == [0, 0]


# ---- the selection rows of the beam search: topk_logprob_row / weighted_topk_logprob_row
@pytest.mark.parametrize("mix", [False, True], ids=["topk", "weighted"])
@pytest.mark.parametrize("k", R.SEL_KS)
@pytest.mark.parametrize("n", R.SEL_NS)
def test_selection_rows(n, k, mix):
    from omr_a2s_multimodal_transformer_amd import kernels as K
    inp = R.sel_inputs(n)
    a, b = inp["a"].to(DEV), inp["b"].to(DEV)
    if mix:
        idx, val = K.weighted_topk_logprob(a, b, R.SEL_ALPHA, k, n=n)
    else:
        idx, val = K.topk_logprob(a[:, :n], k)
    assert R.sel_check(n, k, mix, idx, val, who="gpu ") <= 1.0


# ---- fp8 GEMM at K no multiple of 128, M in {1, 5}, N = 70, ldx > K, one all-zero row
@pytest.mark.parametrize("dtype", DTYPES, ids=[TAG[d] for d in DTYPES])
@pytest.mark.parametrize("M,Kd", R.FP8_CASES)
def test_fp8_gemm_ragged(M, Kd, dtype):
    from omr_a2s_multimodal_transformer_amd import kernels as K
    inp = R.fp8_inputs(M, Kd, dtype)
    x = inp["x_buf"].to(DEV)[:M, :Kd]
    a8, sa = K.quantize_rows_fp8(x)
    w8, sw = K.quantize_rows_fp8(inp["w"].to(DEV))
    want8, want_s = R.fp8_quantize_standin(inp["x_buf"][:M, :Kd])
    assert_bit_equal(sa.cpu(), want_s, "activation scales vs absmax / 448 in fp32")
    assert_bit_equal(sw.cpu(), R.fp8_scale_ref(inp["w"]), "weight scales vs absmax / 448 in fp32")
    assert torch.equal(a8.cpu()[:, :Kd], want8), "codes vs (x / scale).to(float8_e4m3fn)"
    if M > 1:
        assert float(sa[M - 1]) == 1.0 and not bool(a8[M - 1].any())
    cbuf = torch.full((M + 2, R.FP8_N + 8), SENTINEL, dtype=dtype, device=DEV)
    K.gemm_fp8(a8, sa, w8, sw, bias=inp["bias"].to(DEV), out=cbuf[:M, :R.FP8_N])
    c = cbuf.cpu()
    assert R.fp8_gemm_check(M, Kd, a8, sa, w8, sw, inp["bias"], c[:M, :R.FP8_N], dtype, who="gpu ") <= 1.0
    c[:M, :R.FP8_N] = SENTINEL
    assert _is_sentinel(c), "the fp8 GEMM wrote outside its C view"
