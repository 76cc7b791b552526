"""Branch-level tests of the generic GEMM (gemm.hip) and the element-wise, normalisation and loss kernels around it, against the
fp64 references and derived bounds of oracle/kernel_refs.py.  Every shape is the smallest that reaches its branch; the case
table is shared with tests/test_kernel_refs_cpu.py, which shows on the CPU that a correct implementation passes each check.
DESIGN.md ("Kernel branch coverage") maps each kernel instantiation and branch to the test id here that reaches it."""
import pytest
import torch

from oracle import kernel_refs as KR

pytestmark = pytest.mark.gpu

F32, BF16 = KR.F32, KR.BF16


def dev():
    return torch.device("cuda:0")


def K():
    from omr_a2s_multimodal_transformer_amd import kernels
    return kernels


def ids(cases):
    return [c.name for c in cases]


def dtype_id(dt):
    return KR.TAG[dt]


# ------------------------------------------------------------------------------------------------ GEMM

def run_gemm(case, drop=None):
    """The case's GEMM on device copies of its padded buffers -> (whole C buffer, column sums or None)."""
    inp = KR.gemm_inputs(case)
    a_buf, b_buf, c_buf = inp["a_buf"].to(dev()), inp["b_buf"].to(dev()), inp["c_buf"].to(dev())
    cs = inp["colsum0"].to(dev()) if case.colsum else None
    K().gemm(KR.view2d(a_buf, *inp["a_shape"]), KR.view2d(b_buf, *inp["b_shape"]), trans_a=case.ta, trans_b=case.tb,
             bias=None if inp["bias"] is None else inp["bias"].to(dev()), relu=case.relu, out=KR.view2d(c_buf, case.M, case.N),
             accumulate=case.accumulate, split_k=case.split_k, colsum_a=cs, drop=drop)
    return c_buf, cs


@pytest.mark.parametrize("case", KR.GEMM_PRODUCT_CASES, ids=ids(KR.GEMM_PRODUCT_CASES))
def test_gemm_product(case):
    """All four (trans_a, trans_b) x three type pairs x K in {45 (FULLK where there is one), 301 (pipelined)}: M = 130 is two M tiles
    with a 2-row tail, N = 70 one ragged N tile, every operand row ends in a partial 16-byte chunk followed by NaN padding.
    Error <= 4 (K + 2) 2^-24 sum |a||b| (+ 2^-8 |ref| for bf16 C); nothing outside the logical C is written."""
    KR.gemm_check(case, *run_gemm(case))


@pytest.mark.parametrize("case", KR.GEMM_EPILOGUE_CASES, ids=ids(KR.GEMM_EPILOGUE_CASES))
def test_gemm_epilogue(case):
    """bias + ReLU; accumulate onto a random C (bf16 C included); ldc % 8 == 0 with N = 70 (vector stores and a scalar row tail)."""
    KR.gemm_check(case, *run_gemm(case))


@pytest.mark.parametrize("case", KR.GEMM_SPLIT_CASES, ids=ids(KR.GEMM_SPLIT_CASES))
def test_gemm_split_k(case):
    """K = 100 over split_k in {2, 4}: a short last split (fp32), fewer splits than requested (bf16).  With a bias and a non-zero C
    to accumulate onto, a bias added once per split is an error of |bias|, far over the bound."""
    KR.gemm_check(case, *run_gemm(case))


@pytest.mark.parametrize("case", KR.GEMM_COLSUM_CASES, ids=ids(KR.GEMM_COLSUM_CASES))
def test_gemm_colsum(case):
    """Fused column sums of a transposed A with two N tiles (only tile.n == 0 may add them), onto a non-zero buffer, split_k in {1, 3}."""
    KR.gemm_check(case, *run_gemm(case))


@pytest.mark.parametrize("case", KR.GEMM_DROPOUT_CASES, ids=ids(KR.GEMM_DROPOUT_CASES))
def test_gemm_fused_dropout_padded_ldc(case):
    """The epilogue's dropout index is row * ldc + col: with ldc > N the fused result equals omr_dropout over the plain GEMM's whole
    padded [M, ldc] buffer, restricted to the logical columns, to the bit."""
    p, seed = case.drop
    plain, _ = run_gemm(case)
    fused, _ = run_gemm(case, drop=case.drop)
    want = K().dropout(plain[:case.M], p, seed)
    assert want.shape == (case.M, case.ld_c) and case.ld_c > case.N
    KR.assert_bit_equal(fused[:case.M, :case.N].cpu(), want[:, :case.N].cpu(), f"gemm {case.name}")
    KR.assert_outside_untouched(fused, KR.gemm_inputs(case)["c_buf"], case.M, case.N, f"gemm {case.name}")
    kept = (fused[:case.M, :case.N] != 0).float().mean().item()
    assert 0.2 < kept < 0.6                                          # ReLU halves, dropout keeps 3/4: the mask was applied at all


def test_gemm_refusals():
    """Argument combinations the entry refuses, before anything is launched (the output keeps its sentinel)."""
    k = K()
    a, b = torch.zeros((16, 8), device=dev()), torch.zeros((24, 8), device=dev())
    at = torch.zeros((8, 16), device=dev())
    c = torch.full((16, 24), KR.SENTINEL, device=dev())
    cb = torch.full((16, 24), KR.SENTINEL, device=dev(), dtype=BF16)
    cs = torch.full((16,), KR.SENTINEL, device=dev())
    bad = [
        dict(a=at, kw=dict(trans_a=True, drop=(0.5, 1), out=c)),
        dict(a=a, kw=dict(accumulate=True, drop=(0.5, 1), out=c)),
        dict(a=a, kw=dict(split_k=2, drop=(0.5, 1), out=c)),
        dict(a=a.to(BF16), b=b.to(BF16), kw=dict(split_k=2, out=cb)),
    ]
    refused = "omr_gemm failed: invalid argument"
    for q in bad:
        with pytest.raises(RuntimeError, match=refused):
            k.gemm(q["a"], q.get("b", b), **q["kw"])
    from omr_a2s_multimodal_transformer_amd._lib import cur_stream, dtype_code, lib, ptr
    assert len(lib().fns["omr_gemm"].argtypes) == 25, "omr_gemm's prototype changed: update the direct call below"
    with pytest.raises(RuntimeError, match=refused):                 # colsum_a without trans_a: the wrapper asserts first, so call the entry
        lib().call("omr_gemm", dtype_code(F32), dtype_code(F32), 0, 0, 16, 24, 8, ptr(a), 8, ptr(b), 8, ptr(c), 24, None, 0, 0, 1, ptr(cs), 0.0, 0,
                   0, 0, 0, 0, cur_stream())
    torch.cuda.synchronize()
    for t in (c, cb, cs):
        assert bool((t == t.flatten()[0]).all()) and float(t.flatten()[0]) == float(torch.tensor(KR.SENTINEL, dtype=t.dtype))


# ------------------------------------------------------------------------------------------------ element-wise, past the grid cap

@pytest.mark.parametrize("dtype", KR.DTYPES, ids=dtype_id)
def test_add_relu_bwd_second_sweep(dtype):
    """n = (2048 * 256 + 37) * VEC + 5: 37 threads run the vector loop twice and block 0 handles a scalar tail.  One rounded operation each."""
    inp = KR.add_relu_inputs(dtype)
    a, b = inp["a"].to(dev()), inp["b"].to(dev())
    KR.assert_bit_equal(K().add(a, b).cpu(), inp["add"], "add")
    KR.assert_bit_equal(K().relu_bwd(a, b, inp["scale"]).cpu(), inp["relu_bwd"], "relu_bwd")


def test_cast_round_trip():
    """fp32 -> bf16 -> fp32 equals torch's .to(): +-0, the largest finite bf16, exact ties (to even), subnormals, at both ends of a
    buffer longer than one capped launch; fp32 -> fp32 and bf16 -> bf16 copy the bits."""
    x = KR.cast_inputs()["x"]
    xg = x.to(dev())
    lo = K().cast(xg, BF16)
    KR.assert_bit_equal(lo.cpu(), x.to(BF16), "cast fp32 -> bf16")
    KR.assert_bit_equal(K().cast(lo, F32).cpu(), x.to(BF16).float(), "cast bf16 -> fp32")
    KR.assert_bit_equal(K().cast(xg, F32).cpu(), x, "cast fp32 -> fp32")
    KR.assert_bit_equal(K().cast(lo, BF16).cpu(), x.to(BF16), "cast bf16 -> bf16")


@pytest.mark.parametrize("dtype", KR.DTYPES, ids=dtype_id)
def test_dropout_flat_second_sweep(dtype):
    """Deterministic; kept values are x / (1 - p) rounded once; n = (2048 * 256 + 37) * VEC + 5, and the mask of the first 2048 * 256 * VEC elements equals that of
    a call on just that prefix (the element index is 64-bit and independent of the launch); keep rate within 4 binomial sigma."""
    case = KR.DropCase(dtype)
    x = KR.dropout_flat_input(dtype)
    xg = x.to(dev())
    n0 = KR.EW_CAP * KR.VEC[dtype]
    out = K().dropout(xg, case.p, case.seed)
    KR.dropout_flat_check(case, x, out, K().dropout(xg, case.p, case.seed), K().dropout(xg[:n0].contiguous(), case.p, case.seed))


@pytest.mark.parametrize("dtype", KR.DTYPES, ids=dtype_id)
def test_dropout_channel_mode(dtype):
    """B = 3, C = 24 (fp32) / 40 (bf16), 7 x 5 pixels: one decision per (sample, channel), different between samples."""
    x = KR.dropout_channel_input(dtype)
    KR.dropout_channel_check(x, K().dropout(x.to(dev()), 0.5, 77, channel_mode=True), 0.5)


@pytest.mark.parametrize("lowp", [False, True], ids=["fp32-only", "bf16-copy"])
def test_adam_second_sweep(lowp):
    """n = 2048 * 256 + 77, three steps, grad_scale = 0.5 against the fp64 recurrence; the bf16 copy is the rounded parameter."""
    inp, h = KR.adam_inputs(), KR.ADAM
    p = inp["p"].to(dev())
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    lp = torch.full((KR.ADAM_N,), float("nan"), dtype=BF16, device=dev()) if lowp else None
    for step, g in enumerate(inp["grads"], start=1):
        K().adam_step(p, g.to(dev()), m, v, step, h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], grad_scale=h["grad_scale"], p_lowp=lp)
    KR.adam_check(p, lp)


# ------------------------------------------------------------------------------------------------ element-wise, row-wise entries

@pytest.mark.parametrize("dtype", KR.DTYPES, ids=dtype_id)
def test_colsum_padded(dtype):
    """M = 300 (three row slabs, the last short), N = 70 (a ragged column block), ld = 72 with NaN in the padding, db non-zero."""
    inp = KR.colsum_inputs(dtype)
    db = inp["db0"].to(dev())
    K().colsum_into(KR.view2d(inp["buf"].to(dev()), KR.COLSUM_M, KR.COLSUM_N), db)
    KR.colsum_check(dtype, db)


@pytest.mark.parametrize("n", [30, 600])
def test_argmax_rows(n):
    """rows > 1 with ld > n.  n = 30: threads without an element, a maximum in the last column, a tie, an all -inf row (index 0),
    larger values behind the row, an all-NaN row (index 0, inside [0, n)).  n = 600: ties across threads and loop iterations."""
    inp = KR.argmax_inputs(n)
    x = inp["buf"].to(dev())[:, :n]
    idx, val = K().argmax(x)
    assert 0 <= int(idx[4]) < n, f"all-NaN row: index {int(idx[4])} is outside [0, {n})"
    KR.argmax_check(n, idx, val)
    rows = [i for i in range(5) if inp["finite"][i]]
    fin = inp["buf"][rows].to(dev())[:, :n]                          # the finite rows, same row stride
    tidx, _ = K().topk_logprob(fin, 1)
    assert tidx[:, 0].tolist() == [inp["expect"][i] for i in rows]


def test_weighted_argmax_all_nan_row():
    """The same selection in weighted_argmax_kernel: a row pair on which no comparison succeeds gives index 0, also in tokens_out."""
    n = 30
    la, lb = KR.rnd((2, 40), 71).to(dev()), KR.rnd((2, 40), 72).to(dev())
    la[0, 7] = lb[0, 7] = 10.0
    la[1, :n] = float("nan")
    tok = torch.full((2,), -7, dtype=torch.int64, device=dev())
    idx, _ = K().weighted_argmax_rows(la[:, :n], lb[:, :n], 0.5, tokens_out=tok)
    assert idx.tolist() == [7, 0] and tok.tolist() == [7, 0]


@pytest.mark.parametrize("dtype", KR.DTYPES, ids=dtype_id)
def test_embed_pe_second_sweep_and_bad_tokens(dtype):
    """M d = 524 800 elements (past the grid cap); tokens -1 and V give the positional encoding alone.  One rounded add."""
    inp = KR.embed_fwd_inputs(dtype)
    out = K().embed_pe(inp["tok"].to(dev()), inp["table"].to(dev()), inp["pe"].to(dev()))
    KR.assert_bit_equal(out.cpu(), inp["want"], "embed + pe")


@pytest.mark.parametrize("dtype", KR.DTYPES, ids=dtype_id)
def test_embed_bwd_duplicates_and_bad_tokens(dtype):
    """4096 rows over 5 distinct tokens plus pad, -1 and V against an fp64 index_add; the pad row stays exactly zero."""
    inp = KR.embed_bwd_inputs(dtype)
    dtab = torch.zeros((KR.EMB_V, KR.EMB_D), device=dev())
    K().embed_bwd(inp["tok"].to(dev()), inp["dout"].to(dev()), dtab, KR.EMB_PAD)
    KR.embed_bwd_check(dtype, dtab)


@pytest.mark.parametrize("dtype,C", KR.ADD_PE2D_CASES, ids=[f"{KR.TAG[dt]}-C{C}" for dt, C in KR.ADD_PE2D_CASES])
def test_add_pe2d_narrow(dtype, C):
    """h < maxh, w < maxw; C = 12 (bf16) and C = 18 (fp32) select the scalar kernel, C = 20 (fp32) the vector one.  One rounded add."""
    inp = KR.add_pe2d_inputs(dtype, C)
    KR.assert_bit_equal(K().add_pe2d(inp["x"].to(dev()), inp["pe"].to(dev())).cpu(), inp["want"], "add_pe2d")


# ------------------------------------------------------------------------------------------------ LayerNorm

@pytest.mark.parametrize("case", KR.LN_CASES, ids=ids(KR.LN_CASES))
def test_add_layernorm(case):
    """d in {128, 256, 512 (PER = 8)} x M in {1, 3 (decode), 65 (one row past a 64-row backward block)}, with and without the
    residual.  Rows are 100 + 0.1 u (a one-pass variance in fp32 fails here) plus one all-equal row (out = beta, rstd = 1/sqrt(eps));
    dgamma / dbeta start non-zero."""
    inp = KR.ln_inputs(case)
    k = K()
    x, res = inp["x"].to(dev()), None if inp["res"] is None else inp["res"].to(dev())
    gamma, beta = inp["gamma"].to(dev()), inp["beta"].to(dev())
    out, mean, rstd = k.add_layernorm_fwd(x, res, gamma, beta, eps=KR.LN_EPS)
    dg, db = inp["dgamma0"].to(dev()), inp["dbeta0"].to(dev())
    ds = k.add_layernorm_bwd(inp["dy"].to(dev()), x, res, gamma, mean, rstd, dg, db)
    KR.ln_check(case, out, mean, rstd, ds, dg, db)


@pytest.mark.parametrize("dtype", KR.DTYPES, ids=dtype_id)
def test_add_layernorm_fused_dropout_d512(dtype):
    """test_add_layernorm_fused_dropout_matches_dropout_then_add_ln (tests/test_kernels_gpu.py) at d = 512, M = 65."""
    M, d, p, seed = 65, 512, 0.3, 1234
    k = K()
    x, res = KR.rnd((M, d), 25).to(dev(), dtype), KR.rnd((M, d), 26).to(dev(), dtype)
    gamma, beta = (KR.rnd((d,), 27) + 1.5).to(dev()), KR.rnd((d,), 28).to(dev())
    xd = k.dropout(x, p, seed)
    ref, mean0, rstd0 = k.add_layernorm_fwd(xd, res, gamma, beta)
    out, mean, rstd = k.add_layernorm_fwd(x, res, gamma, beta, drop_p=p, drop_seed=seed)
    assert torch.equal(out, ref) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
    g = KR.rnd((M, d), 29).to(dev(), dtype)
    dg0, db0 = torch.zeros(d, device=dev()), torch.zeros(d, device=dev())
    ds0 = k.add_layernorm_bwd(g, xd, res, gamma, mean0, rstd0, dg0, db0)
    dg, db = torch.zeros(d, device=dev()), torch.zeros(d, device=dev())
    ds, dx = k.add_layernorm_bwd(g, x, res, gamma, mean, rstd, dg, db, drop_p=p, drop_seed=seed)
    assert torch.equal(ds, ds0)
    assert torch.equal(dx, k.dropout(ds0, p, seed))
    torch.testing.assert_close(dg, dg0, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(db, db0, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ InstanceNorm

@pytest.mark.parametrize("case", KR.IN_CASES + KR.IN_CONST_CASES, ids=ids(KR.IN_CASES + KR.IN_CONST_CASES))
def test_instnorm(case):
    """C in {32, 64} and the narrowest widths (8 in bf16, 4 in fp32) x HW in {1, 3 (fewer pixels than pixel phases), 333}, B = 2,
    with and without the ReLU mask; and a constant image of 0.7, whose one-pass variance reaches the var < 0 clamp: mean = 0.7 to
    fp32 rounding, rstd = 1 / sqrt(eps) within 1e-6, finite backward."""
    inp = KR.in_inputs(case)
    k = K()
    x, g = inp["x"].to(dev()), inp["g"].to(dev())
    mean, rstd = k.instnorm_stats(x, eps=KR.IN_EPS)
    dx = k.instnorm_bwd(g, x, mean, rstd, relu_mask=False)
    dxm = k.instnorm_bwd(g, x, mean, rstd, relu_mask=True, relu_scale=2.0)
    KR.in_check(case, mean, rstd, dx, dxm)


# ------------------------------------------------------------------------------------------------ cross-entropy

def run_ce(case):
    inp = KR.ce_inputs(case)
    buf, tgt = inp["buf"].to(dev()), inp["tgt"].to(dev())
    logits = buf[:, :case.V]
    loss, lse, acc2 = K().ce_fwd(logits, tgt, case.V, KR.CE_PAD)
    dl = K().ce_bwd(logits, tgt, lse, acc2, case.V, KR.CE_PAD, grad_scale=KR.CE_GRAD_SCALE,
                    grad_out=torch.tensor([KR.CE_GRAD_OUT], device=dev()))
    KR.ce_check(case, loss, lse, acc2, dl if dl._base is None else dl._base)


@pytest.mark.parametrize("case", KR.CE_CASES, ids=ids(KR.CE_CASES))
def test_cross_entropy(case):
    """V = 6997 contiguous (ldv odd: the scalar path) and in a padded buffer (the vector path, NaN in the padding), V = 30 (most
    threads idle), M = 1030 (the finalize loop runs twice).  Logits 80 + 30 u (fp32) / 20 + 8 u (bf16) with a lone spike of +60:
    exp overflows without the running maximum.  Targets include pad, -1 and V; grad_scale = 0.5 and a device grad_out = 3."""
    run_ce(case)


@pytest.mark.parametrize("case", KR.CE_INF_CASES, ids=ids(KR.CE_INF_CASES))
def test_cross_entropy_neg_inf_logits(case):
    """-inf in columns 0..15 and in one column past 256, and a row that is -inf except for one entry (V = 301 on both paths, and
    V = 2101 padded, where a vector-path thread has a second chunk after its -inf one): lse is the fp64 logsumexp
    (finite), dlogits is finite and 0 at the -inf columns.  A thread whose first values are all -inf used to compute
    exp(-inf - -inf) = NaN."""
    run_ce(case)
