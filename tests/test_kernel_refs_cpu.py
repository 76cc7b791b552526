"""CPU self-check of the kernel-branch case table (oracle/kernel_refs.py): torch CPU fp32 / bf16 arithmetic stands in for the HIP
kernels and must satisfy every bound and tolerance tests/test_kernel_branches_gpu.py applies, and each GEMM bound must
reject a stand-in that drops one k index or one output row.  No GPU needed."""
import pytest
import torch

from oracle import kernel_refs as KR

F32, BF16 = KR.F32, KR.BF16


def ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------ GEMM

@pytest.mark.parametrize("case", KR.GEMM_BOUND_CASES, ids=ids(KR.GEMM_BOUND_CASES))
def test_gemm_bound_holds_and_is_not_vacuous(case):
    c_buf, cs = KR.gemm_standin(case)
    KR.gemm_check(case, c_buf, cs)
    # a stand-in that loses the last k index (the one inside the partial 16-byte chunk) or the last row (the M tail) must fail
    for kw in (dict(drop_k=True), dict(drop_row=True)):
        bad, bad_cs = KR.gemm_standin(case, **kw)
        assert KR.gemm_ratio(case, bad) > 1.0, f"{case.name}: the bound accepts a product with {kw}"
        if case.colsum:
            assert KR.colsum_ratio(case, bad_cs) > 1.0, f"{case.name}: the column-sum bound accepts {kw}"
        KR.assert_outside_untouched(bad, KR.gemm_inputs(case)["c_buf"], case.M, case.N, case.name)


def test_gemm_case_table_reaches_the_listed_branches():
    names = set(ids(KR.GEMM_BOUND_CASES + KR.GEMM_DROPOUT_CASES))
    assert len(names) == len(KR.GEMM_BOUND_CASES) + len(KR.GEMM_DROPOUT_CASES) and len(KR.GEMM_PRODUCT_CASES) == 24
    for c in KR.GEMM_BOUND_CASES + KR.GEMM_DROPOUT_CASES:
        inp, vec = KR.gemm_inputs(c), KR.VEC[c.dtype]
        for buf, shape in ((inp["a_buf"], inp["a_shape"]), (inp["b_buf"], inp["b_shape"])):
            assert buf.stride(0) % vec == 0 and buf.shape[0] == shape[0] + 2
            assert bool(torch.isnan(buf[shape[0]:].float()).all()) and bool(torch.isnan(buf[:, shape[1]:].float()).all())
            if c.K in (45, 301):
                assert shape[1] % vec != 0, "every operand row ends in a partial 16-byte chunk"
        assert c.ld_c > c.N and (c.K > 4 * (64 if c.dtype == BF16 else 32)) == (c.K == 301)
    assert [c.ld_c % 8 for c in KR.GEMM_EPILOGUE_CASES if "ldc80" in c.name] == [0, 0, 0]


def test_gemm_outside_check_sees_a_stray_store():
    case = KR.GEMM_PRODUCT_CASES[0]
    c_buf, _ = KR.gemm_standin(case)
    c_buf[case.M, 0] = 0.0
    with pytest.raises(AssertionError):
        KR.gemm_check(case, c_buf)
    c_buf, _ = KR.gemm_standin(case)
    c_buf[0, case.N] = 0.0
    with pytest.raises(AssertionError):
        KR.gemm_check(case, c_buf)


# ------------------------------------------------------------------------------------------------ element-wise

@pytest.mark.parametrize("dtype", KR.DTYPES, ids=KR.TAG.get)
def test_bit_equal_expectations_are_single_roundings(dtype):
    # the vector loops see n / VEC vectors and 2048 * 256 threads: several threads must take a second sweep, and a tail must remain
    n, vec = KR.ew_n(dtype), KR.VEC[dtype]
    assert n // vec >= KR.EW_CAP + 8 and n % vec != 0 and KR.dropout_flat_input(dtype).numel() == n
    inp = KR.add_relu_inputs(dtype)
    assert inp["a"].numel() == n
    KR.assert_rounded_once(inp["add"], inp["add64"], dtype, "add")
    KR.assert_rounded_once(inp["relu_bwd"], inp["relu_bwd64"], dtype, "relu_bwd")
    e = KR.embed_fwd_inputs(dtype)
    bad = (e["tok"] < 0) | (e["tok"] >= KR.EMB_V)
    assert int(bad.sum()) == 4
    KR.assert_bit_equal(e["want"][bad], e["pe"][None].expand(2, -1, -1)[bad].to(dtype), "out-of-range tokens give pe alone")
    for dt, C in KR.ADD_PE2D_CASES:
        if dt == dtype:
            p = KR.add_pe2d_inputs(dt, C)
            KR.assert_rounded_once(p["want"], p["x"].double() + p["pe"][:3, :5].double(), dtype, "add_pe2d")
    assert [C % KR.VEC[dt] != 0 for dt, C in KR.ADD_PE2D_CASES] == [False, True, True]


def test_cast_specials():
    inp = KR.cast_inputs()
    x = inp["x"]
    lo = x.to(BF16)
    back = lo.float()
    k = inp["nspecial"]
    got = KR.bits(back[:k]).tolist()
    u = lambda v: v - (1 << 32) if v >= (1 << 31) else v          # noqa: E731
    assert got[:12] == [u(v) for v in (0x00000000, 0x80000000, 0x7F7F0000, 0xFF7F0000, 0x3F800000, 0x3F820000, 0x3F810000, 0x3F800000,
                                       0xBF800000, 0xBF820000, 0x7F800000, 0x7F7F0000)]
    assert x.numel() > KR.EW_CAP + k and KR.ADAM_N > KR.EW_CAP and torch.equal(KR.bits(back[-k:]), KR.bits(back[:k]))


@pytest.mark.parametrize("dtype", KR.DTYPES, ids=KR.TAG.get)
def test_dropout_checks_hold_for_the_documented_mask(dtype):
    case = KR.DropCase(dtype)
    x = KR.dropout_flat_input(dtype)
    out = KR.dropout_standin(x, case.p, case.seed)
    n0 = KR.EW_CAP * KR.VEC[dtype]
    KR.dropout_flat_check(case, x, out, out.clone(), KR.dropout_standin(x[:n0], case.p, case.seed))
    with pytest.raises(AssertionError):                             # a mask that restarts its index in the second sweep is caught
        KR.dropout_flat_check(case, x, out, out.clone(), torch.roll(out[:n0], 1))
    xc = KR.dropout_channel_input(dtype)
    KR.dropout_channel_check(xc, KR.dropout_standin(xc, 0.5, 77, channel_mode=True), 0.5)
    with pytest.raises(AssertionError):
        KR.dropout_channel_check(xc, KR.dropout_standin(xc, 0.5, 77), 0.5)


def test_adam_colsum_argmax_embed():
    p = KR.adam_standin()
    KR.adam_check(p, p.to(BF16))
    for dtype in KR.DTYPES:
        inp = KR.colsum_inputs(dtype)
        x = KR.view2d(inp["buf"], KR.COLSUM_M, KR.COLSUM_N).float()
        KR.colsum_check(dtype, inp["db0"] + x.sum(0))
        with pytest.raises(AssertionError):
            KR.colsum_check(dtype, inp["db0"] + x[:-1].sum(0))
        KR.embed_bwd_check(dtype, KR.embed_bwd_standin(dtype))
    for n in (30, 600):
        inp = KR.argmax_inputs(n)
        assert inp["finite"] == [True, True, n != 30, True, False]
        KR.argmax_check(n, *KR.argmax_standin(inp["buf"][:, :n]))


# ------------------------------------------------------------------------------------------------ norms

@pytest.mark.parametrize("case", KR.LN_CASES, ids=ids(KR.LN_CASES))
def test_layernorm_tolerances_hold(case):
    KR.ln_check(case, *KR.ln_standin(case))


def test_layernorm_inputs_expose_a_one_pass_variance():
    """E[x^2] - mean^2 in fp32 on rows of 100 + 0.1 u is off by far more than the tolerance: the rows do tell the two apart."""
    case = KR.LnCase(512, 65, F32, True)
    inp = KR.ln_inputs(case)
    out, mean, rstd, ds, dg, db = KR.ln_standin(case)
    s = inp["x"] + inp["res"]
    rstd1 = torch.rsqrt(((s * s).mean(1) - mean * mean).clamp_min(0.0) + KR.LN_EPS)
    with pytest.raises(AssertionError):
        KR.ln_check(case, out, mean, rstd1, ds, dg, db)


def test_layernorm_bf16_rows_are_held_to_one_rounding():
    """An error of 0.1 on a bf16 output passes the project tolerance at this scale (3e-2 * 43) but not the rounded-once check."""
    case = KR.LnCase(256, 65, BF16, True)
    out, mean, rstd, ds, dg, db = KR.ln_standin(case)
    bad = (out.float() + 0.1).to(BF16)
    KR.check_close(bad, KR.ln_fwd_ref(case)[0], BF16, case.scale, "project tolerance")
    with pytest.raises(AssertionError):
        KR.ln_check(case, bad, mean, rstd, ds, dg, db)


@pytest.mark.parametrize("case", KR.IN_CASES + KR.IN_CONST_CASES, ids=ids(KR.IN_CASES + KR.IN_CONST_CASES))
def test_instnorm_tolerances_hold(case):
    mean, rstd = KR.in_standin(case)
    KR.in_check(case, mean, rstd, KR.in_standin(case, mean, rstd), KR.in_standin(case, mean, rstd, True, 2.0))


# ------------------------------------------------------------------------------------------------ cross-entropy

@pytest.mark.parametrize("case", KR.CE_CASES + KR.CE_INF_CASES, ids=ids(KR.CE_CASES + KR.CE_INF_CASES))
def test_cross_entropy_tolerances_hold(case):
    ref = KR.ce_ref(case)
    assert torch.isfinite(ref["lse"]).all() and torch.isfinite(ref["dlogits"]).all()
    KR.ce_check(case, *KR.ce_standin(case))
    if not case.inf:
        assert ref["count"] == case.M - 4 and case.M > 1024
