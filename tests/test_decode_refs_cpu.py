"""CPU-only: the decode case table of oracle/decode_refs.py with torch CPU arithmetic standing in for the kernels.

Every check tests/test_decode_branches_gpu.py makes on the HIP kernels is made here on `lin_standin` / `sel_standin` /
`fp8_quantize_standin`: fp32 products without fma, summed in another order, rounded once to T.  A correct implementation meets
every bound; each damaged one (DAMAGES of oracle/decode_refs.py) is rejected by the case that is there for it."""
import pytest
import torch

from oracle import decode_refs as R
from oracle.kernel_refs import BF16, DTYPES, F32, TAG


@pytest.mark.parametrize("case", R.LIN_CASES, ids=R.case_id)
def test_a_correct_row_linear_meets_every_check(case):
    out = R.lin_standin(case)
    r = R.lin_check(case, out, ln_rows=R.ln_standin_rows(case) if case.pro == 1 else None, who="cpu ")
    assert r <= 1.0


def test_the_case_table_reaches_what_it_names():
    by = R.CASE
    assert by["chunk-f32-k512"].cpt == 8 and by["chunk-f32-k576"].cpt == 9
    for k in ("bf16", "f32-e4m3", "bf16-e4m3"):
        assert by[f"chunk-{k}-k1024"].cpt == 8 and by[f"chunk-{k}-k1152"].cpt == 9
    assert by["big-f32-k2048"].cpt == 32 and by["big-bf16-k2048"].cpt == 16 and by["big-f32-k2048"].M == 9
    assert {c.K // 64 for c in R.PRO_CASES} == {2, 4, 8}
    assert (R.PICK_N + 15) // 16 == 65 and R.PICK_N % 16 == 5
    for H, hd, ns in R.MERGE_SHAPES:
        assert ns <= R.MAXSPLIT and H * ns <= R.MAXHS and hd % (H * hd // 64) == 0
    assert max(H * ns for H, _, ns in R.MERGE_SHAPES) == R.MAXHS and any(ns % 4 for _, _, ns in R.MERGE_SHAPES)
    assert set(R.ROWS_POS) >= {0, R.ROWS_MAXLEN - 1} and len(set(R.ROWS_POS)) < len(R.ROWS_POS)


DAMAGED = [
    # (damage, case that must reject it, cases it cannot touch)
    ("drop_last_klane", "inst-f32-bias-relu"), ("drop_last_klane", "inst-bf16-nobias"), ("drop_last_klane", "inst-f32-e4m3-nobias"),
    ("drop_last_klane", "chunk-bf16-e4m3-k1152"), ("drop_last_klane", "big-bf16-k2048"),
    ("drop_post_prefetch", "chunk-f32-k576"), ("drop_post_prefetch", "chunk-bf16-k1152"), ("drop_post_prefetch", "chunk-f32-e4m3-k1152"),
    ("drop_post_prefetch", "chunk-bf16-e4m3-k1152"), ("drop_post_prefetch", "big-f32-k2048"), ("drop_post_prefetch", "big-bf16-k2048"),
    ("swap_code_halves", "inst-f32-e4m3-bias-relu"), ("swap_code_halves", "inst-bf16-e4m3-nobias"), ("swap_code_halves", "chunk-f32-e4m3-k1024"),
    ("shift_out1_row", "rows-f32"), ("shift_out1_row", "rows-bf16"),
    ("pick_last", "pick-f32-tie-one-wg"), ("pick_last", "pick-bf16-tie-two-wgs"), ("pick_last", "pick-f32-tie-two-sweeps"),
    ("pick_last", "pick-bf16-all-nan"), ("pick_last", "pick-f32-all-neginf"),
    ("merge_no_guard", "merge-f32-h4-hd32-s2"), ("merge_no_guard", "merge-bf16-h8-hd64-s64"), ("merge_no_guard", "merge-f32-h2-hd64-s33"),
]


@pytest.mark.parametrize("damage,name", DAMAGED, ids=[f"{d}-{n}" for d, n in DAMAGED])
def test_a_damaged_row_linear_is_rejected(damage, name):
    case = R.CASE[name]
    out = R.lin_standin(case, damage)
    with pytest.raises(AssertionError):
        R.lin_check(case, out, ln_rows=None, who=f"cpu {damage} ")


def test_the_prefetch_damage_is_invisible_where_the_loop_is_empty():
    """cpt = 8: no chunk past the prefetched ones, so dropping them changes nothing -- the cpt = 9 cases are what reaches the loop."""
    for name in ("chunk-f32-k512", "chunk-bf16-k1024"):
        case = R.CASE[name]
        a, b = R.lin_standin(case), R.lin_standin(case, "drop_post_prefetch")
        assert torch.equal(a["out0_buf"].view(torch.int32 if case.dtype == F32 else torch.int16), b["out0_buf"].view(torch.int32 if case.dtype == F32 else torch.int16))


def test_the_old_pick_sentinel_is_rejected():
    """What the row path returned before the fix for a row on which no comparison succeeds: 0x7fffffff."""
    for name in ("pick-f32-all-nan", "pick-bf16-all-neginf"):
        case = R.CASE[name]
        out = R.lin_standin(case)
        out["idx"] = torch.full_like(out["idx"], R.NO_PICK)
        with pytest.raises(AssertionError):
            R.lin_check(case, out, who="cpu old pick ")


def test_merge_reference_limits():
    """The fp64 merge on the hand-made partials: the all-empty row is 0 with bound 0, the garbage of an empty split never shows,
    and on the underflow row only the last split counts."""
    for case in R.MERGE_CASES:
        H, hd, ns = case.merge
        ref, bound = R.merge_ref(case)
        assert torch.isfinite(ref).all() and bool((ref[1] == 0).all()) and bool((bound[1] == 0).all())
        assert float(ref.abs().max()) < 10.0                          # 7777 took no part
        p = R.merge_part(case).double().view(3, H, ns, hd + 2)
        last = (p[2, :, ns - 1, :hd] / p[2, :, ns - 1, hd + 1:]).reshape(-1)
        assert torch.allclose(ref[2], last, rtol=1e-12, atol=0)
        assert bool((bound[[0, 2]] > 0).all()) and float((bound[[0, 2]] / (ref[[0, 2]].abs() + 1e-30)).median()) < (1e-5 if case.dtype == F32 else 5e-3)


@pytest.mark.parametrize("mix", [False, True], ids=["topk", "weighted"])
@pytest.mark.parametrize("k", R.SEL_KS)
@pytest.mark.parametrize("n", R.SEL_NS)
def test_selection_rows(n, k, mix):
    idx, val = R.sel_standin(n, k, mix)
    assert R.sel_check(n, k, mix, idx, val, who="cpu ") <= 1.0
    if k >= 3:                                                        # a wrong tie rule, an index past the row, a value from elsewhere
        bad = idx.clone(); bad[1, 0], bad[1, 1] = idx[1, 1], idx[1, 0]
        with pytest.raises(AssertionError):
            R.sel_check(n, k, mix, bad, val, who="cpu swapped tie ")
        bad = idx.clone(); bad[4] = R.NO_PICK
        with pytest.raises(AssertionError):
            R.sel_check(n, k, mix, bad, val, who="cpu old all-NaN ")
        bad = val.clone(); bad[0, 2] = val[0, 2] + 1e-3
        with pytest.raises(AssertionError):
            R.sel_check(n, k, mix, idx, bad, who="cpu wrong value ")


@pytest.mark.parametrize("dtype", DTYPES, ids=[TAG[d] for d in DTYPES])
@pytest.mark.parametrize("M,K", R.FP8_CASES)
def test_fp8_ragged_gemm(M, K, dtype):
    inp = R.fp8_inputs(M, K, dtype)
    x = inp["x_buf"][:M, :K]
    a8, sa = R.fp8_quantize_standin(x)
    w8, sw = R.fp8_quantize_standin(inp["w"])
    if M > 1:
        assert float(sa[M - 1]) == 1.0 and not bool(a8[M - 1].any())
    c = ((R.e4m3_decode(a8).float() @ R.e4m3_decode(w8).float().t()) * sa[:, None] * sw[None] + inp["bias"]).to(dtype)
    assert R.fp8_gemm_check(M, K, a8, sa, w8, sw, inp["bias"], c, dtype, who="cpu ") <= 1.0
    with pytest.raises(AssertionError):                               # the last 16 codes of K left out
        c = ((R.e4m3_decode(a8).float()[:, :K - 16] @ R.e4m3_decode(w8).float()[:, :K - 16].t()) * sa[:, None] * sw[None] + inp["bias"]).to(dtype)
        R.fp8_gemm_check(M, K, a8, sa, w8, sw, inp["bias"], c, dtype, who="cpu short ")


def test_e4m3_table_equals_torch():
    codes = torch.arange(256, dtype=torch.uint8)
    t, want = R.e4m3_table(), codes.view(torch.float8_e4m3fn).double()
    assert torch.equal(torch.isnan(t), torch.isnan(want)) and torch.equal(t[~torch.isnan(t)], want[~torch.isnan(want)])
