"""The case table of oracle/gemm_refs.py (panel, tall and grouped weight-gradient GEMMs, the row-group views of omr_gemm) without a
GPU: torch CPU arithmetic in the kernels' formats stands in for the kernels.  Every EXACT case meets the two conditions its
exactness rests on (sums of |products| below 2^24; |ref| <= 256 for a bf16 C), every case meets the acceptance conditions of the
kernel it is named for (the mirrors of the launchers; the library does not report the kernel that ran, so this is all a route
claims), a correct stand-in passes every check, and each of a list of subtly wrong ones fails the case built for it -- which is
what shows that the checks tests/test_gemm_branches_gpu.py shares with this file can see them.

The references are float64 products on the CPU: about 7 GFLOP for the largest case, a fraction of a second on 16 threads."""
import pytest
import torch

from oracle import gemm_refs as R

F32, BF16 = R.F32, R.BF16


def ids(cases):
    return [c.name for c in cases]


EXACT = [c for c in R.CASES if c.exact]


# ------------------------------------------------------------------------------------------------ conditions and routes

@pytest.mark.parametrize("c", EXACT, ids=ids(EXACT))
def test_exact_case_meets_its_conditions(c):
    R.assert_exact_conditions(c)
    inp = R.inputs(c)
    # what surrounds the operands is NaN, what surrounds C the sentinel
    assert torch.isnan(inp["a"]._base[:R.GUARD]).all() and torch.isnan(inp["a"]._base[-R.GUARD:]).all() and torch.isnan(inp["a"]._base[:, c.a_shape[1]:]).all()
    assert torch.isnan(inp["b"]._base[:R.GUARD]).all() and torch.isnan(inp["b"]._base[-R.GUARD:]).all() and torch.isnan(inp["b"]._base[:, c.b_shape[1]:]).all()
    assert c.lda > c.a_shape[1] and c.ldb > c.b_shape[1] and c.ldc > c.N and inp["c_buf"].shape[0] > c.M
    if c.operand in (1, 2):
        n = c.N if c.operand == 1 else c.K
        outside = torch.ones(R.phys_rows(n, c.group), dtype=torch.bool)
        outside[R.group_rows(n, c.group)] = False
        assert int(outside.sum()) == n // 2 and torch.isnan(inp["b"][outside]).all()                   # the Q rows: a third of every block
        if c.bias:
            assert torch.isnan(inp["bias"][outside]).all() and torch.isfinite(inp["bias"][~outside]).all()


@pytest.mark.parametrize("c", R.CASES, ids=ids(R.CASES))
def test_case_reaches_the_kernel_it_is_named_for(c):
    assert R.gemm_route(c) == c.route
    if c.fullk is not None:
        assert R.tile_fullk(c) == c.fullk
    assert c.splits == (3 if c.split_k == 3 else 1)
    if c.route == "tall" and c.operand == 2:
        assert c.group[0] // R.TALL_BK == 2                              # two k-tiles per group: the group changes on every other tile
    if c.route == "panel":
        assert (c.N // R.PANEL_PN) % 2 == (1 if c.name.startswith("P2") else 0)


def test_tall_cases_walk_the_tiles_they_name():
    t1, t2, t3, t4 = (R.tall_plan(c.M) for c in R.TALL_CASES)
    assert t1 == dict(tiles=192, grid=192, busiest=1, second_sweep=0, last_rows=256, last_tile_owner=191)          # the fewest the kernel takes
    for p in (t2, t3):
        assert p["tiles"] == 258 and p["grid"] == 256 and p["busiest"] >= 2 and p["second_sweep"] == 2
        assert p["last_rows"] == 37 and p["last_tile_owner"] == 1        # the ragged tile is the second tile of workgroup 1
    assert t4["tiles"] == 193 and t4["last_rows"] == 5
    assert R.TALL_CASES[0].K // R.TALL_BK == 1 and R.TALL_CASES[1].K // R.TALL_BK == 3 > R.TALL_NST
    # the neighbours miss one condition each
    assert R.tall_plan(R.TALL_NEIGHBOURS[1].M)["tiles"] == R.TALL_MIN_TILES - 1 and R.TALL_NEIGHBOURS[0].K % R.TALL_BK


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_grouped_problems_reach_the_branches_they_name(dtype):
    probs = R.DW_CALLS["25-problems"][0]
    plan = R.dw_plan([q.shape for q in probs], dtype)
    assert len(probs) == R.DW_MAX + 1
    assert [p["table"] for p in plan] == [0] * R.DW_MAX + [1] and plan[R.DW_MAX]["block0"] == 0 and plan[1]["block0"] > 0
    assert all(b["block0"] == a["block0"] + a["blocks"] for a, b in zip(plan[:R.DW_MAX - 1], plan[1:R.DW_MAX]))
    assert plan[0]["splits"] == 1 and probs[0].rows <= 512
    assert sum(p["splits"] > 1 for p in plan) >= 12 and plan[4]["splits"] == 4 and plan[R.DW_MAX]["splits"] == 3
    bk = R.bk_of(dtype)
    assert probs[2].rows % 64 and probs[2].rows % 32 and probs[3].rows == 513 and plan[3]["splits"] == 2 and plan[3]["last_split_rows"] % bk == 1
    assert probs[3].n_out == 50 and probs[2].n_in % R.TILE and plan[3]["nt"] == 2 and plan[R.DW_MAX]["mt"] * plan[R.DW_MAX]["nt"] == 4
    assert not probs[4].db and probs[5].group and any(q.ld_dw > q.n_in for q in probs) and any(q.pad for q in probs) and not probs[2].pad
    single = R.dw_plan([q.shape for q in R.DW_CALLS["single-problem"][0]], dtype)
    assert len(single) == 1 and single[0]["splits"] == 8


# ------------------------------------------------------------------------------------------------ a correct implementation passes

@pytest.mark.parametrize("c", R.CASES, ids=ids(R.CASES))
def test_standin_meets_every_check(c):
    r = R.check(c, *R.standin(c))
    assert (r is None) == c.exact


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("call", list(R.DW_CALLS))
def test_grouped_standin_meets_every_check(call, dtype):
    R.dw_check(call, dtype, R.dw_standin(call, dtype))


# ------------------------------------------------------------------------------------------------ wrong implementations do not

def caught(name, fault):
    c = R.case(name)
    with pytest.raises(AssertionError):
        R.check(c, *R.standin(c, fault))


def passes(name, fault):
    c = R.case(name)
    R.check(c, *R.standin(c, fault))


@pytest.mark.parametrize("fault,name", [
    ("drop_last_ktile", "T2"),               # three k-tiles, the last one alone in the ring
    ("stale_ktile", "T2"),                   # k-tile 2 reuses the stage of k-tile 0
    ("stale_ktile", "T3"),
    ("second_sweep_repeats", "T2"),          # tiles 256 and 257: the second tiles of workgroups 0 and 1
    ("second_sweep_repeats", "T3"),
    ("chunk_permute", "T1"),                 # one swizzle class of rows in every tile
    ("ignore_group_base", "T3"),             # the Q rows are NaN
    ("write_past_M", "T2"),                  # row M of the C buffer holds the sentinel
])
def test_wrong_tall_gemm_is_caught(fault, name):
    caught(name, fault)


def test_accumulator_rounded_between_ktiles_is_caught_by_the_bounded_case_only():
    """Every partial sum of an EXACT case is an integer of at most 256 in size: a bf16 number, which the extra roundings leave
    alone.  Only T4, real-valued over ten k-tiles, sees an accumulator kept in bf16."""
    for name in ("T1", "T2", "T3"):
        passes(name, "round_between_ktiles")
    caught("T4", "round_between_ktiles")


@pytest.mark.parametrize("fault,name", [
    ("bias_next_tile", "P2"),
    ("bias_next_tile", "P3"),
    ("garbage_no_bias", "P1"),
    ("skip_last_tile", "P2"),                # the ninth tile: back in buffer 0
    ("skip_last_tile", "P1"),
    ("stale_c_image", "P1"),
    ("stale_c_image", "P2"),
    ("ignore_group_base", "P3"),
])
def test_wrong_panel_gemm_is_caught(fault, name):
    caught(name, fault)


@pytest.mark.parametrize("name", ["G1-f32", "G1-bf16", "G2-f32-operand2-k256", "G2-bf16-operand2-k256", "G2-f32-operand2-k384", "G2-bf16-operand2-k384"])
def test_tile_kernel_that_ignores_the_group_base_is_caught(name):
    caught(name, "ignore_group_base")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("fault", ["skip_25th", "missing_last_tile", "split_k_tail", "db_two_n_tiles", "ignore_group_base"])
def test_wrong_grouped_weight_gradient_is_caught(fault, dtype):
    with pytest.raises(AssertionError):
        R.dw_check("25-problems", dtype, R.dw_standin("25-problems", dtype, fault))


def test_one_wrong_element_is_caught():
    """The point of bit equality at every element: one unit in one element of 17 million, which a relative norm (or 350 sampled rows)
    lets through."""
    c = R.case("T2")
    c_buf, _ = R.standin(c)
    c_buf[40000, 131] += 1.0
    with pytest.raises(AssertionError):
        R.check(c, c_buf)
    res = R.dw_standin("25-problems", F32)
    res[1][0][200, 77] += 1.0
    with pytest.raises(AssertionError):
        R.dw_check("25-problems", F32, res)
