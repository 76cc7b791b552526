"""CPU-only: the references of tests/ctc_refs.py held to torch -- the fp64 loss and gradient to F.ctc_loss and its autograd, the frame map to
F.avg_pool2d + transpose, the greedy rule to a brute-force collapse -- and the case table's feasibility designations."""
import itertools

import numpy as np
import pytest
import torch

import ctc_refs as R
from oracle import kernel_refs as KR


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_reference_equals_torch_fp64(case):
    r = R.reference(case)
    loss, rows, g = R.torch_ctc(case, torch.float64)
    # torch's own fp64 recursion is un-normalised: one ulp of its largest |log alpha| is what it can resolve (module docstring)
    rel = 1e-12 * max(1.0, r["max_log"] / 100.0)
    assert abs(loss - r["loss"]) <= rel * max(abs(r["loss"]), 1e-300), (loss, r["loss"])
    assert np.all(np.abs(rows - r["rows"]) <= rel * np.maximum(np.abs(r["rows"]), 1e-300)), (rows, r["rows"])
    scale = np.abs(r["dlogits"]).max() if r["dlogits"].any() else 1.0
    assert np.abs(g - r["dlogits"]).max() <= rel * scale, (np.abs(g - r["dlogits"]).max(), scale)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_only_the_designated_samples_are_infeasible(case):
    r = R.reference(case)
    assert [b for b in range(case.B) if not r["feasible"][b]] == list(case.infeasible)
    assert [int(v) for v in r["L"]] == [len(lb) for lb in case.labels]


def test_the_table_covers_what_the_kernels_branch_on():
    Ls = {len(lb) for c in R.CASES for lb in c.labels}
    assert {0, 1, 63, 64, 65, 512} <= Ls
    assert {c.V for c in R.CASES} >= {30, 2101, 6997} and {c.B for c in R.CASES} >= {1, 3, 70}
    assert any(c.frames == (R._need(c.labels[0]),) or R._need(c.labels[0]) == c.frames[0] for c in R.CASES if "repeats" in c.name)
    assert any(c.frames[0] == 2048 and len(c.labels[0]) == 3 for c in R.CASES)
    assert any(not c.pad_cols for c in R.CASES) and any(c.ldv > c.V for c in R.CASES)
    one_short = [c for c in R.CASES if "infeasible" in c.name][0]
    assert one_short.frames[0] == R._need(one_short.labels[0]) - 1


def test_posteriors_sum_to_one_and_gradient_rows_to_zero():
    case = [c for c in R.CASES if c.name == "f32-ragged"][0]
    r = R.reference(case)
    for b, n in enumerate(case.frames):
        assert np.allclose(r["post"][b, :n].sum(1), 1.0, atol=1e-12)
        assert np.abs(r["dlogits"][b, :n].sum(1)).max() < 1e-13


@pytest.mark.parametrize("gh,gw,pool", list(itertools.product((1, 5, 16), (1, 7), (1, 2, 4, 32))))
def test_frame_map_is_avg_pool_over_rows_then_columns_first(gh, gw, pool):
    d = 3
    mem = KR.rnd((1, gh * gw, d), 11 + gh + gw)
    got, lens = R.frames_ref(mem, [(gh, gw)], pool, R.frame_count(gh, gw, pool))
    want = R.frames_torch(mem[0], gh, gw, pool)
    assert lens == [want.shape[0]] == [R.frame_count(gh, gw, pool)]
    assert torch.allclose(got[0].double(), want, rtol=0, atol=4 * 2.0 ** -24 * float(mem.abs().max()))
    if pool == 1:
        assert torch.equal(got[0], mem[0].view(gh, gw, d).permute(1, 0, 2).reshape(-1, d))
    # the adjoint: <frames(x), g> == <x, frames_bwd(g)> in fp64 terms
    g = KR.rnd(tuple(got.shape), 5)
    back = R.frames_bwd_ref(g, [(gh, gw)], pool, gh * gw)
    assert abs(float((got.double() * g.double()).sum()) - float((mem.double() * back.double()).sum())) < 1e-4


def _brute(path, blank):
    out, prev = [], None
    for a in path:
        if a != prev and a != blank:
            out.append(a)
        prev = a
    return out


def test_greedy_rule_against_a_brute_force_collapse():
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, 4, (5, 70, 6), generator=g).double().numpy()           # few distinct values: ties everywhere
    flen = [70, 64, 65, 1, 0]
    toks, arg = R.greedy_ref(x, flen)
    for b, n in enumerate(flen):
        path = []
        for f in range(n):
            row = x[b, f]
            path.append(min(i for i in range(6) if row[i] == row.max()))
        assert toks[b] == _brute(path, R.BLANK)
        assert arg[b, :n].tolist() == path and (arg[b, n:] == R.BLANK).all()
