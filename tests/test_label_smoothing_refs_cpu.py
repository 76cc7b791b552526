"""CPU self-check of tests/label_smoothing_refs.py: the fp64 reference is torch's cross_entropy(label_smoothing=eps), a stand-in
of the kernels' arithmetic passes every check of every case, and each mutant of the reference misses a check by at least 10x."""
import math

import pytest
import torch

import label_smoothing_refs as LS

ids = [c.name for c in LS.ALL_CASES]


@pytest.mark.parametrize("case", LS.ALL_CASES, ids=ids)
def test_reference_is_torch_cross_entropy_in_fp64(case):
    inp, r = LS.inputs(case), LS.reference(case)
    x = inp["buf"][:, :case.V].double().requires_grad_(True)
    tgt = torch.where(r["live"], inp["tgt"], torch.full_like(inp["tgt"], LS.PAD))      # torch refuses -1 and V; here they are ignored rows
    loss = torch.nn.functional.cross_entropy(x, tgt, ignore_index=LS.PAD, label_smoothing=case.eps)
    nll = torch.nn.functional.cross_entropy(x.detach(), tgt, ignore_index=LS.PAD)
    (g,) = torch.autograd.grad(loss, x, torch.tensor(LS.GRAD_SCALE * LS.GRAD_OUT, dtype=torch.float64))
    assert torch.isfinite(g).all()
    if case.inf:
        assert float(loss) == math.inf and r["loss"] == math.inf
    else:
        assert abs(float(loss) - r["loss"]) <= 1e-12 * abs(r["loss"]), (float(loss), r["loss"])
    assert abs(float(nll) - r["nll"]) <= 1e-12 * abs(r["nll"]), (float(nll), r["nll"])
    scale = LS.GRAD_SCALE * LS.GRAD_OUT / r["count"]
    err = float((g - r["dlogits"][:, :case.V]).abs().max())
    assert err <= 1e-12 * scale, err
    assert r["count"] == int(r["live"].sum()) == (2 if case.inf else case.M - 4)


@pytest.mark.parametrize("case", LS.ALL_CASES, ids=ids)
def test_standin_keeps_the_row_sum_of_dlogits(case):
    """sum_v dlogits[row, v] = 0 within 2 u scale, u the dtype's unit round-off."""
    LS.check(case, LS.standin(case), row_sum=True)


@pytest.mark.parametrize("case", LS.ALL_CASES, ids=ids)
def test_standin_passes_every_other_check(case):
    out = LS.standin(case)
    LS.check(case, out, row_sum=False)
    LS.check_zero_bits(case, out["dlogits"])
    if case.inf:
        assert float(out["rowsum"][0]) == -math.inf and out["loss"] == math.inf and math.isfinite(out["nll"])
        assert torch.isfinite(out["dlogits"].float()).all()


def test_rowsum_bound_counts_the_longest_chain():
    by = {c.name: LS.rowsum_adds(c) for c in LS.CASES}
    assert by["f32-V30-ld32-eps0.5"] == 4 + 9 and by["bf16-V30-ld32-eps0.5"] == 8 + 9
    assert by["f32-V301-ld301-eps0.1"] == 2 + 9 and by["f32-V2101-ld2104-eps0.1"] == 4 * 3 + 9
    assert by["f32-V6997-ld7000-eps0.1"] == 4 * 7 + 9 and by["bf16-V6997-ld7000-eps0.1"] == 8 * 4 + 9


@pytest.mark.parametrize("mutant", LS.MUTANTS)
def test_every_mutant_misses_a_check_by_10x(mutant):
    worst, where = 0.0, None
    for case in LS.CASES:
        m = LS.ref(case, mutant)
        res = LS.ratios(case, dict(m, dlogits=m["dlogits"]))
        k = max(res, key=res.get)
        if res[k] > worst:
            worst, where = res[k], (case.name, k)
    print(f"mutant {mutant}: worst error / bound {worst:.3g} at {where}")
    assert worst >= 10.0, (mutant, worst, where)


def test_the_unmutated_reference_passes_its_own_checks():
    for case in LS.ALL_CASES:
        res = LS.ratios(case, LS.reference(case))
        assert max(res.values()) == 0.0 or max(res.values()) < 1e-6, (case.name, res)
