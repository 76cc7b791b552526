"""tests/distill_refs.py checked without a GPU: the fp64 reference against torch's own fp64 cross_entropy + kl_div composition and its autograd
gradient, a torch fp32 stand-in for the kernels' arithmetic against every bound, and each mutant of the reference against the same bounds."""
import math

import pytest
import torch
import torch.nn.functional as F

import distill_refs as DR

ids = lambda cases: [c.name for c in cases]  # noqa: E731
SMALL = tuple(c for c in DR.ALL_CASES if c.V <= 2101)            # the torch composition and the mutants: the quick shapes, every path and parameter


def torch_composition(case):
    """(loss, nll, kd, gradient [M, V]) of torch's fp64 ops with autograd, scaled like the kernels' gradient."""
    inp = DR.inputs(case)
    V, tau, lam = case.V, case.tau, case.lam
    x = inp["xbuf"][:, :V].double().requires_grad_(True)
    a = inp["abuf"][:, :V].double()
    live = DR.live_rows(case, inp["tgt"])
    tgt = torch.where(live, inp["tgt"], torch.full_like(inp["tgt"], -100))
    nll = F.cross_entropy(x, tgt, ignore_index=-100)
    q = F.softmax(a / tau, 1)
    if case.two:
        q = case.alpha * q + (1 - case.alpha) * F.softmax(inp["bbuf"][:, :V].double() / tau, 1)
    kd = tau * tau * F.kl_div(F.log_softmax(x / tau, 1)[live], q[live], reduction="sum") / int(live.sum())
    loss = (1 - lam) * nll + lam * kd if lam < 1 else kd
    (g,) = torch.autograd.grad(loss * (DR.GRAD_SCALE * DR.GRAD_OUT), x)
    return float(loss.detach()), float(nll.detach()), float(kd.detach()), g


@pytest.mark.parametrize("case", SMALL, ids=ids(SMALL))
def test_reference_is_torchs_fp64_composition(case):
    r = DR.reference(case)
    loss, nll, kd, g = torch_composition(case)
    rel = lambda got, want: abs(got - want) <= 1e-11 * max(abs(want), 1e-3)  # noqa: E731
    assert rel(r["loss"], loss) and rel(r["nll"], nll) and rel(r["kd"], kd), (r["loss"], loss, r["nll"], nll, r["kd"], kd)
    assert math.isfinite(loss)
    assert torch.isfinite(g).all()
    err = (r["dlogits"][:, :case.V] - g).abs().max()
    assert float(err) <= 1e-12 * DR.GRAD_SCALE * DR.GRAD_OUT * max(case.tau, 1.0), float(err)


@pytest.mark.parametrize("case", DR.ALL_CASES, ids=ids(DR.ALL_CASES))
def test_fp32_standin_passes_every_bound(case):
    DR.check(case, DR.standin(case))


@pytest.mark.parametrize("case", DR.IDENTITY_CASES, ids=ids(DR.IDENTITY_CASES))
def test_identity_reference_is_zero(case):
    r = DR.reference(case)
    assert abs(r["kd"]) <= 1e-12 and float(r["dlogits"].abs().max()) <= 1e-15


def test_case_table_covers_the_parameters():
    cs = DR.CASES
    assert {c.tau for c in cs} == {1.0, 2.0, 4.0} and {c.lam for c in cs} == {0.5, 1.0} and {c.two for c in cs} == {False, True}
    assert {(c.sdt, c.tdt) for c in cs} == set(DR.TYPE_PAIRS) and all(c.M == 1030 for c in cs)
    for V in (30, 301, 2101, 6997):
        assert {c.two for c in cs if c.V == V} == {False, True}


@pytest.mark.parametrize("mutant", DR.MUTANTS)
def test_every_mutant_misses_a_bound_by_a_wide_margin(mutant):
    """On every case where the mutant differs from the definition its worst error / bound is at least 10 (a correct kernel stays below 1)."""
    shown = [c for c in SMALL if not c.inf and not c.identity and DR.mutant_shows(c, mutant)]
    assert len(shown) >= 3 and any(c.sdt == DR.F32 for c in shown)
    for case in shown:
        m = DR.ref(case, mutant)
        out = dict(lse4=torch.stack([m["lse"], m["lse_xt"], m["lse_a"], m["lse_b"]]), rowkd=m["rowkd"], loss=m["loss"], nll=m["nll"], kd=m["kd"],
                   count=m["count"], dlogits=m["dlogits"])
        res = DR.ratios(case, out)
        print(f"{mutant} on {case.name}: " + ", ".join(f"{k} {v:.3g}" for k, v in res.items() if v > 1))
        assert max(res.values()) >= 10.0, (case.name, res)
