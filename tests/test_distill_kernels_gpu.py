"""The distillation loss kernels (omr_ce_distill_fwd / omr_ce_distill_bwd) against the fp64 reference, bounds and case table of
tests/distill_refs.py: the three (student, teacher) dtype pairs, the 16-byte and the scalar load path per tensor, threads without a chunk
(V = 30), a second chunk per thread (V = 2101), the real vocabulary, M = 1030 (the finalize loop runs twice), one and two teachers,
teacher columns at -inf, a student equal to its teacher."""
import functools
import math

import pytest
import torch

import distill_refs as DR
from oracle import kernel_refs as KR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ids = lambda cases: [c.name for c in cases]  # noqa: E731


def K():
    from omr_a2s_multimodal_transformer_amd import kernels
    return kernels


def device_inputs(case):
    inp = DR.inputs(case)
    x = inp["xbuf"].to(DEV)[:, :case.V]
    a = inp["abuf"].to(DEV)[:, :case.V]
    b = inp["bbuf"].to(DEV)[:, :case.V] if case.two else None
    return x, a, b, inp["tgt"].to(DEV)


def run(case, lam=None, teachers=True):
    """The case through the new entries -> the dict distill_refs.check takes; dlogits is the whole [M, ldv] buffer."""
    lam = case.lam if lam is None else lam
    x, a, b, tgt = device_inputs(case)
    if not teachers:
        a = b = None
    alpha = case.alpha if b is not None else 1.0
    means, lse4, rowkd, acc4 = K().ce_distill_fwd(x, tgt, a, b, case.V, DR.PAD, alpha, case.tau, lam)
    dl = K().ce_distill_bwd(x, tgt, a, b, lse4, acc4, case.V, DR.PAD, alpha, case.tau, lam, grad_scale=DR.GRAD_SCALE,
                            grad_out=torch.tensor([DR.GRAD_OUT], device=DEV))
    dl = dl if dl._base is None else dl._base
    torch.cuda.synchronize()
    means, acc4 = means.cpu(), acc4.cpu()
    return dict(lse4=lse4.cpu(), rowkd=None if rowkd is None else rowkd.cpu(), loss=float(means[0]), nll=float(means[1]), kd=float(means[2]),
                count=float(acc4[1]), acc4=acc4, dlogits=dl.cpu())


@functools.lru_cache(maxsize=None)
def result(case):
    return run(case)


@pytest.mark.parametrize("case", DR.CASES, ids=ids(DR.CASES))
def test_distillation_loss(case):
    """The four row constants, rowkd and kd (within their derived bounds), loss, nll, count, dlogits and its row sums of every case; padding
    columns and ignored rows of dlogits are +0 bits; acc4 holds the sums the means were formed from."""
    out = result(case)
    DR.check(case, out)
    DR.check_zero_bits(case, out["dlogits"])
    acc4 = out["acc4"]
    for i, name in ((0, "loss"), (2, "nll"), (3, "kd")):
        assert float((acc4[i] / acc4[1]).float()) == out[name], name
    dead = ~DR.reference(case)["live"]
    assert bool((out["lse4"][:, dead] == 0).all()) and bool((out["rowkd"][dead] == 0).all())


@pytest.mark.parametrize("case", DR.INF_CASES, ids=ids(DR.INF_CASES))
def test_teacher_columns_at_neg_inf(case):
    """A grammar-masked teacher: q = 0 there, nothing is added to kd, and every output is finite."""
    out = result(case)
    DR.check(case, out)
    DR.check_zero_bits(case, out["dlogits"])
    assert all(math.isfinite(out[k]) for k in ("loss", "nll", "kd"))
    assert torch.isfinite(out["dlogits"].float()).all() and torch.isfinite(out["lse4"]).all() and torch.isfinite(out["rowkd"]).all()
    inp = DR.inputs(case)
    masked = torch.isinf(inp["abuf"][0, :case.V].float())
    if case.two:
        masked &= torch.isinf(inp["bbuf"][0, :case.V].float())
    assert int(masked.sum()) == (8 if case.two else 17)
    # q = 0 in those columns: the gradient there is the student's own share, never negative
    assert bool((out["dlogits"][0, :case.V][masked].float() >= 0).all())


@pytest.mark.parametrize("case", DR.IDENTITY_CASES, ids=ids(DR.IDENTITY_CASES))
def test_student_equal_to_its_teacher(case):
    """kd = 0 within its bound (which is not 0: the row constants carry rounding) and the lam = 1 gradient 0 within the gradient's tolerance."""
    out = result(case)
    res = DR.check(case, out)
    bd = DR.bounds(case)
    assert abs(out["kd"]) <= bd["kd"] and res["dlogits"] <= 1.0
    assert float(out["dlogits"].double().abs().max()) <= KR.tol(KR.F32, bd["gsize"])["atol"]


LAM0_CASES = tuple(c for c in DR.CASES if c.V == 6997) + DR.INF_CASES[:1]


@pytest.mark.parametrize("case", LAM0_CASES, ids=ids(LAM0_CASES))
@pytest.mark.parametrize("teachers", ["poisoned", "absent"])
def test_lam_0_through_the_new_entries_has_the_old_entries_bits(case, teachers):
    """loss, lse, the sum and count, and dlogits of omr_ce_fwd / omr_ce_bwd, bit for bit; nll is the loss, kd is 0.  The teachers are never read:
    their buffers hold NaN everywhere, or the pointers are NULL."""
    x, a, b, tgt = device_inputs(case)
    go = torch.tensor([DR.GRAD_OUT], device=DEV)
    loss, lse, acc2 = K().ce_fwd(x, tgt, case.V, DR.PAD)
    dl = K().ce_bwd(x, tgt, lse, acc2, case.V, DR.PAD, grad_scale=DR.GRAD_SCALE, grad_out=go)
    if teachers == "poisoned":
        nan = lambda t: None if t is None else torch.full_like(t._base, float("nan"))[:, :case.V]  # noqa: E731
        pa, pb = nan(a), nan(b)
        alpha = case.alpha if pb is not None else 1.0
        means, lse4, rowkd, acc4 = K().ce_distill_fwd(x, tgt, pa, pb, case.V, DR.PAD, alpha, case.tau, 0.0)
        dl2 = K().ce_distill_bwd(x, tgt, pa, pb, lse4, acc4, case.V, DR.PAD, alpha, case.tau, 0.0, grad_scale=DR.GRAD_SCALE, grad_out=go)
        new = dict(lse4=lse4.cpu(), rowkd=rowkd, loss=float(means[0]), nll=float(means[1]), kd=float(means[2]), acc4=acc4.cpu(),
                   dlogits=dl2._base.cpu())
    else:
        new = run(case, lam=0.0, teachers=False)
    assert new["rowkd"] is None and math.isfinite(new["loss"]) and new["kd"] == 0.0
    KR.assert_bit_equal(torch.tensor([new["loss"]]), loss.cpu(), "loss")
    KR.assert_bit_equal(torch.tensor([new["nll"]]), loss.cpu(), "nll")
    KR.assert_bit_equal(new["lse4"][0], lse.cpu(), "lse")
    KR.assert_bit_equal(new["acc4"][:2], acc2.cpu(), "sum and count")
    KR.assert_bit_equal(new["acc4"][2:3], acc2.cpu()[:1], "nll sum")
    KR.assert_bit_equal(new["dlogits"], dl._base.cpu() if dl._base is not None else dl.cpu(), "dlogits")


BAD_ARGS = [dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(tau=float("nan")), dict(lam=-0.1), dict(lam=1.5), dict(lam=float("nan")),
            dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(alpha=0.5, no_b=True), dict(ldt=300)]


@pytest.mark.parametrize("bad", BAD_ARGS, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD_ARGS])
def test_bad_arguments_are_refused_before_a_launch(bad):
    """OMR_ERR_ARG (-1) from both C entries, which then write nothing; ValueError from the Python entries for the value ranges."""
    from omr_a2s_multimodal_transformer_amd._lib import cur_stream, lib
    case = DR.INF_CASES[0]
    x, a, b, tgt = device_inputs(case)
    arg = dict(tau=2.0, lam=0.5, alpha=0.3, ldt=case.ldt, no_b=False)
    arg.update(bad)
    if arg["no_b"]:
        b = None
    M, V = case.M, case.V
    out = torch.full((5 * M + 3,), KR.SENTINEL, dtype=torch.float32, device=DEV)
    acc4 = torch.full((4,), KR.SENTINEL, dtype=torch.float64, device=DEV)
    dl = torch.full((M, case.ldv), KR.SENTINEL, dtype=torch.float32, device=DEV)
    lse4, rowkd, means = out[:4 * M], out[4 * M:5 * M], out[5 * M:]
    pb = None if b is None else b.data_ptr()
    rc = lib().query("omr_ce_distill_fwd", 0, x.data_ptr(), case.ldv, 0, a.data_ptr(), pb, arg["ldt"], tgt.data_ptr(), lse4.data_ptr(), rowkd.data_ptr(),
                     acc4.data_ptr(), means.data_ptr(), M, V, DR.PAD, arg["alpha"], arg["tau"], arg["lam"], cur_stream())
    assert rc == -1
    rc = lib().query("omr_ce_distill_bwd", 0, x.data_ptr(), case.ldv, 0, a.data_ptr(), pb, arg["ldt"], tgt.data_ptr(), lse4.data_ptr(), acc4.data_ptr(),
                     dl.data_ptr(), M, V, DR.PAD, arg["alpha"], arg["tau"], arg["lam"], 1.0, None, cur_stream())
    assert rc == -1
    torch.cuda.synchronize()
    assert bool((out == KR.SENTINEL).all()) and bool((acc4 == KR.SENTINEL).all()) and bool((dl == KR.SENTINEL).all())
    if "ldt" not in bad:
        with pytest.raises(ValueError):
            K().ce_distill_fwd(x, tgt, a, b, V, DR.PAD, arg["alpha"], arg["tau"], arg["lam"])
        with pytest.raises(ValueError):
            K().ce_distill_bwd(x, tgt, a, b, lse4.view(4, M), acc4, V, DR.PAD, arg["alpha"], arg["tau"], arg["lam"])


TWICE = tuple(c for c in DR.CASES if c.V == 6997)


@pytest.mark.parametrize("case", TWICE, ids=ids(TWICE))
def test_two_runs_are_bit_equal(case):
    a, b = result(case), run(case)
    for k in ("lse4", "rowkd", "acc4", "dlogits"):
        KR.assert_bit_equal(b[k], a[k], k)
    assert a["loss"] == b["loss"] and a["nll"] == b["nll"] and a["kd"] == b["kd"]
