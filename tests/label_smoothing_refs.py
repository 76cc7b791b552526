"""Float64 reference, error bounds and the case table of the label-smoothed cross-entropy (omr_ce_smooth_fwd / omr_ce_smooth_bwd).

tests/test_label_smoothing_gpu.py runs every case through the HIP kernels; tests/test_label_smoothing_refs_cpu.py checks the reference
against torch's own fp64 cross_entropy, shows that a stand-in of the kernels' arithmetic passes every check and that each
mutant of the reference (MUTANTS) misses one by a wide margin.

Definition (torch's label_smoothing, mean reduction, no class weights).  A row is live when its target is not pad and lies in [0, V).
Per live row, lse = logsumexp_v x_v and S = sum_{v < V} x_v:
    objective = lse - (1 - eps) x_t - (eps / V) S          nll = lse - x_t
    loss = sum objective / count,  nll = sum nll / count,  count = number of live rows
    dlogits[row, v] = (softmax_v - (1 - eps) [v == t] - eps / V) * grad_scale * grad_out / count      (+0 on ignored rows and for v >= V)

Inputs.  Logits amp * u(-1, 1) (amp = 30 in fp32, 8 in bf16); every live row's target logit is set to the row's mean + amp (with random
targets the smoothing term would average out over the rows and a missing term would hide), then each row is shifted by its own
logsumexp, so lse is near 0.  Every padding column holds NaN.

Bounds.
  lse, dlogits, loss, nll   the project's tolerances (oracle/kernel_refs.tol; loss 1e-4 / 1e-2 relative as in ce_check)
  rowsum                    rowsum_adds(case) * 2^-24 * sum_v |x_v|: the longest chain of fp32 additions a logit goes through.  A thread adds
                            its columns in order, VEC at a time from each of its ceil(V / (256 VEC)) chunks (VEC = 1 on the scalar path), the
                            xor butterfly over the wave adds 6 times, ((w0 + w1) + w2) + w3 over the waves 3 times.
  row sum of dlogits        the exact gradient of a live row sums to 0 over v < V; rounding V values to the dtype leaves at most
                            u * sum |d_v| <= u * 2 * scale (sum of softmax + (1 - eps) + eps = 2), u = 2^-24 (fp32) or 2^-8 (bf16).
                            This counts the rounding to the dtype alone, so the value before it has to be much finer than the dtype.  In
                            bf16 the kernel's fp32 arithmetic is 2^16 times finer.  In fp32, fp32 arithmetic is not (an fp32 lse, the
                            exponential and the subtractions round at the same 2^-24: 2 .. 6 times the bound), so the fp32 gradient
                            kernel normalises the softmax by the row's own sum of exponentials and applies the formula in fp64.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from oracle import kernel_refs as KR

F32, BF16 = KR.F32, KR.BF16
PAD = 0
GRAD_SCALE, GRAD_OUT = 0.5, 3.0
AMP = {F32: 30.0, BF16: 8.0}
UNIT = {F32: 2.0 ** -24, BF16: 2.0 ** -8}
LOSS_RTOL = {F32: 1e-4, BF16: 1e-2}
NEG_INF = float("-inf")


@dataclass(frozen=True)
class Case:
    dtype: torch.dtype
    V: int
    ldv: int
    eps: float
    M: int = 1030                            # past the finalize kernel's 1024 threads
    inf: bool = False

    @property
    def name(self) -> str:
        return f"{KR.TAG[self.dtype]}-V{self.V}-ld{self.ldv}-eps{self.eps}" + ("-inf" if self.inf else "")

    @property
    def vec(self) -> int:
        """Columns per load of the path the forward kernel takes: 16 bytes when ldv allows it, else one."""
        return KR.VEC[self.dtype] if self.ldv % KR.VEC[self.dtype] == 0 else 1


def _cases():
    out = []
    for dt in KR.DTYPES:
        out += [Case(dt, 30, 32, 0.5),           # vector path, threads 8 (fp32) / 4 (bf16) and up own no chunk; eps / V = 1 / 60
                Case(dt, 301, 301, 0.1),         # ldv odd: the scalar path, threads 0..44 take a second column
                Case(dt, 2101, 2104, 0.1),       # vector path, a second chunk per thread (column 1024 in fp32, 2048 in bf16)
                Case(dt, 6997, 7000, 0.1)]       # the real vocabulary
    return tuple(out)


CASES = _cases()
INF_CASES = tuple(Case(dt, 301, 304, 0.1, M=3, inf=True) for dt in KR.DTYPES)
ALL_CASES = CASES + INF_CASES


def rowsum_adds(case: Case) -> int:
    return case.vec * math.ceil(case.V / (256 * case.vec)) + 6 + 3


@functools.lru_cache(maxsize=None)
def inputs(case: Case) -> dict:
    """buf [M, ldv] of the case's dtype (NaN in the padding columns), tgt int64 [M].  Cached: never modify."""
    M, V, amp = case.M, case.V, AMP[case.dtype]
    x = (amp * KR.rnd((M, V), 161 + V)).double()
    tgt = torch.randint(1, V, (M,), generator=torch.Generator().manual_seed(162))
    if case.inf:
        tgt[0], tgt[2] = 20, PAD                                     # rows 0 and 1 live, row 2 ignored
    else:
        tgt[3], tgt[4], tgt[5], tgt[M - 1] = PAD, -1, V, PAD         # all three count as ignored
    live = (tgt != PAD) & (tgt >= 0) & (tgt < V)
    rows = live.nonzero()[:, 0]
    x[rows, tgt[rows]] = x[rows].mean(1) + amp
    x -= torch.logsumexp(x, 1, keepdim=True)
    if case.inf:
        x[0, :16] = NEG_INF                                          # whole 16-byte chunks of -inf at the start of the row ...
        x[0, 270] = NEG_INF                                          # ... and one in the second sweep of the scalar path
    buf = torch.full((M, case.ldv), float("nan"), dtype=case.dtype)
    buf[:, :V] = x.to(case.dtype)
    return dict(buf=buf, tgt=tgt)


MUTANTS = ("no_smoothing", "onehot_keeps_1", "no_uniform_in_gradient", "eps_over_ldv", "rowsum_over_ldv", "ignored_rows_in_sum")


def ref(case: Case, mutant: Optional[str] = None) -> dict:
    """The definition in fp64 on the quantised inputs.  mutant: one of MUTANTS, a deliberately wrong variant for the self-check."""
    assert mutant is None or mutant in MUTANTS
    inp = inputs(case)
    V, tgt = case.V, inp["tgt"]
    x = inp["buf"][:, :V].double()
    eps = 0.0 if mutant == "no_smoothing" else case.eps
    uni = eps / (case.ldv if mutant == "eps_over_ldv" else V)
    keep = 1.0 if mutant == "onehot_keeps_1" else 1.0 - eps
    mx = x.max(1, keepdim=True).values
    lse = (mx + torch.log(torch.exp(x - mx).sum(1, keepdim=True)))[:, 0]
    rowsum = (inp["buf"].double() if mutant == "rowsum_over_ldv" else x).sum(1)
    live = (tgt != PAD) & (tgt >= 0) & (tgt < V)
    t = tgt.clamp(0, V - 1)
    xt = x.gather(1, t[:, None])[:, 0]
    count = int(live.sum())
    nll_row = lse - xt
    obj_row = lse - keep * xt - uni * rowsum
    loss = float(obj_row[live].sum() / count)
    if mutant == "ignored_rows_in_sum":
        loss = float((obj_row[live].sum() - (uni * rowsum)[~live].sum()) / count)
    nll = float(nll_row[live].sum() / count)
    onehot = torch.zeros_like(x).scatter_(1, t[:, None], 1.0)
    g_uni = 0.0 if mutant == "no_uniform_in_gradient" else uni
    dl = (torch.exp(x - lse[:, None]) - keep * onehot - g_uni) * (GRAD_SCALE * GRAD_OUT / count) * live[:, None]
    dl_full = torch.zeros((case.M, case.ldv), dtype=torch.float64)
    dl_full[:, :V] = dl
    return dict(lse=lse, rowsum=rowsum, loss=loss, nll=nll, count=count, live=live, dlogits=dl_full)


@functools.lru_cache(maxsize=None)
def reference(case: Case) -> dict:
    return ref(case)


def _f32(v: float) -> torch.Tensor:
    return torch.tensor(v, dtype=torch.float32)


def standin_rowsum(case: Case) -> torch.Tensor:
    """The forward kernel's row sums in its own order, in fp32 (numpy): per thread in column order, butterfly over the 64 lanes,
    then ((w0 + w1) + w2) + w3."""
    V, vec = case.V, case.vec
    x = inputs(case)["buf"][:, :V].float().numpy()
    K = math.ceil(V / (256 * vec))
    xp = np.zeros((case.M, K * 256 * vec), dtype=np.float32)
    xp[:, :V] = x
    xp = xp.reshape(case.M, K, 256, vec)
    with np.errstate(invalid="ignore"):
        rs = np.zeros((case.M, 256), dtype=np.float32)
        for k in range(K):
            for e in range(vec):
                rs = rs + xp[:, k, :, e]
        w = rs.reshape(case.M, 4, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[:, :, lane ^ o]
        w = w[:, :, 0]
        return torch.from_numpy(((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3])


def standin(case: Case) -> dict:
    """torch / numpy arithmetic in the kernels' place: fp32 lse and row sums, the objective formed and summed in fp64; the bf16 gradient
    in fp32, the fp32 gradient in fp64 with the softmax normalised by its own sum (from the fp32 lse), one rounding to the dtype each."""
    inp = inputs(case)
    V, tgt, eps = case.V, inp["tgt"], np.float32(case.eps)
    x = inp["buf"][:, :V].float()
    lse = torch.logsumexp(x, 1)
    rowsum = standin_rowsum(case)
    live = (tgt != PAD) & (tgt >= 0) & (tgt < V)
    t = tgt.clamp(0, V - 1)
    xt = x.gather(1, t[:, None])[:, 0]
    count = float(live.sum())
    plain = (lse - xt).double()
    obj = lse.double() - (1.0 - float(eps)) * xt.double() - (float(eps) / V) * rowsum.double()
    sc = _f32(GRAD_SCALE) * _f32(GRAD_OUT) / _f32(count)
    keep, uni = _f32(1.0) - _f32(float(eps)), _f32(float(eps)) / _f32(float(V))
    onehot = torch.zeros_like(x).scatter_(1, t[:, None], 1.0)
    if case.dtype == F32:
        e = torch.exp(x.double() - lse.double()[:, None])
        d = (e / e.sum(1, keepdim=True) - (1.0 - float(eps)) * onehot.double() - float(eps) / V) * (GRAD_SCALE * GRAD_OUT / count)
    else:
        d = ((torch.exp(x - lse[:, None]) - keep * onehot) - uni) * sc
    dl = torch.zeros((case.M, case.ldv), dtype=case.dtype)
    dl[:, :V] = torch.where(live[:, None], d, torch.zeros((), dtype=d.dtype)).to(case.dtype)
    return dict(lse=lse, rowsum=rowsum, loss=float((obj[live].sum() / count).float()), nll=float((plain[live].sum() / count).float()),
                count=count, dlogits=dl)


def _worst(err: torch.Tensor, allowed: torch.Tensor) -> float:
    """max of err / allowed; an error that is NaN, or positive where nothing is allowed, counts as infinite."""
    r = torch.where(err == 0, torch.zeros_like(err), err / allowed)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


def _scalar_ratio(got: float, want: float, rtol: float) -> float:
    if math.isinf(want):
        return 0.0 if got == want else math.inf
    if not math.isfinite(got):
        return math.inf
    return abs(got - want) / abs(want) / rtol


def ratios(case: Case, out: dict) -> dict:
    """{check: worst error / bound} of a result `out` (keys lse, rowsum, loss, nll, count, dlogits [M, ldv]).  <= 1 everywhere passes."""
    r, V, dt = reference(case), case.V, case.dtype
    x = inputs(case)["buf"][:, :V].double()
    scale = GRAD_SCALE * GRAD_OUT / r["count"]
    as64 = lambda t: t.detach().cpu().double()
    res = {}
    t32 = KR.tol(F32, 1.0)
    lse = as64(out["lse"])
    res["lse"] = _worst((lse - r["lse"]).abs(), t32["atol"] + t32["rtol"] * r["lse"].abs())
    rowsum = as64(out["rowsum"])
    same_inf = torch.isinf(r["rowsum"]) & (rowsum == r["rowsum"])
    err = torch.where(same_inf, torch.zeros_like(rowsum), (rowsum - r["rowsum"]).abs())
    res["rowsum"] = _worst(err, rowsum_adds(case) * KR.U24 * x.abs().sum(1))
    res["loss"] = _scalar_ratio(float(out["loss"]), r["loss"], LOSS_RTOL[dt])
    res["nll"] = _scalar_ratio(float(out["nll"]), r["nll"], LOSS_RTOL[dt])
    res["count"] = 0.0 if float(out["count"]) == float(r["count"]) else math.inf
    dl = as64(out["dlogits"])
    assert tuple(dl.shape) == (case.M, case.ldv), tuple(dl.shape)
    td = KR.tol(dt, scale)
    # |dlogits| <= grad_scale grad_out / count: that is the size the absolute tolerance is scaled to
    res["dlogits"] = _worst((dl[:, :V] - r["dlogits"][:, :V]).abs(), td["atol"] + td["rtol"] * r["dlogits"][:, :V].abs())
    res["dlogits_rowsum"] = _worst(dl[:, :V][r["live"]].sum(1).abs(), torch.full((r["count"],), 2.0 * UNIT[dt] * scale, dtype=torch.float64))
    return res


ROW_SUM = "dlogits_rowsum"                   # asserted by tests of its own: see check


def check(case: Case, out: dict, row_sum: bool) -> dict:
    """Prints every error / bound, then asserts the row sum of dlogits (row_sum = True) or every other check (row_sum = False)."""
    res = ratios(case, out)
    print(f"label smoothing {case.name}: error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not v <= 1.0 and (k == ROW_SUM) == row_sum}
    assert not bad, f"label smoothing {case.name}: error / bound above 1: {bad}"
    return res


def check_zero_bits(case: Case, dl_full: torch.Tensor) -> None:
    """Padding columns and ignored rows of the [M, ldv] gradient buffer are +0, bit for bit."""
    r = reference(case)
    dl_full = dl_full.detach().cpu()
    assert bool((KR.bits(dl_full[:, case.V:]) == 0).all()), f"label smoothing {case.name}: dlogits padding columns are not +0"
    assert bool((KR.bits(dl_full[~r["live"]]) == 0).all()), f"label smoothing {case.name}: ignored rows have a gradient"
