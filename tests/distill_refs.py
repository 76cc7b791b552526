"""Float64 reference, error bounds and the case table of the distillation loss (omr_ce_distill_fwd / omr_ce_distill_bwd).

tests/test_distill_kernels_gpu.py runs every case through the HIP kernels; tests/test_distill_refs_cpu.py checks the reference against
torch's own fp64 cross_entropy + kl_div composition and its autograd gradient, shows that a stand-in of the kernels' arithmetic passes every
check and that each mutant of the reference (MUTANTS) misses one by a wide margin.

Definition.  A row is live when its target is not pad and lies in [0, V).  Per live row over the columns v < V, with k = 1 / tau:
    p = softmax(x)    pt = softmax(k x)    q = alpha softmax(k a) + (1 - alpha) softmax(k b)         (one teacher: q = softmax(k a), alpha = 1)
    nll = lse(x) - x_t        kd = tau^2 sum_v q_v (log q_v - log pt_v)      (terms with q_v = 0 are 0: torch's xlogy / kl_div rule)
    objective = (1 - lam) nll + lam kd;   loss, nll, kd = the three means over the live rows,  count = number of live rows
    dlogits[row, v] = ((1 - lam)(p_v - [v == t]) + lam tau (pt_v - q_v)) * grad_scale * grad_out / count      (+0 on ignored rows, for v >= V)

Inputs.  Student logits amp * u(-1, 1) (amp = 30 in fp32, 8 in bf16) with every live row's target logit raised to the row's mean + amp, as in
the label-smoothing cases.  Each teacher is built the same way but peaked on a token of its own: target + 1 for a, target + 2 for b (mod V), so
neither teacher agrees with the hard label and a mixture of softmaxes is far from a softmax of mixed logits.  Every row is shifted by its own
logsumexp.  Every padding column holds NaN in all three tensors; rows 3, 4, 5 and M - 1 are ignored (pad, -1, V, pad).

Bounds.  u = 2^-24 (the kernels compute in fp32 whatever the storage dtypes; the reference reads the quantised inputs).
  lse, dlogits, loss, nll   the project's tolerances (oracle/kernel_refs.tol; loss 1e-4 / 1e-2 relative as in ce_check).  The gradient's
                            absolute tolerance is scaled to its size ((1 - lam) + lam tau) * grad_scale * grad_out / count.  A bf16 gradient takes
                            the project's tolerance for a value computed in fp32 and rounded once (oracle/kernel_refs.check_rounded_once: the fp32
                            tolerance plus 2^-8 relative), not the 3e-2 of tol(bf16): at tau = 4 the soft part of the gradient is a few per cent of
                            its scale everywhere, and an absolute 3e-2 of the scale would pass a gradient without its factor tau.
  rowkd, kd                 derived from the kernels' arithmetic.  adds(case) = 8 ceil(V / 2048) + 6 + 3 is the longest chain of fp32 additions a
                            column goes through (8 per chunk of a thread, 6 butterfly steps, 3 over the waves).  Every logarithmic quantity
                            (k x_v - lse_xt, k a_v - lse_a, log q_v) is a product, a difference and a row constant lse = k m + log(sum): the sum carries
                            adds * u relative error plus that of its exponentials, whose argument error is u times the argument's terms.  With
                            A_v = k (|x_v| + |a_v| + |b_v|) + |lse_xt| + |lse_a| + |lse_b| the absolute error of d_v = log q_v - log pt_v and the
                            relative error of q_v are each at most E_v = u (adds + 8 + 4 A_v)   (8: the handful of single roundings, the exponential's
                            and the logarithm's own error of a few ulp).  Hence
                                |rowkd error| <= tau^2 [ sum_v q_v (1 + |d_v|) E_v + adds u sum_v |q_v d_v| ] + u |rowkd| + floor,
                            floor = tau^2 V 2^-126 * 256: a q_v below the smallest normal fp32 number may be flushed to 0 (its |d_v| stays below 256).
                            kd is the fp64 mean of rowkd: the mean of the row bounds, plus the fp32 rounding of the result.
  row sum of dlogits        the exact gradient of a live row sums to 0.  Its three softmaxes each sum to 1 within max_v E'_v, E'_v = E_v with
                            |x_v| + |lse_x| added to A_v, and the values are rounded once to the student's dtype (unit roundoff ud):
                                |sum_v dlogits[row, v]| <= 2 ((1 - lam) + lam tau) scale (ud + max_v E'_v).
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional

import torch

from oracle import kernel_refs as KR

F32, BF16 = KR.F32, KR.BF16
PAD = 0
GRAD_SCALE, GRAD_OUT = 0.5, 3.0
AMP = {F32: 30.0, BF16: 8.0}
UNIT = {F32: 2.0 ** -24, BF16: 2.0 ** -8}
LOSS_RTOL = {F32: 1e-4, BF16: 1e-2}
NEG_INF = float("-inf")
U = KR.U24
TYPE_PAIRS = ((F32, F32), (BF16, BF16), (BF16, F32))             # (student, teacher)


@dataclass(frozen=True)
class Case:
    sdt: torch.dtype
    tdt: torch.dtype
    V: int
    ldv: int
    ldt: int
    two: bool
    tau: float
    lam: float
    M: int = 1030                            # past the finalize kernel's 1024 threads
    inf: bool = False
    identity: bool = False                   # the student's logits are the single teacher's

    @property
    def alpha(self) -> float:
        return 0.3 if self.two else 1.0

    @property
    def name(self) -> str:
        return (f"{KR.TAG[self.sdt]}-{KR.TAG[self.tdt]}-V{self.V}-ld{self.ldv}-{self.ldt}-{'two' if self.two else 'one'}-tau{self.tau:g}-lam{self.lam:g}"
                + ("-inf" if self.inf else "") + ("-identity" if self.identity else ""))


SHAPES = ((30, 32, 32),                      # threads 4 and up own no chunk
          (301, 301, 304),                   # student on the scalar path, teachers on the 16-byte path
          (2101, 2104, 2101),                # the reverse; threads 0..6 take a second chunk (column 2048)
          (6997, 7000, 7000))                # the real vocabulary
TAUS = (1.0, 2.0, 4.0)


def _cases():
    out = []
    for p, (sdt, tdt) in enumerate(TYPE_PAIRS):
        for j, (V, ldv, ldt) in enumerate(SHAPES):
            out.append(Case(sdt, tdt, V, ldv, ldt, two=(j + p) % 2 == 1, tau=TAUS[(j + p) % 3], lam=(0.5, 1.0)[(j // 2 + p) % 2]))
    return tuple(out)


CASES = _cases()
INF_CASES = tuple(Case(sdt, tdt, 301, 304, 304, two=p != 1, tau=2.0, lam=0.5, M=3, inf=True) for p, (sdt, tdt) in enumerate(TYPE_PAIRS))
IDENTITY_CASES = tuple(Case(dt, dt, 2101, 2104, 2104, two=False, tau=2.0, lam=1.0, M=40, identity=True) for dt in KR.DTYPES)
ALL_CASES = CASES + INF_CASES + IDENTITY_CASES


def adds(case: Case) -> int:
    return 8 * math.ceil(case.V / 2048) + 6 + 3


def live_rows(case: Case, tgt: torch.Tensor) -> torch.Tensor:
    return (tgt != PAD) & (tgt >= 0) & (tgt < case.V)


def _peaked(M: int, V: int, amp: float, seed: int, tok: torch.Tensor) -> torch.Tensor:
    x = (amp * KR.rnd((M, V), seed)).double()
    rows = torch.arange(M)
    x[rows, tok] = x.mean(1) + amp
    return x - torch.logsumexp(x, 1, keepdim=True)


def _buf(x: torch.Tensor, ld: int, dtype) -> torch.Tensor:
    buf = torch.full((x.shape[0], ld), float("nan"), dtype=dtype)
    buf[:, :x.shape[1]] = x.to(dtype)
    return buf


@functools.lru_cache(maxsize=None)
def inputs(case: Case) -> dict:
    """xbuf [M, ldv] (student dtype), abuf / bbuf [M, ldt] (teacher dtype; bbuf None with one teacher), NaN in the padding columns; tgt int64 [M].
    Cached: never modify."""
    M, V = case.M, case.V
    tgt = torch.randint(1, V, (M,), generator=torch.Generator().manual_seed(262))
    if case.inf:
        tgt[0], tgt[2] = 20, PAD                                     # rows 0 and 1 live, row 2 ignored
    else:
        tgt[3], tgt[4], tgt[5], tgt[M - 1] = PAD, -1, V, PAD         # all count as ignored
    t = tgt.clamp(0, V - 1)
    x = _peaked(M, V, AMP[case.sdt], 261 + V, t)
    a = _peaked(M, V, AMP[case.tdt], 263 + V, (t + 1) % V)
    b = _peaked(M, V, AMP[case.tdt], 265 + V, (t + 2) % V) if case.two else None
    if case.inf:
        a[0, :16] = NEG_INF                                          # whole 16-byte chunks of -inf at the start of a's row ...
        a[0, 270] = NEG_INF                                          # ... and one further on
        if b is not None:
            b[0, 8:24] = NEG_INF                                     # columns 8..15: both teachers at -inf, q = 0 exactly
            b[1, 100:200] = NEG_INF
    abuf = _buf(a, case.ldt, case.tdt)
    if case.identity:
        assert case.sdt == case.tdt and case.ldv == case.ldt and not case.two
        return dict(xbuf=abuf, abuf=abuf.clone(), bbuf=None, tgt=tgt)
    return dict(xbuf=_buf(x, case.ldv, case.sdt), abuf=abuf, bbuf=None if b is None else _buf(b, case.ldt, case.tdt), tgt=tgt)


MUTANTS = ("no_tau_squared", "no_tau_in_gradient", "logit_space_mixture", "alpha_swapped", "dead_rows_counted", "kd_on_dead_rows")


def mutant_shows(case: Case, mutant: str) -> bool:
    """Whether the mutant differs from the definition on this case at all."""
    if mutant in ("no_tau_squared", "no_tau_in_gradient"):
        return case.tau != 1.0
    if mutant in ("logit_space_mixture", "alpha_swapped"):
        return case.two
    return True


def _lse(z: torch.Tensor) -> torch.Tensor:
    mx = z.max(1, keepdim=True).values
    return (mx + torch.log(torch.exp(z - mx).sum(1, keepdim=True)))[:, 0]


def ref(case: Case, mutant: Optional[str] = None) -> dict:
    """The definition in fp64 on the quantised inputs.  mutant: one of MUTANTS, a deliberately wrong variant for the self-check."""
    assert mutant is None or mutant in MUTANTS
    inp = inputs(case)
    V, tgt, tau, lam = case.V, inp["tgt"], case.tau, case.lam
    k = 1.0 / tau
    x = inp["xbuf"][:, :V].double()
    a = inp["abuf"][:, :V].double()
    b = inp["bbuf"][:, :V].double() if case.two else None
    alpha = 1.0 - case.alpha if (mutant == "alpha_swapped" and case.two) else case.alpha
    lse, lse_xt, lse_a = _lse(x), _lse(k * x), _lse(k * a)
    lse_b = _lse(k * b) if case.two else torch.zeros_like(lse)
    logpt = k * x - lse_xt[:, None]
    if case.two and mutant == "logit_space_mixture":
        mix = k * (alpha * a + (1.0 - alpha) * b)
        q = torch.exp(mix - _lse(mix)[:, None])
    elif case.two:
        q = alpha * torch.exp(k * a - lse_a[:, None]) + (1.0 - alpha) * torch.exp(k * b - lse_b[:, None])
    else:
        q = torch.exp(k * a - lse_a[:, None])
    pos = q > 0
    d = torch.where(pos, torch.log(torch.where(pos, q, torch.ones_like(q))) - torch.where(pos, logpt, torch.zeros_like(q)), torch.zeros_like(q))
    t2 = 1.0 if mutant == "no_tau_squared" else tau * tau
    rowkd = t2 * (q * d).sum(1)
    live = live_rows(case, tgt)
    t = tgt.clamp(0, V - 1)
    xt = x.gather(1, t[:, None])[:, 0]
    n_live = int(live.sum())
    count = case.M if mutant == "dead_rows_counted" else n_live
    nll_row = lse - xt
    kd_rows = torch.ones_like(live) if mutant == "kd_on_dead_rows" else live
    nll = float(nll_row[live].sum() / count)
    kd = float(rowkd[kd_rows].sum() / count)
    loss = (1.0 - lam) * nll + lam * kd if lam < 1.0 else kd
    onehot = torch.zeros_like(x).scatter_(1, t[:, None], 1.0)
    gt = 1.0 if mutant == "no_tau_in_gradient" else tau
    scale = GRAD_SCALE * GRAD_OUT / count
    hard = (1.0 - lam) * (torch.exp(x - lse[:, None]) - onehot) * live[:, None]
    soft = lam * gt * (torch.exp(logpt) - q) * kd_rows[:, None]
    dl_full = torch.zeros((case.M, case.ldv), dtype=torch.float64)
    dl_full[:, :V] = (hard + soft) * scale
    return dict(lse=lse, lse_xt=lse_xt, lse_a=lse_a, lse_b=lse_b, rowkd=rowkd, q=q, d=d, loss=loss, nll=nll, kd=kd, count=count, live=live,
                dlogits=dl_full)


@functools.lru_cache(maxsize=None)
def reference(case: Case) -> dict:
    return ref(case)


def standin(case: Case) -> dict:
    """torch fp32 arithmetic in the kernels' place: fp32 row constants, q, terms and row sums; the objective formed and summed in fp64; the gradient
    in fp32 with one rounding to the student's dtype."""
    inp = inputs(case)
    V, tgt = case.V, inp["tgt"]
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    k, alpha, tau, lam = f(1.0) / f(case.tau), f(case.alpha), f(case.tau), f(case.lam)
    x, a = inp["xbuf"][:, :V].float(), inp["abuf"][:, :V].float()
    lse, lse_xt, lse_a = torch.logsumexp(x, 1), torch.logsumexp(x * k, 1), torch.logsumexp(a * k, 1)
    logpt = x * k - lse_xt[:, None]
    if case.two:
        b = inp["bbuf"][:, :V].float()
        lse_b = torch.logsumexp(b * k, 1)
        q = alpha * torch.exp(a * k - lse_a[:, None]) + (f(1.0) - alpha) * torch.exp(b * k - lse_b[:, None])
        lq = torch.log(q)
    else:
        lse_b = torch.zeros_like(lse)
        lq = a * k - lse_a[:, None]
        q = torch.exp(lq)
    term = torch.where(q > 0, q * (lq - logpt), torch.zeros_like(q))
    rowkd = tau * tau * term.sum(1)
    live = live_rows(case, tgt)
    t = tgt.clamp(0, V - 1)
    xt = x.gather(1, t[:, None])[:, 0]
    count = float(live.sum())
    plain, kdr = (lse - xt).double(), rowkd.double()
    obj = (1.0 - case.lam) * plain + case.lam * kdr if case.lam < 1.0 else kdr
    sc = f(GRAD_SCALE) * f(GRAD_OUT) / f(count)
    onehot = torch.zeros_like(x).scatter_(1, t[:, None], 1.0)
    g = ((f(1.0) - lam) * (torch.exp(x - lse[:, None]) - onehot) + lam * tau * (torch.exp(logpt) - q)) * sc
    dl = torch.zeros((case.M, case.ldv), dtype=case.sdt)
    dl[:, :V] = torch.where(live[:, None], g, torch.zeros_like(g)).to(case.sdt)
    mean = lambda r: float((r[live].sum() / count).float())  # noqa: E731
    z = torch.zeros_like(lse)
    lse4 = torch.stack([torch.where(live, v, z) for v in (lse, lse_xt, lse_a, lse_b)])
    return dict(lse4=lse4, rowkd=torch.where(live, rowkd, z), loss=mean(obj), nll=mean(plain), kd=mean(kdr), count=count, dlogits=dl)


def _worst(err: torch.Tensor, allowed: torch.Tensor) -> float:
    """max of err / allowed; an error that is NaN, or positive where nothing is allowed, counts as infinite."""
    r = torch.where(err == 0, torch.zeros_like(err), err / allowed)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


def _scalar_ratio(got: float, want: float, allowed: float) -> float:
    if math.isinf(want):
        return 0.0 if got == want else math.inf
    if not math.isfinite(got):
        return math.inf
    return 0.0 if got == want else abs(got - want) / allowed


def _mag(z: Optional[torch.Tensor], like: torch.Tensor) -> torch.Tensor:
    if z is None:
        return torch.zeros_like(like)
    return torch.where(torch.isfinite(z), z.abs(), torch.zeros_like(z))


@functools.lru_cache(maxsize=None)
def bounds(case: Case) -> dict:
    """The derived bounds of the module docstring: rowkd [live rows], kd, and the row sum of dlogits [live rows]."""
    r, inp, V, tau = reference(case), inputs(case), case.V, case.tau
    k, n = 1.0 / tau, adds(case)
    x = inp["xbuf"][:, :V].double()
    a = inp["abuf"][:, :V].double()
    b = inp["bbuf"][:, :V].double() if case.two else None
    A = k * (_mag(x, x) + _mag(a, x) + _mag(b, x)) + (r["lse_xt"].abs() + r["lse_a"].abs() + r["lse_b"].abs())[:, None]
    E = U * (n + 8 + 4 * A)
    q, d = r["q"], r["d"]
    floor = tau * tau * V * 2.0 ** -126 * 256
    rowkd = tau * tau * ((q * (1 + d.abs()) * E).sum(1) + n * U * (q * d).abs().sum(1)) + U * r["rowkd"].abs() + floor
    live = r["live"]
    kd = float(rowkd[live].sum() / r["count"]) + U * abs(r["kd"])
    Ep = U * (n + 8 + 4 * (A + _mag(x, x) + r["lse"].abs()[:, None]))
    scale = GRAD_SCALE * GRAD_OUT / r["count"]
    gsize = ((1.0 - case.lam) + case.lam * tau) * scale
    rowsum = 2.0 * gsize * (UNIT[case.sdt] + Ep.max(1).values)
    return dict(rowkd=rowkd[live], kd=kd, dlogits_rowsum=rowsum[live], gsize=gsize)


def ratios(case: Case, out: dict) -> dict:
    """{check: worst error / bound} of a result `out` (keys lse4 [4, M], rowkd [M], loss, nll, kd, count, dlogits [M, ldv]).  <= 1 everywhere passes."""
    r, V, sdt = reference(case), case.V, case.sdt
    bd = bounds(case)
    live = r["live"]
    as64 = lambda t: t.detach().cpu().double()  # noqa: E731
    res = {}
    t32 = KR.tol(F32, 1.0)
    lse4 = as64(out["lse4"])
    names = ("lse", "lse_xt", "lse_a") + (("lse_b",) if case.two else ())
    for i, name in enumerate(names):
        res[name] = _worst((lse4[i][live] - r[name][live]).abs(), t32["atol"] + t32["rtol"] * r[name][live].abs())
    res["rowkd"] = _worst((as64(out["rowkd"])[live] - r["rowkd"][live]).abs(), bd["rowkd"])
    res["loss"] = _scalar_ratio(float(out["loss"]), r["loss"], LOSS_RTOL[sdt] * abs(r["loss"]))
    res["nll"] = _scalar_ratio(float(out["nll"]), r["nll"], LOSS_RTOL[sdt] * abs(r["nll"]))
    res["kd"] = _scalar_ratio(float(out["kd"]), r["kd"], bd["kd"])
    res["count"] = 0.0 if float(out["count"]) == float(r["count"]) else math.inf
    dl = as64(out["dlogits"])
    assert tuple(dl.shape) == (case.M, case.ldv), tuple(dl.shape)
    td, want = KR.tol(F32, bd["gsize"]), r["dlogits"][:, :V]
    allowed = (td["atol"] + td["rtol"] * want.abs()) * (1 + UNIT[BF16]) + (UNIT[BF16] * want.abs() if sdt == BF16 else 0.0)
    res["dlogits"] = _worst((dl[:, :V] - want).abs(), allowed)
    res["dlogits_rowsum"] = _worst(dl[:, :V][live].sum(1).abs(), bd["dlogits_rowsum"])
    return res


def check(case: Case, out: dict) -> dict:
    """Prints every error / bound, then asserts them all."""
    res = ratios(case, out)
    print(f"distillation {case.name}: error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, f"distillation {case.name}: error / bound above 1: {bad}"
    return res


def check_zero_bits(case: Case, dl_full: torch.Tensor) -> None:
    """Padding columns and ignored rows of the [M, ldv] gradient buffer are +0, bit for bit."""
    r = reference(case)
    dl_full = dl_full.detach().cpu()
    assert bool((KR.bits(dl_full[:, case.V:]) == 0).all()), f"distillation {case.name}: dlogits padding columns are not +0"
    assert bool((KR.bits(dl_full[~r["live"]]) == 0).all()), f"distillation {case.name}: ignored rows have a gradient"
