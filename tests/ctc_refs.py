"""Float64 reference, error bounds and the case table of the CTC auxiliary head (omr_ctc_fwd / omr_ctc_bwd / omr_ctc_frames_* / omr_ctc_greedy).

tests/test_ctc_kernels_gpu.py, test_ctc_frames_gpu.py and test_ctc_greedy_gpu.py run the cases through the HIP kernels; tests/test_ctc_refs_cpu.py
holds the references themselves to torch on the CPU (F.ctc_loss and its autograd gradient in fp64, F.avg_pool2d, a brute-force collapse) and
asserts which samples of the case table are feasible.

Definition.  Sample b's labels are the prefix of targets[b] before the first element equal to `blank` or `eos`; L_b their number.  With
lp = log_softmax(logits[b, f]) over the columns v < V and the lattice states 0 .. 2 L_b (even: blank, 2 j + 1: label j),
    nll_b = -log P_b (the sum over all alignments of the F_b frames),   loss = (1 / B) sum_b nll_b / max(L_b, 1),
    post[b, f, v] = sum over the states s that carry v of alpha[f, s] beta[f, s] / (P_b exp(lp[f, v])),
    dlogits[b, f, v] = s_b (softmax(logits[b, f])[v] - post[b, f, v]),   s_b = grad_scale grad_out / (B max(L_b, 1)).
A sample with P_b = 0 (F_b < L_b + repeats_b, or -inf logits) is infeasible: nll_b counts 0 and its gradient is +0 (torch's zero_infinity).

Reference.  alpha and beta in fp64 log space, each frame's maximum taken out and the offsets summed in extended precision (np.longdouble), so
that the reference stays accurate to ~1e-14 where torch's own fp64 recursion (|log alpha| up to ~1e4 on the long case, one fp64 ulp of that is
2e-12) does not: the self-check scales its 1e-12 by max(1, max |log alpha| / 100).  bf16 cases are computed from the rounded inputs.

Bounds.  u = 2^-24.
  lse          the project's fp32 tolerance (oracle/kernel_refs.tol), as for every loss kernel.
  rows (nll)   4 x |torch fp32 CPU ctc_loss - fp64| of the same sample: the recursion's rounding is not closed in a derivation here (the kernel
               adds in another order than torch, and keeps its values near 0 by an fp64 offset, so it has to BEAT torch's fp32 on the long
               case, not match it), plus the frames' log-sum-exp term: every alignment holds each frame's lse once, so the lse errors add up
               over the F_b frames, each at most E_f = u (adds + 8 + 4 (max_v |x_fv| + |lse_f|)) in the manner of distill_refs (adds = the longest
               chain of fp32 additions of the row pass: VEC ceil(V / (256 VEC)) + 6 + 3), plus the fp32 rounding u |nll| of the result.
  loss         the mean of the row bounds over max(L_b, 1), plus u |loss|.
  dlogits      4 x the largest |torch fp32 autograd gradient - fp64| over the SAMPLE (the error of log alpha / log beta at a frame is the
               rounding accumulated over all frames before / behind it, so the yardstick is the sample's worst element: at single frames
               torch's two accumulated errors happen to cancel, which says nothing about another summation order), plus
               s_b (p_v + post_v) (E_f + 8 u) for the two exponentials against the fp32 lse, plus s_b u, plus for bf16 half an output ulp
               2^-8 |dlogits|.
  row sums     the exact gradient of a frame sums to 0 over v < V: |sum_v dlogits| <= the sum of the frame's element bounds.
Infeasible samples, the columns [V, ldv) and the frames >= F_b are +0 bit for bit.

Test infrastructure only: nothing here is imported by the package.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import kernel_refs as KR

F32, BF16 = KR.F32, KR.BF16
U = KR.U24
UNIT = {F32: 2.0 ** -24, BF16: 2.0 ** -8}
BLANK, SOS, EOS = 0, 1, 2                       # the vocabulary's <PAD> is the blank; labels are drawn from [3, V)
GRAD_SCALE, GRAD_OUT = 0.5, 3.0
NEG_INF = float("-inf")


# ================================================================================================ the loss

def labels_of(row, blank: int = BLANK, eos: int = EOS) -> List[int]:
    out = []
    for t in (int(v) for v in row):
        if t == blank or t == eos:
            break
        out.append(t)
    return out


def _sweep(e: np.ndarray, ext: np.ndarray):
    """Normalised log alpha of emissions e [F, S] over the extended labels ext [S] -> (stored [F, S] <= 0, offsets longdouble [F])."""
    Fn, S = e.shape
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != BLANK) & (ext[2:] != ext[:-2])
    st = np.full((Fn, S), NEG_INF)
    off = np.zeros(Fn, dtype=np.longdouble)
    a = np.full(S, NEG_INF)
    a[0] = e[0, 0]
    if S > 1:
        a[1] = e[0, 1]
    total = np.longdouble(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(Fn):
            if t > 0:
                a1, a2 = np.full(S, NEG_INF), np.full(S, NEG_INF)
                a1[1:] = a[:-1]
                a2[2:] = np.where(skip[2:], a[:-2], NEG_INF)
                a = e[t] + np.logaddexp(np.logaddexp(a, a1), a2)
            m = a.max()
            if np.isfinite(m):
                a = a - m
                total = total + np.longdouble(m)
            st[t], off[t] = a, total
    return st, off


@dataclass
class SampleRef:
    L: int
    F: int
    feasible: bool
    nll: float
    max_log: float                              # max |log alpha| over the finite values: what torch's un-normalised fp64 recursion carries
    post: Optional[np.ndarray]                  # [F, V]


def sample_ref(x: np.ndarray, labels: List[int]) -> Tuple[SampleRef, np.ndarray, np.ndarray]:
    """x fp64 [F, V] -> (SampleRef, lse [F], softmax [F, V])."""
    Fn, V = x.shape
    L = len(labels)
    with np.errstate(invalid="ignore", divide="ignore"):
        mx = x.max(1, keepdims=True)
        lse = (mx + np.log(np.exp(x - mx).sum(1, keepdims=True)))[:, 0]
        lp = x - lse[:, None]
    soft = np.exp(lp)
    ext = np.full(2 * L + 1, BLANK, dtype=np.int64)
    ext[1::2] = labels
    e = lp[:, ext]
    al, oa = _sweep(e, ext)
    be_r, ob_r = _sweep(e[::-1, ::-1], ext[::-1])
    be, ob = be_r[::-1, ::-1], ob_r[::-1]
    S = 2 * L + 1
    with np.errstate(invalid="ignore", divide="ignore"):
        tail = np.logaddexp(al[-1, S - 1], al[-1, S - 2]) if S > 1 else al[-1, 0]
    if not np.isfinite(tail):
        return SampleRef(L, Fn, False, 0.0, 0.0, None), lse, soft
    logp = oa[-1] + np.longdouble(tail)
    c = (oa + ob - logp).astype(np.float64)                                        # [F]
    with np.errstate(invalid="ignore", divide="ignore"):
        z = al + be + c[:, None] - e
    ps = np.where(np.isfinite(al) & np.isfinite(be), np.exp(np.where(np.isfinite(z), z, NEG_INF)), 0.0)
    post = np.zeros((Fn, V))
    for s in range(S):
        post[:, ext[s]] += ps[:, s]
    full = al + oa.astype(np.float64)[:, None]
    max_log = float(np.abs(full[np.isfinite(full)]).max())
    return SampleRef(L, Fn, True, float(-logp), max_log, post), lse, soft


# ================================================================================================ the case table

@dataclass(frozen=True)
class Case:
    name: str
    dtype: torch.dtype
    V: int
    T: int                                       # width of the target rows
    frames: Tuple[int, ...]                      # F_b
    labels: Tuple[Tuple[int, ...], ...]          # every sample's labels
    infeasible: Tuple[int, ...] = ()             # the samples designated infeasible
    sigma: float = 2.0
    pad_cols: bool = True                        # ldv = V rounded up to 8 with NaN behind V; False: ldv = V
    neg_inf_label: Tuple[int, ...] = ()          # samples whose first label's column is -inf on every frame

    @property
    def B(self) -> int:
        return len(self.frames)

    @property
    def Fmax(self) -> int:
        return max(self.frames)

    @property
    def ldv(self) -> int:
        return KR.round_up(self.V, 8) if self.pad_cols else self.V


def _rand_labels(n: int, V: int, seed: int) -> Tuple[int, ...]:
    g = torch.Generator().manual_seed(seed)
    return tuple(int(v) for v in torch.randint(3, V, (n,), generator=g))


def _need(labels) -> int:
    """Frames a label sequence needs: L + the number of adjacent repeats."""
    return len(labels) + sum(1 for a, b in zip(labels, labels[1:]) if a == b)


def _cases():
    out = []
    for dt in (F32, BF16):
        tag = KR.TAG[dt]
        wave = tuple(_rand_labels(n, 30, 100 + n) for n in (0, 1, 63, 64, 65))
        out.append(Case(f"{tag}-wave-edges", dt, 30, 66, tuple(_need(lb) + 3 for lb in wave), wave))          # L around one wave of threads
        l512 = _rand_labels(512, 30, 7)
        out.append(Case(f"{tag}-L512", dt, 30, 512, (_need(l512) + 5,), (l512,)))                              # 1 025 states, no terminator in the row
        rep = ((5, 5, 5), (5, 6, 6, 5), (7, 7), (4, 5, 4, 5))
        out.append(Case(f"{tag}-repeats", dt, 30, 6, (5, 9, 3, 4), rep))                                       # a a a in exactly L + repeats frames: one path
        out.append(Case(f"{tag}-F1", dt, 30, 3, (1, 1), ((), (9,))))
        out.append(Case(f"{tag}-infeasible", dt, 30, 5, (3, 6, 6), ((5, 5, 6), (8, 9), (8, 9)), infeasible=(0, 1), neg_inf_label=(1,)))   # 0: one frame short
        out.append(Case(f"{tag}-long-thin", dt, 30, 4, (2048,), ((4, 9, 4),), sigma=3.0))                      # the precision case
        out.append(Case(f"{tag}-ragged", dt, 30, 9, (17, 40, 5), (_rand_labels(6, 30, 1), _rand_labels(8, 30, 2), (3,))))
        out.append(Case(f"{tag}-contiguous", dt, 30, 4, (6, 7), ((3, 4), (5,)), pad_cols=False))               # ldv = V = 30: the scalar row pass
        out.append(Case(f"{tag}-V2101", dt, 2101, 5, (12, 9), (_rand_labels(4, 2101, 3), _rand_labels(3, 2101, 4))))
        out.append(Case(f"{tag}-V6997", dt, 6997, 12, (40,), (_rand_labels(10, 6997, 5),)))
        many = tuple(_rand_labels(b % 5, 30, 200 + b) for b in range(70))
        out.append(Case(f"{tag}-B70", dt, 30, 5, tuple(_need(lb) + 1 + b % 4 for b, lb in enumerate(many)), many))
    return tuple(out)


CASES = _cases()


@functools.lru_cache(maxsize=None)
def inputs(case: Case) -> dict:
    """-> buf [B, Fmax, ldv] of case.dtype (NaN in the padding columns and in the frames >= F_b), frame_len int32 [B], targets int64 [B, T]."""
    g = torch.Generator().manual_seed(len(case.name) * 1000 + case.V + case.Fmax)
    x = (torch.randn((case.B, case.Fmax, case.V), generator=g) * case.sigma).to(case.dtype)
    for b in case.neg_inf_label:
        x[b, :, case.labels[b][0]] = NEG_INF
    buf = torch.full((case.B, case.Fmax, case.ldv), float("nan"), dtype=case.dtype)
    buf[:, :, :case.V] = x
    for b, n in enumerate(case.frames):
        buf[b, n:] = float("nan")
    tgt = torch.zeros((case.B, case.T), dtype=torch.int64)
    for b, lb in enumerate(case.labels):
        assert len(lb) <= case.T
        tgt[b, :len(lb)] = torch.tensor(lb, dtype=torch.int64)
        if len(lb) < case.T:
            tgt[b, len(lb)] = EOS if b % 2 == 0 else BLANK                 # either terminator ends the labels
        if len(lb) + 2 < case.T:
            tgt[b, len(lb) + 2] = 7                                         # behind the terminator: never a label
    return dict(buf=buf, frame_len=torch.tensor(case.frames, dtype=torch.int32), targets=tgt)


@functools.lru_cache(maxsize=None)
def reference(case: Case) -> dict:
    inp = inputs(case)
    assert all(tuple(labels_of(inp["targets"][b].tolist())) == tuple(case.labels[b]) for b in range(case.B))
    return reference_of(inp["buf"][:, :, :case.V], case.frames, case.labels)


def reference_of(x: torch.Tensor, frames, labels) -> dict:
    """The fp64 reference of logits x [B, Fmax, V] (any dtype; what lies in the frames >= F_b is not read), F_b = frames[b], labels[b]."""
    B, Fm, V = x.shape
    x = x.double().numpy()
    rows, feas, Ls, max_log = np.zeros(B), np.zeros(B, dtype=bool), np.zeros(B, dtype=np.int64), 0.0
    lse = np.zeros((B, Fm))
    soft, post, dl = np.zeros((B, Fm, V)), np.zeros((B, Fm, V)), np.zeros((B, Fm, V))
    for b in range(B):
        n = frames[b]
        r, l, s = sample_ref(x[b, :n], list(labels[b]))
        Ls[b], feas[b], rows[b] = r.L, r.feasible, r.nll
        lse[b, :n], soft[b, :n] = l, s
        if r.feasible:
            max_log = max(max_log, r.max_log)
            post[b, :n] = r.post
            dl[b, :n] = (s - r.post) * (GRAD_SCALE * GRAD_OUT / (B * max(r.L, 1)))
    loss = float((rows / np.maximum(Ls, 1)).sum() / B)
    return dict(rows=rows, feasible=feas, L=Ls, loss=loss, lse=lse, soft=soft, post=post, dlogits=dl, max_log=max_log)


def torch_ctc(case: Case, dtype: torch.dtype):
    """F.ctc_loss on the CPU in `dtype` (fp64: what the reference is held to; fp32: the yardstick of the recursion's error) ->
    (loss, rows [B], the autograd gradient of GRAD_SCALE * GRAD_OUT * loss w.r.t. the logits [B, Fmax, V], zeros in the frames >= F_b)."""
    return torch_ctc_of(inputs(case)["buf"][:, :, :case.V], case.frames, case.labels, dtype)


def torch_ctc_of(x: torch.Tensor, frames, labels, dtype: torch.dtype):
    B = x.shape[0]
    x = torch.nan_to_num(x.to(dtype), nan=0.0, neginf=NEG_INF).requires_grad_(True)
    lens = torch.tensor([len(lb) for lb in labels], dtype=torch.int64)
    tg = torch.zeros((B, max(1, int(lens.max()))), dtype=torch.int64)
    for b, lb in enumerate(labels):
        tg[b, :len(lb)] = torch.tensor(lb, dtype=torch.int64)
    lp = F.log_softmax(x, dim=2).permute(1, 0, 2)
    flen = torch.tensor(list(frames), dtype=torch.int64)
    rows = F.ctc_loss(lp, tg, flen, lens, blank=BLANK, reduction="none", zero_infinity=True)
    loss = F.ctc_loss(lp, tg, flen, lens, blank=BLANK, reduction="mean", zero_infinity=True)
    (g,) = torch.autograd.grad(loss * (GRAD_SCALE * GRAD_OUT), x)
    g = torch.nan_to_num(g.detach(), nan=0.0)
    for b, n in enumerate(frames):
        g[b, n:] = 0
    return float(loss.detach()), rows.detach().double().numpy(), g.double().numpy()


def row_adds(dtype, V: int) -> int:
    vec = KR.VEC[dtype]
    return vec * math.ceil(V / (256 * vec)) + 6 + 3


@functools.lru_cache(maxsize=None)
def bounds(case: Case) -> dict:
    return bounds_of(inputs(case)["buf"][:, :, :case.V], case.frames, case.labels, reference(case))


def bounds_of(xt: torch.Tensor, frames, labels, r: dict) -> dict:
    """The bounds of the module docstring for logits xt [B, Fmax, V] of the kernel's dtype; r = reference_of(xt, frames, labels)."""
    B, Fm, V = xt.shape
    _, rows32, g32 = torch_ctc_of(xt, frames, labels, torch.float32)
    _, _, g64 = torch_ctc_of(xt, frames, labels, torch.float64)
    x = torch.nan_to_num(xt.double(), nan=0.0, neginf=0.0, posinf=0.0).abs().numpy()
    E = U * (row_adds(xt.dtype, V) + 8 + 4 * (x.max(2) + np.abs(r["lse"])))           # [B, Fmax]
    live = np.arange(Fm)[None, :] < np.asarray(frames)[:, None]
    E = E * live
    rows = 4 * np.abs(rows32 - r["rows"]) + E.sum(1) + U * np.abs(r["rows"])
    rows = rows * r["feasible"]
    loss = float((rows / np.maximum(r["L"], 1)).sum() / B) + U * abs(r["loss"])
    s = (GRAD_SCALE * GRAD_OUT / (B * np.maximum(r["L"], 1)))[:, None, None]
    dl = 4 * np.abs(g32 - g64).max(axis=(1, 2), keepdims=True) + s * (r["soft"] + r["post"]) * (E[:, :, None] + 8 * U) + s * U \
        + (UNIT[BF16] * np.abs(r["dlogits"]) if xt.dtype == BF16 else 0.0)
    dl = dl * (r["feasible"][:, None, None] & live[:, :, None])
    return dict(rows=rows, loss=loss, dlogits=dl, rowsum=dl.sum(2))


def _worst(err: np.ndarray, allowed: np.ndarray) -> float:
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / allowed)
    r = np.where(np.isnan(r), math.inf, r)
    return float(r.max()) if r.size else 0.0


def ratios(case: Case, out: dict) -> dict:
    """{quantity: worst error / bound} of a result `out` (loss, rows [B], infeasible, lse [B, Fmax], dlogits [B, Fmax, ldv]); <= 1 passes."""
    r, bd, V = reference(case), bounds(case), case.V
    as64 = lambda t: t.detach().cpu().double().numpy()  # noqa: E731
    live = np.arange(case.Fmax)[None, :] < np.asarray(case.frames)[:, None]
    t32 = KR.tol(F32, 1.0)
    res = {}
    res["lse"] = _worst(np.abs(as64(out["lse"]) - r["lse"])[live], (t32["atol"] + t32["rtol"] * np.abs(r["lse"]))[live])
    res["rows"] = _worst(np.abs(as64(out["rows"]) - r["rows"]), bd["rows"])
    res["loss"] = _worst(np.abs(np.array([float(out["loss"])]) - r["loss"]), np.array([bd["loss"]]))
    res["infeasible"] = 0.0 if int(out["infeasible"]) == int((~r["feasible"]).sum()) else math.inf
    dl = as64(out["dlogits"])
    assert dl.shape == (case.B, case.Fmax, case.ldv), dl.shape
    res["dlogits"] = _worst(np.abs(dl[:, :, :V] - r["dlogits"]), bd["dlogits"])
    res["rowsum"] = _worst(np.abs(dl[:, :, :V].sum(2)), bd["rowsum"])
    return res


def check(case: Case, out: dict) -> dict:
    """Prints every error / bound, then asserts them all."""
    res = ratios(case, out)
    print(f"ctc {case.name}: error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, f"ctc {case.name}: error / bound above 1: {bad}"
    return res


def check_zero_bits(case: Case, dl_full: torch.Tensor, rows: torch.Tensor) -> None:
    """+0 bit for bit: the columns [V, ldv), the frames >= F_b, every frame and the nll of an infeasible sample."""
    r = reference(case)
    dl_full = dl_full.detach().cpu()
    assert bool((KR.bits(dl_full[:, :, case.V:]) == 0).all()), f"ctc {case.name}: dlogits padding columns are not +0"
    for b, n in enumerate(case.frames):
        assert bool((KR.bits(dl_full[b, n:]) == 0).all()), f"ctc {case.name}: sample {b} has a gradient behind its {n} frames"
        if not r["feasible"][b]:
            assert bool((KR.bits(dl_full[b]) == 0).all()), f"ctc {case.name}: infeasible sample {b} has a gradient"
            assert int(KR.bits(rows.detach().cpu()[b:b + 1])[0]) == 0, f"ctc {case.name}: infeasible sample {b} has a loss"


# ================================================================================================ frames

def frame_count(gh: int, gw: int, pool: int) -> int:
    return -(-gh // pool) * gw


def frames_ref(mem: torch.Tensor, grids, pool: int, fmax: int) -> Tuple[torch.Tensor, List[int]]:
    """The documented order in numpy fp32: mem [B, S, d] (sample b's gh x gw grid row-major, pitch gw) -> (frames [B, fmax, d], [F_b])."""
    B, S, d = mem.shape
    x = mem.float().numpy()
    out = np.zeros((B, fmax, d), dtype=np.float32)
    lens = []
    for b, (gh, gw) in enumerate(grids):
        G = -(-gh // pool)
        lens.append(G * gw)
        for j in range(gw):
            for q in range(G):
                r0, r1 = q * pool, min((q + 1) * pool, gh)
                s = x[b, r0 * gw + j].copy()
                for i in range(r0 + 1, r1):
                    s = s + x[b, i * gw + j]                                       # fp32 additions, top to bottom
                out[b, j * G + q] = s if r1 - r0 == 1 else s / np.float32(r1 - r0)  # one IEEE division; a group of one row is a copy
    return torch.from_numpy(out).to(mem.dtype), lens


def frames_bwd_ref(g: torch.Tensor, grids, pool: int, S: int) -> torch.Tensor:
    """The adjoint: every grid row gets its frame's gradient over the frame's row count, rounded once."""
    B, fmax, d = g.shape
    x = g.float().numpy()
    out = np.zeros((B, S, d), dtype=np.float32)
    for b, (gh, gw) in enumerate(grids):
        G = -(-gh // pool)
        for i in range(gh):
            q = i // pool
            cnt = min((q + 1) * pool, gh) - q * pool
            for j in range(gw):
                v = x[b, j * G + q]
                out[b, i * gw + j] = v if cnt == 1 else v / np.float32(cnt)
    return torch.from_numpy(out).to(g.dtype)


def frames_torch(mem: torch.Tensor, gh: int, gw: int, pool: int) -> torch.Tensor:
    """One sample [gh * gw, d] -> [F, d] by torch: avg_pool2d over the grid rows (ceil_mode, the last group averages the rows that exist), then
    the transpose that reads columns first."""
    d = mem.shape[1]
    g = mem.double().view(gh, gw, d).permute(2, 0, 1).unsqueeze(0)                 # [1, d, gh, gw]
    p = F.avg_pool2d(g, kernel_size=(pool, 1), ceil_mode=True, count_include_pad=False)[0]   # [d, G, gw]
    return p.permute(2, 1, 0).reshape(-1, d)                                       # frame j * G + q


# ================================================================================================ greedy

def greedy_ref(logits: np.ndarray, frame_len, blank: int = BLANK):
    """logits [B, Fmax, V] -> (tokens [[..]], arg [B, Fmax] with blank behind F_b): arg-max with ties to the lowest index, repeats collapsed,
    blanks dropped."""
    B, Fm, _ = logits.shape
    arg = np.full((B, Fm), blank, dtype=np.int64)
    toks = []
    for b in range(B):
        n = int(frame_len[b])
        arg[b, :n] = logits[b, :n].argmax(1)                                       # numpy: the first maximum
        seq, prev = [], -1
        for a in arg[b, :n].tolist():
            if a != prev and a != blank:
                seq.append(a)
            prev = a
        toks.append(seq)
    return toks, arg
