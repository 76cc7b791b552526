"""Reference, yardstick and case table of the CTC prefix scores (omr_ctc_prefix_init / _scores / _advance; include/omr_hip.h "joint CTC /
attention beam search").

Definition (per input, frames f = 0 .. F - 1, y_f(v) = logit[f][v] - lse[f], blank = <PAD>).  A hypothesis g keeps
    gn[f] / gb[f]   log P(frames 0..f emit exactly g, the last one a label / a blank);   empty g: gn = -inf, gb[f] = sum_{k <= f} y_k(blank)
    logpsi          log P(the frames emit something that starts with g); 0 for the empty g
and a label c extends it to h = g c by
    phi[f]  = logaddexp(gb^g[f], -inf if c == last(g) else gn^g[f]),     phi[-1] = 0 if g is empty else -inf
    gn^h[f] = logaddexp(gn^h[f-1], phi[f-1]) + y_f(c),   gb^h[f] = logaddexp(gb^h[f-1], gn^h[f-1]) + y_f(blank),   gn^h[-1] = gb^h[-1] = -inf
    logpsi(h) = logaddexp over f of (phi[f-1] + y_f(c)), accumulated in frame order.
<eos>: logpsi = logaddexp(gn^g[F-1], gb^g[F-1]) (F = 0: 0 for the empty g, else -inf); blank, <sos>, anything outside [0, V): -inf.
    delta(g, c) = -inf if logpsi(g c) == -inf else min(logpsi(g c) - logpsi(g), 0).

`run_chain(case, dtype)` evaluates exactly these formulae with every array in `dtype`: np.float64 is the reference, np.float32 the
yardstick -- "the same formulae in plain numpy float32".  The kernel may err 4 x the yardstick's largest error over the same case and the
same kind of output (delta / stored rows / logpsi), plus, for bf16 logits, half a bf16 ulp of the largest logit (2^-9 max |x|): the margin
tests/ctc_refs.py gives omr_ctc_fwd against torch's fp32.  bf16 cases are computed from the rounded inputs.  An output that is -inf in the
reference must be -inf.

`brute_*`: all V^F alignments of a tiny input, for the self-checks of tests/test_ctc_prefix_refs_cpu.py.

Test infrastructure only: nothing here is imported by the package.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

BLANK, SOS, EOS = 0, 1, 2                       # labels are the tokens [3, V)
NINF = float("-inf")
CHUNK = 32                                      # frames per LDS tile of ctc_prefix_kernel (PFX_CH of csrc/ctc_prefix.hip)
F32, BF16 = "fp32", "bf16"


# ================================================================================================ the formulae, in any numpy dtype

def lse_rows(x: np.ndarray) -> np.ndarray:
    """log sum_v exp(x[f][v]) in x's dtype."""
    with np.errstate(invalid="ignore", divide="ignore"):
        m = x.max(axis=1)
        return m + np.log(np.exp(x - m[:, None]).sum(axis=1, dtype=x.dtype))


@dataclass
class Hyp:
    gn: np.ndarray          # [F]
    gb: np.ndarray          # [F]
    logpsi: float           # a numpy scalar of the dtype
    last: int


def empty_hyp(y: np.ndarray, sos: int = SOS) -> Hyp:
    dt = y.dtype.type
    F = y.shape[0]
    gb = np.empty(F, dtype=dt)
    acc = dt(0)
    for f in range(F):
        acc = dt(acc + y[f, BLANK])
        gb[f] = acc
    return Hyp(np.full(F, NINF, dtype=dt), gb, dt(0), sos)


def is_label(c: int, V: int, sos: int = SOS, eos: int = EOS) -> bool:
    return 0 <= c < V and c not in (BLANK, sos, eos)


def extend(y: np.ndarray, g: Hyp, c: int, sos: int = SOS, eos: int = EOS) -> Tuple[Optional[Hyp], float]:
    """-> (h = g c for a label c, else None; logpsi(g c)).  sos / eos: the two specials besides the blank (the brute-force checks put them
    outside a vocabulary of 3)."""
    dt = y.dtype.type
    F, V = y.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if c == eos:
            if F == 0:
                return None, dt(0) if g.last == sos else dt(NINF)
            return None, dt(np.logaddexp(g.gn[F - 1], g.gb[F - 1]))
        if not is_label(c, V, sos, eos):
            return None, dt(NINF)
        gn, gb = np.full(F, NINF, dtype=dt), np.full(F, NINF, dtype=dt)
        pn, pb, psi = dt(NINF), dt(NINF), dt(NINF)
        for f in range(F):
            if f == 0:
                phi = dt(0) if g.last == sos else dt(NINF)
            else:
                phi = dt(np.logaddexp(g.gb[f - 1], dt(NINF) if c == g.last else g.gn[f - 1]))
            nn = dt(np.logaddexp(pn, phi) + y[f, c])
            nb = dt(np.logaddexp(pb, pn) + y[f, BLANK])
            psi = dt(np.logaddexp(psi, dt(phi + y[f, c])))
            pn, pb = nn, nb
            gn[f], gb[f] = nn, nb
    return Hyp(gn, gb, psi, c), psi


def delta_of(psi_h, psi_g):
    dt = type(psi_h)
    if psi_h == NINF:
        return dt(NINF)
    return min(dt(psi_h - psi_g), dt(0))


# ================================================================================================ the case table

@dataclass(frozen=True)
class Case:
    name: str
    dtype: str
    V: int
    beam: int
    frames: Tuple[int, ...]         # F_n per input
    seed: int
    positions: int = 4
    scale: float = 2.0              # logits are scale * N(0, 1)

    @property
    def N(self) -> int:
        return len(self.frames)

    @property
    def Fmax(self) -> int:
        return max(max(self.frames), 1)

    @property
    def ldv(self) -> int:
        return (self.V + 7) // 8 * 8


def _cases() -> List[Case]:
    out, seed = [], 100
    for dt in (F32, BF16):
        for name, V, beam, frames in [
                ("F1", 11, 3, (1, 1)), ("F2", 11, 8, (2, 2)),
                ("chunk-1", 13, 3, (CHUNK - 1,)), ("chunk", 13, 8, (CHUNK,)), ("chunk+1", 21, 3, (CHUNK + 1,)), ("2chunk+1", 21, 8, (2 * CHUNK + 1,)),
                ("ragged", 19, 4, (2 * CHUNK + 5, 0, 7)), ("ragged8", 30, 8, (5, 3 * CHUNK - 2))]:
            seed += 1
            out.append(Case(f"{dt}-{name}", dt, V, beam, frames, seed))
    out.append(Case("fp32-long", F32, 24, 4, (1500,), 300, positions=3, scale=3.0))
    return out


CASES = _cases()


def inputs(case: Case) -> Dict[str, torch.Tensor]:
    """buf [N, Fmax, ldv] in the case's dtype (the padding columns and the frames >= F_n hold a large value no kernel may read into a result),
    frame_len int32 [N]."""
    g = torch.Generator().manual_seed(case.seed)
    x = torch.randn((case.N, case.Fmax, case.ldv), generator=g) * case.scale
    x[:, :, case.V:] = 77.0
    for n, F in enumerate(case.frames):
        x[n, F:, :] = 99.0
    dt = torch.float32 if case.dtype == F32 else torch.bfloat16
    return dict(buf=x.to(dt), frame_len=torch.tensor(case.frames, dtype=torch.int32))


def plan(case: Case, pos: int, lasts: List[int]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """What the chain does at position `pos`, given every row's last token: (cand int64 [rows, beam], parents int32 [rows], tokens int64
    [rows]).  Candidate 0 of a row is its own last token (<sos> at position 0, the repeat rule behind it), candidate 1 alternates between
    <eos> and the blank, the others are labels; beam = 8 gets a token outside the vocabulary too.  New row i continues row (i + pos) % beam by
    one of that row's label candidates; from position 1 on new row 0 repeats its parent's last token."""
    rng = np.random.RandomState(case.seed * 31 + pos)
    beam, rows, V = case.beam, case.N * case.beam, case.V
    cand = np.zeros((rows, beam), dtype=np.int64)
    for r in range(rows):
        labels = [int(v) for v in rng.permutation(np.arange(3, V)) if int(v) != lasts[r]]
        row = [lasts[r], EOS if (pos + r) % 2 == 0 else BLANK] + labels
        if beam == 8:
            row[7] = V + 3
        cand[r] = row[:beam]
    parents, tokens = np.zeros(rows, dtype=np.int32), np.zeros(rows, dtype=np.int64)
    for n in range(case.N):
        for i in range(beam):
            p = (i + pos) % beam
            r = n * beam + p
            options = [int(c) for c in cand[r] if is_label(int(c), V) and (int(c) != lasts[r] or (i == 0 and pos >= 1))]
            if i == 0 and pos >= 1:
                options = [lasts[r]]
            parents[n * beam + i], tokens[n * beam + i] = p, options[i % len(options)]
    return cand, parents, tokens


def run_chain(case: Case, dtype=np.float64):
    """`case.positions` positions of score -> advance over every input, all arithmetic in `dtype` -> per position a dict:
    delta [rows, beam], and after the advance gn / gb [rows, Fmax] (NaN behind F_n), logpsi [rows], last [rows]; plus 'lse' [N, Fmax]."""
    inp = inputs(case)
    x_all = inp["buf"].float().numpy().astype(dtype)[:, :, :case.V]
    beam, rows = case.beam, case.N * case.beam
    ys, lses = [], np.zeros((case.N, case.Fmax), dtype=dtype)
    for n, F in enumerate(case.frames):
        x = x_all[n, :F]
        lse = lse_rows(x) if F else np.zeros(0, dtype=dtype)
        lses[n, :F] = lse
        ys.append((x - lse[:, None]).astype(dtype))
    hyps = [empty_hyp(ys[r // beam]) for r in range(rows)]
    out = []
    for pos in range(case.positions):
        cand, parents, tokens = plan(case, pos, [h.last for h in hyps])
        delta = np.zeros((rows, beam), dtype=dtype)
        for r in range(rows):
            for j in range(beam):
                _, psi = extend(ys[r // beam], hyps[r], int(cand[r, j]))
                delta[r, j] = delta_of(psi, hyps[r].logpsi)
        new = []
        for i in range(rows):
            n = i // beam
            h, _ = extend(ys[n], hyps[n * beam + int(parents[i])], int(tokens[i]))
            new.append(h)
        gn, gb = np.full((rows, case.Fmax), np.nan, dtype=dtype), np.full((rows, case.Fmax), np.nan, dtype=dtype)
        for i, h in enumerate(new):
            F = case.frames[i // beam]
            gn[i, :F], gb[i, :F] = h.gn, h.gb
        out.append(dict(cand=cand, parents=parents, tokens=tokens, delta=delta, gn=gn, gb=gb, logpsi=np.array([h.logpsi for h in new], dtype=dtype),
                        last=np.array([h.last for h in new]), old_logpsi=np.array([h.logpsi for h in hyps], dtype=dtype)))
        hyps = new
    return dict(lse=lses, positions=out)


KINDS = ("delta", "rows", "logpsi")


def _kind_arrays(pos: dict) -> Dict[str, np.ndarray]:
    return dict(delta=pos["delta"].ravel(), rows=np.concatenate([pos["gn"].ravel(), pos["gb"].ravel()]), logpsi=pos["logpsi"].ravel())


def errors(got: dict, ref: dict) -> Dict[str, float]:
    """The largest |got - ref| per kind over all positions, over the entries that are finite in the reference; asserts that got is -inf
    exactly where the reference is, and NaN (no frame) nowhere else."""
    worst = {k: 0.0 for k in KINDS}
    for t, (g, r) in enumerate(zip(got["positions"], ref["positions"])):
        ga, ra = _kind_arrays(g), _kind_arrays(r)
        for k in KINDS:
            a, b = np.asarray(ga[k], dtype=np.float64), np.asarray(ra[k], dtype=np.float64)
            frame = ~np.isnan(b)
            assert np.array_equal(np.isneginf(a[frame]), np.isneginf(b[frame])), (t, k, "-inf where the reference is finite, or the reverse")
            fin = frame & np.isfinite(b)
            assert np.isfinite(a[fin]).all(), (t, k, "a non-finite value where the reference is finite")
            if fin.any():
                worst[k] = max(worst[k], float(np.abs(a[fin] - b[fin]).max()))
    return worst


def bounds(case: Case, ref: dict) -> Dict[str, float]:
    """4 x the float32 yardstick's largest error over the case, per kind, + half a bf16 ulp of the largest logit for bf16 logits."""
    e32 = errors(run_chain(case, np.float32), ref)
    extra = 0.0
    if case.dtype == BF16:
        x = inputs(case)["buf"].float()[:, :, :case.V]
        mx = max([float(x[n, :F].abs().max()) for n, F in enumerate(case.frames) if F] + [0.0])
        extra = 2.0 ** -9 * mx
    return {k: 4.0 * e32[k] + extra for k in KINDS}, e32


# ================================================================================================ brute force (tiny inputs)

def collapse(path) -> Tuple[int, ...]:
    out, prev = [], None
    for v in path:
        if v != prev and v != BLANK:
            out.append(v)
        prev = v
    return tuple(out)


def brute_masses(p: np.ndarray) -> Dict[Tuple[int, ...], float]:
    """p [F, V] probabilities -> {collapsed label sequence: the mass of the alignments that collapse to it}."""
    F, V = p.shape
    mass: Dict[Tuple[int, ...], float] = {}
    for path in itertools.product(range(V), repeat=F):
        w = 1.0
        for f, v in enumerate(path):
            w *= p[f, v]
        key = collapse(path)
        mass[key] = mass.get(key, 0.0) + w
    return mass
