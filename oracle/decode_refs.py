"""Float64 references, error bounds, the shared case table and CPU stand-ins for the decode path's kernels: the row linear
(`decode_linear_kernel` + `decode_pick_kernel`, csrc/decode_linear.hip), the selection rows (`topk_logprob_row`,
`weighted_topk_logprob_row`, csrc/omr_common.h) and the ragged fp8 GEMM.

tests/test_decode_branches_gpu.py runs every case below through the HIP kernels; tests/test_decode_refs_cpu.py runs the same
cases with torch CPU arithmetic standing in for the kernels (`lin_standin` and friends), which shows without a GPU that a
correct implementation meets every check and that a list of damaged ones does not.  `lin_inputs` builds the operands of a case
(views into NaN-filled buffers, outputs as sentinel-filled buffers; cached, never modified: callers clone what a kernel writes
into), `lin_check` holds the assertions both test files share.  Derivations: DESIGN.md, "Decode branch coverage".

Test infrastructure only: nothing here is imported by the package.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from oracle.attention_refs import merge_partials, ratio
from oracle.kernel_refs import (BF16, DTYPES, F32, GEMM_FACTOR, LN_EPS, SENTINEL, TAG, U24, LnCase, assert_bit_equal, assert_outside_untouched,
                                bits, check_close, check_rounded_once, ln_fwd_ref, ln_inputs, padded, rnd)

U8 = 2.0 ** -8                               # bf16 unit roundoff
NEG_INF, NAN = float("-inf"), float("nan")
RM, NOUT, KL, WCH = 8, 16, 16, 8             # decode_linear.hip: rows / columns per workgroup, k-lanes, prefetched chunks per thread
MAXSPLIT, MAXHS = 64, 512
NO_PICK = 0x7FFFFFFF                         # what the row path's pick returned for a row on which no comparison succeeds, before the fix


def vec_of(dtype, w8: bool) -> int:
    """Weight elements per chunk (VEC of decode_linear_kernel)."""
    return 8 if (w8 or dtype == BF16) else 4


# ================================================================================================ e4m3

@functools.lru_cache(maxsize=None)
def e4m3_table() -> torch.Tensor:
    """The 256 OCP e4m3 (fn) values in fp64, NaN at 0x7f / 0xff: sign, 4 exponent bits (bias 7), 3 mantissa bits, no infinities."""
    t = []
    for c in range(256):
        s, e, m = -1.0 if c & 0x80 else 1.0, (c >> 3) & 0xF, c & 7
        t.append(NAN if (e == 15 and m == 7) else s * (m / 8.0 * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)))
    return torch.tensor(t, dtype=torch.float64)


def e4m3_decode(codes: torch.Tensor) -> torch.Tensor:
    return e4m3_table()[codes.long()]


def e4m3_codes(shape, seed: int) -> torch.Tensor:
    """Random codes with exponent fields 4 .. 9 (|value| in [1/8, 7.5]) and both signs: no NaN code, no two equal halves of a chunk
    to speak of, and products of one size, so that a permutation inside a chunk shows."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(4, 10, shape, generator=g)
    m = torch.randint(0, 8, shape, generator=g)
    s = torch.randint(0, 2, shape, generator=g)
    return (s * 128 + e * 8 + m).to(torch.uint8)


# ================================================================================================ row linear: cases

@dataclass(frozen=True)
class LinCase:
    name: str
    dtype: torch.dtype
    K: int
    N: int
    M: int
    w8: bool = False
    pro: int = 0                             # 0 rows | 1 add + LayerNorm | 2 embedding + positional row | 3 merge (with `merge`)
    bias: bool = True
    relu: bool = False
    n0: Optional[int] = None                 # None: N (everything to out0)
    identity: bool = False                   # w = I (N == K, no bias): out0 is the built rows, to the bit
    merge: Optional[Tuple[int, int, int]] = None      # (H, hd, nsplit)
    rows: bool = False                       # the per-row-position form (omr_decode_linear_rows)
    pick: Optional[str] = None               # scenario of the greedy pick (PICK_SCENARIOS)

    @property
    def n_0(self) -> int:
        return self.N if self.n0 is None else self.n0

    @property
    def cpt(self) -> int:
        """Chunks per thread: the kernel's K loop runs min(cpt, 8) prefetched chunks, then chunks 8 .. cpt - 1."""
        return self.K // vec_of(self.dtype, self.w8) // KL


def _kind(dt, w8) -> str:
    return TAG[dt] + ("-e4m3" if w8 else "")


PICK_N = NOUT * 64 + 5                       # G = 65 candidates: decode_pick_kernel's strided loop runs twice for lane 0
PICK_SCENARIOS = {                           # name -> (columns that share the largest value, expected index)
    "tie-one-wg": ((35, 40), 35),            # both in workgroup 2
    "tie-two-wgs": ((700, 21), 21),
    "tie-two-sweeps": ((NOUT * 64 + 3, 3), 3),      # workgroups 0 and 64: lane 0 of the pick kernel on its two sweeps
    "last-column": ((PICK_N - 1,), PICK_N - 1),
    "all-nan": ((), 0),                      # NaN bias: no comparison succeeds; index 0, as omr_argmax and torch.argmax
    "all-neginf": ((), 0),                   # -inf bias
}
ROWS_MAXLEN = 7
ROWS_POS = (0, 5, 2, ROWS_MAXLEN - 1, 5, 1, 3, ROWS_MAXLEN - 1, 0)
MERGE_SHAPES = ((4, 32, 2), (4, 64, 5), (8, 64, 64), (2, 64, 33))


def _cases():
    C = LinCase
    inst, chunk, big, groups, strides, pro, merge, pick, rows = [], [], [], [], [], [], [], [], []
    for dt in DTYPES:
        t = TAG[dt]
        for w8 in (False, True):
            k = _kind(dt, w8)
            inst.append(C(f"inst-{k}-bias-relu", dt, 128, 37, 11, w8=w8, relu=True))
            inst.append(C(f"inst-{k}-nobias", dt, 128, 37, 11, w8=w8, bias=False))
            for K in ((512, 576) if (dt == F32 and not w8) else (1024, 1152)):
                chunk.append(C(f"chunk-{k}-k{K}", dt, K, 20, 2, w8=w8))
        big.append(C(f"big-{t}-k2048", dt, 2048, 20, 9))
        for M in (1, 8, 9, 11):
            groups.append(C(f"groups-{t}-m{M}", dt, 128, 37, M))
        for n0 in (0, 16, 37):
            strides.append(C(f"strides-{t}-n0_{n0}", dt, 128, 37, 3, pro=1, n0=n0))
        for K in (128, 256, 512):
            for p in (1, 2):
                pro.append(C(f"pro{p}-{t}-k{K}", dt, K, K, 3 if p == 1 else 5, pro=p, bias=False, identity=True))
        for H, hd, ns in MERGE_SHAPES:
            merge.append(C(f"merge-{t}-h{H}-hd{hd}-s{ns}", dt, H * hd, H * hd, 3, pro=3, bias=False, identity=True, merge=(H, hd, ns)))
        for sc in PICK_SCENARIOS:
            pick.append(C(f"pick-{t}-{sc}", dt, 128, PICK_N, 3, pick=sc))
        rows.append(C(f"rows-{t}", dt, 128, 384, 9, pro=2, n0=128, rows=True))
    return tuple(inst), tuple(chunk), tuple(big), tuple(groups), tuple(strides), tuple(pro), tuple(merge), tuple(pick), tuple(rows)


INST_CASES, CHUNK_CASES, BIG_CASES, GROUP_CASES, STRIDE_CASES, PRO_CASES, MERGE_CASES, PICK_CASES, ROWS_CASES = _cases()
LIN_CASES = INST_CASES + CHUNK_CASES + BIG_CASES + GROUP_CASES + STRIDE_CASES + PRO_CASES + MERGE_CASES + PICK_CASES + ROWS_CASES
CASE = {c.name: c for c in LIN_CASES}


def case_id(c) -> str:
    return c.name


# ================================================================================================ row linear: inputs

def _seed(name: str) -> int:
    return 7000 + 13 * sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100000


def _view(buf: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    return buf[:rows, :cols]


@functools.lru_cache(maxsize=None)
def merge_part(case: LinCase) -> torch.Tensor:
    """Hand-made key-split partials [M * H, nsplit, hd + 2] (un-normalised O | maximum, log2 domain | sum), M = 3:
    row 0: ordinary splits, except that split 1 of every head is empty (m = -inf, l = 0) and holds finite garbage in O (7777:
           it must never show in the result.  The garbage has to be finite, because the kernel multiplies it by the weight 0, so
           this row alone cannot tell the `m_j == -inf ? 0` guard from exp2(-inf - mm) = 0; the guard is what row 1 needs);
    row 1: every split of every head empty: the merged row is 0;
    row 2: the maxima of consecutive splits differ by 200, so every weight but the last split's underflows to exactly 0."""
    H, hd, ns = case.merge
    s = _seed(case.name)
    l = 0.5 + 3.5 * rnd((3, H, ns), s, 0.0, 1.0)
    o = l[..., None] * rnd((3, H, ns, hd), s + 1)
    m = 3.0 * rnd((3, H, ns), s + 2)
    m[0, :, 1], l[0, :, 1], o[0, :, 1] = NEG_INF, 0.0, 7777.0
    m[1], l[1], o[1] = NEG_INF, 0.0, 7777.0
    m[2] = m[2] + 200.0 * torch.arange(ns, dtype=F32)
    return torch.cat([o, m[..., None], l[..., None]], dim=-1).view(3 * H, ns, hd + 2).contiguous()


@functools.lru_cache(maxsize=None)
def lin_inputs(case: LinCase) -> dict:
    """Everything a case feeds the entry.  Row operands are views into NaN-filled buffers with ldx = K + 8 and ldres = K + 16,
    outputs are sentinel-filled buffers with ld0 = n0 + 8, ld1 = (N - n0) + 24, ld32 = N + 8 and two rows past M; the built rows
    (xn_out, contiguous by the ABI) have two sentinel rows behind them.  The per-row-position form's out1 is a cache
    [M + 1, ROWS_MAXLEN, 2 K + 8] (out1_pos_ld = 2 K + 8, ld1 = ROWS_MAXLEN * out1_pos_ld)."""
    M, N, K, dt, s = case.M, case.N, case.K, case.dtype, _seed(case.name)
    inp: dict = {}
    if case.pro == 0:
        xb = padded(M, K, dt, NAN, ld=K + 8)
        _view(xb, M, K).copy_(rnd((M, K), s))
        inp["x_buf"] = xb
    elif case.pro == 1:
        ln = ln_inputs(LnCase(K, 3, dt, True))                        # rows 100 + 0.1 u with one all-equal row: M = 3
        assert M == 3
        xb, rb = padded(M, K, dt, NAN, ld=K + 8), padded(M, K, dt, NAN, ld=K + 16)
        _view(xb, M, K).copy_(ln["x"])
        _view(rb, M, K).copy_(ln["res"])
        inp.update(x_buf=xb, res_buf=rb, gamma=ln["gamma"], beta=ln["beta"], eps=LN_EPS)
    elif case.pro == 2:
        V = 11
        inp["emb"] = rnd((V, K), s).to(dt)
        inp["pe"] = rnd((ROWS_MAXLEN, K) if case.rows else (K,), s + 1)
        tok = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(s + 2))
        tok[1], tok[M - 1] = -1, V                                    # outside [0, V): the positional row alone
        inp["tokens"] = tok
        if case.rows:
            inp["row_pos"] = torch.tensor(ROWS_POS[:M], dtype=torch.int32)
    else:
        inp["part"] = merge_part(case)
    if case.identity:
        assert N == K and not case.bias and not case.w8
        inp["w"] = torch.eye(K, dtype=dt)
    elif case.w8:
        inp["w8"] = e4m3_codes((N, K), s + 3)
        inp["w8_scale"] = (0.5 + rnd((N,), s + 4, 0.0, 1.0)) / 8.0
    else:
        inp["w"] = rnd((N, K), s + 3).to(dt)
    bias = rnd((N,), s + 5) if case.bias else None
    if case.pick:
        cols, _ = PICK_SCENARIOS[case.pick]
        for c in cols:
            inp["w"][c] = inp["w"][cols[0]]
            bias[c] = 50.0                                            # |w . x| <= 128: 50 + w . x of duplicated rows are bit-equal, and
        if cols:                                                      # make sure nothing else gets there
            keep = torch.ones(N, dtype=torch.bool)
            keep[list(cols)] = False
            inp["w"][keep] *= 0.01
        if case.pick == "all-nan":
            bias[:] = NAN
        if case.pick == "all-neginf":
            bias[:] = NEG_INF
    inp["bias"] = bias
    n0 = case.n_0
    inp["out0_buf"] = padded(M, n0, dt, SENTINEL, ld=n0 + 8)
    if case.rows:
        inp["out1_buf"] = torch.full((M + 1, ROWS_MAXLEN, N - n0 + 8), SENTINEL, dtype=dt)
    else:
        inp["out1_buf"] = padded(M, N - n0, dt, SENTINEL, ld=N - n0 + 24)
    inp["out32_buf"] = padded(M, N, F32, SENTINEL, ld=N + 8)
    inp["built_buf"] = padded(M, K, dt, SENTINEL, ld=K)
    return inp


def weights64(case: LinCase) -> torch.Tensor:
    inp = lin_inputs(case)
    return e4m3_decode(inp["w8"]) * inp["w8_scale"].double()[:, None] if case.w8 else inp["w"].double()


# ================================================================================================ row linear: references

def ln_rows_ref(case: LinCase):
    """fp64 LayerNorm(x + res) of a pro 1 case and the LnCase whose tolerance (ln_check's) it is held to."""
    lc = LnCase(case.K, 3, case.dtype, True)
    return ln_fwd_ref(lc)[0], lc


def exact_rows(case: LinCase) -> Optional[torch.Tensor]:
    """The built rows where IEEE arithmetic fixes them to the bit: pro 0 (the rows themselves) and pro 2,
    round_T(fp32(emb[t]) + pe), pe alone for a token outside [0, V).  None for pro 1 and 3."""
    inp = lin_inputs(case)
    if case.pro == 0:
        return _view(inp["x_buf"], case.M, case.K).clone()
    if case.pro == 2:
        tok, V = inp["tokens"], inp["emb"].shape[0]
        ok = (tok >= 0) & (tok < V)
        e = torch.where(ok[:, None], inp["emb"].float()[tok.clamp(0, V - 1)], torch.zeros((), dtype=F32))
        pe = inp["pe"][inp["row_pos"].long()] if case.rows else inp["pe"][None]
        return (e + pe).to(case.dtype)
    return None


def merge_ref(case: LinCase):
    """(rows [3, K], bound [3, K]) of the merge prologue in fp64 (merge_partials of oracle/attention_refs.py).

    The kernel: w_j = exp2(m_j - mm) (0 for m_j = -inf), l = sum_j l_j w_j, o_i = sum_j O_ji w_j, row_i = round_T(o_i (1 / l)),
    all fp32 (u = 2^-24).  Relative error of a weight: the subtraction is one rounding of an exponent, ln2 u |m_j - mm|, and
    the hardware exp2 (v_exp_f32) is taken as good to 2 ulp <= 4 u, the figure DESIGN.md's "Attention error bounds" relies on
    (the CDNA ISA guides state 1 ulp): e_j = (4 + ln2 |m_j - mm|) u.  v_exp_f32 flushes results below 2^-126 to 0: an absolute
    2^-126 per weight.  Each of the two sums is nsplit products and nsplit additions onto 0: (nsplit + 1) u relative to the sum
    of absolute terms.  1 / l is one correctly rounded division or a v_rcp_f32 (1 ulp <= 2 u), the product with it one more
    rounding: 3 u.  With A_i = sum_j |O_ji| w_j / l, E_l = sum_j l_j w_j (e_j + (nsplit + 1) u) / l:

        |row_i - ref_i| <= (1 + 2^-10) (sum_j |O_ji| w_j (e_j + (nsplit + 1) u) / l  +  A_i (E_l + 3 u))
                           + 2^-126 sum_j |O_ji| / l  (+ 2^-8 |ref_i| when T is bf16)

    (1 + 2^-10) covers the second-order terms: every first-order relative term sums to under 200 u ~ 1.2e-5.
    A row all of whose splits are empty is 0 with bound 0: exact."""
    H, hd, ns = case.merge
    p = merge_part(case).double().view(3, H, ns, hd + 2)
    ref = merge_partials(p.view(3 * H, ns, 1, hd + 2), hd)[0].view(3, H * hd)
    o, m, l = p[..., :hd], p[..., hd], p[..., hd + 1]
    mm = m.max(dim=-1, keepdim=True).values
    live = m > NEG_INF
    dm = torch.where(live, (m - torch.where(mm > NEG_INF, mm, 0.0)).abs(), 0.0)
    w = torch.where(live, torch.exp2(-dm), 0.0)
    e = (4.0 + math.log(2.0) * dm + ns + 1) * U24                       # e_j + (nsplit + 1) u
    lt = (l * w).sum(-1)
    ok = lt > 0
    ls = torch.where(ok, lt, 1.0)
    El = (l * w * e).sum(-1) / ls
    oa = torch.where(live[..., None], o.abs(), 0.0)
    A = (oa * w[..., None]).sum(-2) / ls[..., None]
    first = (oa * (w * e)[..., None]).sum(-2) / ls[..., None]
    bound = (1 + 2.0 ** -10) * (first + A * (El[..., None] + 3 * U24)) + 2.0 ** -126 * oa.sum(-2) / ls[..., None]
    bound = torch.where(ok[..., None], bound, 0.0).reshape(3, H * hd)
    if case.dtype == BF16:
        bound = bound + U8 * ref.abs()
    return ref, bound


def lin_ref(case: LinCase, rows_t: torch.Tensor):
    """(ref, bound) [M, N] in fp64 for input rows `rows_t` (x~: the rows as the kernel holds them, values of T).

        |got - ref| <= (K + 2) 2^-24 sum_k |w_nk| |x~_mk|     (+ 2^-8 |ref| when T is bf16)

    ref = sum_k w_nk x~_mk + bias_n: the order-independent bound of an fp32 sum of K fused products and the bias add (Higham,
    Accuracy and Stability of Numerical Algorithms, eq. 3.5); the kernel uses no MFMA, so there is no tree factor.  The e4m3
    path has (K + 3), for the extra rounding of fmaf(acc, scale, bias); there w = code * scale in fp64.  ReLU is 1-Lipschitz:
    it does not widen the bound."""
    inp = lin_inputs(case)
    x, w = rows_t.double(), weights64(case)
    ref = x @ w.t()
    if inp["bias"] is not None:
        ref = ref + inp["bias"].double()
    if case.relu:
        ref = ref.clamp_min(0.0)
    bound = (case.K + (3 if case.w8 else 2)) * U24 * (x.abs() @ w.abs().t())
    if case.dtype == BF16:
        bound = bound + U8 * torch.where(torch.isfinite(ref), ref.abs(), 0.0)
    return ref, bound


# ================================================================================================ row linear: CPU stand-in

def ln_standin_rows(case: LinCase) -> torch.Tensor:
    inp = lin_inputs(case)
    s = _view(inp["x_buf"], case.M, case.K).float() + _view(inp["res_buf"], case.M, case.K).float()
    mean = s.mean(1, keepdim=True)
    t = s - mean
    rstd = torch.rsqrt((t * t).mean(1, keepdim=True) + LN_EPS)
    return (t * rstd * inp["gamma"] + inp["beta"]).to(case.dtype)


def merge_standin_rows(case: LinCase, no_guard: bool = False) -> torch.Tensor:
    """The merge in fp32 torch arithmetic, sums by torch.sum (another order).  no_guard: the weight of an empty split is
    exp2(m_j - mm) like any other, which is NaN on a row whose splits are all empty (-inf - -inf)."""
    H, hd, ns = case.merge
    p = merge_part(case).view(3, H, ns, hd + 2)
    o, m, l = p[..., :hd], p[..., hd], p[..., hd + 1]
    mm = m.max(dim=-1, keepdim=True).values
    w = torch.exp2(m - mm)
    if not no_guard:
        w = torch.where(m == NEG_INF, torch.zeros((), dtype=F32), w)
    lt = (l * w).sum(-1)
    on = (o * w[..., None]).sum(-2)
    inv = torch.where(lt > 0, 1.0 / lt, torch.zeros((), dtype=F32)) if not no_guard else 1.0 / lt
    return (on * inv[..., None]).reshape(3, H * hd).to(case.dtype)


def pick_standin(out32: torch.Tensor, last: bool = False):
    """First index of the row maximum (torch.argmax: index 0 for a row of NaN or of -inf) and the value there.  last: the LAST
    maximum instead (a reduction that prefers the larger index)."""
    n = out32.shape[1]
    idx = (n - 1 - torch.argmax(out32.flip(1), dim=1)) if last else torch.argmax(out32, dim=1)
    return idx, out32.gather(1, idx[:, None])[:, 0]


DAMAGES = ("drop_last_klane", "drop_post_prefetch", "swap_code_halves", "shift_out1_row", "pick_last", "merge_no_guard")


def lin_standin(case: LinCase, damage: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """torch CPU arithmetic in the kernel's formats and another order: fp32 products without fma, summed 16 at a time, then
    over the groups; one rounding to T.  -> the buffers after the call (out0_buf, out1_buf, out32_buf, built_buf) and idx / val.
    damage (DAMAGES): drop_last_klane: k-lane 15's chunk of the last chunk group is left out (the last VEC columns of K);
    drop_post_prefetch: the chunks i >= 8 of every thread (columns from 8 * 16 * VEC on); swap_code_halves: the two 32-bit
    halves of every 8-code e4m3 chunk change places; shift_out1_row: out1 lands one position row further (mod the cache);
    pick_last; merge_no_guard."""
    assert damage is None or damage in DAMAGES
    inp = lin_inputs(case)
    M, N, K, dt, n0 = case.M, case.N, case.K, case.dtype, case.n_0
    if case.pro == 1:
        rows = ln_standin_rows(case)
    elif case.pro == 3:
        rows = merge_standin_rows(case, no_guard=damage == "merge_no_guard")
    else:
        rows = exact_rows(case)
    if case.w8:
        codes = inp["w8"]
        if damage == "swap_code_halves":
            codes = codes.view(N, K // 8, 2, 4).flip(2).reshape(N, K)
        w = e4m3_decode(codes).float()
    else:
        w = inp["w"].float()
    x = rows.float()
    vec = vec_of(dt, case.w8)
    if damage == "drop_last_klane":
        x = x.clone(); x[:, K - vec:] = 0.0
    if damage == "drop_post_prefetch":
        x = x.clone(); x[:, WCH * KL * vec:] = 0.0
    acc = (x[:, None, :] * w[None]).view(M, N, K // 16, 16).sum(-1).sum(-1)
    bias = inp["bias"] if inp["bias"] is not None else torch.zeros(N)
    v = acc * inp["w8_scale"] + bias if case.w8 else acc + bias
    if case.relu:
        v = v.clamp_min(0.0)
    o = v.to(dt)
    out = {k: inp[k].clone() for k in ("out0_buf", "out1_buf", "out32_buf", "built_buf")}
    _view(out["out0_buf"], M, n0).copy_(o[:, :n0])
    if case.rows:
        pos = inp["row_pos"].long()
        if damage == "shift_out1_row":
            pos = (pos + 1) % ROWS_MAXLEN
        out["out1_buf"][torch.arange(M), pos, :N - n0] = o[:, n0:]
    else:
        _view(out["out1_buf"], M, N - n0).copy_(o[:, n0:])
    _view(out["out32_buf"], M, N).copy_(o.float())
    if case.pro in (1, 2):
        out["built_buf"][:M] = rows
    out["idx"], out["val"] = pick_standin(o.float(), last=damage == "pick_last")
    return out


# ================================================================================================ row linear: the shared checks

def stored(case: LinCase, out: Dict[str, torch.Tensor]) -> torch.Tensor:
    """The logical [M, N] output in T, gathered from out0 | out1 (the cache rows row_pos names, in the per-row-position form)."""
    inp = lin_inputs(case)
    M, N, n0 = case.M, case.N, case.n_0
    o0 = _view(out["out0_buf"].cpu(), M, n0)
    if case.rows:
        o1 = out["out1_buf"].cpu()[torch.arange(M), inp["row_pos"].long(), :N - n0]
    else:
        o1 = _view(out["out1_buf"].cpu(), M, N - n0)
    return torch.cat([o0, o1], dim=1)


def lin_check(case: LinCase, out: Dict[str, torch.Tensor], ln_rows: Optional[torch.Tensor] = None, who: str = "") -> float:
    """Every assertion a row-linear case makes on the buffers after the call; returns the largest |err| / bound.
    ln_rows (pro 1): the rows another implementation of add + LayerNorm built, which the built rows must equal to the bit."""
    inp = lin_inputs(case)
    M, N, K, dt, n0 = case.M, case.N, case.K, case.dtype, case.n_0
    name = f"decode linear {who}{case.name}"
    got = stored(case, out)
    built = out["built_buf"].cpu()[:M]
    # ---- nothing outside the logical outputs
    assert_outside_untouched(out["out0_buf"].cpu(), inp["out0_buf"], M, n0, f"{name}: out0")
    assert_outside_untouched(out["out32_buf"].cpu(), inp["out32_buf"], M, N, f"{name}: out32")
    assert_outside_untouched(out["built_buf"].cpu(), inp["built_buf"], M if case.pro in (1, 2) else 0, K, f"{name}: xn_out")
    if case.rows:
        o1, want = bits(out["out1_buf"]).clone(), bits(inp["out1_buf"])
        o1[torch.arange(M), inp["row_pos"].long(), :N - n0] = want[0, 0, 0]
        assert bool((o1 == want).all()), f"{name}: {int((o1 != want).sum())} cache elements outside the rows' own positions were written"
    else:
        assert_outside_untouched(out["out1_buf"].cpu(), inp["out1_buf"], M, N - n0, f"{name}: out1")
    # ---- the rows the product saw
    rows = exact_rows(case)
    if case.pro == 1:
        ref64, lc = ln_rows_ref(case)
        check_close(built, ref64, dt, lc.scale, f"{name}: built rows vs fp64 LayerNorm")
        check_rounded_once(built, ref64, dt, lc.scale, f"{name}: built rows, fp32 value rounded once")
        if ln_rows is not None:
            assert_bit_equal(built, ln_rows.cpu(), f"{name}: built rows vs the stand-alone add + LayerNorm")
        rows = built
    elif case.pro == 2:
        assert_bit_equal(built, rows, f"{name}: built rows vs round_T(fp32(emb[t]) + pe)")
    r_rows = 0.0
    if case.pro == 3:
        assert case.identity
        mref, mbound = merge_ref(case)
        r_rows = ratio(got, mref, mbound)
        print(f"{name}: merged rows, max |err| / bound = {r_rows:.4f}")
        assert r_rows <= 1.0, f"{name}: merged rows are {r_rows:.3f} x the bound off"
        assert bool((bits(got[1]) == 0).all()), f"{name}: the row whose splits are all empty is not +0"
        rows = got                                                       # identity weight: out0 IS the rows
    if case.identity and case.pro != 3:
        assert_bit_equal(got, rows, f"{name}: identity weight, out0 vs the built rows")
    # ---- the product
    r = 0.0
    if not case.pick or case.pick not in ("all-nan", "all-neginf"):
        ref, bound = lin_ref(case, rows)
        r = ratio(got, ref, bound)
        print(f"{name}: max |err| / bound = {r:.4f}")
        assert r <= 1.0, f"{name}: error is {r:.3f} x the bound"
    assert_bit_equal(_view(out["out32_buf"].cpu(), M, N), got.float(), f"{name}: out32 vs the fp32 value of what was stored")
    # ---- the pick
    if "idx" in out and out["idx"] is not None:
        idx, val = out["idx"].cpu(), out["val"].cpu()
        want_idx, want_val = pick_standin(got.float())
        assert idx.dtype == torch.int64 and idx.tolist() == want_idx.tolist(), f"{name}: pick {idx.tolist()}, first maximum at {want_idx.tolist()}"
        if case.pick:
            assert idx.tolist() == [PICK_SCENARIOS[case.pick][1]] * M, f"{name}: pick {idx.tolist()}, the scenario says {PICK_SCENARIOS[case.pick][1]}"
        if case.pick != "all-nan":
            assert_bit_equal(val, want_val, f"{name}: amax_val vs the stored value")
    return max(r, r_rows)


# ================================================================================================ selection rows

SEL_NS, SEL_KS, SEL_ALPHA = (30, 600), (1, 3, 8), 0.3


@functools.lru_cache(maxsize=None)
def sel_inputs(n: int) -> dict:
    """Two [7, ld] fp32 logit buffers (ld = n + 10 / 640, ordinary LARGER values behind the rows), logical width n:
    row 0: ordinary; row 1: equal largest values at i, i + 1 (and i + 256 when n = 600): one thread's two sweeps and two threads;
    row 2: two finite entries, the rest -inf; row 3: ordinary values, the maximum in the last column; row 4: all NaN;
    row 5: all -inf; row 6: comparable entries at 2 and 5 only (1.0 and 2.0), the rest NaN -- both buffers of the pair get the
    same special rows."""
    assert n in SEL_NS
    ld = n + 10 if n == 30 else 640
    out = {}
    for which, seed in (("a", 81), ("b", 82)):
        buf = 4.0 * rnd((7, ld), seed + n)
        buf[:, n:] = 100.0
        i = 7
        buf[1, i] = buf[1, i + 1] = 9.0
        if n == 600:
            buf[1, i + 256] = 9.0
        buf[2, :n] = NEG_INF
        buf[2, 5], buf[2, n - 2] = 1.0, 2.0
        buf[3, n - 1] = 9.0
        buf[4, :n] = NAN
        buf[5, :n] = NEG_INF
        buf[6, :n] = NAN
        buf[6, 2], buf[6, 5] = 1.0, 2.0
        out[which] = buf
    return dict(n=n, ld=ld, **out)


def sel_ref(n: int, mix: bool):
    """(values [7, n] fp64, bound [7, n]): log_softmax(a), or log(alpha softmax(a) + (1 - alpha) softmax(b)).

    topk: val = x - (mx + log(sum exp(x - mx))): the sum of n terms in (0, 1], each expf good to 2 ulp after one rounding of
    its argument (|x - mx| u), is relative (n + 4 + max|x - mx|) u; logf 2 ulp (4 u relative to |log|, absolute <= 4 u log n);
    two more roundings relative to |lse| and |val|.  Bound: (n + 8 + D) u + 4 u (|mx| + log n + |val|), D = max |x - mx| over the
    finite entries.  mix: each softmax term has relative error (n + 10 + 2 D) u (exp, sum, division), the two products and the
    add 3 u, logf 4 u |val| + 2u: bound (n + 16 + 2 D) u + 4 u |val|.  Entries of -inf give -inf exactly (ratio())."""
    inp = sel_inputs(n)
    a, b = inp["a"][:, :n].double(), inp["b"][:, :n].double()

    def lsm(x):
        fin = torch.isfinite(x)
        mx = torch.where(fin, x, NEG_INF).max(1, keepdim=True).values
        mx0 = torch.where(torch.isfinite(mx), mx, 0.0)
        lse = mx0 + torch.log(torch.where(fin, torch.exp(x - mx0), 0.0).sum(1, keepdim=True))
        D = torch.where(fin, (x - mx0).abs(), 0.0).max(1, keepdim=True).values
        return x - lse, mx0.abs(), D
    la, ma, Da = lsm(a)
    if not mix:
        bound = (n + 8 + Da) * U24 + 4 * U24 * (ma + math.log(n) + torch.where(torch.isfinite(la), la.abs(), 0.0))
        return la, bound.expand_as(la).clone()
    lb, _, Db = lsm(b)
    wa, wb = float(np.float32(SEL_ALPHA)), float(np.float32(1.0) - np.float32(SEL_ALPHA))
    p = wa * torch.exp(la) + wb * torch.exp(lb)
    val = torch.log(p)
    bound = (n + 16 + 2 * torch.maximum(Da, Db)) * U24 + 4 * U24 * torch.where(torch.isfinite(val), val.abs(), 0.0)
    return val, bound.expand_as(val).clone()


def sel_standin(n: int, k: int, mix: bool):
    """torch CPU fp32: log_softmax / log of the mix, then a stable descending sort (ties towards the smaller index) of the
    entries that can win a comparison: the logits themselves (topk) or the mixed probabilities (mix) that are not NaN.  Pass j
    of a row with fewer than j + 1 such entries emits index j, as the kernels are defined to: an all-NaN row gives 0 .. k - 1."""
    inp = sel_inputs(n)
    a, b = inp["a"][:, :n], inp["b"][:, :n]
    if mix:
        wa = torch.tensor(SEL_ALPHA, dtype=F32)
        v = torch.log(wa * torch.softmax(a, 1) + (1 - wa) * torch.softmax(b, 1))
    else:
        v = torch.log_softmax(a, 1)
    rank = v if mix else a                                              # what the selection passes compare
    idx = torch.empty((a.shape[0], k), dtype=torch.int64)
    for r in range(a.shape[0]):
        can = (~torch.isnan(rank[r])).nonzero()[:, 0]
        order = can[torch.sort(rank[r][can], descending=True, stable=True).indices][:k]
        idx[r] = torch.cat([order, torch.arange(len(order), k)])
    return idx, v.gather(1, idx)


def sel_check(n: int, k: int, mix: bool, idx: torch.Tensor, val: torch.Tensor, who: str = "") -> float:
    """Indices inside [0, n), and distinct on every row but the partly NaN one; every value within the bound of the fp64 value AT THE INDEX the kernel named; the
    j-th pick's fp64 value is not below any unpicked entry's by more than the two bounds (so the order is right wherever the
    fp64 margin exceeds the bound); the tie rows and the special rows exactly."""
    name = f"{'weighted ' if mix else ''}topk {who}n={n} k={k}"
    idx, val = idx.cpu(), val.cpu()
    ref, bound = sel_ref(n, mix)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (7, k) and bool(((idx >= 0) & (idx < n)).all()), f"{name}: indices outside [0, {n}): {idx.tolist()}"
    worst = 0.0
    for r in range(7):
        ids = idx[r].tolist()
        if r == 6:
            # two comparable entries, the rest NaN.  topk ranks the logits: 5, then 2, and the passes without a candidate emit
            # their own number j -- inside [0, n), but pass 2 names index 2 a second time: only a row that is ALL NaN is promised
            # distinct indices.  The mix is NaN everywhere (the sums of exponentials are), so it is an all-NaN row.  Values: NaN.
            assert ids == ([5, 2][:k] + list(range(2, k)) if not mix else list(range(k))), f"{name}: partly NaN row gives {ids}"
            assert bool(torch.isnan(val[r]).all()), f"{name}: partly NaN row has values {val[r].tolist()}"
            continue
        assert len(set(ids)) == k, f"{name}: row {r} names an index twice: {ids}"
        if r == 4:                                                        # all NaN: indices 0 .. k - 1, values NaN
            assert ids == list(range(k)) and bool(torch.isnan(val[r]).all()), f"{name}: all-NaN row gives {ids}, {val[r].tolist()}"
            continue
        if r == 5:                                                        # all -inf: ties in index order; lse = NaN (-inf - -inf)
            assert ids == list(range(k)), f"{name}: all -inf row gives {ids}"
            continue
        rr = ratio(val[r], ref[r, idx[r]], bound[r, idx[r]])
        worst = max(worst, rr)
        assert rr <= 1.0, f"{name}: row {r} values are {rr:.3f} x the bound off"
        rest = torch.ones(n, dtype=torch.bool)
        for j, i in enumerate(ids):
            rest[i] = False
            if rest.any():
                margin = ref[r, i] + bound[r, i] - (ref[r][rest] - bound[r][rest]).max()
                assert not margin < 0, f"{name}: row {r} pick {j} (index {i}) is below an unpicked entry by more than the bounds"
    want1 = [7, 8, 263] if n == 600 else [7, 8]                            # bit-equal inputs: the smaller index first
    assert idx[1].tolist()[:min(k, len(want1))] == want1[:min(k, len(want1))], f"{name}: tie row gives {idx[1].tolist()}"
    want2 = [n - 2, 5] + [i for i in range(n) if i not in (5, n - 2)]     # two finite entries, then the -inf ones in index order
    assert idx[2].tolist() == want2[:k], f"{name}: -inf row gives {idx[2].tolist()}"
    assert idx[3, 0].item() == n - 1, f"{name}: the maximum in the last column was missed"
    print(f"{name}: max |err| / bound = {worst:.4f}")
    return worst


# ================================================================================================ fp8 GEMM over ragged shapes

FP8_CASES = tuple((M, K) for M in (1, 5) for K in (48, 80))
FP8_N = 70


@functools.lru_cache(maxsize=None)
def fp8_inputs(M: int, K: int, dtype) -> dict:
    """x [M, K] in a NaN-filled buffer with ldx = K + 8 (row M - 1 all zero when M > 1) and the weight [70, K]."""
    xb = padded(M, K, dtype, NAN, ld=K + 8)
    _view(xb, M, K).copy_(rnd((M, K), 91 + M + K))
    if M > 1:
        xb[M - 1, :K] = 0.0
    return dict(x_buf=xb, w=rnd((FP8_N, K), 92 + K).to(dtype), bias=rnd((FP8_N,), 93))


def fp8_scale_ref(x: torch.Tensor) -> torch.Tensor:
    """absmax / 448 in fp32, 1 for a row of zeros."""
    am = x.float().abs().max(dim=1).values
    return torch.where(am > 0, am / torch.tensor(448.0, dtype=F32), torch.ones((), dtype=F32))


def fp8_quantize_standin(x: torch.Tensor):
    s = fp8_scale_ref(x)
    return (x.float() / s[:, None]).to(torch.float8_e4m3fn).view(torch.uint8), s


def fp8_gemm_check(M: int, K: int, a8, sa, w8, sw, bias, c: torch.Tensor, cdtype, who: str = "") -> float:
    """C against the fp64 product of the de-quantised operands (code * scale), with gemm_ref's bound of oracle/kernel_refs.py:
    GEMM_FACTOR (K + 2) 2^-24 sum |a||b| (+ 2^-8 |ref| for a bf16 C).  The products of e4m3 codes are exact in fp32, so the two
    scale multiplications of the epilogue take the place of the operand roundings the (K + 2) count has room for."""
    A = e4m3_decode(a8.cpu()[:, :K]) * sa.cpu().double()[:, None]
    B = e4m3_decode(w8.cpu()[:, :K]) * sw.cpu().double()[:, None]
    ref = A @ B.t() + bias.cpu().double()
    bound = GEMM_FACTOR * (K + 2) * U24 * (A.abs() @ B.abs().t()) + (U8 * ref.abs() if cdtype == BF16 else 0.0)
    r = ratio(c, ref, bound)
    print(f"fp8 gemm {who}M={M} K={K} {TAG[cdtype]}: max |err| / bound = {r:.4f}")
    assert r <= 1.0
    return r
