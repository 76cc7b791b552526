"""Float64 reference, per-element error bounds and the shared case table for the attention kernels (csrc/attention.hip,
csrc/attention_bwd.hip, csrc/attn_common.h).

tests/test_attention_branches_gpu.py runs every case below through the HIP kernels; tests/test_attention_refs_cpu.py runs the
same cases with a torch CPU emulation of the kernels' arithmetic in their place, which shows without a GPU that a correct
implementation meets every bound and that a list of subtly wrong ones does not.  `attn_inputs` builds the operands of a case
(views into NaN-filled buffers; cached, never modified), `attention_ref` restates attention in plain fp64 arithmetic and returns
a bound beside every result (derivation: DESIGN.md, "Attention error bounds"), `attn_ratios` / `attn_check` hold the
comparison both test files share.

Test infrastructure only: nothing here is imported by the package.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from oracle.kernel_refs import BF16, DTYPES, F32, SENTINEL, TAG, U24, bits, rnd
from oracle.ref_cpu import tgt_attn_mask

U8 = 2.0 ** -8                               # bf16 unit roundoff
PAD = 8                                      # padding columns of every non-packed operand row (a multiple of both vector widths)
NEG_INF = float("-inf")


def unit(dtype) -> float:
    """Roundoff of the roundings to the operand type T; 0 for fp32, whose roundings sit in the accumulation terms."""
    return U8 if dtype == BF16 else 0.0


# ================================================================================================ cases

@dataclass(frozen=True)
class AttnCase:
    name: str
    entry: str                               # fwd (omr_attn_fwd_ws + omr_attn_bwd_ws) | split | partials | varlen | rows
    B: int
    H: int
    T: int
    S: int
    hd: int
    family: str = "peaked"                   # peaked | needles | growing
    causal: bool = False                     # self-attention: q, k and v are the thirds of one packed [B, T, 3d] buffer
    window: int = -1
    bias: str = "none"                       # none | plus1 | inf_tail (+1 on odd keys, -inf on each row's tail) | inf_row (inf_tail, last batch row all -inf)
    blk: Optional[Tuple[Tuple[int, ...], Tuple[int, ...]]] = None      # (blk_lq, blk_lkv)
    drop: Optional[Tuple[float, int]] = None                           # (p, seed)
    kv_len: Optional[Tuple[int, ...]] = None
    kv_start: Optional[Tuple[int, ...]] = None
    nsplit: int = 1                          # key splits the plan must give (asserted by the GPU tests)
    split_len: int = 0
    bwd: bool = False

    @property
    def d(self) -> int:
        return self.H * self.hd


def _cases():
    C = AttnCase
    fwd = (
        # query-per-wave kernel <T, HD, false, false>: T tails, tile counts, masks
        C("t33-s65-hd32-plus1", "fwd", 2, 2, 33, 65, 32, bias="plus1", bwd=True),
        C("t129-s64-hd64-needles", "fwd", 1, 2, 129, 64, 64, family="needles", bwd=True),
        C("t33-s129-hd64-infrow", "fwd", 3, 2, 33, 129, 64, family="needles", bias="inf_row", bwd=True),
        C("t40-s300-hd32-inftail", "fwd", 2, 2, 40, 300, 32, bias="inf_tail", bwd=True),
        C("causal-t129-hd64", "fwd", 1, 2, 129, 129, 64, family="needles", causal=True, bwd=True),
        C("causal-t129-hd32-peaked", "fwd", 2, 1, 129, 129, 32, causal=True, bwd=True),
        C("causal-win20-t150-hd32", "fwd", 1, 2, 150, 150, 32, family="needles", causal=True, window=20, bwd=True),
        C("causal-win64-t40-hd64", "fwd", 2, 1, 40, 40, 64, causal=True, window=64, bwd=True),        # window >= T: plain causal
        C("blk-b3-h2-t40-s100-hd32", "fwd", 3, 2, 40, 100, 32, blk=((10, 40, 0), (30, 50, 64)), bwd=True),
        C("grow-t64-s640-hd64", "fwd", 1, 1, 64, 640, 64, family="growing", bias="minus300"),          # forward only: with score errors of
        # tens of nats (u |s|, |s| up to 9600) every backward bound is vacuous
        # the same construction at a size where the bf16 bound still says something: u A_k < 1 / 8, and the reference maximum
        # moves on later tiles (asserted by tests/test_attention_refs_cpu.py)
        C("grow-mild-t64-s640-hd64", "fwd", 1, 1, 64, 640, 64, family="growing_mild", bias="minus300", bwd=True),
        C("split2-t40-s1041-hd64", "fwd", 1, 2, 40, 1041, 64, family="needles", bias="plus1", nsplit=2, split_len=768, bwd=True),
        C("split3-t129-s1553-hd32", "fwd", 2, 2, 129, 1553, 32, bias="inf_tail", nsplit=3, split_len=768, bwd=True),
    )
    drop = (
        C("drop-t33-s65-hd64", "fwd", 2, 2, 33, 65, 64, drop=(0.25, 1234), bwd=True),
        C("drop-causal-t129-hd32", "fwd", 1, 2, 129, 129, 32, family="needles", causal=True, drop=(0.25, 77), bwd=True),
        C("drop-win20-t150-hd64", "fwd", 1, 2, 150, 150, 64, causal=True, window=20, drop=(0.25, 2 ** 40 + 5), bwd=True),
        C("drop-split2-t40-s1041-hd32", "fwd", 1, 2, 40, 1041, 32, family="needles", nsplit=2, split_len=768, drop=(0.25, 99), bwd=True),
    )
    dec = (
        # decode kernel <T, HD, true, false> through omr_attn_fwd_split
        C("dec-t1-s65-hd64", "split", 2, 2, 1, 65, 64, family="needles", bias="plus1"),
        C("dec-t20-s256-hd32", "split", 1, 2, 20, 256, 32, family="needles", bias="plus1"),
        C("dec-t20-s257-hd64", "split", 2, 2, 20, 257, 64, family="needles", bias="plus1", nsplit=2, split_len=256),
        C("dec-t1-s700-hd32", "split", 2, 2, 1, 700, 32, family="needles", bias="inf_tail", nsplit=3, split_len=256),
        C("dec-t20-s700-hd64", "split", 1, 2, 20, 700, 64, bias="plus1", nsplit=3, split_len=256),
        # the 64-split cap: 33 splits of 512 keys, two staging blocks each; one needle per (b, h), see cap_needles
        C("dec-cap-hd32", "split", 3, 2, 1, 64 * 256 + 300, 32, family="needles", bias="plus1", nsplit=33, split_len=512),
        C("dec-cap-hd64", "split", 3, 2, 1, 64 * 256 + 300, 64, family="needles", bias="plus1", nsplit=33, split_len=512),
    )
    part = (
        C("part-t1-s700-hd64", "partials", 2, 2, 1, 700, 64, family="needles", nsplit=3, split_len=256),
        C("part-t1-s200-hd32", "partials", 2, 2, 1, 200, 32, family="needles"),
    )
    ragged = (
        C("varlen-hd64", "varlen", 4, 1, 2, 700, 64, family="needles", bias="plus1", kv_len=(65, 256, 257, 700), nsplit=3, split_len=256),
        C("varlen-hd32-peaked", "varlen", 4, 1, 1, 700, 32, bias="plus1", kv_len=(65, 256, 257, 700), nsplit=3, split_len=256),
        C("rows-hd32", "rows", 5, 1, 2, 300, 32, family="needles", bias="plus1", kv_len=(1, 63, 64, 65, 300), kv_start=(5, 0, 5, 0, 5), nsplit=2,
          split_len=256),
        C("rows-hd64-peaked", "rows", 5, 1, 1, 300, 64, bias="plus1", kv_len=(1, 63, 64, 65, 300), kv_start=(5, 0, 5, 0, 5), nsplit=2, split_len=256),
    )
    return fwd, drop, dec, part, ragged


FWD_CASES, DROP_CASES, DECODE_CASES, PARTIAL_CASES, RAGGED_CASES = _cases()
ALL_CASES = FWD_CASES + DROP_CASES + DECODE_CASES + PARTIAL_CASES + RAGGED_CASES
CASE = {c.name: c for c in ALL_CASES}


def case_id(c) -> str:
    return c.name if isinstance(c, AttnCase) else TAG[c]


def expected_split(case: AttnCase, min_wg: int = 512) -> Tuple[int, int]:
    """choose_split of attn_common.h restated: (nsplit, split_len).  The case table's nsplit / split_len must agree with it."""
    B, H, T, S = case.B, case.H, case.T, case.S
    if case.causal or S <= 256:
        return 1, 0
    if T <= 32:
        want = min((S + 255) // 256, 64)
    else:
        blocks = B * H * ((T + 127) // 128)
        want = min((min_wg + blocks - 1) // blocks, S // 512)
    if want <= 1:
        return 1, 0
    ln = ((S + want - 1) // want + 255) // 256 * 256
    n = (S + ln - 1) // ln
    return (n, ln) if n > 1 else (1, 0)


# ================================================================================================ dropout keep mask

def _hash32(lo, hi, idx):
    h = (idx * np.uint32(0x9E3779B1) + lo).astype(np.uint32)
    h ^= h >> np.uint32(16); h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13); h += hi; h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def keep_mask(B: int, H: int, T: int, S: int, p: float, seed: int) -> torch.Tensor:
    """The keep mask of the attention-probability dropout as attn_common.h defines it (attn_bh_key, attn_rand2), bool
    [B, H, T, S].  The GPU tests show it equal to omr_attn_dropout_mask, which an existing test links to the kernels' words."""
    with np.errstate(over="ignore"):
        thr = np.uint32(int(p * 65536.0 + 0.5))
        bh = np.arange(B * H, dtype=np.uint32)
        key = _hash32(np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF), bh)                # [BH]
        s2 = np.uint32((S + 1) >> 1)
        q = np.arange(T, dtype=np.uint32)[:, None]
        pair = (q * s2 + (np.arange(S, dtype=np.uint32)[None, :] >> np.uint32(1))).astype(np.uint32)       # [T, S]
        x = pair[None] ^ key[:, None, None]
        x = (x * np.uint32(0x9E3779B1)).astype(np.uint32); x ^= x >> np.uint32(15)
        x = (x * np.uint32(0x85EBCA6B)).astype(np.uint32); x ^= x >> np.uint32(16)
        odd = (np.arange(S) & 1).astype(bool)[None, None, :]
        half = np.where(odd, x >> np.uint32(16), x & np.uint32(0xFFFF))
        keep = (half >= thr) | (thr == 0)
    return torch.from_numpy(keep.reshape(B, H, T, S))


# ================================================================================================ inputs

def _seed(case: AttnCase) -> int:
    return 5000 + 11 * sum((i + 1) * ord(ch) for i, ch in enumerate(case.name)) % 100000


def row_len(case: AttnCase, b: int) -> int:
    return case.kv_len[b] if case.kv_len else case.S


def row_start(case: AttnCase, b: int) -> int:
    return case.kv_start[b] if case.kv_start else 0


def inf_cut(case: AttnCase, b: int) -> Optional[int]:
    """First key of batch row b that key_bias masks with -inf (None: no such key).  S > 600: the keys of every row but the first
    end at 200, inside the first split, so the later splits of those rows merge with weight 0."""
    if case.bias not in ("inf_tail", "inf_row"):
        return None
    if case.bias == "inf_row" and b == case.B - 1:
        return 0
    if case.S > 600:
        return case.S - 37 if b == 0 else 200
    return case.S - 5 - 3 * b


def cap_needles(case: AttnCase):
    """The needle key of each (b, h) of a 64-split-cap case (T = 1, B H = 6), index b H + h: the last key; the last key of the
    first staging block of a middle split and the first and the last key of its second block; a key in the second block of the
    short last split; key 0."""
    ln, mid = case.split_len, (case.nsplit // 2) * case.split_len
    return [case.S - 1, mid + ln // 2 - 1, mid + ln // 2, mid + ln - 1, (case.nsplit - 1) * ln + ln // 2 + 10, 0]


def needle_keys(case: AttnCase, b: int) -> Dict[int, int]:
    """{query row: key} of the needles of batch row b: the key positions at which a tile, a staging block, a split or the
    valid range begins or ends; for causal cases the diagonal and the window's lower edge."""
    n, T = row_len(case, b), case.T
    if inf_cut(case, b) is not None:
        n = inf_cut(case, b)                                 # the last key the bias leaves visible
    if case.causal:
        win = case.window if 0 < case.window < T else 0
        return {t: (t if t % 2 == 0 or not win else max(0, t - win)) for t in range(0, T, 3)}
    want = [n - 1, 0, 63, 64, 255, 256, case.split_len - 1, case.split_len, 2 * case.split_len - 1, 2 * case.split_len, 127, 128, n - 2]
    keys = []
    for k in want:
        if 0 <= k < n and k not in keys:
            keys.append(k)
    return {t: k for t, k in enumerate(keys[:T])}


def _bias(case: AttnCase) -> Optional[torch.Tensor]:
    B, S = case.B, case.S
    if case.bias == "none":
        return None
    if case.bias == "minus300":
        return torch.full((B, S), -300.0)
    bias = torch.zeros(B, S)
    bias[:, 1::2] = 1.0                                     # float padding masks ADD 1.0 (quirk 1)
    if case.bias in ("inf_tail", "inf_row"):
        for b in range(B):
            bias[b, inf_cut(case, b):] = NEG_INF
    return bias


@functools.lru_cache(maxsize=None)
def attn_inputs(case: AttnCase, dtype) -> dict:
    """The operands of a case, quantised to `dtype`, as views into NaN-filled buffers: q / k / v (and dout) [B, rows, d] with a row
    stride > d -- the thirds of one packed [B, T + 1, 3d] buffer for self-attention, rows of d + PAD elements otherwise -- and one
    NaN row past the end.  K / V rows outside [kv_start[b], kv_start[b] + kv_len[b]) are NaN."""
    B, H, T, S, hd, d = case.B, case.H, case.T, case.S, case.hd, case.d
    seed = _seed(case)
    slot = max(row_start(case, b) + row_len(case, b) for b in range(B))          # K / V rows per batch row
    a = math.sqrt(6.0)
    if case.family == "peaked":
        q, k = rnd((B, T, d), seed, -a, a), rnd((B, slot, d), seed + 1, -a, a)
        v = rnd((B, slot, d), seed + 2)
    elif case.family == "growing":
        q, k, v = rnd((B, T, d), seed), rnd((B, slot, d), seed + 1), rnd((B, slot, d), seed + 2)
        k = k * torch.linspace(0.2, 30.0, slot).view(1, slot, 1)                 # |score| grows with the key index: the maximum keeps moving
        q[:, 40:48] *= 40.0                                                      # rows with huge scores of both signs
    elif case.family == "growing_mild":
        q, k, v = rnd((B, T, d), seed), rnd((B, slot, d), seed + 1), rnd((B, slot, d), seed + 2)
        k = k * torch.linspace(0.2, 10.0, slot).view(1, slot, 1)
    else:
        q, k = rnd((B, T, d), seed), rnd((B, slot, d), seed + 1)
        v = torch.where(rnd((B, slot, d), seed + 2) < 0, -1.0, 1.0)              # +-1 patterns, distinct per key
        c = 4.0 if hd == 64 else 6.0
        if case.S > 64 * 256:                                                    # one needle per (b, h), stronger: 16 684 keys compete
            assert T == 1 and B * H == 6
            for i, key in enumerate(cap_needles(case)):
                b, ch = i // H, slice((i % H) * hd, (i % H + 1) * hd)
                q[b, 0, ch] = (c + 2.0) * k[b, key, ch]
        else:
            for b in range(B):
                for t, key in needle_keys(case, b).items():
                    q[b, t] = c * k[b, row_start(case, b) + key]
    if case.causal:
        assert T == S and slot == S
        buf = torch.full((B, T + 1, 3 * d), float("nan"), dtype=dtype)
        qv, kv, vv = buf[:, :T, :d], buf[:, :T, d:2 * d], buf[:, :T, 2 * d:]
        qv.copy_(q); kv.copy_(k); vv.copy_(v)
        bufs = dict(qkv=buf)
    else:
        qb = torch.full((B, T + 1, d + PAD), float("nan"), dtype=dtype)
        kb = torch.full((B, slot + 1, d + PAD), float("nan"), dtype=dtype)
        vb = torch.full((B, slot + 1, d + PAD), float("nan"), dtype=dtype)
        qv, kv, vv = qb[:, :T, :d], kb[:, :slot, :d], vb[:, :slot, :d]
        qv.copy_(q); kv.copy_(k); vv.copy_(v)
        for b in range(B):
            lo, hi = row_start(case, b), row_start(case, b) + row_len(case, b)
            for t in (kv, vv):
                t[b, :lo] = float("nan")
                t[b, hi:] = float("nan")
        bufs = dict(q=qb, k=kb, v=vb)
    inp = dict(bufs=bufs, q=qv, k=kv, v=vv, bias=_bias(case), slot=slot, keep=None)
    if case.bwd:
        dob = torch.full((B, T + 1, d + PAD), float("nan"), dtype=dtype)
        dov = dob[:, :T, :d]
        dov.copy_(rnd((B, T, d), seed + 3))
        inp["dout"], inp["dout_buf"] = dov, dob
    if case.drop:
        inp["keep"] = keep_mask(B, H, T, S, *case.drop)
    return inp


def out_buffer(rows: int, cols_total: int, B: int, dtype) -> torch.Tensor:
    """A sentinel-filled [B, rows + 1, cols_total] buffer an output is a view into."""
    return torch.full((B, rows + 1, cols_total), SENTINEL, dtype=dtype)


def assert_view_only_written(buf_after: torch.Tensor, rows: int, col0: int, cols: int, what: str) -> None:
    """Everything of a sentinel-filled buffer outside [:, :rows, col0:col0+cols] still holds the sentinel, bit for bit."""
    after = bits(buf_after).clone()
    want = bits(torch.full((1,), SENTINEL, dtype=buf_after.dtype))[0]
    after[:, :rows, col0:col0 + cols] = want
    bad = after != want
    if bad.any():
        i = [int(x) for x in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the output view were written, first at {i}")


# ================================================================================================ reference

def visibility(case: AttnCase, b: int, h: int, n: int, bias_row: Optional[torch.Tensor]) -> torch.Tensor:
    """bool [T, n]: which of its n keys each query row of (b, h) sees."""
    T = case.T
    vis = torch.ones(T, n, dtype=torch.bool)
    if case.causal:
        vis &= tgt_attn_mask(T, case.window) == 0.0
    if case.blk is not None:
        bb = (b * case.H + h) % case.B                      # quirk 2: the block mask of batch row (b*H + h) % B
        lq, lkv = case.blk[0][bb], case.blk[1][bb]
        vis &= ~((torch.arange(T)[:, None] >= lq) & (torch.arange(n)[None, :] >= lkv))
    if bias_row is not None:
        vis &= (bias_row > NEG_INF)[None, :]
    return vis


def _ref_bh(Q, K, V, bias, vis, keep, c, dO, uT, hd):
    """Attention of one (batch row, head) in fp64 with its bounds.  Q [T, hd], K / V [n, hd], bias [n] or None, vis / keep bool
    [T, n], c = 1 / (1 - p).  Every symbol is the one of DESIGN.md's derivation."""
    T, n = vis.shape
    scale = 1.0 / math.sqrt(hd)
    absb = torch.zeros(n, dtype=torch.float64) if bias is None else torch.where(bias > NEG_INF, bias.abs(), 0.0)
    s = scale * Q @ K.t() + (0.0 if bias is None else torch.where(bias > NEG_INF, bias, 0.0))
    Aq = scale * Q.abs() @ K.abs().t()
    A = Aq + absb
    s = torch.where(vis, s, NEG_INF)
    m = s.max(dim=1).values
    has = m > NEG_INF
    ex = torch.where(vis, torch.exp(s - torch.where(has, m, 0.0)[:, None]), 0.0)
    l = ex.sum(dim=1)
    p = ex / torch.where(has, l, 1.0)[:, None]
    lse = torch.where(has, m + torch.log(torch.where(has, l, 1.0)), NEG_INF)
    Av = torch.where(vis, A, 0.0)
    Mrow = Av.max(dim=1).values + math.log(n + 1.0)
    cacc = 4.0 * (hd + 8) * U24
    E = torch.where(vis, uT * Aq + uT * uT * absb + cacc * (A + Mrow[:, None]) + 2 * U24, 0.0)
    Ebar = (p * E).sum(dim=1)
    Emax = E.max(dim=1).values
    F = torch.exp(2.0 * Emax)
    csum_n = (6.0 * (n + 2) + 160.0) * U24
    csum_t = (6.0 * (T + 2) + 160.0) * U24
    pk = p * keep * c
    O = pk @ V
    relp = E + Ebar[:, None] + uT + csum_n
    bO = (F[:, None] * ((pk * relp) @ V.abs())) * (1.0 + uT) + (uT + U24) * O.abs()
    lse_f = torch.where(has, lse, 0.0)
    blse = Ebar * F + (n + 2) * U24 * (1.0 + lse_f.abs())
    out = dict(o=(O, bO), lse=(lse, blse))
    if dO is None:
        return out
    Else = blse + uT * uT * lse_f.abs()
    rP = (E + Else[:, None]) * torch.exp(Emax + Else)[:, None]
    dP, AdP = dO @ V.t(), dO.abs() @ V.abs().t()
    delta, adelta = (dO * O).sum(dim=1), (dO.abs() * O.abs()).sum(dim=1)
    Edelta = (dO.abs() * bO).sum(dim=1) + (hd + 2) * U24 * adelta
    g = keep * c * dP - delta[:, None]
    Eg = cacc * (keep * c * AdP + delta.abs()[:, None]) + (Edelta + (uT * uT + 2 * U24) * delta.abs())[:, None]
    dS = p * g
    EdS = p * (rP * g.abs() + (1.0 + rP) * Eg)
    EdS = EdS + (uT + U24) * p * (1.0 + rP) * (g.abs() + Eg)
    dQ = scale * dS @ K
    bdQ = (scale * (EdS @ K.abs()) + csum_n * scale * (dS.abs() @ K.abs())) * (1.0 + uT) + (uT + U24) * dQ.abs()
    dK = scale * dS.t() @ Q
    bdK = (scale * (EdS.t() @ Q.abs()) + csum_t * scale * (dS.abs().t() @ Q.abs())) * (1.0 + uT) + (uT + U24) * dK.abs()
    dV = pk.t() @ dO
    bdV = ((pk * (rP + uT * (1.0 + rP))).t() @ dO.abs() + csum_t * (pk.t() @ dO.abs())) * (1.0 + uT) + (uT + U24) * dV.abs()
    out.update(dq=(dQ, bdQ), dk=(dK, bdK), dv=(dV, bdV))
    return out


def attention_ref(q, k, v, H, *, case: AttnCase, dtype, key_bias=None, keep=None, dout=None) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """Attention as the kernels define it (attention.hip's header), from the definition in fp64: q [B, T, d], k / v [B, slot, d]
    already quantised to `dtype`; masks, lengths and dropout as `case` says.  -> {name: (reference, bound)} for o [B, T, d],
    lse [B, H, T] and, with dout, dq / dk / dv (dk, dv [B, slot, d]: exactly 0, with bound 0, outside a row's keys)."""
    B, T, d = q.shape
    hd = d // H
    q, k, v = q.double(), k.double(), v.double()
    dout = None if dout is None else dout.double()
    c = 1.0 / (1.0 - case.drop[0]) if case.drop else 1.0
    uT = unit(dtype)
    res = {n: (torch.zeros(s, dtype=torch.float64), torch.zeros(s, dtype=torch.float64))
           for n, s in (("o", q.shape), ("lse", (B, H, T)), ("dq", q.shape), ("dk", k.shape), ("dv", v.shape))}
    for b in range(B):
        lo, n = row_start(case, b), row_len(case, b)
        bias = None if key_bias is None else key_bias[b, :n].double()            # key_bias[b][j] belongs to key kv_start[b] + j
        for h in range(H):
            ch = slice(h * hd, (h + 1) * hd)
            vis = visibility(case, b, h, n, bias)
            kp = torch.ones(T, n, dtype=torch.float64) if keep is None else keep[b, h, :, :n].double()
            r = _ref_bh(q[b, :, ch], k[b, lo:lo + n, ch], v[b, lo:lo + n, ch], bias, vis, kp, c, None if dout is None else dout[b, :, ch], uT, hd)
            for name, (val, bnd) in r.items():
                for dst, src in ((res[name][0], val), (res[name][1], bnd)):
                    if name == "lse":
                        dst[b, h] = src
                    elif name in ("o", "dq"):
                        dst[b, :, ch] = src
                    else:
                        dst[b, lo:lo + n, ch] = src
    if dout is None:
        res = {n: res[n] for n in ("o", "lse")}
    return res


@functools.lru_cache(maxsize=None)
def case_ref(case: AttnCase, dtype):
    inp = attn_inputs(case, dtype)
    return attention_ref(inp["q"], inp["k"], inp["v"], case.H, case=case, dtype=dtype, key_bias=inp["bias"], keep=inp["keep"],
                         dout=inp.get("dout"))


# ================================================================================================ comparison

def ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max |got - ref| / bound.  Where the reference is -inf (lse of a row without keys) or the bound is 0 (gradients of keys
    nobody sees) the output must equal the reference exactly; a NaN counts as infinitely wrong."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, f"shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    exact = (bound == 0) | ~torch.isfinite(ref)
    err = torch.where(exact, 0.0, (got - ref).abs())
    r = torch.where(exact, torch.where(got == ref, 0.0, float("inf")), err / torch.where(exact, 1.0, bound))
    r = torch.where(torch.isnan(r), float("inf"), r)
    return float(r.max())


def attn_ratios(case: AttnCase, dtype, outs: Dict[str, torch.Tensor]) -> Dict[str, float]:
    ref = case_ref(case, dtype)
    return {name: ratio(t, *ref[name]) for name, t in outs.items()}


def attn_check(case: AttnCase, dtype, outs: Dict[str, torch.Tensor], who: str = "") -> Dict[str, float]:
    """Prints the largest error / bound ratio of every output, then asserts that none exceeds 1."""
    r = attn_ratios(case, dtype, outs)
    print(f"attention {who}{case.name}-{TAG[dtype]}: max |err| / bound: " + ", ".join(f"{n} {x:.4f}" for n, x in r.items()))
    bad = {n: x for n, x in r.items() if not x <= 1.0}
    assert not bad, f"{case.name}-{TAG[dtype]}: outside the bound: {bad}"
    return r


def merge_partials(part: torch.Tensor, hd: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The documented merge of key-split partials in fp64.  part [..., nsplit, T, hd + 2]: un-normalised O, the reference
    maximum (log2 domain) and the sum of every split -> (o [..., T, hd], lse [..., T] in nats)."""
    part = part.double()
    o_j, m_j, l_j = part[..., :hd], part[..., hd], part[..., hd + 1]
    mm = m_j.max(dim=-2).values
    w = torch.where(m_j > NEG_INF, torch.exp2(m_j - torch.where(mm > NEG_INF, mm, 0.0).unsqueeze(-2)), 0.0)
    l = (l_j * w).sum(dim=-2)
    o = (o_j * w.unsqueeze(-1)).sum(dim=-3)
    ok = l > 0
    return torch.where(ok.unsqueeze(-1), o / torch.where(ok, l, 1.0).unsqueeze(-1), 0.0), \
        torch.where(ok, (mm + torch.log2(torch.where(ok, l, 1.0))) * math.log(2.0), NEG_INF)
