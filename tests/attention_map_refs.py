"""Float64 reference and per-element error bound of the attention map kernel (csrc/attention_map.hip, omr_attn_weights), the
case table of tests/test_attention_map_gpu.py, and the decoder-level reference of Decoder.cross_attention_maps written with the
pieces of oracle/ref_cpu.py.  oracle/attention_refs.py is used as it stands (AttnCase, attn_inputs, visibility, keep_mask,
ratio, unit); the cases here are this file's own.

    w[b][t][s] = out_scale * sum_h c m_bhts p_bhts,      p = softmax over the visible keys of q.k / sqrt(hd) + key_bias

The bound ("Attention maps"; symbols of "Attention error bounds"): the kernel recomputes P = exp2(score - lse log2e)
from the forward's lse, so the relative error of one P is the backward's  rP_k = (E_k + E_lse) exp(Emax + E_lse)  with the
score error E_k of that section and  E_lse = bound(lse) + (u^2 + e) |lse|  -- the forward's own bound on lse, the hi + lo split
of `Aug` (u^2) and the fp32 product lse * log2e (e), which the kernel forms before the split.  P stays in fp32 (nothing is
rounded to T after the score chain), and the fp32 side is counted from the source: H - 1 adds in head order, the rounding of
out_scale itself to fp32, the product out_scale * c on the host, the one multiply by it, and the add of `accumulate`: H + 3
roundings, taken as gamma = (H + 3) e / (1 - (H + 3) e) on the computed value:

    |w - ref| <= (1 + gamma) out_scale sum_h c m p rP  +  gamma ref

Hidden keys (mask, -inf bias, past kv_len) and rows without a visible key have ref = 0 with bound 0: exact zeros.
Test infrastructure only: nothing here is imported by the package."""
from __future__ import annotations

import functools
import math
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from oracle import attention_refs as R
from oracle import ref_cpu as O
from oracle.kernel_refs import U24

NEG_INF = float("-inf")


def _cases():
    C = R.AttnCase
    return (
        C("map-peaked-t1-s5-hd64", "fwd", 2, 4, 1, 5, 64),
        C("map-t33-s65-hd32-plus1", "fwd", 2, 2, 33, 65, 32, family="needles", bias="plus1"),
        C("map-h3-t70-s64-hd32", "fwd", 1, 3, 70, 64, 32, family="needles"),
        C("map-t33-s129-hd64-infrow", "fwd", 3, 2, 33, 129, 64, family="needles", bias="inf_row"),
        C("map-t40-s300-hd32-inftail", "fwd", 2, 2, 40, 300, 32, family="needles", bias="inf_tail"),
        C("map-blk-b3-h4-t40-s100-hd32", "fwd", 3, 4, 40, 100, 32, blk=((10, 40, 0), (30, 50, 64))),
        C("map-kvlen-t20-s300-hd64", "varlen", 4, 2, 20, 300, 64, family="needles", kv_len=(1, 64, 65, 300)),
        C("map-causal-t129-hd64", "fwd", 1, 2, 129, 129, 64, family="needles", causal=True),
        C("map-causal-win20-t150-hd32", "fwd", 1, 2, 150, 150, 32, family="needles", causal=True, window=20),
        C("map-drop-t33-s65-hd64", "fwd", 2, 2, 33, 65, 64, drop=(0.25, 1234)),
        C("map-drop-causal-t129-hd32", "fwd", 1, 2, 129, 129, 32, family="needles", causal=True, drop=(0.25, 77)),
    )


def _range_cases():
    """Shapes at which the launcher's own plan (omr_attn_weights_range) gives a workgroup MORE than one 64-key tile: B ceil(T / 128)
    is large enough that ~1 024 workgroups need fewer ranges than there are tiles.  64 x 1 block, 18 tiles: 16 ranges wanted, 2 tiles
    each; 128 x 3 blocks, 5 tiles: 3 ranges wanted, 2 tiles each."""
    C = R.AttnCase
    lens = (1, 64, 65, 129, 700, 1089, 128, 200) * 8         # rows that end inside a range, on a range's edge, in its second tile
    return (
        C("map-range2-kvlen-b64-t1-s1089-hd32", "varlen", 64, 2, 1, 1089, 32, family="needles", kv_len=lens),
        C("map-range2-inftail-drop-b64-t1-s1089-hd64", "fwd", 64, 2, 1, 1089, 64, bias="inf_tail", drop=(0.25, 4321)),
        # causal + window 20, three query blocks: block 1 (q0 = 128) computes tile 64 of range [0, 128) and zero-fills tile 0;
        # block 0 zero-fills all of range [128, 256); block 2 (q0 = 256) computes tiles 192 and 256, each in another range
        C("map-range2-causal-win20-b128-t300-hd32", "fwd", 128, 2, 300, 300, 32, family="needles", causal=True, window=20),
    )


MAP_CASES = _cases()
RANGE_CASES = _range_cases()
MAP_CASE = {c.name: c for c in MAP_CASES + RANGE_CASES}


def expected_range(B: int, T: int, S: int, min_wg: int = 1024) -> int:
    """choose_range of csrc/attention_map.hip restated: keys per workgroup."""
    blocks = B * ((T + 127) // 128)
    ntile = (S + 63) // 64
    want = max(1, min((min_wg + blocks - 1) // blocks, ntile))
    return (ntile + want - 1) // want * 64


def _p_and_rel(Q, K, bias, vis, uT, hd):
    """One (batch row, head) in fp64: the exact probabilities p [T, n], the relative error bound rP [T, n] of the kernel's
    recomputed ones, and the row's lse (0 where no key is visible) with the forward's bound on it -- the quantities of
    oracle.attention_refs' own per-head routine, to which tests/test_attention_map_refs_cpu.py holds lse and its bound.
    Q [T, hd], K [n, hd], bias [n] or None, vis bool [T, n]."""
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
    lse = torch.where(has, m + torch.log(torch.where(has, l, 1.0)), 0.0)
    Mrow = torch.where(vis, A, 0.0).max(dim=1).values + math.log(n + 1.0)
    cacc = 4.0 * (hd + 8) * U24
    E = torch.where(vis, uT * Aq + uT * uT * absb + cacc * (A + Mrow[:, None]) + 2 * U24, 0.0)
    Ebar = (p * E).sum(dim=1)
    Emax = E.max(dim=1).values
    blse = Ebar * torch.exp(2.0 * Emax) + (n + 2) * U24 * (1.0 + lse.abs())          # the forward's bound on its lse
    Else = blse + (uT * uT + U24) * lse.abs()
    rP = (E + Else[:, None]) * torch.exp(Emax + Else)[:, None]
    return p, rP, lse, blse


def weights_ref(q, k, H: int, *, case: R.AttnCase, dtype, key_bias=None, keep=None, out_scale: Optional[float] = None):
    """-> (w_ref fp64 [B, T, S], bound fp64 [B, T, S]) of omr_attn_weights for q [B, T, d], k [B, slot, d] already quantised to
    `dtype`; masks, lengths and dropout as `case` says (keep: bool [B, H, T, S]).  out_scale defaults to 1 / H."""
    B, T, d = q.shape
    hd = d // H
    q, k = q.double(), k.double()
    c = 1.0 / (1.0 - case.drop[0]) if case.drop else 1.0
    out_scale = 1.0 / H if out_scale is None else out_scale
    uT = R.unit(dtype)
    w = torch.zeros(B, T, case.S, dtype=torch.float64)
    bp = torch.zeros(B, T, case.S, dtype=torch.float64)
    for b in range(B):
        lo, n = R.row_start(case, b), R.row_len(case, b)
        bias = None if key_bias is None else key_bias[b, :n].double()
        for h in range(H):
            ch = slice(h * hd, (h + 1) * hd)
            vis = R.visibility(case, b, h, n, bias)
            p, rP, _, _ = _p_and_rel(q[b, :, ch], k[b, lo:lo + n, ch], bias, vis, uT, hd)
            pk = p * c if keep is None else p * keep[b, h, :, :n].double() * c
            w[b, :, :n] += out_scale * pk
            bp[b, :, :n] += out_scale * pk * rP
    g = (H + 3) * U24 / (1.0 - (H + 3) * U24)
    return w, (1.0 + g) * bp + g * w


@functools.lru_cache(maxsize=None)
def map_case_ref(case: R.AttnCase, dtype):
    inp = R.attn_inputs(case, dtype)
    return weights_ref(inp["q"], inp["k"], case.H, case=case, dtype=dtype, key_bias=inp["bias"], keep=inp["keep"])


def map_check(name: str, got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """Prints the largest error / bound ratio, then asserts that it does not exceed 1 (equality where the bound is 0)."""
    r = R.ratio(got, ref, bound)
    print(f"attention map {name}: max |err| / bound: {r:.4f}")
    assert r <= 1.0, f"{name}: outside the bound: {r}"
    return r


# ================================================================================================ decoder level

def mha_weights(q_in, kv_in, in_w, in_b, nhead: int, score_bias=None):
    """The head-averaged softmax of oracle.ref_cpu.mha's scores (its projections, scale and bias rule): [B, T, S]."""
    b, t, d = q_in.shape
    s = kv_in.shape[1]
    hd = d // nhead
    q = F.linear(q_in, in_w[:d], in_b[:d]).view(b, t, nhead, hd).transpose(1, 2)
    k = F.linear(kv_in, in_w[d:2 * d], in_b[d:2 * d]).view(b, s, nhead, hd).transpose(1, 2)
    scores = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(hd)
    if score_bias is not None:
        scores = scores + score_bias
    return torch.softmax(scores, dim=-1).mean(dim=1)


def decoder_maps_ref(sd, p: str, tgt, memory, memory_len, cfg: O.OracleCfg, layers: Optional[Sequence[int]] = None,
                     tgt_padding_bias: bool = True) -> Tuple[torch.Tensor, torch.Tensor, List[torch.Tensor]]:
    """oracle.ref_cpu.decoder (eval mode) restated with its own pieces, keeping the cross-attention map of every layer:
    -> (logits [B, V, T], the average of the maps of `layers` [B, T, S], every layer's map)."""
    b, t = tgt.shape
    x = sd[p + "embedding.weight"][tgt] + O.pe1d_table(t, cfg.d_model)
    mem_bias = O.memory_key_bias(memory, memory_len)
    self_bias = O.tgt_attn_mask(t, cfg.attn_window).view(1, 1, t, t)
    if mem_bias is not None:
        if tgt_padding_bias:
            self_bias = self_bias + (tgt == cfg.pad_idx).to(torch.float32).view(b, 1, 1, t)
        mem_bias = mem_bias.view(b, 1, 1, -1)
    maps = []
    for i in range(cfg.num_layers):
        lp = f"{p}transformer_decoder.layers.{i}."
        sa = O.mha(x, x, sd[lp + "self_attn.in_proj_weight"], sd[lp + "self_attn.in_proj_bias"], sd[lp + "self_attn.out_proj.weight"],
                   sd[lp + "self_attn.out_proj.bias"], cfg.nhead, self_bias)
        x = O.layer_norm(x + sa, sd[lp + "norm1.weight"], sd[lp + "norm1.bias"])
        ca_w, ca_b = sd[lp + "multihead_attn.in_proj_weight"], sd[lp + "multihead_attn.in_proj_bias"]
        maps.append(mha_weights(x, memory, ca_w, ca_b, cfg.nhead, mem_bias))
        ca = O.mha(x, memory, ca_w, ca_b, sd[lp + "multihead_attn.out_proj.weight"], sd[lp + "multihead_attn.out_proj.bias"], cfg.nhead, mem_bias)
        x = O.layer_norm(x + ca, sd[lp + "norm2.weight"], sd[lp + "norm2.bias"])
        ff = F.linear(F.relu(F.linear(x, sd[lp + "linear1.weight"], sd[lp + "linear1.bias"])), sd[lp + "linear2.weight"], sd[lp + "linear2.bias"])
        x = O.layer_norm(x + ff, sd[lp + "norm3.weight"], sd[lp + "norm3.bias"])
    logits = F.linear(x, sd[p + "out_layer.weight"][:, :, 0], sd[p + "out_layer.bias"]).permute(0, 2, 1).contiguous()
    sel = list(range(cfg.num_layers)) if layers is None else list(layers)
    return logits, torch.stack([maps[i] for i in sel]).mean(dim=0), maps
