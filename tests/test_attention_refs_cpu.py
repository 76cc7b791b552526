"""The attention case table of oracle/attention_refs.py without a GPU: a torch CPU emulation of the kernels' arithmetic (fp32 with
the kernels' roundings to bf16: Q * scale * log2 e, the hi / lo slots of the augmented k-step, P and dS before their MFMAs,
the outputs; 64-key tiles with the lagged reference maximum; the documented merge of key-split partials) stands in for the
kernels.  It must meet every bound of the fp64 reference, and each of a list of subtly wrong variants must exceed the bound on
the case designed for it -- which is what shows that the bounds tests/test_attention_branches_gpu.py asserts can see them."""
import math

import pytest
import torch

from oracle import attention_refs as R
from oracle.kernel_refs import BF16, DTYPES, F32

LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
NEG_INF = float("-inf")


def _rd(x, dtype):
    """Rounded to the operand type, held in fp32."""
    return x.to(dtype).float()


def _aug(x, dtype):
    """A value carried by the augmented k-step: exact in fp32; hi + lo bf16 slots otherwise (inf - inf = NaN is dropped)."""
    if dtype == F32:
        return x
    hi = _rd(x, dtype)
    lo = _rd(torch.nan_to_num(x - hi, nan=0.0, posinf=0.0, neginf=0.0), dtype)
    return hi + lo


def _fwd_range(qf, K, V, b2, vis, keep, beg, end, dtype, mut):
    """One key split [beg, end) of the forward, tile by tile: -> (un-normalised O [T, hd], reference maximum, sum)."""
    T, hd = qf.shape
    m_ref, l, acc = torch.zeros(T), torch.zeros(T), torch.zeros(T, hd)
    m_set = torch.zeros(T, dtype=torch.bool)
    for t0 in range(beg, end, 64):
        t1 = min(t0 + 64, end)
        if mut == "tile_renorm" and t0 == 64:
            continue
        st = qf @ K[t0:t1].t() + b2[t0:t1] - m_ref[:, None]
        st = torch.where(vis[:, t0:t1], st, NEG_INF)
        mx = st.max(dim=1).values
        fix = torch.where(m_set, mx > 8.0, mx > NEG_INF)
        m2 = torch.where(fix, _rd(m_ref + torch.where(fix, mx, 0.0), dtype), m_ref)
        delta = m2 - m_ref
        alpha = torch.where(fix & m_set, torch.exp2(-delta), 1.0)
        st = st - delta[:, None]
        l, acc, m_ref, m_set = l * alpha, acc * alpha[:, None], m2, m_set | fix
        p = torch.exp2(st)
        l = l + p.sum(dim=1)
        if mut == "tile" and t0 == 64:
            continue
        acc = acc + _rd(p * keep[:, t0:t1], dtype) @ V[t0:t1]
    return acc, torch.where(l > 0, m_ref, NEG_INF), l


def _emulate_bh(Q, K, V, bias, vis, keep, c, dO, dtype, splits, mut):
    T, hd = Q.shape
    n = K.shape[0]
    scale = 1.0 / math.sqrt(hd)
    sc2 = (1.0 if mut == "scale" else scale) * LOG2E
    qf = _rd(Q * sc2, dtype)
    b2 = torch.zeros(n) if bias is None else _aug(bias * LOG2E, dtype)
    parts = [_fwd_range(qf, K, V, b2, vis, keep, beg, end, dtype, mut) for beg, end in splits]
    if mut == "merge_skip":
        parts = parts[:1] + parts[2:]
    m_j, l_j = torch.stack([p[1] for p in parts]), torch.stack([p[2] for p in parts])
    mm = m_j.max(dim=0).values
    w = torch.where(m_j > NEG_INF, torch.exp2(m_j - torch.where(mm > NEG_INF, mm, 0.0)), 0.0)
    if mut == "merge_w1":
        w = torch.where(m_j > NEG_INF, 1.0, 0.0)
    l = (l_j * w).sum(dim=0)
    acc = sum(p[0] * w[j][:, None] for j, p in enumerate(parts))
    ok = l > 0
    inv = torch.where(ok, c / torch.where(ok, l, 1.0), 0.0)
    O = _rd(acc * inv[:, None], dtype)
    lse = torch.where(ok, (mm + torch.log2(torch.where(ok, l, 1.0))) * LN2, NEG_INF)
    out = dict(o=O, lse=lse)
    if dO is None:
        return out
    lse2 = torch.where(ok, lse * LOG2E, 0.0)
    ndc = -(O * dO).sum(dim=1) / c
    dp = dO @ V.t() + _aug(ndc, dtype)[:, None]
    dp = torch.where(keep > 0, dp, ndc[:, None])
    gone = torch.zeros(n, dtype=torch.bool)
    if mut in ("tile", "tile_renorm"):
        gone[64:128] = True

    def probs(a, bmat):
        st = a @ bmat.t() + b2 - _aug(lse2, dtype)[:, None]
        return torch.where(vis & ~gone, torch.exp2(st), 0.0)
    # dQ kernel: Q * scale * log2 e rounded, K raw; partial sums per key split in fp32
    dS = _rd(probs(qf, K) * dp, dtype)
    pq = [(dS[:, beg:end] @ K[beg:end]) * (scale * c) for beg, end in splits]
    if mut == "dq_skip":
        pq = pq[:1] + pq[2:]
    dQ = _rd(sum(pq), dtype)
    # dK / dV kernel: K * scale * log2 e rounded, Q raw
    P2 = probs(Q, _rd(K * sc2, dtype))
    dK = _rd((_rd(P2 * dp, dtype).t() @ Q) * (scale * c), dtype)
    dV = _rd((_rd(P2 * keep, dtype).t() @ dO) * c, dtype)
    if mut == "dk_zero":
        dK = torch.zeros_like(dK)
    if mut == "dv_zero":
        dV = torch.zeros_like(dV)
    out.update(dq=dQ, dk=dK, dv=dV)
    return out


def emulate(case, dtype, mut=None):
    """Every output of a case from the emulation, in the layout of attention_ref.  mut: one of the wrong variants."""
    inp = R.attn_inputs(case, dtype)
    B, H, T, hd = case.B, case.H, case.T, case.hd
    q, k, v = inp["q"].float(), inp["k"].float().clone(), inp["v"].float().clone()
    dout = inp["dout"].float() if case.bwd else None
    c = 1.0 / (1.0 - case.drop[0]) if case.drop else 1.0
    outs = dict(o=torch.zeros_like(q), lse=torch.zeros(B, H, T))
    if case.bwd:
        outs.update(dq=torch.zeros_like(q), dk=torch.zeros_like(k), dv=torch.zeros_like(v))
    for b in range(B):
        lo, n = R.row_start(case, b), R.row_len(case, b)
        bias = None if inp["bias"] is None else inp["bias"][b, :n].clone()
        if mut == "bias_off":
            bias = None
        if mut == "bias_shift":                               # key_bias read at kv_start + j in place of j
            bias = inp["bias"][b, torch.clamp(torch.arange(n) + lo, max=case.S - 1)]
        kb, vb = k[b, lo:lo + n], v[b, lo:lo + n]
        extra = mut == "extra_key"
        if extra:                                             # one key past the end: a finite stand-in that looks like the last key
            kb, vb = torch.cat([kb, kb[-1:]]), torch.cat([vb, -vb[-1:]])
            bias = None if bias is None else torch.cat([bias, bias[-1:]])
        if mut == "swap_v":
            vb = vb.clone()
            m2 = n // 2 * 2
            vb[:m2] = vb[:m2].view(m2 // 2, 2, -1).flip(1).reshape(m2, -1)
        if mut in ("block_stale", "block_drop"):              # the second 256-key staging block of every 512-key split
            kb, vb, bias = kb.clone(), vb.clone(), bias.clone()
            for beg in range(0, n, case.split_len):
                m = max(0, min(n, beg + case.split_len) - (beg + 256))
                if mut == "block_stale":                      # ... holds the first block's K, V and bias again
                    for t in (kb, vb, bias):
                        t[beg + 256:beg + 256 + m] = t[beg:beg + m]
                else:                                         # ... is never walked
                    bias[beg + 256:beg + 256 + m] = NEG_INF
        nn = kb.shape[0]
        if case.nsplit > 1:
            splits = [(j * case.split_len, min((j + 1) * case.split_len, nn)) for j in range(case.nsplit)]
            splits = [(beg, max(beg, end)) for beg, end in splits]
        else:
            splits = [(0, nn)]
        for h in range(H):
            ch = slice(h * hd, (h + 1) * hd)
            vis = R.visibility(case, b, h, n, None if inp["bias"] is None else inp["bias"][b, :n])
            if extra:
                vis = torch.cat([vis, torch.ones(T, 1, dtype=torch.bool)], dim=1)
            qi = torch.arange(T)[:, None]
            ki = torch.arange(nn)[None, :]
            if mut == "last_key":
                seen = vis.any(dim=0).nonzero()
                if seen.numel():
                    vis = vis & (ki != int(seen.max()))
            if mut == "causal_plus":
                vis = vis | (ki == qi + 1)
            if mut == "causal_minus":
                vis = vis & (ki != qi)
            if mut == "window_edge":
                vis = vis & (ki != qi - case.window)
            if inp["keep"] is None:
                keep = torch.ones(T, nn)
            else:
                bh = b * H + h
                if mut == "keep_other":
                    bh = (bh + 1) % (B * H)
                keep = inp["keep"][bh // H, bh % H].float()
            r = _emulate_bh(q[b, :, ch], kb[:, ch], vb[:, ch], bias, vis, keep, c, None if dout is None else dout[b, :, ch], dtype, splits, mut)
            outs["o"][b, :, ch], outs["lse"][b, h] = r["o"], r["lse"]
            if case.bwd:
                outs["dq"][b, :, ch] = r["dq"]
                outs["dk"][b, lo:lo + n, ch], outs["dv"][b, lo:lo + n, ch] = r["dk"][:n], r["dv"][:n]
    if case.bwd:                                               # the kernels write nothing outside a row's keys; the reference is 0 there
        for name in ("dk", "dv"):
            outs[name] = torch.nan_to_num(outs[name], nan=0.0)
    return outs


CPU_CASES = [c for c in R.ALL_CASES]


def test_case_table_states_the_split_plan():
    for c in R.ALL_CASES:
        assert R.expected_split(c) == (c.nsplit, c.split_len), c.name
        assert c.B * c.H <= 6 and c.d <= 128, c.name


def test_mild_growing_scores_move_the_reference_on_later_tiles():
    """The case exists for the rescale branch of the lagged maximum: a later tile's maximum exceeds the reference by more than
    2^8 for most rows, while the bf16 score error u A_k stays small enough for the bound to mean something."""
    case = R.CASE["grow-mild-t64-s640-hd64"]
    inp = R.attn_inputs(case, BF16)
    q, k = inp["q"].double()[0], inp["k"].double()[0]
    s2 = (q @ k.t()) / 8.0 * LOG2E                             # log2 domain; the constant bias moves nothing
    first = s2[:, :64].max(dim=1).values
    assert int((s2.max(dim=1).values > first + 8.0).sum()) >= 48
    assert float((q.abs() @ k.abs().t()).max()) / 8.0 * R.U8 < 0.125


def test_keep_mask_rate_and_independence():
    m = R.keep_mask(2, 2, 40, 1041, 0.25, 99)
    assert abs(m.float().mean().item() - 0.75) < 0.01
    assert not torch.equal(m[0, 0], m[0, 1]) and not torch.equal(m[0, 0], m[1, 0])
    assert R.keep_mask(1, 1, 3, 5, 0.0, 1).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=R.case_id)
@pytest.mark.parametrize("case", CPU_CASES, ids=R.case_id)
def test_emulation_meets_every_bound(case, dtype):
    R.attn_check(case, dtype, emulate(case, dtype), who="emulation ")


# mutant -> (case designed for it, outputs on which it must show)
MUTANTS = [
    ("tile", "t40-s300-hd32-inftail", ("o", "dq", "dk", "dv")),               # one 64-key tile dropped, the sum keeps it
    ("tile", "split2-t40-s1041-hd64", ("o", "dk", "dv")),                     # (the needle rows' softmax is saturated: dQ ~ 0)
    ("tile_renorm", "t40-s300-hd32-inftail", ("o", "lse", "dq", "dk", "dv")),
    ("tile_renorm", "split2-t40-s1041-hd64", ("o", "lse", "dq", "dk", "dv")),  # ... and renormalised
    ("tile", "dec-t20-s256-hd32", ("o",)),
    ("tile_renorm", "dec-t20-s700-hd64", ("o", "lse")),
    ("block_stale", "dec-cap-hd32", ("o", "lse")),
    ("block_stale", "dec-cap-hd64", ("o", "lse")),
    ("block_drop", "dec-cap-hd32", ("o", "lse")),
    ("block_drop", "dec-cap-hd64", ("o", "lse")),
    ("last_key", "dec-t1-s700-hd32", ("o", "lse")),
    ("last_key", "varlen-hd64", ("o", "lse")),
    ("last_key", "rows-hd32", ("o", "lse")),
    ("last_key", "t33-s129-hd64-infrow", ("o", "lse", "dq", "dk", "dv")),
    ("extra_key", "varlen-hd64", ("o", "lse")),
    ("extra_key", "rows-hd32", ("o", "lse")),
    ("extra_key", "dec-t1-s65-hd64", ("o", "lse")),
    ("extra_key", "t129-s64-hd64-needles", ("o", "lse")),
    ("swap_v", "dec-t1-s700-hd32", ("o",)),
    ("swap_v", "split2-t40-s1041-hd64", ("o", "dq", "dk")),                    # dV does not depend on V
    ("bias_off", "t33-s65-hd32-plus1", ("o", "lse", "dq", "dk", "dv")),
    ("bias_off", "dec-t20-s700-hd64", ("o", "lse")),
    ("bias_off", "varlen-hd32-peaked", ("o", "lse")),
    ("bias_shift", "rows-hd64-peaked", ("o", "lse")),
    ("bias_shift", "rows-hd32", ("lse",)),
    ("scale", "t33-s65-hd32-plus1", ("o", "lse", "dq", "dk", "dv")),
    ("scale", "dec-t20-s700-hd64", ("o", "lse")),
    ("causal_plus", "causal-t129-hd32-peaked", ("o", "lse", "dq", "dk", "dv")),
    ("causal_minus", "causal-t129-hd64", ("o", "lse", "dq", "dk", "dv")),
    ("window_edge", "causal-win20-t150-hd32", ("o", "lse", "dq", "dk", "dv")),
    ("merge_skip", "split2-t40-s1041-hd64", ("o", "lse")),
    ("merge_skip", "dec-t20-s257-hd64", ("o", "lse")),
    ("merge_w1", "split3-t129-s1553-hd32", ("o", "lse")),
    ("merge_w1", "dec-t20-s700-hd64", ("o", "lse")),
    ("dk_zero", "split2-t40-s1041-hd64", ("dk",)),
    ("dk_zero", "t33-s65-hd32-plus1", ("dk",)),
    ("dv_zero", "split2-t40-s1041-hd64", ("dv",)),
    ("dv_zero", "t33-s65-hd32-plus1", ("dv",)),
    ("dq_skip", "split3-t129-s1553-hd32", ("dq",)),
    ("keep_other", "drop-t33-s65-hd64", ("o", "dq", "dk", "dv")),
    ("keep_other", "drop-split2-t40-s1041-hd32", ("o", "dq", "dk", "dv")),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=R.case_id)
@pytest.mark.parametrize("mut,name,shows", MUTANTS, ids=[f"{m}-{n}" for m, n, _ in MUTANTS])
def test_wrong_variant_exceeds_its_bound(mut, name, shows, dtype):
    case = R.CASE[name]
    r = R.attn_ratios(case, dtype, emulate(case, dtype, mut))
    print(f"mutant {mut} on {name}-{R.TAG[dtype]}: " + ", ".join(f"{n} {x:.3g}" for n, x in r.items()))
    for out in shows:
        assert r[out] > 1.0, (mut, name, out, r[out])
