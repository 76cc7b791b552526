"""Branch-level tests of the attention kernels (csrc/attention.hip, csrc/attention_bwd.hip, csrc/attn_common.h) against the fp64
reference of oracle/attention_refs.py.  Every output is held to the reference's per-element error bound (derivation: DESIGN.md,
"Attention error bounds"); each test prints its largest error / bound ratio before it asserts <= 1.  Operands are views into
NaN-filled buffers with row strides > d, outputs views into sentinel-filled ones that must come back untouched outside the view.
tests/test_attention_refs_cpu.py runs the same case table with a CPU emulation and shows which wrong kernels these bounds see."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from omr_a2s_multimodal_transformer_amd import kernels as K  # noqa: E402
from omr_a2s_multimodal_transformer_amd._lib import cur_stream, dtype_code, lib, ptr  # noqa: E402
from oracle import attention_refs as R  # noqa: E402
from oracle.kernel_refs import BF16, DTYPES, F32, SENTINEL, assert_bit_equal  # noqa: E402

DEV = "cuda:0"
ENTRY = {"split": "omr_attn_fwd_split", "varlen": "omr_attn_fwd_split_varlen", "rows": "omr_attn_fwd_split_rows"}


def _is_sentinel(t) -> bool:
    return bool((t == torch.full((), SENTINEL, dtype=t.dtype, device=t.device)).all())


def _strides(*ts):
    """(row strides..., batch strides...) of [B, rows, cols] views, the order every entry takes them in."""
    assert all(t.stride(2) == 1 for t in ts)
    return tuple(t.stride(1) for t in ts) + tuple(t.stride(0) for t in ts)


class Run:
    """The device side of one (case, dtype): operands uploaded with their NaN padding, outputs as views into sentinel buffers."""

    def __init__(self, case, dtype):
        self.case, self.dtype = case, dtype
        inp = self.inp = R.attn_inputs(case, dtype)
        B, H, T, d, slot = case.B, case.H, case.T, case.d, inp["slot"]
        self.bufs = {n: t.to(DEV) for n, t in inp["bufs"].items()}
        if case.causal:
            g = self.bufs["qkv"]
            self.q, self.k, self.v = g[:, :T, :d], g[:, :T, d:2 * d], g[:, :T, 2 * d:]
        else:
            self.q, self.k, self.v = self.bufs["q"][:, :T, :d], self.bufs["k"][:, :slot, :d], self.bufs["v"][:, :slot, :d]
        self.bias = None if inp["bias"] is None else inp["bias"].to(DEV)
        self.o_buf = R.out_buffer(T, d + R.PAD, B, dtype).to(DEV)
        self.o = self.o_buf[:, :T, :d]
        self.lse_buf = torch.full((B * H * T + 16,), SENTINEL, dtype=torch.float32, device=DEV)
        self.lse = self.lse_buf[:B * H * T].view(B, H, T)
        self.blk = (None, None) if case.blk is None else tuple(torch.tensor(x, dtype=torch.int32, device=DEV) for x in case.blk)
        self.kv_len = None if case.kv_len is None else torch.tensor(case.kv_len, dtype=torch.int32, device=DEV)
        self.kv_start = None if case.kv_start is None else torch.tensor(case.kv_start, dtype=torch.int32, device=DEV)
        self.p, self.seed = case.drop or (0.0, 0)
        self.words = None
        if case.drop:       # the words the kernels read and the byte mask of the same (p, seed); the reference uses the latter
            self.words = K.attn_dropout_words(B, H, T, case.S, self.p, self.seed, DEV)
            mask = K.attn_dropout_mask(B, H, T, case.S, self.p, self.seed, DEV)
            assert torch.equal(mask.cpu().bool(), inp["keep"]), "omr_attn_dropout_mask differs from the hash restated in oracle/attention_refs.py"

    def workspace(self, split_entry: bool):
        c = self.case
        if split_entry:
            n = lib().query("omr_attn_split_workspace_floats", c.B, c.H, c.T, c.S, c.hd)
        else:
            n = lib().query("omr_attn_workspace_floats", c.B, c.H, c.T, c.S, c.hd, int(c.causal), 0)
        want = c.B * c.H * c.T * (c.hd + 2) * c.nsplit if c.nsplit > 1 else 0
        assert n == want, f"{c.name}: the plan gives {n / (c.B * c.H * c.T * (c.hd + 2))} splits, the case wants {c.nsplit}"
        return torch.full((max(n, 1) + 8,), SENTINEL, dtype=torch.float32, device=DEV), n

    def shape_args(self):
        c = self.case
        return (dtype_code(self.dtype), ptr(self.q), ptr(self.k), ptr(self.v), ptr(self.o), ptr(self.lse),
                *_strides(self.q, self.k, self.v, self.o), c.B, c.H, c.T, c.S, c.hd)

    def forward(self):
        c = self.case
        if c.entry == "fwd":
            ws, n = self.workspace(False)
            lib().call("omr_attn_fwd_ws", *self.shape_args(), int(c.causal), c.window, ptr(self.bias), ptr(self.blk[0]), ptr(self.blk[1]),
                       float(self.p), self.seed, ptr(self.words), ptr(ws) if n else None, n, cur_stream())
        elif c.entry == "partials":
            ws, n = self.workspace(True)
            ns = ctypes.c_int(0)
            lib().call("omr_attn_fwd_split_partials", *self.shape_args(), ptr(ws), n, ctypes.byref(ns), cur_stream())
            self.nsplit_out = ns.value
        else:
            ws, n = self.workspace(True)
            extra = {"split": (), "varlen": (ptr(self.kv_len),), "rows": (ptr(self.kv_len), ptr(self.kv_start))}[c.entry]
            lib().call(ENTRY[c.entry], *self.shape_args(), ptr(self.bias), *extra, ptr(ws), n, cur_stream())
        torch.cuda.synchronize()
        self.ws, self.ws_n = ws, n
        assert _is_sentinel(ws[n:]), "the workspace was written past its size"
        return dict(o=self.o.cpu(), lse=self.lse.cpu())

    def backward(self):
        c, inp = self.case, self.inp
        B, T, d, slot = c.B, c.T, c.d, inp["slot"]
        self.dout_buf = inp["dout_buf"].to(DEV)
        dout = self.dout_buf[:, :T, :d]
        o_before = self.o_buf.clone()
        if c.causal:
            self.g_bufs = dict(dqkv=R.out_buffer(T, 3 * d, B, self.dtype).to(DEV))
            g = self.g_bufs["dqkv"]
            dq, dk, dv = g[:, :T, :d], g[:, :T, d:2 * d], g[:, :T, 2 * d:]
        else:
            self.g_bufs = dict(dq=R.out_buffer(T, d + R.PAD, B, self.dtype).to(DEV), dk=R.out_buffer(slot, d + R.PAD, B, self.dtype).to(DEV),
                               dv=R.out_buffer(slot, d + R.PAD, B, self.dtype).to(DEV))
            dq, dk, dv = self.g_bufs["dq"][:, :T, :d], self.g_bufs["dk"][:, :slot, :d], self.g_bufs["dv"][:, :slot, :d]
        n = lib().query("omr_attn_workspace_floats", c.B, c.H, c.T, c.S, c.hd, int(c.causal), 1)
        assert n == (c.nsplit * B * T * d if c.nsplit > 1 else 0), (c.name, n)
        K.attn_bwd(self.q, self.k, self.v, self.o, dout, self.lse, dq, dk, dv, c.H, causal=c.causal, window=c.window, key_bias=self.bias,
                   blk_lq=self.blk[0], blk_lkv=self.blk[1], dropout_p=self.p, seed=self.seed, drop_words=self.words)
        torch.cuda.synchronize()
        assert_bit_equal(self.o_buf, o_before.cpu(), f"{c.name}: o after the backward")
        assert_bit_equal(self.dout_buf, inp["dout_buf"], f"{c.name}: dout after the backward")
        return dict(dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu())

    def check_untouched(self):
        """No operand changed, and nothing outside an output view was written."""
        c, T, d = self.case, self.case.T, self.case.d
        for n, t in self.inp["bufs"].items():
            assert_bit_equal(self.bufs[n], t, f"{c.name}: operand buffer {n}")
        R.assert_view_only_written(self.o_buf, T, 0, d, f"{c.name}: o")
        B, H = c.B, c.H
        assert _is_sentinel(self.lse_buf[B * H * T:]), f"{c.name}: lse was written past [B, H, T]"
        for n, g in getattr(self, "g_bufs", {}).items():
            if n == "dqkv":
                R.assert_view_only_written(g, T, 0, 3 * d, f"{c.name}: {n}")
            else:
                R.assert_view_only_written(g, T if n == "dq" else self.inp["slot"], 0, d, f"{c.name}: {n}")


def _run_and_check(case, dtype):
    run = Run(case, dtype)
    outs = run.forward()
    if case.bwd:
        outs.update(run.backward())
    run.check_untouched()
    R.attn_check(case, dtype, outs)
    return run, outs


@pytest.mark.parametrize("dtype", DTYPES, ids=R.case_id)
@pytest.mark.parametrize("case", R.FWD_CASES, ids=R.case_id)
def test_attention_fwd_bwd(case, dtype):
    """attn_fwd_kernel<T, HD, false, false>, attn_split_merge_kernel, attn_bwd_dq_kernel / attn_dq_sum_kernel / attn_bwd_dkv_kernel
    <T, HD, false>."""
    run, outs = _run_and_check(case, dtype)
    # the kernels.py wrapper takes the same path: bit-equal output from contiguous-output calls
    o2, lse2 = K.attn_fwd(run.q, run.k, run.v, case.H, causal=case.causal, window=case.window, key_bias=run.bias, blk_lq=run.blk[0],
                          blk_lkv=run.blk[1])
    assert_bit_equal(o2, outs["o"], f"{case.name}: kernels.attn_fwd o")
    assert_bit_equal(lse2, outs["lse"], f"{case.name}: kernels.attn_fwd lse")
    if case.bias == "inf_row":
        # a batch row whose every key is masked with -inf: the kernel defines lse = -inf, O = 0 and zero gradients (torch's
        # softmax gives NaN there)
        b = case.B - 1
        assert bool((outs["lse"][b] == float("-inf")).all())
        for n in ("o", "dq", "dk", "dv"):
            assert bool((outs[n][b].float() == 0).all()), n


@pytest.mark.parametrize("dtype", DTYPES, ids=R.case_id)
@pytest.mark.parametrize("case", R.DROP_CASES, ids=R.case_id)
def test_attention_dropout_fwd_bwd(case, dtype):
    """The DROP = true instantiations of the three kernels; keep bits of the byte mask and of the words from one (p, seed)."""
    _run_and_check(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.case_id)
@pytest.mark.parametrize("case", R.DECODE_CASES, ids=R.case_id)
def test_decode_attention(case, dtype):
    """attn_fwd_kernel<T, HD, true, false> through omr_attn_fwd_split, with key_bias and lse."""
    _run_and_check(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.case_id)
@pytest.mark.parametrize("case", R.PARTIAL_CASES, ids=R.case_id)
def test_decode_attention_partials(case, dtype):
    """omr_attn_fwd_split_partials: the raw partials, merged here in fp64 as the header documents them."""
    run = Run(case, dtype)
    outs = run.forward()
    assert run.nsplit_out == case.nsplit
    B, H, T, hd = case.B, case.H, case.T, case.hd
    if case.nsplit > 1:
        assert _is_sentinel(run.o_buf), "o was written although the keys were split"
        assert _is_sentinel(run.lse_buf)
        part = run.ws[:run.ws_n].view(B, H, case.nsplit, T, hd + 2).cpu()
        o, lse = R.merge_partials(part, hd)                               # [B, H, T, hd], [B, H, T]
        outs = dict(o=o.permute(0, 2, 1, 3).reshape(B, T, H * hd), lse=lse)
        # the wrapper hands out the same partials
        p2, ns2 = K.attn_fwd_split_partials(run.q, run.k, run.v, H)
        assert ns2 == case.nsplit
        assert_bit_equal(p2.view(B, H, case.nsplit, T, hd + 2), part, "kernels.attn_fwd_split_partials")
    run.check_untouched()                                                 # operands; o and lse outside (nsplit > 1: all of) their views
    R.attn_check(case, dtype, outs)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.case_id)
@pytest.mark.parametrize("case", R.RAGGED_CASES, ids=R.case_id)
def test_ragged_decode_attention(case, dtype):
    """omr_attn_fwd_split_varlen / omr_attn_fwd_split_rows with key_bias: K / V rows outside a row's keys are NaN."""
    _run_and_check(case, dtype)


# ------------------------------------------------------------------------------------------------------------ refusals

def _refusal_args(dtype=F32, B=2, H=2, T=4, S=100, hd=32, pad=R.PAD, opad=R.PAD):
    d = H * hd
    q = torch.zeros((B, T, d + pad), dtype=dtype, device=DEV)[:, :, :d]
    k = torch.zeros((B, S, d + pad), dtype=dtype, device=DEV)[:, :, :d]
    o_buf = torch.full((B, T, d + opad), SENTINEL, dtype=dtype, device=DEV)
    o = o_buf[:, :, :d]
    lse = torch.full((B, H, T), SENTINEL, dtype=torch.float32, device=DEV)
    args = (dtype_code(dtype), ptr(q), ptr(k), ptr(k), ptr(o), ptr(lse), *_strides(q, k, k, o), B, H, T, S, hd)
    return args, (o_buf, lse), (q, k)


def _refused(match, name, args, outs):
    with pytest.raises(RuntimeError, match=match):
        lib().call(name, *args)
    torch.cuda.synchronize()
    for t in outs:
        assert _is_sentinel(t), f"{name}: an output was written by a refused call"


def test_attention_refusals():
    full = (0, -1, None, None, None, 0.0, 0, None)                      # causal, window, key_bias, blk_lq, blk_lkv, p, seed, words
    st = cur_stream()
    ws = torch.full((1 << 16,), SENTINEL, dtype=torch.float32, device=DEV)
    # hd = 48
    a, outs, _ = _refusal_args(hd=48)
    _refused("unsupported", "omr_attn_fwd", a + full + (st,), outs)
    # ldq % vec != 0 (bf16 rows of d + 4 elements: 8 bytes short of the 16-byte fragments); ldo % 4 != 0
    a, outs, _ = _refusal_args(dtype=BF16, pad=4)
    _refused("invalid argument", "omr_attn_fwd", a + full + (st,), outs)
    a, outs, _ = _refusal_args(opad=2)
    _refused("invalid argument", "omr_attn_fwd", a + full + (st,), outs)
    # dropout without the keep words
    a, outs, _ = _refusal_args()
    _refused("invalid argument", "omr_attn_fwd", a + (0, -1, None, None, None, 0.25, 7, None, st), outs)
    # T > 32 on every split entry
    a, outs, _ = _refusal_args(T=33, S=300)
    kv = torch.full((2,), 300, dtype=torch.int32, device=DEV)
    ns = ctypes.c_int(-7)
    _refused("invalid argument", "omr_attn_fwd_split", a + (None, ptr(ws), ws.numel(), st), outs)
    _refused("invalid argument", "omr_attn_fwd_split_partials", a + (ptr(ws), ws.numel(), ctypes.byref(ns), st), outs)
    _refused("invalid argument", "omr_attn_fwd_split_varlen", a + (None, ptr(kv), ptr(ws), ws.numel(), st), outs)
    _refused("invalid argument", "omr_attn_fwd_split_rows", a + (None, ptr(kv), ptr(kv), ptr(ws), ws.numel(), st), outs)
    assert ns.value == -7
    # kv_len with S <= 64 on the varlen entry
    a, outs, _ = _refusal_args(T=1, S=64)
    _refused("unsupported", "omr_attn_fwd_split_varlen", a + (None, ptr(kv), ptr(ws), ws.numel(), st), outs)
    # a workspace smaller than the plan: decode split (S = 700: 3 splits), query-per-wave split (T = 40, S = 1041: 2 splits)
    a, outs, _ = _refusal_args(T=1, S=700)
    need = lib().query("omr_attn_split_workspace_floats", 2, 2, 1, 700, 32)
    assert need == 2 * 2 * 3 * (32 + 2)
    _refused("invalid argument", "omr_attn_fwd_split", a + (None, ptr(ws), need - 1, st), outs)
    a, outs, _ = _refusal_args(T=40, S=1041)
    need = lib().query("omr_attn_workspace_floats", 2, 2, 40, 1041, 32, 0, 0)
    assert need == 2 * 2 * 40 * 2 * (32 + 2)
    _refused("invalid argument", "omr_attn_fwd_ws", a + full + (ptr(ws), need - 1, st), outs)
    assert _is_sentinel(ws)
    # the backward: lddo % vec != 0, and a dQ workspace smaller than the plan
    B, H, T, S, hd = 2, 2, 40, 1041, 32
    d = H * hd
    z = lambda rows, p=R.PAD: torch.zeros((B, rows, d + p), device=DEV)[:, :, :d]       # noqa: E731
    s = lambda rows: torch.full((B, rows, d), SENTINEL, device=DEV)                     # noqa: E731
    q, k, o, do_bad, do = z(T), z(S), z(T), z(T, 2), z(T)
    dq, dk, dv = s(T), s(S), s(S)
    lse, delta = torch.zeros((B, H, T), device=DEV), torch.full((B, H, T), SENTINEL, device=DEV)

    def bwd_args(dout, nws):
        return (0, ptr(q), ptr(k), ptr(k), ptr(o), ptr(dout), ptr(lse), ptr(delta), ptr(dq), ptr(dk), ptr(dv),
                *(t.stride(1) for t in (q, k, k, o, dout, dq, dk, dv)), *(t.stride(0) for t in (q, k, k, o, dout, dq, dk, dv)),
                B, H, T, S, hd, 0, -1, None, None, None, 0.0, 0, None, ptr(ws), nws, st)
    need = lib().query("omr_attn_workspace_floats", B, H, T, S, hd, 0, 1)
    assert need == 2 * B * T * d
    _refused("invalid argument", "omr_attn_bwd_ws", bwd_args(do_bad, need), (dq, dk, dv, delta))
    _refused("invalid argument", "omr_attn_bwd_ws", bwd_args(do, need - 1), (dq, dk, dv, delta))
    assert _is_sentinel(ws)
