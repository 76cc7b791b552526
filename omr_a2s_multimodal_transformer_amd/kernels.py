"""Host-side launchers: tensor-level wrappers over the C ABI (include/omr_hip.h) with shape checks.

No autograd here (see functional.py).  Layout conventions: encoder activations are NHWC tensors
[B,H,W,C]; 3x3 conv weights are given as their physical [COUT,3,3,CIN] view; token matrices are 2-D
row-major with unit inner stride (row stride may exceed the width).
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import torch

from ._lib import cur_stream, dtype_code, header_constant, lib, ptr, require_cuda

Tensor = torch.Tensor


def _rows2d(t: Tensor) -> Tuple[int, int, int]:
    assert t.dim() == 2 and t.stride(1) == 1, f"expected a row-major 2-D tensor, got shape {tuple(t.shape)} strides {t.stride()}"
    return t.shape[0], t.shape[1], t.stride(0)


def _omr_gemm(a: Tensor, b: Tensor, out: Tensor, M: int, N: int, K: int, trans_a, trans_b, bias, relu, accumulate, split_k, colsum_a, drop, group) -> Tensor:
    """The one spelling of the omr_gemm call and of the checks both wrappers share; `group` as gemm_row_groups takes it ((0, 0, 0, 0): off)."""
    require_cuda(a, b, bias, out, colsum_a)
    assert a.dtype == b.dtype
    lib().call("omr_gemm", dtype_code(a.dtype), dtype_code(out.dtype), int(trans_a), int(trans_b), M, N, K, ptr(a), a.stride(0), ptr(b), b.stride(0),
               ptr(out), out.stride(0), ptr(bias), int(relu), int(accumulate), split_k, ptr(colsum_a), float(drop[0]) if drop else 0.0,
               (int(drop[1]) & (2**64 - 1)) if drop else 0, *group, cur_stream())
    return out


def gemm(a: Tensor, b: Tensor, *, trans_a: bool = False, trans_b: bool = False, bias: Optional[Tensor] = None, relu: bool = False,
         out: Optional[Tensor] = None, out_dtype: Optional[torch.dtype] = None, accumulate: bool = False, split_k: int = 1,
         colsum_a: Optional[Tensor] = None, drop: Optional[Tuple[float, int]] = None) -> Tensor:
    """C[M,N] (+)= act(opA(a) @ opB(b)^T + bias).  a is [M,K] ([K,M] if trans_a); b is [N,K] ([K,N] if trans_b)."""
    ar, ac, _ = _rows2d(a)
    br, bc, _ = _rows2d(b)
    M, K = (ac, ar) if trans_a else (ar, ac)
    N, Kb = (bc, br) if trans_b else (br, bc)
    assert K == Kb, f"gemm inner dims differ: {K} vs {Kb}"
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype or a.dtype, device=a.device)
        assert not accumulate and split_k == 1, "accumulating gemm needs an initialised `out`"
    assert _rows2d(out)[:2] == (M, N), f"gemm out shape {tuple(out.shape)} != {(M, N)}"
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == N and bias.is_contiguous()
    if colsum_a is not None:
        assert trans_a and colsum_a.dtype == torch.float32 and colsum_a.numel() == M and colsum_a.is_contiguous()
    return _omr_gemm(a, b, out, M, N, K, trans_a, trans_b, bias, relu, accumulate, split_k, colsum_a, drop, (0, 0, 0, 0))


def gemm_row_groups(a: Tensor, b: Tensor, out: Tensor, M: int, N: int, Kd: int, *, trans_a: bool = False, trans_b: bool = False,
                    bias: Optional[Tensor] = None, accumulate: bool = False, split_k: int = 1, colsum_a: Optional[Tensor] = None,
                    group: Tuple[int, int, int, int] = (0, 0, 0, 0)) -> Tensor:
    """omr_gemm over a row-group view of the weight-side operand (include/omr_hip.h): `group` = (rows per group, physical
    group stride, first row inside a group, operand 1|2|3).  The grouped tensor (b, or out/colsum_a/bias) is the PHYSICAL
    2-D block that contains every group; M, N, Kd are the logical GEMM sizes, so only strides are taken from the tensors."""
    assert a.dim() == b.dim() == out.dim() == 2 and a.stride(1) == b.stride(1) == out.stride(1) == 1
    grp, stride, base, operand = group
    ngroups = {1: N, 2: Kd, 3: M}[operand] // grp
    phys_rows = (ngroups - 1) * stride + base + grp
    grouped = out if operand == 3 else b
    assert grouped.shape[0] >= phys_rows, f"grouped operand has {grouped.shape[0]} rows, the view needs {phys_rows}"
    for vec, need in ((bias, operand == 1), (colsum_a, operand == 3)):
        if vec is not None:
            assert vec.dtype == torch.float32 and vec.is_contiguous() and vec.numel() >= (phys_rows if need else 0)
    return _omr_gemm(a, b, out, M, N, Kd, trans_a, trans_b, bias, False, accumulate, split_k, colsum_a, None, group)


class _DwProblem(ctypes.Structure):
    """omr_dw_problem of include/omr_hip.h."""
    _fields_ = [("dy", ctypes.c_void_p), ("x", ctypes.c_void_p), ("dw", ctypes.c_void_p), ("db", ctypes.c_void_p),
                ("rows", ctypes.c_int), ("n_out", ctypes.c_int), ("n_in", ctypes.c_int), ("row_group", ctypes.c_int),
                ("ld_dy", ctypes.c_long), ("ld_x", ctypes.c_long), ("ld_dw", ctypes.c_long),
                ("row_group_stride", ctypes.c_int), ("row_group_base", ctypes.c_int)]


class _DecodeLinearArgs(ctypes.Structure):
    """omr_decode_linear_args of include/omr_hip.h."""
    _fields_ = [(n, ctypes.c_int) for n in ("dtype", "pro", "M", "N", "K", "relu", "n0", "nsplit", "H", "hd", "vocab", "pad_")] + \
               [("eps", ctypes.c_float), ("pad2_", ctypes.c_float),
                ("x", ctypes.c_void_p), ("ldx", ctypes.c_long), ("res", ctypes.c_void_p), ("ldres", ctypes.c_long),
                ("gamma", ctypes.c_void_p), ("beta", ctypes.c_void_p), ("xn_out", ctypes.c_void_p),
                ("tokens", ctypes.c_void_p), ("emb", ctypes.c_void_p), ("pe_row", ctypes.c_void_p), ("part", ctypes.c_void_p),
                ("w", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("out0", ctypes.c_void_p), ("ld0", ctypes.c_long),
                ("out1", ctypes.c_void_p), ("ld1", ctypes.c_long), ("out32", ctypes.c_void_p), ("ld32", ctypes.c_long),
                ("amax_idx", ctypes.c_void_p), ("amax_val", ctypes.c_void_p), ("amax_part", ctypes.c_void_p),
                ("w8", ctypes.c_void_p), ("w8_scale", ctypes.c_void_p)]


def _view_ptr(t: Tensor) -> int:
    """Address of a view's first element, also where the view is empty (data_ptr() of a tensor without elements is NULL)."""
    return t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()


def decode_linear(w: Optional[Tensor], bias: Optional[Tensor], *, x: Optional[Tensor] = None, res: Optional[Tensor] = None, ln=None,
                  tokens: Optional[Tensor] = None, emb: Optional[Tensor] = None, pe_row: Optional[Tensor] = None, part: Optional[Tensor] = None,
                  heads: int = 0, relu: bool = False, n0: Optional[int] = None, want32: bool = False, want_argmax: bool = False,
                  w8: Optional[Tensor] = None, w8_scale: Optional[Tensor] = None, dtype: Optional[torch.dtype] = None,
                  out0: Optional[Tensor] = None, out1: Optional[Tensor] = None, out32: Optional[Tensor] = None, built: Optional[Tensor] = None,
                  row_pos: Optional[Tensor] = None, out1_pos_ld: int = 0):
    """One linear of a decode position with the preceding element-wise step folded into its input rows (omr_decode_linear):
    x alone -> plain rows; x + res + ln=(gamma, beta, eps) -> LayerNorm(x + res); tokens + emb + pe_row -> embedding row + pe;
    part [M*heads, nsplit, hd+2] + heads -> merged key-split attention.  Returns (out0 [M, n0], out1 [M, N-n0] or None,
    built rows [M, K] or None, fp32 copy or None) and, with want_argmax, (first index of the row maximum int64 [M], its value fp32 [M]).
    w8 (uint8 e4m3 codes [N, K]) + w8_scale (fp32 [N]) replace `w`; `dtype` then names the row type (w may be None).
    out0 / out1 / out32 (row-major 2-D views, unit inner stride; their row strides become ld0 / ld1 / ld32) and built
    (contiguous [M, K]) are written in place of fresh tensors.  row_pos (int32 [M]) selects omr_decode_linear_rows: pe_row is
    then the whole table [positions, K] and row m's out1 part lands row_pos[m] * out1_pos_ld elements further."""
    require_cuda(w, bias, x, res, tokens, emb, pe_row, part, w8, w8_scale, out0, out1, out32, built, row_pos)
    if w8 is not None:
        assert w8.dtype == torch.uint8 and w8.dim() == 2 and w8.is_contiguous() and w8_scale is not None
        assert w8_scale.dtype == torch.float32 and w8_scale.is_contiguous() and w8_scale.numel() == w8.shape[0]
        N, K = w8.shape
        assert dtype is not None or w is not None, "with w8, name the row type with `dtype` (or pass a `w` of that type)"
        dt = dtype if dtype is not None else w.dtype
    else:
        N, K = w.shape
        dt = w.dtype
        assert dtype is None or dtype == dt
    dev = w8.device if w8 is not None else w.device
    a = _DecodeLinearArgs()
    if built is not None:
        assert built.dtype == dt and built.is_contiguous() and built.shape[1] == K
    if part is not None:
        pro, M = 3, part.shape[0] // heads
        assert part.dtype == torch.float32 and part.is_contiguous() and part.shape[2] - 2 == K // heads
        a.part, a.nsplit, a.H, a.hd = part.data_ptr(), part.shape[1], heads, K // heads
    elif tokens is not None:
        pro, M = 2, tokens.numel()
        assert tokens.dtype == torch.int64 and emb.dtype == dt and emb.is_contiguous() and pe_row.dtype == torch.float32 and pe_row.is_contiguous()
        assert pe_row.numel() == K if row_pos is None else (pe_row.dim() == 2 and pe_row.shape[1] == K)
        built = torch.empty((M, K), dtype=dt, device=dev) if built is None else built
        a.tokens, a.emb, a.pe_row, a.vocab, a.xn_out = tokens.data_ptr(), emb.data_ptr(), pe_row.data_ptr(), emb.shape[0], built.data_ptr()
    elif ln is not None:
        pro, M = 1, x.shape[0]
        gamma, beta, eps = ln
        assert x.dtype == res.dtype == dt and x.stride(1) == res.stride(1) == 1 and gamma.dtype == beta.dtype == torch.float32
        built = torch.empty((M, K), dtype=dt, device=dev) if built is None else built
        a.x, a.ldx, a.res, a.ldres, a.gamma, a.beta, a.eps, a.xn_out = x.data_ptr(), x.stride(0), res.data_ptr(), res.stride(0), gamma.data_ptr(), beta.data_ptr(), eps, built.data_ptr()
    else:
        pro, M = 0, x.shape[0]
        assert x.dtype == dt and x.stride(1) == 1 and x.shape[1] == K
        a.x, a.ldx = x.data_ptr(), x.stride(0)
    assert built is None or built.shape[0] == M
    n0 = N if n0 is None else n0
    if out0 is None:
        out0 = torch.empty((M, max(n0, 1)), dtype=dt, device=dev)[:, :n0]      # n0 = 0: the entry still wants a pointer
    if out1 is None and n0 < N:
        out1 = torch.empty((M, N - n0), dtype=dt, device=dev)
    if out32 is None and want32:
        out32 = torch.empty((M, N), dtype=torch.float32, device=dev)
    for t, cols, tdt in ((out0, n0, dt), (out1 if n0 < N else None, N - n0, dt), (out32, N, torch.float32)):
        assert t is None or (t.dtype == tdt and t.dim() == 2 and tuple(t.shape) == (M, cols) and (t.stride(1) == 1 or cols <= 1)), "output view"
    assert (w is None or w.is_contiguous()) and (bias is None or (bias.dtype == torch.float32 and bias.numel() == N))
    a.dtype, a.pro, a.M, a.N, a.K, a.relu, a.n0 = dtype_code(dt), pro, M, N, K, int(relu), n0
    a.w, a.bias, a.out0, a.ld0 = (w.data_ptr() if w is not None else None), (bias.data_ptr() if bias is not None else None), _view_ptr(out0), out0.stride(0)
    if w8 is not None:
        a.w8, a.w8_scale = w8.data_ptr(), w8_scale.data_ptr()
    if n0 < N:
        a.out1, a.ld1 = _view_ptr(out1), out1.stride(0)
    else:
        out1 = None
    if out32 is not None:
        a.out32, a.ld32 = _view_ptr(out32), out32.stride(0)
    amax = None
    if want_argmax:
        idx = torch.empty(M, dtype=torch.int64, device=dev)
        val = torch.empty(M, dtype=torch.float32, device=dev)
        part = torch.empty(2 * M * ((N + 15) // 16), dtype=torch.float32, device=dev)
        a.amax_idx, a.amax_val, a.amax_part = idx.data_ptr(), val.data_ptr(), part.data_ptr()
        amax = (idx, val)
    if row_pos is not None:
        assert row_pos.dtype == torch.int32 and row_pos.is_contiguous() and row_pos.numel() == M
        lib().call("omr_decode_linear_rows", ctypes.byref(a), row_pos.data_ptr(), int(out1_pos_ld), cur_stream())
    else:
        lib().call("omr_decode_linear", ctypes.byref(a), cur_stream())
    return (out0, out1, built, out32) if amax is None else (out0, out1, built, out32, amax)


def linear_wgrad_grouped(problems) -> None:
    """Weight / bias gradients of several linear layers in ONE launch (omr_linear_wgrad_grouped).  problems: sequence of
    (dy [rows, n_out], x [rows, n_in], dw fp32 [n_out(+), n_in] accumulated in place, db fp32 or None, group) with
    group = None or (rows per group, physical group stride, first row inside a group) for a row-group view of dw / db."""
    if not problems:
        return
    arr = (_DwProblem * len(problems))()
    dt = problems[0][0].dtype
    for q, (dy, x, dw, db, group) in zip(arr, problems):
        require_cuda(dy, x, dw, db)
        assert dy.dtype == x.dtype == dt and dw.dtype == torch.float32 and dy.dim() == x.dim() == dw.dim() == 2
        assert dy.stride(1) == x.stride(1) == dw.stride(1) == 1 and dy.shape[0] == x.shape[0]
        rows, n_out = dy.shape
        n_in = x.shape[1]
        grp, gstride, gbase = group if group is not None else (0, 0, 0)
        phys_rows = n_out if not grp else (n_out // grp - 1) * gstride + gbase + grp
        assert dw.shape[1] == n_in and dw.shape[0] >= phys_rows, (tuple(dw.shape), n_out, n_in)
        if db is not None:
            assert db.dtype == torch.float32 and db.is_contiguous() and db.numel() >= phys_rows
        q.dy, q.x, q.dw, q.db = dy.data_ptr(), x.data_ptr(), dw.data_ptr(), (db.data_ptr() if db is not None else None)
        q.rows, q.n_out, q.n_in, q.row_group = rows, n_out, n_in, grp
        q.ld_dy, q.ld_x, q.ld_dw, q.row_group_stride, q.row_group_base = dy.stride(0), x.stride(0), dw.stride(0), gstride, gbase
    lib().call("omr_linear_wgrad_grouped", dtype_code(dt), len(problems), ctypes.byref(arr), cur_stream())


def quantize_rows_fp8(x: Tensor) -> Tuple[Tensor, Tensor]:
    """x [M, K] (fp32 / bf16, unit inner stride) -> (OCP e4m3 codes uint8 [M, K], fp32 scale per row [M]): x ~ codes * scale."""
    require_cuda(x)
    M, K, ld = _rows2d(x)
    q = torch.empty((M, (K + 15) // 16 * 16), dtype=torch.uint8, device=x.device)
    if q.shape[1] != K:
        q.zero_()                                # padded k columns must read as fp8 zeros
    scale = torch.empty(M, dtype=torch.float32, device=x.device)
    lib().call("omr_quantize_rows_fp8", dtype_code(x.dtype), ptr(x), ld, ptr(q), q.stride(0), ptr(scale), M, K, cur_stream())
    return q, scale


def gemm_fp8(a8: Tensor, scale_a: Tensor, w8: Tensor, scale_w: Tensor, bias: Optional[Tensor] = None, relu: bool = False,
             out_dtype: torch.dtype = torch.bfloat16, out: Optional[Tensor] = None) -> Tensor:
    """C[M, N] = (a8 . w8^T) * scale_a[m] * scale_w[n] + bias on the fp8 MFMA (a8 [M, K], w8 [N, K]: quantize_rows_fp8 outputs)."""
    require_cuda(a8, w8, scale_a, scale_w, bias, out)
    assert a8.dtype == w8.dtype == torch.uint8 and a8.shape[1] == w8.shape[1] and a8.stride(1) == w8.stride(1) == 1
    M, K = a8.shape
    N = w8.shape[0]
    assert scale_a.numel() == M and scale_w.numel() == N and scale_a.dtype == scale_w.dtype == torch.float32
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a8.device)
    assert tuple(out.shape) == (M, N) and out.stride(1) == 1
    lib().call("omr_gemm_fp8", dtype_code(out.dtype), M, N, K, ptr(a8), a8.stride(0), ptr(scale_a), ptr(w8), w8.stride(0), ptr(scale_w), ptr(out),
               out.stride(0), ptr(bias), int(relu), cur_stream())
    return out


def cast(x: Tensor, dtype: torch.dtype, out: Optional[Tensor] = None) -> Tensor:
    require_cuda(x)
    assert x.is_contiguous()
    if out is None:
        out = torch.empty_like(x, dtype=dtype)
    lib().call("omr_cast", ptr(x), dtype_code(x.dtype), ptr(out), dtype_code(dtype), x.numel(), cur_stream())
    return out


def add(a: Tensor, b: Tensor, out: Optional[Tensor] = None) -> Tensor:
    require_cuda(a, b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous() and b.is_contiguous()
    if out is None:
        out = torch.empty_like(a)
    lib().call("omr_add", dtype_code(a.dtype), ptr(a), ptr(b), ptr(out), a.numel(), cur_stream())
    return out


def relu_bwd(dy: Tensor, y: Tensor, scale: float = 1.0) -> Tensor:
    require_cuda(dy, y)
    assert dy.shape == y.shape and dy.dtype == y.dtype and dy.is_contiguous() and y.is_contiguous()
    dx = torch.empty_like(dy)
    lib().call("omr_relu_bwd", dtype_code(dy.dtype), ptr(dy), ptr(y), ptr(dx), dy.numel(), float(scale), cur_stream())
    return dx


def dropout(x: Tensor, p: float, seed: int, channel_mode: bool = False) -> Tensor:
    """Elementwise dropout, or per-(sample, channel) dropout of an NHWC tensor when channel_mode."""
    require_cuda(x)
    assert x.is_contiguous()
    out = torch.empty_like(x)
    per_sample = x.numel() // x.shape[0]
    lib().call("omr_dropout", dtype_code(x.dtype), ptr(x), ptr(out), x.numel(), float(p), int(seed) & (2**64 - 1), int(channel_mode),
               per_sample, x.shape[-1], cur_stream())
    return out


def embed_pe(tokens: Tensor, table: Tensor, pe: Tensor) -> Tensor:
    """tokens int64 [B,T]; table [V,d]; pe fp32 [>=T, d] -> [B,T,d]."""
    require_cuda(tokens, table, pe)
    assert tokens.dtype == torch.int64 and tokens.is_contiguous() and table.is_contiguous()
    B, T = tokens.shape
    V, d = table.shape
    assert pe.dtype == torch.float32 and pe.is_contiguous() and pe.shape[-1] == d and pe.shape[-2] >= T, "sequence longer than the PE table"
    out = torch.empty((B, T, d), dtype=table.dtype, device=table.device)
    lib().call("omr_embed_pe_fwd", dtype_code(table.dtype), ptr(tokens), ptr(table), ptr(pe), ptr(out), B * T, T, d, V, cur_stream())
    return out


def embed_bwd(tokens: Tensor, dout: Tensor, dtable: Tensor, pad_idx: int) -> None:
    require_cuda(tokens, dout, dtable)
    assert dtable.dtype == torch.float32 and dout.is_contiguous()
    V, d = dtable.shape
    lib().call("omr_embed_bwd", dtype_code(dout.dtype), ptr(tokens), ptr(dout), ptr(dtable), tokens.numel(), d, pad_idx, V, cur_stream())


def add_pe2d(x: Tensor, pe_hwc: Tensor) -> Tensor:
    """x NHWC [B,h,w,C] + pe_hwc fp32 [maxh,maxw,C][:h,:w]."""
    require_cuda(x, pe_hwc)
    B, h, w, C = x.shape
    maxh, maxw, Cp = pe_hwc.shape
    assert Cp == C and pe_hwc.dtype == torch.float32 and pe_hwc.is_contiguous() and x.is_contiguous()
    assert h <= maxh and w <= maxw, f"feature map {h}x{w} exceeds the positional-encoding table {maxh}x{maxw}"
    out = torch.empty_like(x)
    lib().call("omr_add_pe2d", dtype_code(x.dtype), ptr(x), ptr(pe_hwc), ptr(out), B, h, w, C, maxh, maxw, cur_stream())
    return out


def colsum_into(dy2d: Tensor, db: Tensor) -> None:
    """db[n] += sum_m dy2d[m, n]  (db fp32)."""
    require_cuda(dy2d, db)
    M, N, ld = _rows2d(dy2d)
    assert db.dtype == torch.float32 and db.numel() == N
    lib().call("omr_colsum", dtype_code(dy2d.dtype), ptr(dy2d), ptr(db), M, N, ld, cur_stream())


class StepCtl(ctypes.Structure):
    """omr_step_ctl of include/omr_hip.h: the device-resident record of the guarded optimizer step."""
    _fields_ = [("sumsq", ctypes.c_double), ("norm", ctypes.c_float), ("clip", ctypes.c_float), ("apply", ctypes.c_int),
                ("nonfinite", ctypes.c_int), ("range_sumsq", ctypes.c_double * 16)]


GRAD_NORM_K = header_constant("OMR_GRAD_NORM_K")              # elements a thread adds in fp32: the norm's error is <= (K / 2 + 2) 2^-24
GRAD_NORM_CHUNK = header_constant("OMR_GRAD_NORM_CHUNK")      # elements per slot of the reduction
GRAD_NORM_MAX_RANGES = header_constant("OMR_GRAD_NORM_MAX_RANGES")


def grad_norm_workspace_bytes(n: int, n_ranges: int) -> int:
    nbytes = lib().query("omr_grad_norm_workspace_bytes", n, n_ranges)
    if nbytes < 0:
        raise RuntimeError(f"libomr_hip: omr_grad_norm_workspace_bytes refused n = {n}, n_ranges = {n_ranges}")
    return nbytes


def new_step_ctl(device) -> Tensor:
    """One omr_step_ctl in device memory (as bytes; read_step_ctl decodes a host copy)."""
    return torch.zeros(ctypes.sizeof(StepCtl), dtype=torch.uint8, device=device)


def read_step_ctl(host_bytes: Tensor) -> StepCtl:
    """Decode a HOST copy of the record (a uint8 tensor of sizeof(omr_step_ctl) bytes whose copy has completed)."""
    assert not host_bytes.is_cuda and host_bytes.dtype == torch.uint8 and host_bytes.numel() == ctypes.sizeof(StepCtl)
    return StepCtl.from_buffer_copy(host_bytes.numpy().tobytes())


def grad_norm(g: Tensor, ranges, grad_scale: float, max_norm: Optional[float], ws: Tensor, ctl: Tensor) -> None:
    """Global L2 norm of g over the element ranges [(begin, end), ...] (sorted, disjoint, begins multiples of 4; at most 16), the
    clip factor for max_norm (None / <= 0 / inf: no clipping) and the apply / skip decision, into the record `ctl` -- two
    launches, nothing is read back (omr_grad_norm)."""
    require_cuda(g, ws, ctl)
    assert g.dtype == torch.float32 and g.is_contiguous()
    nr = len(ranges)
    assert ctl.numel() * ctl.element_size() == ctypes.sizeof(StepCtl)
    assert 1 <= nr <= GRAD_NORM_MAX_RANGES and ws.numel() * ws.element_size() >= grad_norm_workspace_bytes(g.numel(), nr)
    begins = (ctypes.c_long * nr)(*[b for b, _ in ranges])
    ends = (ctypes.c_long * nr)(*[e for _, e in ranges])
    lib().call("omr_grad_norm", ptr(g), g.numel(), begins, ends, nr, grad_scale, 0.0 if max_norm is None else max_norm, ptr(ws), ptr(ctl),
               cur_stream())


DECAY_BLOCK = header_constant("OMR_ADAM_DECAY_BLOCK")        # elements per byte of decay_blocks; divides params.ALIGN


def adam_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
              grad_scale: float = 1.0, p_lowp: Optional[Tensor] = None, *, weight_decay: float = 0.0, decay_blocks: Optional[Tensor] = None,
              ema: Optional[Tensor] = None, ema_decay: float = 0.0, ctl: Optional[Tensor] = None) -> None:
    """The optimizer step, one launch (omr_adamw_ema): torch.optim.Adam; with weight_decay, decoupled weight decay in front (AdamW);
    with ema, the moving average of the new weights behind; with ctl, behind the record grad_norm filled -- no write at all when it
    says skip, else g * grad_scale * clip.  decay_blocks: uint8, one byte per DECAY_BLOCK elements counted from p[0] (None: every
    element decays); ema: fp32 like p (None: no average).  p, g, m, v, p_lowp and ema start on 16-byte boundaries."""
    require_cuda(p, g, m, v, p_lowp, decay_blocks, ema, ctl)
    n = p.numel()
    for t in (p, g, m, v):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
    pp, pg, pm, pv, plp, pe = ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_lowp), ptr(ema)
    if p_lowp is not None:
        assert p_lowp.dtype == torch.bfloat16 and p_lowp.numel() == n
    if ema is not None:
        assert ema.dtype == torch.float32 and ema.is_contiguous() and ema.numel() == n
    if (pp | pg | pm | pv | (plp or 0) | (pe or 0)) & 15:
        raise RuntimeError("adam_step: invalid argument: p, g, m, v, p_lowp and ema must start on 16-byte boundaries (the kernel moves "
                           "16-byte vectors); slices of the flat buffers that begin on a multiple of params.ALIGN do")
    if decay_blocks is not None:
        assert decay_blocks.dtype == torch.uint8 and decay_blocks.is_contiguous() and decay_blocks.numel() >= (n + DECAY_BLOCK - 1) // DECAY_BLOCK
    if ctl is not None:
        assert ctl.numel() * ctl.element_size() == ctypes.sizeof(StepCtl)
    lib().call("omr_adamw_ema", pp, pg, pm, pv, plp, pe, ptr(decay_blocks), n, step, lr, betas[0], betas[1], eps, weight_decay, ema_decay,
               grad_scale, ptr(ctl), cur_stream())


def swap_f32(a: Tensor, b: Tensor) -> None:
    """Exchange the contents of two fp32 tensors in place (omr_swap_f32); overlapping tensors are refused."""
    require_cuda(a, b)
    assert a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel()
    lib().call("omr_swap_f32", ptr(a), ptr(b), a.numel(), cur_stream())


def argmax(x: Tensor) -> Tuple[Tensor, Tensor]:
    """x fp32 [n] or [rows, n] (unit inner stride) -> (indices int64 [rows], top-1 values fp32 [rows])."""
    require_cuda(x)
    assert x.dtype == torch.float32 and x.dim() in (1, 2) and x.stride(-1) == 1
    rows, n, ld = (1, x.numel(), x.numel()) if x.dim() == 1 else (x.shape[0], x.shape[1], x.stride(0))
    idx = torch.empty(rows, dtype=torch.int64, device=x.device)
    val = torch.empty(rows, dtype=torch.float32, device=x.device)
    lib().call("omr_argmax", ptr(x), rows, n, ld, ptr(idx), ptr(val), cur_stream())
    return idx, val


def weighted_argmax(la: Tensor, lb: Tensor, alpha: float) -> Tuple[Tensor, Tensor]:
    """argmax(alpha * softmax(la) + (1 - alpha) * softmax(lb)) of two fp32 logit rows [n] -> (index int64 [1], probability fp32 [1])."""
    require_cuda(la, lb)
    assert la.dtype == lb.dtype == torch.float32 and la.dim() == lb.dim() == 1 and la.numel() == lb.numel() and la.is_contiguous() and lb.is_contiguous()
    idx = torch.empty(1, dtype=torch.int64, device=la.device)
    prob = torch.empty(1, dtype=torch.float32, device=la.device)
    lib().call("omr_weighted_argmax", ptr(la), ptr(lb), la.numel(), float(alpha), ptr(idx), ptr(prob), cur_stream())
    return idx, prob


def weighted_argmax_rows(la: Tensor, lb: Tensor, alpha: float, n: Optional[int] = None,
                         tokens_out: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """weighted_argmax row by row in one launch: fp32 [rows, >= n] logits (row strides free, unit column stride; n defaults to
    the narrower width) -> (indices int64 [rows], probabilities fp32 [rows]); tokens_out (int64 [rows]) gets the indices too."""
    require_cuda(la, lb, tokens_out)
    assert la.dtype == lb.dtype == torch.float32 and la.dim() == lb.dim() == 2 and la.shape[0] == lb.shape[0]
    rows = la.shape[0]
    n = min(la.shape[1], lb.shape[1]) if n is None else n
    assert n <= min(la.shape[1], lb.shape[1]) and (la.stride(1) == 1 and lb.stride(1) == 1 or n == 1)
    assert tokens_out is None or (tokens_out.dtype == torch.int64 and tokens_out.numel() == rows and tokens_out.is_contiguous())
    idx = torch.empty(rows, dtype=torch.int64, device=la.device)
    prob = torch.empty(rows, dtype=torch.float32, device=la.device)
    lib().call("omr_weighted_argmax_rows", ptr(la), la.stride(0), ptr(lb), lb.stride(0), rows, n, float(alpha), ptr(idx), ptr(prob), ptr(tokens_out),
               cur_stream())
    return idx, prob


def weighted_topk_logprob(la: Tensor, lb: Tensor, alpha: float, k: int, n: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """The k best tokens of alpha * softmax(la) + (1 - alpha) * softmax(lb) row by row (weighted_argmax_rows' arithmetic; beam
    search over the weighted fusion, an extension: the reference decodes greedily): fp32 [rows, >= n] logits (row strides free,
    unit column stride; n defaults to the narrower width) -> (token ids int64 [rows, k], log of the mixed probability fp32
    [rows, k]), best first, ties towards the smaller id."""
    require_cuda(la, lb)
    assert la.dtype == lb.dtype == torch.float32 and la.dim() == lb.dim() == 2 and la.shape[0] == lb.shape[0]
    rows = la.shape[0]
    n = min(la.shape[1], lb.shape[1]) if n is None else n
    assert n <= min(la.shape[1], lb.shape[1]) and (la.stride(1) == 1 and lb.stride(1) == 1 or n == 1)
    idx = torch.empty((rows, k), dtype=torch.int64, device=la.device)
    val = torch.empty((rows, k), dtype=torch.float32, device=la.device)
    lib().call("omr_weighted_topk_logprob", ptr(la), la.stride(0), ptr(lb), lb.stride(0), rows, n, float(alpha), k, ptr(idx), ptr(val), cur_stream())
    return idx, val


def topk_logprob(x: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """x fp32 [rows, n] -> (token ids int64 [rows, k], log-probabilities fp32 [rows, k]), best first."""
    require_cuda(x)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and 0 < k <= x.shape[1]
    idx = torch.empty((x.shape[0], k), dtype=torch.int64, device=x.device)
    val = torch.empty((x.shape[0], k), dtype=torch.float32, device=x.device)
    lib().call("omr_topk_logprob", ptr(x), x.shape[0], x.shape[1], x.stride(0), k, ptr(idx), ptr(val), cur_stream())
    return idx, val


# ------------------------------------------------------------------------------------------------ normalisation

def slot_workspace(slot_query: str, B: int, C: int, device, *dims: int) -> Tuple[Tensor, int]:
    """(fp64 statistics workspace, slots per image) of the InstanceNorm slot protocol: partial slots [B][slots][C][2] +
    compact sums [B][C][2].  The library owns both numbers: slots = slot_query(B, *dims) (a value < 1 is its error code), the size is
    omr_instnorm_workspace_bytes.  Uninitialised: the producer launch writes every slot."""
    slots = lib().query(slot_query, B, *dims)
    assert slots >= 1, f"{slot_query}{(B,) + dims} failed: {slots}"
    return torch.empty(slot_workspace_elems(B, C, slots), dtype=torch.float64, device=device), slots


def slot_workspace_elems(B: int, C: int, slots: int) -> int:
    """fp64 elements of a statistics workspace with `slots` slots per image (compact sums included)."""
    return lib().query("omr_instnorm_workspace_bytes", B, C, slots) // 8


def conv_stat_ws(B: int, Ho: int, Wo: int, C: int, device) -> Tuple[Tensor, int]:
    """Workspace + slot count for a conv launch with a fused statistics epilogue (stat_mode 1 / 2)."""
    return slot_workspace("omr_conv3x3_stat_slots", B, C, device, Ho, Wo)


def instnorm_stats(x: Tensor, eps: float = 1e-3) -> Tuple[Tensor, Tensor]:
    """x NHWC -> (mean, rstd) fp32 [B,C]."""
    require_cuda(x)
    B, H, W, C = x.shape
    assert x.is_contiguous()
    mean = torch.empty((B, C), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    ws, _ = slot_workspace("omr_instnorm_slots", B, C, x.device, H * W)
    lib().call("omr_instnorm_stats", dtype_code(x.dtype), ptr(x), ptr(mean), ptr(rstd), B, H * W, C, eps, ptr(ws), cur_stream())
    return mean, rstd


def instnorm_finalize(ws: Tensor, slots: int, B: int, C: int, HW: int, eps: float = 1e-3) -> Tuple[Tensor, Tensor]:
    """fp64 {sum, sum of squares} slots (conv_stat_ws layout) -> (mean, rstd) fp32 [B,C]."""
    require_cuda(ws)
    mean = torch.empty((B, C), dtype=torch.float32, device=ws.device)
    rstd = torch.empty_like(mean)
    lib().call("omr_instnorm_finalize", ptr(ws), slots, ptr(mean), ptr(rstd), B, HW, C, eps, cur_stream())
    return mean, rstd


def instnorm_bwd_apply(dxhat: Tensor, x: Tensor, mean: Tensor, rstd: Tensor, ws: Tensor, slots: int, relu_mask: bool, relu_scale: float = 1.0) -> Tensor:
    """InstanceNorm backward apply step with the {sum g, sum g*xhat} sums already in the slots of ws (conv_stat_ws layout)."""
    require_cuda(dxhat, x, ws)
    B, H, W, C = x.shape
    assert dxhat.shape == x.shape and dxhat.is_contiguous() and x.is_contiguous() and ws.dtype == torch.float64
    dx = torch.empty_like(x)
    lib().call("omr_instnorm_bwd_apply", dtype_code(x.dtype), ptr(dxhat), ptr(x), ptr(mean), ptr(rstd), ptr(dx), B, H * W, C, int(relu_mask),
               float(relu_scale), ptr(ws), slots, cur_stream())
    return dx


def instnorm_bwd(dxhat: Tensor, x: Tensor, mean: Tensor, rstd: Tensor, relu_mask: bool, relu_scale: float = 1.0) -> Tensor:
    require_cuda(dxhat, x)
    B, H, W, C = x.shape
    assert dxhat.shape == x.shape and dxhat.is_contiguous() and x.is_contiguous()
    dx = torch.empty_like(x)
    ws, _ = slot_workspace("omr_instnorm_slots", B, C, x.device, H * W)
    lib().call("omr_instnorm_bwd", dtype_code(x.dtype), ptr(dxhat), ptr(x), ptr(mean), ptr(rstd), ptr(dx), B, H * W, C, int(relu_mask),
               float(relu_scale), ptr(ws), cur_stream())
    return dx


# ------------------------------------------------------------------------------------------------ ragged batches (csrc/extent.hip)

def _check_extents(x: Tensor, ext: Tensor) -> Tuple[int, int, int, int]:
    """x NHWC, ext int32 [B, 2] on x's device = (rows, columns) of each sample's content in the top-left corner of its plane."""
    require_cuda(x, ext)
    assert x.dim() == 4 and x.is_contiguous(), f"expected a contiguous NHWC tensor, got shape {tuple(x.shape)} strides {x.stride()}"
    assert ext.dtype == torch.int32 and ext.is_contiguous() and tuple(ext.shape) == (x.shape[0], 2) and ext.device == x.device, \
        f"extents must be int32 [B, 2] on the device of x, got {ext.dtype} {tuple(ext.shape)} on {ext.device}"
    return tuple(x.shape)


def extent_zero(x: Tensor, ext: Tensor) -> Tensor:
    """x[b, i, j, :] = 0 for i >= ext[b, 0] or j >= ext[b, 1], IN PLACE (returns x).  Stores to the outside only."""
    B, H, W, C = _check_extents(x, ext)
    lib().call("omr_extent_zero", dtype_code(x.dtype), ptr(x), ptr(ext), B, H, W, C, cur_stream())
    return x


def instnorm_extent_fwd(x: Tensor, ext: Tensor, eps: float = 1e-3) -> Tuple[Tensor, Tensor, Tensor]:
    """InstanceNorm over each sample's extent: -> (y = (x - mean) * rstd inside / 0 outside, mean [B, C], rstd [B, C])."""
    B, H, W, C = _check_extents(x, ext)
    y = torch.empty_like(x)
    mean = torch.empty((B, C), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    ws, _ = slot_workspace("omr_instnorm_extent_slots", B, C, x.device, H * W)
    lib().call("omr_instnorm_extent_fwd", dtype_code(x.dtype), ptr(x), ptr(ext), ptr(y), ptr(mean), ptr(rstd), B, H, W, C, eps, ptr(ws), cur_stream())
    return y, mean, rstd


def instnorm_extent_bwd(dxhat: Tensor, x: Tensor, mean: Tensor, rstd: Tensor, ext: Tensor, relu_mask: bool = False, relu_scale: float = 1.0) -> Tensor:
    """Backward of instnorm_extent_fwd (dxhat = gradient of y; its values outside the extents are not read); optionally times
    (x > 0) * relu_scale, the activation backward of the producer of x."""
    B, H, W, C = _check_extents(x, ext)
    assert dxhat.shape == x.shape and dxhat.dtype == x.dtype and dxhat.is_contiguous()
    assert mean.dtype == rstd.dtype == torch.float32 and mean.numel() == rstd.numel() == B * C
    dx = torch.empty_like(x)
    ws, _ = slot_workspace("omr_instnorm_extent_slots", B, C, x.device, H * W)
    lib().call("omr_instnorm_extent_bwd", dtype_code(x.dtype), ptr(dxhat), ptr(x), ptr(mean), ptr(rstd), ptr(ext), ptr(dx), B, H, W, C, int(relu_mask),
               float(relu_scale), ptr(ws), cur_stream())
    return dx


def pack_memory_fwd(x: Tensor, ext: Tensor, smax: int) -> Tensor:
    """Feature grid [B, H, W, d] -> decoder memory [B, smax, d]: row i * w_b + j of sample b = cell (i, j); rows >= h_b * w_b zero."""
    B, H, W, C = _check_extents(x, ext)
    assert smax >= 1
    out = torch.empty((B, smax, C), dtype=x.dtype, device=x.device)
    lib().call("omr_pack_memory_fwd", dtype_code(x.dtype), ptr(x), ptr(ext), ptr(out), B, H, W, C, smax, cur_stream())
    return out


def pack_memory_bwd(dout: Tensor, ext: Tensor, H: int, W: int) -> Tensor:
    """Adjoint of pack_memory_fwd: gradient [B, smax, d] -> [B, H, W, d], zeros outside the extents."""
    require_cuda(dout, ext)
    assert dout.dim() == 3 and dout.is_contiguous() and ext.dtype == torch.int32 and ext.is_contiguous() and tuple(ext.shape) == (dout.shape[0], 2)
    B, smax, C = dout.shape
    dx = torch.empty((B, H, W, C), dtype=dout.dtype, device=dout.device)
    lib().call("omr_pack_memory_bwd", dtype_code(dout.dtype), ptr(dout), ptr(ext), ptr(dx), B, H, W, C, smax, cur_stream())
    return dx


def _check_lengths(lens: Tensor, B: int, device) -> None:
    assert lens.dtype == torch.int32 and lens.is_contiguous() and tuple(lens.shape) == (B,) and lens.device == device, \
        f"lengths must be int32 [B] on the device of the memory, got {lens.dtype} {tuple(lens.shape)} on {lens.device}"


def concat_memory_fwd(a: Tensor, len_a: Tensor, b: Optional[Tensor], len_b: Optional[Tensor], smax: int, out: Optional[Tensor] = None) -> Tensor:
    """Packed memories a [B, La, d], b [B, Lb, d] with per-sample lengths -> [B, smax, d]: rows [0, la) of a, then rows [0, lb) of b,
    then zeros (torch.cat of each sample alone).  b = None: the first la rows of a, zeros behind them.  out: write there ([B, smax, d])."""
    require_cuda(a, len_a, b, len_b)
    assert a.dim() == 3 and a.is_contiguous() and smax >= 1
    B, La, C = a.shape
    _check_lengths(len_a, B, a.device)
    Lb = 0
    if b is not None:
        assert b.is_contiguous() and b.dtype == a.dtype and b.dim() == 3 and b.shape[0] == B and b.shape[2] == C and b.device == a.device
        Lb = b.shape[1]
        _check_lengths(len_b, B, a.device)
    if out is None:
        out = torch.empty((B, smax, C), dtype=a.dtype, device=a.device)
    assert out.is_contiguous() and tuple(out.shape) == (B, smax, C) and out.dtype == a.dtype and out.device == a.device
    lib().call("omr_concat_memory_fwd", dtype_code(a.dtype), ptr(a), ptr(len_a), La, ptr(b), ptr(len_b) if Lb else None, Lb, ptr(out), B, C, smax,
               cur_stream())
    return out


def concat_memory_bwd(dout: Tensor, len_a: Tensor, La: int, len_b: Optional[Tensor], Lb: int) -> Tuple[Tensor, Optional[Tensor]]:
    """Adjoint of concat_memory_fwd: gradient [B, smax, d] -> (da [B, La, d], db [B, Lb, d] or None when Lb = 0), zeros at and past
    each length; rows of dout at or past la + lb are not read."""
    require_cuda(dout, len_a, len_b)
    assert dout.dim() == 3 and dout.is_contiguous() and La >= 1 and Lb >= 0
    B, smax, C = dout.shape
    _check_lengths(len_a, B, dout.device)
    da = torch.empty((B, La, C), dtype=dout.dtype, device=dout.device)
    db = None
    if Lb:
        _check_lengths(len_b, B, dout.device)
        db = torch.empty((B, Lb, C), dtype=dout.dtype, device=dout.device)
    lib().call("omr_concat_memory_bwd", dtype_code(dout.dtype), ptr(dout), ptr(len_a), La, ptr(len_b) if Lb else None, Lb, ptr(da), ptr(db), B, C, smax,
               cur_stream())
    return da, db


_GATHER_SRC_CODE = {torch.uint8: header_constant("OMR_DTYPE_U8"), torch.float32: dtype_code(torch.float32)}


def gather_ragged_batch(src: Tensor, offsets: Tensor, sizes: Tensor, idx: Tensor, H: int, W: int, dtype: torch.dtype, pad_value: float = 0.0,
                        out: Optional[Tensor] = None) -> Tensor:
    """Packed store `src` (1-D uint8 or fp32; sample n = the sizes[n, 0] x sizes[n, 1] plane at element offsets[n]) and sample indices
    idx int32 [B] -> [B, 1, H, W] in `dtype` (fp32 / bf16): the samples (uint8: / 255) in the top-left corners, pad_value elsewhere
    (csrc/batch_gather.hip).  offsets int64 [N], sizes int32 [N, 2], idx: all on src's device.  out: write there ([B, 1, H, W])."""
    require_cuda(src, offsets, sizes, idx)
    assert src.dim() == 1 and src.is_contiguous() and src.dtype in _GATHER_SRC_CODE, f"expected a flat uint8 / float32 store, got {src.dtype} {tuple(src.shape)}"
    N = offsets.numel()
    assert offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.is_contiguous() and offsets.device == src.device, \
        f"offsets must be int64 [N] on the device of src, got {offsets.dtype} {tuple(offsets.shape)} on {offsets.device}"
    assert sizes.dtype == torch.int32 and sizes.is_contiguous() and tuple(sizes.shape) == (N, 2) and sizes.device == src.device, \
        f"sizes must be int32 [N, 2] on the device of src, got {sizes.dtype} {tuple(sizes.shape)} on {sizes.device}"
    assert idx.dtype == torch.int32 and idx.dim() == 1 and idx.is_contiguous() and idx.device == src.device, \
        f"idx must be int32 [B] on the device of src, got {idx.dtype} {tuple(idx.shape)} on {idx.device}"
    B = idx.numel()
    if out is None:
        out = torch.empty((B, 1, H, W), dtype=dtype, device=src.device)
    assert out.is_contiguous() and tuple(out.shape) == (B, 1, H, W) and out.dtype == dtype and out.device == src.device
    lib().call("omr_gather_ragged_batch", _GATHER_SRC_CODE[src.dtype], ptr(src), ptr(offsets), ptr(sizes), N, ptr(idx), dtype_code(dtype), ptr(out), B, H, W,
               float(pad_value), cur_stream())
    return out


AUGMENT_RECORD_BYTES = 88            # sizeof(OmrAugment) (include/omr_hip.h); augment.AUG_DTYPE is its numpy mirror


def gather_augmented_batch(src: Tensor, offsets: Tensor, sizes: Tensor, idx: Tensor, aug: Tensor, H: int, W: int, dtype: torch.dtype,
                           pad_value: float = 0.0, out: Optional[Tensor] = None) -> Tensor:
    """`gather_ragged_batch` with one OmrAugment record per batch row (csrc/batch_augment.hip; include/omr_hip.h states the value of
    every pixel): aug uint8 [B, 88] on src's device, the bytes of `augment.AUG_DTYPE` records.  Row b holds sample idx[b] mapped,
    blended, scaled and masked by record b inside its extent (out_h, out_w), pad_value outside.  out: write there ([B, 1, H, W])."""
    require_cuda(src, offsets, sizes, idx, aug)
    assert src.dim() == 1 and src.is_contiguous() and src.dtype in _GATHER_SRC_CODE, f"expected a flat uint8 / float32 store, got {src.dtype} {tuple(src.shape)}"
    N = offsets.numel()
    assert offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.is_contiguous() and offsets.device == src.device, \
        f"offsets must be int64 [N] on the device of src, got {offsets.dtype} {tuple(offsets.shape)} on {offsets.device}"
    assert sizes.dtype == torch.int32 and sizes.is_contiguous() and tuple(sizes.shape) == (N, 2) and sizes.device == src.device, \
        f"sizes must be int32 [N, 2] on the device of src, got {sizes.dtype} {tuple(sizes.shape)} on {sizes.device}"
    assert idx.dtype == torch.int32 and idx.dim() == 1 and idx.is_contiguous() and idx.device == src.device, \
        f"idx must be int32 [B] on the device of src, got {idx.dtype} {tuple(idx.shape)} on {idx.device}"
    B = idx.numel()
    assert aug.dtype == torch.uint8 and aug.is_contiguous() and tuple(aug.shape) == (B, AUGMENT_RECORD_BYTES) and aug.device == src.device, \
        f"aug must be uint8 [B, {AUGMENT_RECORD_BYTES}] on the device of src, got {aug.dtype} {tuple(aug.shape)} on {aug.device}"
    if out is None:
        out = torch.empty((B, 1, H, W), dtype=dtype, device=src.device)
    assert out.is_contiguous() and tuple(out.shape) == (B, 1, H, W) and out.dtype == dtype and out.device == src.device
    lib().call("omr_gather_augmented_batch", _GATHER_SRC_CODE[src.dtype], ptr(src), ptr(offsets), ptr(sizes), N, ptr(idx), ptr(aug), dtype_code(dtype),
               ptr(out), B, H, W, float(pad_value), cur_stream())
    return out


def add_layernorm_fwd(x: Tensor, res: Optional[Tensor], gamma: Tensor, beta: Tensor, eps: float = 1e-5, drop_p: float = 0.0, drop_seed: int = 0):
    """LayerNorm(dropout(x) + res); drop_p = 0 is the plain residual add."""
    require_cuda(x, res, gamma, beta)
    d = x.shape[-1]
    M = x.numel() // d
    assert x.is_contiguous() and (res is None or (res.is_contiguous() and res.shape == x.shape))
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == d
    out = torch.empty_like(x)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    lib().call("omr_add_layernorm_fwd", dtype_code(x.dtype), ptr(x), ptr(res), ptr(gamma), ptr(beta), ptr(out), ptr(mean), ptr(rstd), M, d, eps,
               float(drop_p), int(drop_seed) & (2**64 - 1), cur_stream())
    return out, mean, rstd


def add_layernorm_bwd(dy: Tensor, x: Tensor, res: Optional[Tensor], gamma: Tensor, mean: Tensor, rstd: Tensor, dgamma: Tensor, dbeta: Tensor,
                      drop_p: float = 0.0, drop_seed: int = 0):
    """Returns ds (gradient of res, and of x without dropout); with drop_p > 0 returns (ds, dx)."""
    require_cuda(dy, x)
    d = x.shape[-1]
    M = x.numel() // d
    assert dy.is_contiguous() and dy.shape == x.shape and dgamma.dtype == torch.float32 and dbeta.dtype == torch.float32
    ds = torch.empty_like(x)
    dx = torch.empty_like(x) if drop_p > 0.0 else None
    lib().call("omr_add_layernorm_bwd", dtype_code(x.dtype), ptr(dy), ptr(x), ptr(res), ptr(gamma), ptr(mean), ptr(rstd), ptr(ds), ptr(dgamma),
               ptr(dbeta), M, d, float(drop_p), int(drop_seed) & (2**64 - 1), ptr(dx), cur_stream())
    return ds if dx is None else (ds, dx)


# ------------------------------------------------------------------------------------------------ convolutions

def conv_out_hw(H: int, W: int, stride: Tuple[int, int]) -> Tuple[int, int]:
    """k=3, pad=1: out = ceil(in / stride)."""
    return (H + stride[0] - 1) // stride[0], (W + stride[1] - 1) // stride[1]


def conv3x3(x: Tensor, w_phys: Tensor, bias: Optional[Tensor], stride=(1, 1), relu: bool = False, in_stats=None, out_mask: Optional[Tensor] = None,
            mask_scale: float = 1.0, dil=(1, 1), out_hw: Optional[Tuple[int, int]] = None, drop=None, stat_mode: int = 0,
            stat_ws: Optional[Tensor] = None, stat_slots: int = 0, stat_x: Optional[Tensor] = None, stat_stats=None) -> Tensor:
    """x NHWC [B,H,W,CIN]; w_phys [COUT,3,3,CIN] contiguous; returns NHWC [B,Ho,Wo,COUT].
    drop = (p, seed, channel_mode): fused dropout after the ReLU.  stat_mode 1/2: fused per-(image, channel) reductions of
    the stored output into the fp64 slot workspace (stat_ws, stat_slots) = conv_stat_ws(...) (see include/omr_hip.h)."""
    require_cuda(x, w_phys, bias, out_mask, stat_ws, stat_x)
    B, H, W, CIN = x.shape
    COUT = w_phys.shape[0]
    assert x.is_contiguous() and w_phys.is_contiguous() and tuple(w_phys.shape) == (COUT, 3, 3, CIN) and w_phys.dtype == x.dtype
    if out_hw is None:
        out_hw = conv_out_hw(H, W, stride)
    Ho, Wo = out_hw
    y = torch.empty((B, Ho, Wo, COUT), dtype=x.dtype, device=x.device) if stat_mode != 4 else None      # mode 4 takes sums only
    mean = rstd = None
    if in_stats is not None:
        mean, rstd = in_stats
        assert tuple(mean.shape) == (B, CIN) and mean.dtype == torch.float32
    if out_mask is not None:
        assert tuple(out_mask.shape) == (B, Ho, Wo, COUT) and out_mask.is_contiguous() and out_mask.dtype == x.dtype
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == COUT
    p, seed, chan = drop if drop is not None else (0.0, 0, False)
    smean = srstd = None
    if stat_mode:
        assert stat_ws is not None and stat_ws.dtype == torch.float64 and stat_slots >= 1 and stat_ws.numel() >= slot_workspace_elems(B, COUT, stat_slots)
    if stat_mode >= 2:
        smean, srstd = stat_stats
        assert stat_x is not None and tuple(stat_x.shape) == (B, Ho, Wo, COUT) and stat_x.is_contiguous() and tuple(smean.shape) == (B, COUT)
    lib().call("omr_conv3x3_fwd", dtype_code(x.dtype), ptr(x), ptr(w_phys), ptr(bias), ptr(y), ptr(mean), ptr(rstd), ptr(out_mask), float(mask_scale),
               B, H, W, CIN, COUT, stride[0], stride[1], dil[0], dil[1], Ho, Wo, int(relu), float(p), int(seed) & (2**64 - 1), int(chan),
               int(stat_mode), ptr(stat_ws), int(stat_slots), ptr(stat_x), ptr(smean), ptr(srstd), cur_stream())
    return y


def instnorm_reduce_sums(ws: Tensor, slots: int, B: int, C: int) -> None:
    """Per-image sums of the slots a conv3x3(stat_mode=2 / 4) launch filled, into the compact region of the same workspace."""
    require_cuda(ws)
    lib().call("omr_instnorm_reduce_sums", ptr(ws), slots, B, C, cur_stream())


def conv3x3_weight_flip(w_phys: Tensor) -> Tensor:
    """[COUT,3,3,CIN] -> [CIN,3,3,COUT] with mirrored taps (weights of the data-gradient conv)."""
    require_cuda(w_phys)
    COUT, _, _, CIN = w_phys.shape
    wd = torch.empty((CIN, 3, 3, COUT), dtype=w_phys.dtype, device=w_phys.device)
    lib().call("omr_conv3x3_weight_flip", dtype_code(w_phys.dtype), ptr(w_phys), ptr(wd), COUT, CIN, cur_stream())
    return wd


class _FlipDesc(ctypes.Structure):
    _fields_ = [("w", ctypes.c_void_p), ("wd", ctypes.c_void_p), ("cout", ctypes.c_int), ("cin", ctypes.c_int)]


def conv3x3_weight_flip_table(pairs):
    """Host table for conv3x3_weight_flip_grouped: pairs of (w_phys [COUT,3,3,CIN], wd [CIN,3,3,COUT]) in one dtype.  Built once
    (the tensors are fixed views of the flat parameter buffers) and reused every optimizer step."""
    arr = (_FlipDesc * len(pairs))()
    dt = pairs[0][0].dtype
    for q, (w, wd) in zip(arr, pairs):
        require_cuda(w, wd)
        COUT, _, _, CIN = w.shape
        assert w.dtype == wd.dtype == dt and w.is_contiguous() and wd.is_contiguous() and tuple(wd.shape) == (CIN, 3, 3, COUT)
        q.w, q.wd, q.cout, q.cin = w.data_ptr(), wd.data_ptr(), COUT, CIN
    return dtype_code(dt), len(pairs), arr


def conv3x3_weight_flip_grouped(table) -> None:
    """All data-gradient weight re-layouts of a model in ONE launch (omr_conv3x3_weight_flip_grouped)."""
    code, n, arr = table
    lib().call("omr_conv3x3_weight_flip_grouped", code, n, ctypes.byref(arr), cur_stream())


def conv3x3_wgrad(x: Tensor, dy: Tensor, dw_phys: Tensor, stride=(1, 1), in_stats=None, db: Optional[Tensor] = None) -> None:
    """dw_phys (fp32 [COUT,3,3,CIN], accumulated in place) += grad; db (fp32 [COUT]) += bias grad (same pass over dy)."""
    require_cuda(x, dy, dw_phys, db)
    if db is not None:
        assert db.dtype == torch.float32 and db.numel() == dy.shape[-1]
    B, H, W, CIN = x.shape
    _, Ho, Wo, COUT = dy.shape
    assert (Ho, Wo) == conv_out_hw(H, W, stride) and dy.shape[0] == B
    assert dw_phys.dtype == torch.float32 and dw_phys.is_contiguous() and tuple(dw_phys.shape) == (COUT, 3, 3, CIN)
    assert x.is_contiguous() and dy.is_contiguous() and x.dtype == dy.dtype
    mean, rstd = in_stats if in_stats is not None else (None, None)
    lib().call("omr_conv3x3_wgrad", dtype_code(x.dtype), ptr(x), ptr(dy), ptr(dw_phys), ptr(db), ptr(mean), ptr(rstd), B, H, W, CIN, COUT, stride[0], stride[1],
               Ho, Wo, cur_stream())


def conv3x3_bwd_fused_covers(bf16: bool, cin: int, cout: int, stride=(1, 1)) -> bool:
    """Shapes omr_conv3x3_bwd_fused covers: bf16, stride 1, (COUT, CIN) in {(32, 32), (32, 16), (16, 16)}."""
    return bf16 and tuple(stride) == (1, 1) and (cout, cin) in ((32, 32), (32, 16), (16, 16))


def conv3x3_bwd_fused_ok(x: Tensor, g: Tensor, stride=(1, 1)) -> bool:
    """conv3x3_bwd_fused_covers of an NHWC input x and output gradient g."""
    return x.dim() == 4 and conv3x3_bwd_fused_covers(x.dtype == torch.bfloat16, x.shape[-1], g.shape[-1], stride)


def conv3x3_bwd_fused(g: Tensor, x: Tensor, w_flipped: Tensor, dw_phys: Tensor, db: Optional[Tensor], mask_input: bool, mask_scale: float = 1.0,
                      norm=None, xnorm=None) -> Tensor:
    """Data gradient, weight gradient and bias gradient of a stride-1 3x3 conv in one pass (bf16, <= 32 channels): returns
    dx = conv^T(g) [* (x > 0) * mask_scale]; dw_phys / db (fp32, accumulated in place).  norm = (y, mean, rstd, ws, slots, relu_mask,
    relu_scale): g is the gradient w.r.t. InstanceNorm(y) and the InstanceNorm backward (sums in ws, reduced by
    instnorm_reduce_sums) + the ReLU / dropout mask of y are applied on load.  xnorm = (mean, rstd, ws, slots) (16 -> 16 channels): the
    conv normalised x on load; returns dL/dxhat and fills the InstanceNorm-backward slots of ws (conv_stat_ws layout)."""
    require_cuda(g, x, w_flipped, dw_phys, db)
    B, H, W, CIN = x.shape
    COUT = g.shape[-1]
    assert conv3x3_bwd_fused_ok(x, g) and g.shape[:3] == x.shape[:3] and g.dtype == x.dtype and g.is_contiguous() and x.is_contiguous()
    assert tuple(w_flipped.shape) == (CIN, 3, 3, COUT) and w_flipped.dtype == x.dtype and w_flipped.is_contiguous()
    assert dw_phys.dtype == torch.float32 and dw_phys.is_contiguous() and tuple(dw_phys.shape) == (COUT, 3, 3, CIN)
    if db is not None:
        assert db.dtype == torch.float32 and db.numel() == COUT
    dx = torch.empty_like(x)
    if norm is None:
        ny = mean = rstd = ws = None
        slots, relu_mask, relu_scale = 0, False, 1.0
    else:
        ny, mean, rstd, ws, slots, relu_mask, relu_scale = norm
        require_cuda(ny, mean, rstd, ws)
        assert ny.shape == g.shape and ny.is_contiguous() and ny.dtype == g.dtype and ws.dtype == torch.float64
    xm = xr = xws = None
    xslots = 0
    if xnorm is not None:
        xm, xr, xws, xslots = xnorm
        require_cuda(xm, xr, xws)
        assert xws.dtype == torch.float64 and norm is None and not mask_input
    lib().call("omr_conv3x3_bwd_fused", ptr(g), ptr(x), ptr(w_flipped), ptr(dx), ptr(dw_phys), ptr(db), B, H, W, CIN, COUT, int(mask_input), float(mask_scale),
               ptr(ny), ptr(mean), ptr(rstd), ptr(ws), int(slots), int(relu_mask), float(relu_scale), ptr(xm), ptr(xr), ptr(xws), int(xslots), cur_stream())
    return dx


def conv3x3_bwd_fused_s2(g: Tensor, x: Tensor, w_flipped: Tensor, dw_phys: Tensor, db: Optional[Tensor], mean: Tensor, rstd: Tensor, ws: Tensor,
                         slots: int) -> Tensor:
    """One-pass backward of the stride-(2,2), 32 -> 32 channel conv that normalised x on load (bf16): returns dL/dxhat, accumulates
    dw_phys / db and fills the InstanceNorm-backward slots of ws (conv_stat_ws layout for x's shape)."""
    require_cuda(g, x, w_flipped, dw_phys, db, mean, rstd, ws)
    B, H, W, C = x.shape
    assert C == 32 and x.dtype == torch.bfloat16 and g.dtype == x.dtype and tuple(g.shape) == (B, (H + 1) // 2, (W + 1) // 2, 32)
    assert g.is_contiguous() and x.is_contiguous() and tuple(w_flipped.shape) == (32, 3, 3, 32) and w_flipped.is_contiguous() and w_flipped.dtype == x.dtype
    assert dw_phys.dtype == torch.float32 and dw_phys.is_contiguous() and tuple(dw_phys.shape) == (32, 3, 3, 32) and ws.dtype == torch.float64
    dx = torch.empty_like(x)
    lib().call("omr_conv3x3_bwd_fused_s2", ptr(g), ptr(x), ptr(w_flipped), ptr(dx), ptr(dw_phys), ptr(db), B, H, W, ptr(mean), ptr(rstd), ptr(ws), int(slots),
               cur_stream())
    return dx


def dwconv3x3(x: Tensor, w: Tensor, bias: Optional[Tensor], in_stats=None, out_mask: Optional[Tensor] = None, mask_scale: float = 1.0,
              flip: bool = False) -> Tensor:
    """Depthwise 3x3 on NHWC; w is [C,9] (= [C,1,3,3] storage)."""
    require_cuda(x, w, bias, out_mask)
    B, H, W, C = x.shape
    assert x.is_contiguous() and w.is_contiguous() and w.numel() == C * 9 and w.dtype == x.dtype
    y = torch.empty_like(x)
    mean, rstd = in_stats if in_stats is not None else (None, None)
    if out_mask is not None:
        assert out_mask.shape == x.shape and out_mask.is_contiguous()
    lib().call("omr_dwconv3x3", dtype_code(x.dtype), ptr(x), ptr(w), ptr(bias), ptr(y), ptr(mean), ptr(rstd), ptr(out_mask), float(mask_scale), B, H, W,
               C, int(flip), cur_stream())
    return y


def dwconv3x3_wgrad(x: Tensor, dy: Tensor, dw: Tensor, db: Optional[Tensor], in_stats=None) -> None:
    require_cuda(x, dy, dw, db)
    B, H, W, C = x.shape
    assert dy.shape == x.shape and dw.dtype == torch.float32 and dw.numel() == C * 9 and x.is_contiguous() and dy.is_contiguous()
    mean, rstd = in_stats if in_stats is not None else (None, None)
    lib().call("omr_dwconv3x3_wgrad", dtype_code(x.dtype), ptr(x), ptr(dy), ptr(dw), ptr(db), ptr(mean), ptr(rstd), B, H, W, C, cur_stream())


# ------------------------------------------------------------------------------------------------ attention

def _bts(t: Tensor) -> Tuple[int, int]:
    assert t.dim() == 3 and t.stride(2) == 1, f"expected [B,rows,cols] with unit inner stride, got {tuple(t.shape)} / {t.stride()}"
    return t.stride(1), t.stride(0)


def attn_dropout_words(B: int, H: int, T: int, S: int, p: float, seed: int, device) -> Tensor:
    """The keep bits of the attention-probability dropout for (p, seed) in the kernels' word layout (omr_attn_dropout_words):
    int64 [omr_attn_dropout_words_count].  Generated once per (layer, step); forward and backward read the same buffer."""
    n = lib().query("omr_attn_dropout_words_count", B, H, T, S)
    out = torch.empty(n, dtype=torch.int64, device=device)
    lib().call("omr_attn_dropout_words", ptr(out), B, H, T, S, float(p), int(seed) & (2**64 - 1), cur_stream())
    return out


def attn_fwd(q: Tensor, k: Tensor, v: Tensor, nhead: int, *, causal: bool = False, window: int = -1, key_bias: Optional[Tensor] = None,
             blk_lq: Optional[Tensor] = None, blk_lkv: Optional[Tensor] = None, dropout_p: float = 0.0, seed: int = 0,
             drop_words: Optional[Tensor] = None):
    """q [B,T,d], k/v [B,S,d] (may be strided views of packed projections) -> (o [B,T,d], lse [B,H,T]).  dropout_p > 0: the keep
    bits come from drop_words (attn_dropout_words; generated here from (dropout_p, seed) when not given)."""
    require_cuda(q, k, v, key_bias, blk_lq, blk_lkv)
    B, T, d = q.shape
    S = k.shape[1]
    assert k.shape == (B, S, d) and v.shape == (B, S, d) and d % nhead == 0 and q.dtype == k.dtype == v.dtype
    hd = d // nhead
    o = torch.empty((B, T, d), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, nhead, T), dtype=torch.float32, device=q.device)
    if key_bias is not None:
        assert key_bias.dtype == torch.float32 and tuple(key_bias.shape) == (B, S) and key_bias.is_contiguous()
    for t in (blk_lq, blk_lkv):
        if t is not None:
            assert t.dtype == torch.int32 and t.numel() == B and t.is_contiguous()
    (ldq, bsq), (ldk, bsk), (ldv, bsv), (ldo, bso) = _bts(q), _bts(k), _bts(v), _bts(o)
    ws, nws = _attn_ws(B, nhead, T, S, hd, causal, False, q.device)
    if dropout_p > 0.0 and drop_words is None:
        drop_words = attn_dropout_words(B, nhead, T, S, dropout_p, seed, q.device)
    lib().call("omr_attn_fwd_ws", dtype_code(q.dtype), ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, B, nhead, T, S, hd,
               int(causal), int(window), ptr(key_bias), ptr(blk_lq), ptr(blk_lkv), float(dropout_p), int(seed) & (2**64 - 1), ptr(drop_words), ptr(ws), nws,
               cur_stream())
    return o, lse


def attn_fwd_split_partials(q: Tensor, k: Tensor, v: Tensor, nhead: int):
    """Decode attention (q [B,1,d]) stopped before its merge pass: -> (partials [B*H, nsplit, hd+2], nsplit); with nsplit == 1
    the first return value is the finished output [B,1,d] instead (omr_attn_fwd_split_partials)."""
    require_cuda(q, k, v)
    B, T, d = q.shape
    S, hd = k.shape[1], d // nhead
    assert T == 1
    o = torch.empty((B, T, d), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, nhead, T), dtype=torch.float32, device=q.device)
    n = lib().query("omr_attn_split_workspace_floats", B, nhead, T, S, hd)
    ws = torch.empty(max(n, 1), dtype=torch.float32, device=q.device)
    ns = ctypes.c_int(0)
    (ldq, bsq), (ldk, bsk), (ldv, bsv), (ldo, bso) = _bts(q), _bts(k), _bts(v), _bts(o)
    lib().call("omr_attn_fwd_split_partials", dtype_code(q.dtype), ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, B, nhead, T, S,
               hd, ptr(ws), n, ctypes.byref(ns), cur_stream())
    if ns.value <= 1:
        return o, 1
    return ws[:B * nhead * ns.value * (hd + 2)].view(B * nhead, ns.value, hd + 2), ns.value


def _attn_ws(B: int, H: int, T: int, S: int, hd: int, causal: bool, backward: bool, device):
    """Scratch for the key split of the query-per-lane attention kernels (include/omr_hip.h omr_attn_workspace_floats)."""
    n = lib().query("omr_attn_workspace_floats", B, H, T, S, hd, int(causal), int(backward))
    return (torch.empty(n, dtype=torch.float32, device=device), n) if n > 0 else (None, 0)


def attn_bwd(q, k, v, o, dout, lse, dq, dk, dv, nhead: int, *, causal=False, window=-1, key_bias=None, blk_lq=None, blk_lkv=None,
             dropout_p: float = 0.0, seed: int = 0, drop_words: Optional[Tensor] = None) -> None:
    """Writes dq [B,T,d], dk/dv [B,S,d] (views allowed, unit inner stride)."""
    require_cuda(q, k, v, o, dout, dq, dk, dv)
    B, T, d = q.shape
    S = k.shape[1]
    hd = d // nhead
    delta = torch.empty((B, nhead, T), dtype=torch.float32, device=q.device)
    assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape and dout.shape == o.shape
    (ldq, bsq), (ldk, bsk), (ldv, bsv), (ldo, bso), (lddo, bsdo) = _bts(q), _bts(k), _bts(v), _bts(o), _bts(dout)
    (lddq, bsdq), (lddk, bsdk), (lddv, bsdv) = _bts(dq), _bts(dk), _bts(dv)
    ws, nws = _attn_ws(B, nhead, T, S, hd, causal, True, q.device)
    if dropout_p > 0.0 and drop_words is None:
        drop_words = attn_dropout_words(B, nhead, T, S, dropout_p, seed, q.device)
    lib().call("omr_attn_bwd_ws", dtype_code(q.dtype), ptr(q), ptr(k), ptr(v), ptr(o), ptr(dout), ptr(lse), ptr(delta), ptr(dq), ptr(dk), ptr(dv), ldq, ldk,
               ldv, ldo, lddo, lddq, lddk, lddv, bsq, bsk, bsv, bso, bsdo, bsdq, bsdk, bsdv, B, nhead, T, S, hd, int(causal), int(window),
               ptr(key_bias), ptr(blk_lq), ptr(blk_lkv), float(dropout_p), int(seed) & (2**64 - 1), ptr(drop_words), ptr(ws), nws, cur_stream())


def attn_weights(q: Tensor, k: Tensor, lse: Tensor, nhead: int, *, causal: bool = False, window: int = -1, key_bias: Optional[Tensor] = None,
                 blk_lq: Optional[Tensor] = None, blk_lkv: Optional[Tensor] = None, kv_len: Optional[Tensor] = None, dropout_p: float = 0.0,
                 drop_words: Optional[Tensor] = None, out: Optional[Tensor] = None, out_scale: Optional[float] = None,
                 accumulate: bool = False) -> Tensor:
    """Head-averaged attention weights (omr_attn_weights) of the attention whose forward wrote `lse` [B,H,T] for these q [B,T,d] /
    k [B,S,d] and masks -> fp32 [B,T,S].  out_scale defaults to 1 / nhead (torch's head average); `out` (fp32 [B,T,S], unit inner
    stride, any row pitch) with accumulate=True is added to instead of written.  A new buffer has its rows padded to 16 bytes;
    the returned tensor is the [B,T,S] view of it.  dropout_p > 0 needs the forward's drop_words."""
    require_cuda(q, k, lse, key_bias, blk_lq, blk_lkv, kv_len, drop_words, out)
    B, T, d = q.shape
    S = k.shape[1]
    assert k.shape == (B, S, d) and d % nhead == 0 and q.dtype == k.dtype
    assert lse.dtype == torch.float32 and tuple(lse.shape) == (B, nhead, T) and lse.is_contiguous()
    if key_bias is not None:
        assert key_bias.dtype == torch.float32 and tuple(key_bias.shape) == (B, S) and key_bias.is_contiguous()
    for t in (blk_lq, blk_lkv, kv_len):
        if t is not None:
            assert t.dtype == torch.int32 and t.numel() == B and t.is_contiguous()
    assert dropout_p == 0.0 or drop_words is not None, "the post-dropout weights need the keep words the forward read"
    if out is None:
        assert not accumulate, "accumulate adds to a buffer of the caller's"
        out = torch.empty((B, T, round_up(S, 4)), dtype=torch.float32, device=q.device)[:, :, :S]
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, T, S)
    (ldq, bsq), (ldk, bsk), (ldw, bsw) = _bts(q), _bts(k), _bts(out)
    lib().call("omr_attn_weights", dtype_code(q.dtype), ptr(q), ptr(k), ptr(lse), ptr(out), ldq, ldk, ldw, bsq, bsk, bsw, B, nhead, T, S, d // nhead,
               int(causal), int(window), ptr(key_bias), ptr(blk_lq), ptr(blk_lkv), ptr(kv_len), float(dropout_p), ptr(drop_words),
               float(1.0 / nhead if out_scale is None else out_scale), int(accumulate), cur_stream())
    return out


def attn_dropout_mask(B: int, H: int, T: int, S: int, p: float, seed: int, device) -> Tensor:
    """uint8 [B,H,T,S] keep-mask of the attention-probability dropout for (p, seed): test / debug entry."""
    out = torch.empty((B, H, T, S), dtype=torch.uint8, device=device)
    lib().call("omr_attn_dropout_mask", ptr(out), B, H, T, S, float(p), int(seed) & (2**64 - 1), cur_stream())
    return out


# ------------------------------------------------------------------------------------------------ loss

def _loss_fwd(logits2d: Tensor, target: Tensor, V: int, n: int, lse_shape: Tuple[int, ...] = ()):
    """The checks every loss forward makes of its rows logits2d [M, ldv >= V] and targets int64 [M], and the buffers every one writes
    -> (M, ldv, lse fp32 [*lse_shape, M], acc fp64 [n], means fp32 [n - 1])."""
    require_cuda(logits2d, target)
    M, cols, ldv = _rows2d(logits2d)
    assert cols >= V and target.numel() == M and target.dtype == torch.int64 and target.is_contiguous()
    new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=logits2d.device)  # noqa: E731
    return M, ldv, new(lse_shape + (M,)), new(n, torch.float64), new(n - 1)


def _loss_grad(logits2d: Tensor, target: Tensor, grad_out: Optional[Tensor]) -> Tuple[int, int, Tensor, Tensor]:
    """The checks every loss backward makes, and its gradient -> (M, ldv, the [M, ldv] buffer the kernel writes, its view to return)."""
    require_cuda(logits2d, target, grad_out)
    if grad_out is not None:
        assert grad_out.dtype == torch.float32 and grad_out.numel() == 1
    M, cols, ldv = _rows2d(logits2d)
    dl = torch.empty((M, ldv), dtype=logits2d.dtype, device=logits2d.device)
    return M, ldv, dl, dl[:, :cols]


def ce_fwd(logits2d: Tensor, target: Tensor, V: int, pad_idx: int):
    """logits2d [M, ldv>=V]; target int64 [M] -> (loss fp32 [1], lse [M], acc2 fp64 [2])."""
    M, ldv, lse, acc2, loss = _loss_fwd(logits2d, target, V, 2)
    lib().call("omr_ce_fwd", dtype_code(logits2d.dtype), ptr(logits2d), ptr(target), ptr(lse), ptr(acc2), ptr(loss), M, V, ldv, pad_idx, cur_stream())
    return loss, lse, acc2


def ce_bwd(logits2d: Tensor, target: Tensor, lse: Tensor, acc2: Tensor, V: int, pad_idx: int, grad_scale: float = 1.0,
           grad_out: Optional[Tensor] = None) -> Tensor:
    M, ldv, dl, out = _loss_grad(logits2d, target, grad_out)
    lib().call("omr_ce_bwd", dtype_code(logits2d.dtype), ptr(logits2d), ptr(target), ptr(lse), ptr(acc2), ptr(dl), M, V, ldv, pad_idx, float(grad_scale),
               ptr(grad_out), cur_stream())
    return out


def check_label_smoothing(eps) -> float:
    """torch's range for label_smoothing; refused here, before anything is allocated or launched."""
    eps = float(eps)
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"label_smoothing must be between 0.0 and 1.0, got {eps}")
    return eps


def ce_smooth_fwd(logits2d: Tensor, target: Tensor, V: int, pad_idx: int, eps: float):
    """ce_fwd with label smoothing eps in [0, 1] -> (loss fp32 [1], nll fp32 [1], lse [M], rowsum [M] or None, acc3 fp64 [3]).
    loss is the mean smoothed objective, nll the mean un-smoothed lse - logit[target], rowsum the per-row sum of the logits over the
    columns < V, acc3 = {objective sum, live rows, nll sum}.  eps == 0 runs ce_fwd's kernels (same bits) and has no rowsum."""
    eps = check_label_smoothing(eps)
    M, ldv, lse, acc3, means = _loss_fwd(logits2d, target, V, 3)
    rowsum = torch.empty_like(lse) if eps > 0 else None
    lib().call("omr_ce_smooth_fwd", dtype_code(logits2d.dtype), ptr(logits2d), ptr(target), ptr(lse), ptr(rowsum), ptr(acc3), ptr(means),
               means.data_ptr() + 4, M, V, ldv, pad_idx, eps, cur_stream())
    return means[:1], means[1:], lse, rowsum, acc3


def ce_smooth_bwd(logits2d: Tensor, target: Tensor, lse: Tensor, acc3: Tensor, V: int, pad_idx: int, eps: float, grad_scale: float = 1.0,
                  grad_out: Optional[Tensor] = None) -> Tensor:
    """ce_bwd with label smoothing eps: (softmax - (1 - eps) onehot - eps / V) * grad_scale * grad_out / count.  eps == 0 runs ce_bwd's kernel."""
    eps = check_label_smoothing(eps)
    M, ldv, dl, out = _loss_grad(logits2d, target, grad_out)
    lib().call("omr_ce_smooth_bwd", dtype_code(logits2d.dtype), ptr(logits2d), ptr(target), ptr(lse), ptr(acc3), ptr(dl), M, V, ldv, pad_idx, eps,
               float(grad_scale), ptr(grad_out), cur_stream())
    return out


def check_distill(alpha, temperature, weight, two_teachers: bool) -> Tuple[float, float, float]:
    """The ranges omr_ce_distill_fwd accepts; refused here, before anything is allocated or launched."""
    alpha, tau, lam = float(alpha), float(temperature), float(weight)
    if not (tau > 0.0 and math.isfinite(tau)):
        raise ValueError(f"distillation temperature must be finite and > 0, got {tau}")
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"distillation weight must be between 0.0 and 1.0, got {lam}")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"distillation alpha must be between 0.0 and 1.0, got {alpha}")
    if not two_teachers and alpha != 1.0:
        raise ValueError(f"distillation with one teacher takes alpha = 1, got {alpha}")
    return alpha, tau, lam


def _distill_teachers(logits2d: Tensor, teacher_a: Optional[Tensor], teacher_b: Optional[Tensor], V: int, lam: float):
    """-> (tdtype code, ldt).  weight == 0 never reads the teachers: they may be None."""
    if lam == 0.0 and teacher_a is None:
        return dtype_code(logits2d.dtype), V
    M = logits2d.shape[0]
    require_cuda(teacher_a, teacher_b)
    Ma, cols, ldt = _rows2d(teacher_a)
    assert Ma == M and cols >= V, "teacher logits must have the student's rows and at least its V columns"
    if teacher_b is not None:
        assert teacher_b.dtype == teacher_a.dtype and _rows2d(teacher_b) == (M, cols, ldt), "the two teachers share dtype, shape and pitch"
    return dtype_code(teacher_a.dtype), ldt


def ce_distill_fwd(logits2d: Tensor, target: Tensor, teacher_a: Optional[Tensor], teacher_b: Optional[Tensor], V: int, pad_idx: int, alpha: float,
                   temperature: float, weight: float):
    """Hard-label cross-entropy plus the KL divergence to one or two teachers (omr_ce_distill_fwd): student logits2d [M, ldv >= V],
    teacher logits [M, ldt >= V] (teacher_b may be None, then alpha = 1) -> (means fp32 [3] = {loss, nll, kd}, lse4 fp32 [4, M],
    rowkd fp32 [M] or None, acc4 fp64 [4]).  weight == 0 runs ce_fwd's kernels (same bits), reads no teacher and has no rowkd."""
    alpha, tau, lam = check_distill(alpha, temperature, weight, teacher_b is not None)
    M, ldv, lse4, acc4, means = _loss_fwd(logits2d, target, V, 4, lse_shape=(4,))
    tdtype, ldt = _distill_teachers(logits2d, teacher_a, teacher_b, V, lam)
    rowkd = torch.empty_like(lse4[0]) if lam > 0 else None
    lib().call("omr_ce_distill_fwd", dtype_code(logits2d.dtype), ptr(logits2d), ldv, tdtype, ptr(teacher_a), ptr(teacher_b), ldt, ptr(target),
               ptr(lse4), ptr(rowkd), ptr(acc4), ptr(means), M, V, pad_idx, alpha, tau, lam, cur_stream())
    return means, lse4, rowkd, acc4


def ce_distill_bwd(logits2d: Tensor, target: Tensor, teacher_a: Optional[Tensor], teacher_b: Optional[Tensor], lse4: Tensor, acc4: Tensor, V: int,
                   pad_idx: int, alpha: float, temperature: float, weight: float, grad_scale: float = 1.0,
                   grad_out: Optional[Tensor] = None) -> Tensor:
    """((1 - weight)(softmax - onehot) + weight tau (softmax(x / tau) - q)) * grad_scale * grad_out / count.  weight == 0 runs ce_bwd's kernel."""
    alpha, tau, lam = check_distill(alpha, temperature, weight, teacher_b is not None)
    M, ldv, dl, out = _loss_grad(logits2d, target, grad_out)
    tdtype, ldt = _distill_teachers(logits2d, teacher_a, teacher_b, V, lam)
    assert lse4.dtype == torch.float32 and tuple(lse4.shape) == (4, M) and lse4.is_contiguous()
    lib().call("omr_ce_distill_bwd", dtype_code(logits2d.dtype), ptr(logits2d), ldv, tdtype, ptr(teacher_a), ptr(teacher_b), ldt, ptr(target),
               ptr(lse4), ptr(acc4), ptr(dl), M, V, pad_idx, alpha, tau, lam, float(grad_scale), ptr(grad_out), cur_stream())
    return out


def round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ CTC auxiliary head (csrc/ctc.hip)

def check_ctc(weight, pool) -> Tuple[float, int]:
    """The ranges of ModelConfig.ctc_weight ([0, 1]) and ctc_pool (an integer >= 1); refused here, before anything is allocated or launched."""
    if isinstance(weight, bool) or not isinstance(weight, (int, float)):
        raise ValueError(f"ctc_weight must be a number, got {weight!r}")
    weight = float(weight)
    if not 0.0 <= weight <= 1.0:
        raise ValueError(f"ctc_weight must be between 0.0 and 1.0, got {weight}")
    if isinstance(pool, bool) or not isinstance(pool, int) or pool < 1:
        raise ValueError(f"ctc_pool must be an integer >= 1, got {pool!r}")
    return weight, pool


def ctc_frame_count(gh: int, gw: int, pool: int) -> int:
    """Frames of a gh x gw feature grid: ceil(gh / pool) groups per column, column by column."""
    return (gh + pool - 1) // pool * gw


def _check_grid(grid: Optional[Tensor], B: int, device) -> None:
    if grid is not None:
        assert grid.dtype == torch.int32 and grid.is_contiguous() and tuple(grid.shape) == (B, 2) and grid.device == device, \
            f"grid must be int32 [B, 2] on the memory's device, got {grid.dtype} {tuple(grid.shape)} on {grid.device}"


def ctc_frames_fwd(mem: Tensor, grid: Optional[Tensor], gh: int, gw: int, pool: int, fmax: int) -> Tuple[Tensor, Tensor]:
    """Memory [B, S, d] (sample b's own gh_b x gw_b grid row-major, zeros behind) -> (frames [B, fmax, d], frame_len int32 [B]): column by
    column, `pool` grid rows averaged per frame (omr_ctc_frames_fwd).  grid int32 [B, 2] on the device: the ragged route; None: every sample has
    the grid gh x gw."""
    require_cuda(mem, grid)
    assert mem.dim() == 3 and mem.is_contiguous(), f"expected a contiguous [B, S, d] memory, got shape {tuple(mem.shape)} strides {mem.stride()}"
    B, S, d = mem.shape
    _check_grid(grid, B, mem.device)
    frames = torch.empty((B, fmax, d), dtype=mem.dtype, device=mem.device)
    frame_len = torch.empty(B, dtype=torch.int32, device=mem.device)
    lib().call("omr_ctc_frames_fwd", dtype_code(mem.dtype), ptr(mem), ptr(grid), ptr(frames), ptr(frame_len), B, S, d, gh, gw, pool, fmax, cur_stream())
    return frames, frame_len


def ctc_frames_bwd(dframes: Tensor, grid: Optional[Tensor], gh: int, gw: int, pool: int, S: int) -> Tensor:
    """Adjoint of ctc_frames_fwd: gradient [B, fmax, d] -> [B, S, d], zeros outside each sample's grid."""
    require_cuda(dframes, grid)
    assert dframes.dim() == 3 and dframes.is_contiguous()
    B, fmax, d = dframes.shape
    _check_grid(grid, B, dframes.device)
    dmem = torch.empty((B, S, d), dtype=dframes.dtype, device=dframes.device)
    lib().call("omr_ctc_frames_bwd", dtype_code(dframes.dtype), ptr(dframes), ptr(grid), ptr(dmem), B, S, d, gh, gw, pool, fmax, cur_stream())
    return dmem


def _ctc_logits(logits: Tensor, frame_len: Tensor, V: int) -> Tuple[int, int, int]:
    """The checks every CTC entry makes of logits [B, Fmax, >= V] (unit inner stride, frames and samples back to back) -> (B, Fmax, ldv)."""
    require_cuda(logits, frame_len)
    assert logits.dim() == 3 and logits.stride(2) == 1 and logits.shape[2] >= V, f"expected logits [B, F, >= {V}], got {tuple(logits.shape)}"
    B, fmax, _ = logits.shape
    ldv = logits.stride(1)
    assert ldv >= V and logits.stride(0) == fmax * ldv, f"logits rows must lie back to back at one pitch, got strides {logits.stride()}"
    assert frame_len.dtype == torch.int32 and frame_len.is_contiguous() and tuple(frame_len.shape) == (B,) and frame_len.device == logits.device
    return B, fmax, ldv


def ctc_workspace_bytes(B: int, fmax: int, tmax: int, V: int) -> int:
    n = lib().query("omr_ctc_workspace_bytes", B, fmax, tmax, V)
    if n < 0:
        raise ValueError(f"the CTC loss takes 1 <= B <= 32767, F >= 1 and 1 <= T <= 1023, got B = {B}, F = {fmax}, T = {tmax}")
    return n


def ctc_workspace_lse(ws: Tensor, B: int, fmax: int) -> Tensor:
    """The frames' log-sum-exp fp32 [B, fmax] inside a workspace omr_ctc_fwd has filled (frames >= F_b are not written): it lies behind the
    fp64 offsets [2][B][fmax] and log P [2][B], each block rounded up to 16 bytes (csrc/ctc.hip, ctc_ws_layout)."""
    r16 = lambda n: (n + 15) // 16 * 16  # noqa: E731
    start = r16(2 * B * fmax * 8) + r16(2 * B * 8)
    return ws[start:start + B * fmax * 4].view(torch.float32).view(B, fmax)


def ctc_fwd(logits: Tensor, frame_len: Tensor, targets: Tensor, V: int, blank: int, eos: int):
    """F.ctc_loss(log_softmax(logits), ..., blank, reduction="mean", zero_infinity=True) on logits [B, Fmax, ldv >= V]; targets int64 [B, T], each
    row's labels end in front of its first `blank` or `eos` (omr_ctc_fwd) -> (loss fp32 [1], rows fp32 [B] = the samples' nll, 0 where
    infeasible, infeasible int32 [1], acc2 fp64 [2], the workspace omr_ctc_bwd reads)."""
    B, fmax, ldv = _ctc_logits(logits, frame_len, V)
    require_cuda(targets)
    assert targets.dtype == torch.int64 and targets.is_contiguous() and targets.dim() == 2 and targets.shape[0] == B
    T = targets.shape[1]
    dev = logits.device
    ws = torch.empty(ctc_workspace_bytes(B, fmax, T, V), dtype=torch.uint8, device=dev)
    acc2 = torch.empty(2, dtype=torch.float64, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    rows = torch.empty(B, dtype=torch.float32, device=dev)
    infeasible = torch.empty(1, dtype=torch.int32, device=dev)
    lib().call("omr_ctc_fwd", dtype_code(logits.dtype), ptr(logits), ldv, ptr(frame_len), ptr(targets), ptr(ws), ptr(acc2), ptr(loss), ptr(rows),
               ptr(infeasible), B, fmax, T, V, blank, eos, cur_stream())
    return loss, rows, infeasible, acc2, ws


def ctc_bwd(logits: Tensor, frame_len: Tensor, targets: Tensor, ws: Tensor, V: int, blank: int, grad_scale: float = 1.0,
            grad_out: Optional[Tensor] = None) -> Tensor:
    """dlogits of ctc_fwd (omr_ctc_bwd), in the logits' dtype and pitch; the view of the logits' own columns is returned."""
    B, fmax, ldv = _ctc_logits(logits, frame_len, V)
    require_cuda(targets, ws, grad_out)
    if grad_out is not None:
        assert grad_out.dtype == torch.float32 and grad_out.numel() == 1
    dl = torch.empty((B, fmax, ldv), dtype=logits.dtype, device=logits.device)
    lib().call("omr_ctc_bwd", dtype_code(logits.dtype), ptr(logits), ldv, ptr(frame_len), ptr(targets), ptr(ws), ptr(dl), B, fmax, targets.shape[1], V,
               blank, float(grad_scale), ptr(grad_out), cur_stream())
    return dl[:, :, :logits.shape[2]]


def ctc_greedy(logits: Tensor, frame_len: Tensor, V: int, blank: int):
    """Best-path transcript of logits [B, Fmax, ldv >= V] (omr_ctc_greedy) -> (tokens int32 [B, Fmax], lengths int32 [B], each frame's arg-max
    column int32 [B, Fmax] and its value fp32 [B, Fmax]), all on the device."""
    B, fmax, ldv = _ctc_logits(logits, frame_len, V)
    new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=logits.device)  # noqa: E731
    arg, val, tokens, lengths = new(torch.int32, B, fmax), new(torch.float32, B, fmax), new(torch.int32, B, fmax), new(torch.int32, B)
    lib().call("omr_ctc_greedy", dtype_code(logits.dtype), ptr(logits), ldv, ptr(frame_len), ptr(arg), ptr(val), ptr(tokens), ptr(lengths), B, fmax, V,
               blank, cur_stream())
    return tokens, lengths, arg, val


# ------------------------------------------------------------------------------------------------ CTC prefix scores (csrc/ctc_prefix.hip)

def check_ctc_decode(weight) -> float:
    """The range of `ctc_decode` (the CTC weight of the joint beam search): a number strictly between 0 and 1, also as the fp32 the kernels mix
    with; refused here, before anything is encoded, allocated or launched."""
    if isinstance(weight, bool) or not isinstance(weight, (int, float)):
        raise ValueError(f"ctc_decode must be a number, got {weight!r}")
    weight = float(weight)
    lam32 = ctypes.c_float(weight).value
    if not (0.0 < weight < 1.0 and 0.0 < lam32 < 1.0):
        raise ValueError(f"ctc_decode must lie strictly between 0.0 and 1.0, got {weight}")
    return weight


def ctc_mix_weights(weight: float) -> Tuple[float, float]:
    """(wa, wc) as omr_beam_select_ctc rounds them: wc = (float)weight, wa = (float)(1 - (double)wc); both exactly representable in fp32."""
    wc = ctypes.c_float(weight).value
    return ctypes.c_float(1.0 - wc).value, wc


class _CtcBeamDesc(ctypes.Structure):
    """omr_ctc_beam_desc of include/omr_hip.h."""
    WS_FIELDS = ("lse", "state0", "state1", "last0", "last1", "logpsi", "cand_tok", "cand_val", "advanced")
    _fields_ = [(n, ctypes.c_int) for n in ("dtype", "N", "beam", "V", "Fmax", "blank", "sos", "eos")] + [("ldv", ctypes.c_long), ("lam", ctypes.c_float)] + [
        (n, ctypes.c_void_p) for n in ("logits", "frame_len", "ws")] + [("ws_bytes", ctypes.c_long)] + [(n, ctypes.c_void_p) for n in WS_FIELDS]


class CtcPrefixBlock:
    """The CTC side of a joint beam search over N inputs of `beam` rows each (include/omr_hip.h, omr_ctc_beam_desc): the head's logits
    [N, Fmax, >= V] (kept alive here), one device block with the frames' lse, the two parities of the hypotheses' gn / gb rows, their last
    tokens and logpsi, and the descriptor.  Creating it runs omr_ctc_prefix_init: every row holds the empty hypothesis in parity 0."""

    def __init__(self, logits: Tensor, frame_len: Tensor, V: int, beam: int, blank: int, sos: int, eos: int, weight: float):
        self.weight = check_ctc_decode(weight)
        N, fmax, ldv = _ctc_logits(logits, frame_len, V)
        self.N, self.beam, self.rows, self.fmax, self.V = N, beam, N * beam, fmax, V
        self.logits, self.frame_len = logits, frame_len
        d = self.desc = _CtcBeamDesc()
        d.dtype, d.N, d.beam, d.V, d.Fmax, d.blank, d.sos, d.eos = dtype_code(logits.dtype), N, beam, V, fmax, blank, sos, eos
        d.ldv, d.lam, d.logits, d.frame_len, d.ws = ldv, self.weight, logits.data_ptr(), frame_len.data_ptr(), None
        nbytes = lib().query("omr_ctc_beam_workspace_bytes", ctypes.byref(d))
        if nbytes <= 0:
            raise ValueError(f"the CTC prefix state takes N >= 1, Fmax >= 1 and 1 <= beam <= 8, got N = {N}, Fmax = {fmax}, beam = {beam}")
        self._off = {n: int(getattr(d, n) or 0) for n in _CtcBeamDesc.WS_FIELDS}          # ws == NULL: the fields are offsets
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=logits.device)
        d.ws, d.ws_bytes = self.ws.data_ptr(), nbytes
        if lib().query("omr_ctc_beam_workspace_bytes", ctypes.byref(d)) != nbytes:
            raise RuntimeError("libomr_hip: omr_ctc_beam_workspace_bytes changed its answer")
        lib().call("omr_ctc_prefix_init", ctypes.byref(d), cur_stream())

    def byref(self):
        return ctypes.byref(self.desc)

    def _view(self, name: str, dtype: torch.dtype, *shape: int) -> Tensor:
        n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        return self.ws[self._off[name]:self._off[name] + n].view(dtype).view(*shape)

    def lse(self) -> Tensor:
        """fp32 [N, Fmax] (frames >= F_n are not written)."""
        return self._view("lse", torch.float32, self.N, self.fmax)

    def state(self, parity: int) -> Tensor:
        """fp32 [rows, 2, Fmax]: every row's gn and gb of that parity (a view of the block)."""
        return self._view(f"state{parity}", torch.float32, self.rows, 2, self.fmax)

    def last(self, parity: int) -> Tensor:
        return self._view(f"last{parity}", torch.int32, self.rows)

    def logpsi(self) -> Tensor:
        return self._view("logpsi", torch.float32, self.rows)

    def advanced(self) -> Tensor:
        """int32 [N]: the advances that took each input since the block was initialised (in a search: the position at which it stopped)."""
        return self._view("advanced", torch.int32, self.N)

    def scores(self, parity: int, cand: Tensor, out: Optional[Tensor] = None) -> Tensor:
        """delta fp32 [rows, beam] of the candidates cand int64 [rows, beam] against the rows' hypotheses (omr_ctc_prefix_scores)."""
        require_cuda(cand, out)
        assert cand.dtype == torch.int64 and cand.is_contiguous() and tuple(cand.shape) == (self.rows, self.beam), tuple(cand.shape)
        if out is None:
            out = torch.empty((self.rows, self.beam), dtype=torch.float32, device=cand.device)
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (self.rows, self.beam)
        lib().call("omr_ctc_prefix_scores", self.byref(), parity, ptr(cand), ptr(out), cur_stream())
        return out

    def advance(self, parity: int, parents: Tensor, tokens: Tensor, scores: Optional[Tensor] = None, done: Optional[Tensor] = None) -> None:
        """New row i continues the LOCAL row parents[i] (int32 [rows]) of its input by tokens[i] (int64 [rows]): written into the other parity
        (omr_ctc_prefix_advance).  scores fp64 [rows] / done int32 [N] (both optional): dead rows and finished inputs are skipped."""
        require_cuda(parents, tokens, scores, done)
        assert parents.dtype == torch.int32 and parents.is_contiguous() and parents.numel() == self.rows
        assert tokens.dtype == torch.int64 and tokens.is_contiguous() and tokens.numel() == self.rows
        assert scores is None or (scores.dtype == torch.float64 and scores.is_contiguous() and scores.numel() == self.rows)
        assert done is None or (done.dtype == torch.int32 and done.is_contiguous() and done.numel() == self.N)
        lib().call("omr_ctc_prefix_advance", self.byref(), parity, ptr(parents), ptr(tokens), ptr(scores), ptr(done), cur_stream())
