"""Reference code for the ragged-batch path (csrc/extent.hip, the encoder's ragged route): plain torch on the CPU, fp64 where a
tolerance is taken from it.  Shared by tests/test_extent_refs_cpu.py (which pins it against the oracle encoder run on each cropped
sample) and the GPU tests of the kernels and of ragged training.

A ragged batch is B samples in one padded plane, sample b's content in the top-left sizes[b] = (h_b, w_b) corner.  THE invariant:
every activation is zero outside its sample's extent; then a 3x3 / pad-1 conv inside the extent reads what the sample run alone
reads (its zero padding), also for the strided layers with the out extent ceil(h / s)."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch
import torch.nn.functional as F

from oracle import ref_cpu as R

# the shapes of the issue: one full sample, one with odd sizes that are no multiples of 16 / 8, one smaller than a conv tile whose
# deepest map is 2 x 2
PLANE = (64, 96)
SIZES = ((64, 96), (37, 50), (17, 9))
IN_EPS = 1e-3


# ------------------------------------------------------------------------------------------------ extent arithmetic

def extent_levels(sizes: Sequence[Tuple[int, int]]) -> List[List[Tuple[int, int]]]:
    """[level][b] = (rows, columns): level 0 the pixel sizes, level i + 1 behind conv block i: ceil(previous / stride)."""
    levels = [[(int(h), int(w)) for h, w in sizes]]
    for sh, sw in R.CONV_STRIDES:
        levels.append([(-(-h // sh), -(-w // sw)) for h, w in levels[-1]])
    return levels


def conv_out_brute(n: int, s: int) -> int:
    """Number of outputs of a k = 3, pad = 1, stride s conv over n inputs, by enumeration: outputs o whose window centre s * o is an input."""
    return sum(1 for o in range(n + 2) if s * o <= n - 1)


def inside_mask(shape_hw: Tuple[int, int], ext: Sequence[Tuple[int, int]]) -> torch.Tensor:
    """bool [B, H, W]: True inside sample b's extent."""
    H, W = shape_hw
    i = torch.arange(H).view(1, H, 1)
    j = torch.arange(W).view(1, 1, W)
    e = torch.tensor(list(ext))
    return (i < e[:, 0].view(-1, 1, 1)) & (j < e[:, 1].view(-1, 1, 1))


def zero_outside_nchw(x: torch.Tensor, ext) -> torch.Tensor:
    return torch.where(inside_mask(x.shape[2:], ext).unsqueeze(1), x, torch.zeros((), dtype=x.dtype))


def zero_outside_nhwc(x: torch.Tensor, ext) -> torch.Tensor:
    return torch.where(inside_mask(x.shape[1:3], ext).unsqueeze(-1), x, torch.zeros((), dtype=x.dtype))


def nan_outside_nhwc(x: torch.Tensor, ext) -> torch.Tensor:
    """The test inputs: NaN wherever a kernel must not look."""
    return torch.where(inside_mask(x.shape[1:3], ext).unsqueeze(-1), x, torch.full((), float("nan"), dtype=x.dtype))


# ------------------------------------------------------------------------------------------------ kernels (NHWC)

def extent_norm_fwd_ref(x: torch.Tensor, ext, eps: float = IN_EPS):
    """x NHWC (any float dtype; values outside the extents are not used) -> (y, mean [B, C], rstd [B, C]) in fp64: statistics over
    each sample's extent (biased variance), y = (x - mean) * rstd inside and 0 outside."""
    B, H, W, C = x.shape
    y = torch.zeros((B, H, W, C), dtype=torch.float64)
    mean = torch.zeros((B, C), dtype=torch.float64)
    rstd = torch.zeros((B, C), dtype=torch.float64)
    for b, (h, w) in enumerate(ext):
        c = x[b, :h, :w].double()
        mean[b] = c.mean((0, 1))
        var = ((c - mean[b]) ** 2).mean((0, 1))
        rstd[b] = 1.0 / torch.sqrt(var + eps)
        y[b, :h, :w] = (c - mean[b]) * rstd[b]
    return y, mean, rstd


def extent_norm_bwd_ref(g: torch.Tensor, x: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, ext, relu_mask: bool = False,
                        relu_scale: float = 1.0) -> torch.Tensor:
    """dx = rstd (g - mean_ext(g) - xhat mean_ext(g xhat)) inside [* (x > 0) * relu_scale], 0 outside, in fp64 with the SAVED mean /
    rstd the kernel is given (oracle.kernel_refs.in_bwd_ref over the extent)."""
    B, H, W, C = x.shape
    dx = torch.zeros((B, H, W, C), dtype=torch.float64)
    for b, (h, w) in enumerate(ext):
        xc, gc = x[b, :h, :w].double(), g[b, :h, :w].double()
        mu, rs = mean[b].double(), rstd[b].double()
        xhat = (xc - mu) * rs
        d = rs * (gc - gc.mean((0, 1)) - xhat * (gc * xhat).mean((0, 1)))
        if relu_mask:
            d = torch.where(xc > 0, d * relu_scale, torch.zeros_like(d))
        dx[b, :h, :w] = d
    return dx


def pack_rows(x: torch.Tensor, ext, smax: int) -> torch.Tensor:
    """[B, H, W, d] -> [B, smax, d] by indexing: row i * w_b + j of sample b = cell (i, j); rows >= h_b * w_b zero."""
    B, H, W, C = x.shape
    out = torch.zeros((B, smax, C), dtype=x.dtype)
    for b, (h, w) in enumerate(ext):
        out[b, :h * w] = x[b, :h, :w].reshape(h * w, C)
    return out


def pack_row_map_brute(ext_b: Tuple[int, int]) -> dict:
    """{row of the packed memory: (i, j)} of one sample, cell by cell: the order of x.flatten(2) of the sample's own grid (model.py:147)."""
    h, w = ext_b
    rows, r = {}, 0
    for i in range(h):
        for j in range(w):
            rows[r] = (i, j)
            r += 1
    return rows


# ------------------------------------------------------------------------------------------------ the masked encoder (NCHW, fp64)

def _norm_nchw(x: torch.Tensor, ext) -> torch.Tensor:
    return extent_norm_fwd_ref(x.permute(0, 2, 3, 1), ext)[0].permute(0, 3, 1, 2).to(x.dtype)


def masked_conv_block(sd, p: str, x: torch.Tensor, stride, ext_in, ext_out) -> torch.Tensor:
    """oracle.ref_cpu.conv_block (eval mode) on a padded batch: every conv followed by the zeroing, the norm over the extent."""
    x = zero_outside_nchw(F.relu(F.conv2d(x, sd[p + "conv1.weight"], sd[p + "conv1.bias"], padding=1)), ext_in)
    x = zero_outside_nchw(F.relu(F.conv2d(x, sd[p + "conv2.weight"], sd[p + "conv2.bias"], padding=1)), ext_in)
    x = _norm_nchw(x, ext_in)
    return zero_outside_nchw(F.relu(F.conv2d(x, sd[p + "conv3.weight"], sd[p + "conv3.bias"], padding=1, stride=stride)), ext_out)


def masked_depth_sep(sd, p: str, x: torch.Tensor, ext) -> torch.Tensor:
    x = zero_outside_nchw(F.conv2d(x, sd[p + "depth_conv.weight"], sd[p + "depth_conv.bias"], padding=1, groups=x.shape[1]), ext)
    return zero_outside_nchw(F.conv2d(x, sd[p + "point_conv.weight"], sd[p + "point_conv.bias"]), ext)


def masked_dsc_block(sd, p: str, x: torch.Tensor, ext) -> torch.Tensor:
    x = zero_outside_nchw(F.relu(masked_depth_sep(sd, p + "conv1.", x, ext)), ext)
    x = zero_outside_nchw(F.relu(masked_depth_sep(sd, p + "conv2.", x, ext)), ext)
    return masked_depth_sep(sd, p + "conv3.", _norm_nchw(x, ext), ext)


def masked_encoder(sd, p: str, x: torch.Tensor, sizes, strides=R.CONV_STRIDES, out_extent_of=None) -> torch.Tensor:
    """oracle.ref_cpu.encoder (eval mode) over a padded batch x [B, 1, H, W] (any pad value) with per-sample pixel sizes: the
    written-out form of the ragged route.  out_extent_of(extent, stride) overrides the stride rule (the CPU test breaks it on purpose)."""
    rule = out_extent_of or (lambda n, s: -(-n // s))
    ext = [(int(h), int(w)) for h, w in sizes]
    x = zero_outside_nchw(x, ext)
    for i, s in enumerate(strides):
        nxt = [(rule(h, s[0]), rule(w, s[1])) for h, w in ext]
        x = masked_conv_block(sd, f"{p}conv_blocks.{i}.", x, s, ext, nxt)
        ext = nxt
    for i in range(4):
        xt = masked_dsc_block(sd, f"{p}dscblocks.{i}.", x, ext)
        x = x + xt if x.shape == xt.shape else xt
    return x
