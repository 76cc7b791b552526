"""Float64 references, the exact-sum argument, a mirror of the launchers' grid arithmetic and the shared case table for the
convolution kernels (csrc/conv3x3_mfma.h, conv.hip, conv_wgrad_dma.hip, conv_bwd_fused.hip, conv1.hip, dwconv.hip).

tests/test_conv_branches_gpu.py runs every case below through the HIP kernels; tests/test_conv_refs_cpu.py runs the same cases
with torch CPU fp32 / bf16 arithmetic standing in for the kernels, which shows without a GPU that a correct implementation
passes every check and that a list of subtly wrong ones does not.

Most cases are EXACT: every operand is a small integer (or a dyadic fraction), so every product and every partial sum is a
multiple of `unit` below 2^24 * unit, fp32 accumulation is exact in any order (MFMA chains, per-thread partials, atomics) and the
output must equal the fp64 result, rounded once to the output type, bit for bit.  `assert_exact` checks that and, through
`assert_sums_fit`, the < 2^24 condition itself.  A few BOUNDED cases with real-valued operands check what integers cannot
(fp32 accumulation, one rounding of the output, the rounding of a normalised operand) against a per-element bound
(`gemm_bound`; derivation in DESIGN.md, "Convolution branch coverage").

Every conv kernel is persistent: a workgroup walks tiles with stride gridDim.x.  The `*_plan` functions restate each launcher's
grid arithmetic with the occupancy replaced by an upper bound, so a test can assert that its busiest workgroup really walks
several tiles (and crosses an image boundary) instead of passing for the wrong reason.

Test infrastructure only: nothing here is imported by the package.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle.kernel_refs import BF16, F32, U24, VEC, bits, drop_keep_np, f32_scalar, rnd, round_up

U8 = 2.0 ** -8                               # bf16 unit roundoff
NAN = float("nan")
NUM_CU = 256                                 # csrc/launch_setup.h:6
LDS_BYTES = 160 * 1024                       # LDS of a CU: what bounds the resident workgroups from above
TW = 32                                      # csrc/conv3x3_mfma.h:12 (every tile of the family is 32 output columns wide)
DROP_P, DROP_SEED = 0.5, 2 ** 33 + 12345     # p = 0.5: the scale 1 / (1 - p) = 2 keeps integers exact


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def out_hw(H: int, W: int, stride) -> Tuple[int, int]:
    return cdiv(H, stride[0]), cdiv(W, stride[1])


# ================================================================================================ operands

def ints(shape, seed: int, lo: int, hi: int) -> torch.Tensor:
    """Integers of [lo, hi] as fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def guarded(t: torch.Tensor, dtype=None) -> torch.Tensor:
    """`t` (as `dtype`) as the interior slice of a NaN-filled buffer with one image (the leading index) of NaN in front and one
    behind: a kernel that reads outside its operand meets a NaN.  The guards are multiples of 64 elements, so the view keeps the
    16-byte alignment of its buffer."""
    t = t.to(dtype) if dtype is not None else t
    guard = round_up(max(t[0].numel() if t.dim() > 1 else t.numel(), 1), 64)
    buf = torch.full((2 * guard + t.numel(),), NAN, dtype=t.dtype)
    view = buf[guard:guard + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def on_device(t: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    """A fresh device copy of the whole buffer behind the view `t`, viewed the same way (the NaN guards travel along)."""
    if t is None:
        return None
    base = t._base if t._base is not None else t
    return base.to(device).as_strided(t.shape, t.stride(), t.storage_offset())


def stats_pair(B: int, C: int, seed: int):
    """(mean, rstd) fp32 [B, C] with integer means and rstd of {0.5, 1, 2}: (x - mean) * rstd and fmaf(x, rstd, -mean * rstd) are
    exact.  Every image and channel has its own pair, so the statistics of a neighbouring image or channel give another result."""
    mean = ints((B, C), seed, -1, 1)
    rstd = torch.tensor([0.5, 1.0, 2.0])[ints((B, C), seed + 1, 0, 2).long()]
    return guarded(mean), guarded(rstd)


# ================================================================================================ definitions (fp64 / fp32)

def nchw(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 3, 1, 2)


def nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 3, 1)


def conv_def(x: torch.Tensor, w: torch.Tensor, stride=(1, 1), dil=(1, 1), out: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """3x3 conv from the definition, NHWC in and out, in x's precision: out[b, oh, ow, n] = sum over taps and channels of
    w[n, kh, kw, c] * xv[b, oh * sh - 1 + kh, ow * sw - 1 + kw, c], where xv is x with dil - 1 zeros between its pixels (the data
    gradient of a strided conv reads its operand so) and zero outside."""
    B, Hr, Wr, C = x.shape
    xv = nchw(x)
    if tuple(dil) != (1, 1):
        z = x.new_zeros((B, C, (Hr - 1) * dil[0] + 1, (Wr - 1) * dil[1] + 1))
        z[:, :, ::dil[0], ::dil[1]] = xv
        xv = z
    Ho, Wo = out if out is not None else out_hw(xv.shape[2], xv.shape[3], stride)
    pb = max((Ho - 1) * stride[0] + 2 - xv.shape[2], 0)
    pr = max((Wo - 1) * stride[1] + 2 - xv.shape[3], 0)
    y = F.conv2d(F.pad(xv, (1, pr, 1, pb)), nchw(w), stride=tuple(stride))
    return nhwc(y[:, :, :Ho, :Wo])


def wgrad_def(x: torch.Tensor, dy: torch.Tensor, stride=(1, 1)) -> torch.Tensor:
    """Weight gradient of the 3x3 / pad 1 conv, [COUT, 3, 3, CIN], NHWC operands, in x's precision."""
    cout, cin = dy.shape[-1], x.shape[-1]
    g = torch.nn.grad.conv2d_weight(nchw(x).contiguous(), (cout, cin, 3, 3), nchw(dy).contiguous(), stride=tuple(stride), padding=1)
    return g.permute(0, 2, 3, 1).contiguous()


def dw_def(x: torch.Tensor, w9: torch.Tensor, flip: bool = False) -> torch.Tensor:
    """Depthwise 3x3 / pad 1, NHWC, w9 = [C, 9]; flip mirrors the taps (the data gradient)."""
    C = x.shape[-1]
    w = w9.view(C, 1, 3, 3)
    if flip:
        w = w.flip(2, 3)
    return nhwc(F.conv2d(nchw(x), w, padding=1, groups=C))


def dw_wgrad_def(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """Depthwise weight gradient [C, 9]: dw[c, kh * 3 + kw] = sum of dy[b, i, j, c] * x[b, i + kh - 1, j + kw - 1, c]."""
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    return torch.stack([(dy * xp[:, kh:kh + H, kw:kw + W]).sum(dim=(0, 1, 2)) for kh in range(3) for kw in range(3)], dim=1)


def flip_weights(w: torch.Tensor) -> torch.Tensor:
    """[COUT, 3, 3, CIN] -> [CIN, 3, 3, COUT] with mirrored taps: the weights of the data-gradient conv."""
    return w.flip(1, 2).permute(3, 1, 2, 0).contiguous()


def normalised(x: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor) -> torch.Tensor:
    B, C = mean.shape
    return (x - mean.view(B, 1, 1, C).to(x.dtype)) * rstd.view(B, 1, 1, C).to(x.dtype)


def keep_elem(shape, p: float = DROP_P, seed: int = DROP_SEED, pitch: Optional[int] = None) -> torch.Tensor:
    """Element-wise keep mask of an NHWC tensor: drop_keep of the flat index (csrc/omr_common.h).  pitch: a (wrong) row pitch."""
    B, H, W, C = shape
    if pitch is None:
        idx = np.arange(B * H * W * C)
    else:
        b, h, w_, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(C), indexing="ij")
        idx = (((b * H + h) * pitch + w_) * C + c).reshape(-1)
    return torch.from_numpy(drop_keep_np(seed, idx, p)).view(shape)


def keep_chan(shape, p: float = DROP_P, seed: int = DROP_SEED) -> torch.Tensor:
    B, H, W, C = shape
    return torch.from_numpy(drop_keep_np(seed, np.arange(B * C), p)).view(B, 1, 1, C).expand(shape)


# ================================================================================================ checks

def assert_sums_fit(x_abs: torch.Tensor, what: str, unit: float = 1.0) -> None:
    """The condition of the exactness argument: the largest sum of |products| a case can produce, in multiples of `unit`
    (the granularity of its operands' products), stays below 2^24."""
    top = float(x_abs.max()) / unit
    assert top < 2.0 ** 24, f"{what}: partial sums reach {top:.3g} units, not below 2^24: the case is not exact in fp32"


def assert_exact(got: torch.Tensor, exact64: torch.Tensor, dtype, what: str, tile: Optional[Tuple[int, int]] = None) -> None:
    """Bit equality of `got` with the fp64 result rounded once to `dtype`; reports the first differing index (NHWC for an
    activation) and, with tile = (TH, TW), the tile it lies in."""
    want = exact64.to(dtype)
    got = got.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{tuple(got.shape)} vs {want.dtype}{tuple(want.shape)}"
    bad = bits(got) != bits(want)
    if bad.any():
        idx = tuple(int(v) for v in bad.nonzero()[0])
        where = f"index {idx}"
        if tile is not None and len(idx) == 4:
            where += f" (tile row {idx[1] // tile[0]}, tile column {idx[2] // tile[1]}, row {idx[1] % tile[0]} / column {idx[2] % tile[1]} inside it)"
        if len(idx) == 4 and got.shape[1:3] == (3, 3):
            where = f"index {idx} (cout {idx[0]}, tap ({idx[1]}, {idx[2]}), cin {idx[3]})"
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result, first at {where}: "
                             f"{got[idx].item()!r} vs {want[idx].item()!r}")


def gemm_bound(K: int, sum_abs: torch.Tensor, ref: torch.Tensor, out_dtype, extra: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-element bound of a K-term fp32 sum of products whose result is rounded to out_dtype: 4 (K + 2) 2^-24 sum|a||b|
    for the accumulation in any order, 2^-8 |ref| for a rounding to bf16, plus `extra` for the roundings a kernel adds."""
    b = 4.0 * (K + 2) * U24 * sum_abs + (U8 if out_dtype == BF16 else U24) * ref.abs()
    return b if extra is None else b + extra


def ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str) -> float:
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    r = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"{what}: error / bound = {r:.3g}")
    return r


def assert_bounded(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str) -> float:
    r = ratio(got, ref, bound, what)
    assert r <= 1.0, f"{what}: error / bound = {r:.3g}"
    return r


# ================================================================================================ conv3x3_mfma: forward + data gradient

@dataclass(frozen=True)
class ConvCase:
    """One omr_conv3x3_fwd call.  (H, W) is the tensor the kernel READS: the input of a forward conv, or (with dil = the conv's
    stride, out = the conv's input size and flipped weights) the output gradient of a data-gradient call."""
    name: str
    dtype: torch.dtype
    B: int
    H: int
    W: int
    cin: int
    cout: int
    stride: Tuple[int, int] = (1, 1)
    dil: Tuple[int, int] = (1, 1)
    out: Optional[Tuple[int, int]] = None
    bias: bool = False
    relu: bool = False
    norm: bool = False                       # in_stats: normalise on load
    mask: float = 0.0                        # out_mask with this mask_scale (0: none)
    drop: Optional[str] = None               # elem | chan
    stat_mode: int = 0
    stat_slots: int = 0                      # 0: omr_conv3x3_stat_slots; n > 0: that many (the launcher clamps the grid to it); -1: tiles + 3 (spare slots)
    min_tiles: int = 1                       # tiles the busiest workgroup must walk (asserted from conv_plan)
    real: bool = False                       # bounded case with real-valued operands

    @property
    def out_hw(self) -> Tuple[int, int]:
        if self.out is not None:
            return self.out
        return out_hw((self.H - 1) * self.dil[0] + 1, (self.W - 1) * self.dil[1] + 1, self.stride)


def _conv_cases():
    C = ConvCase
    stat = (
        # fused epilogues through several tiles per workgroup: stat_slots clamps the grid.  3 tile rows x 3 tile columns of 8 x 32,
        # ragged both ways (19 = 2 * 8 + 3, 70 = 2 * 32 + 6), two images
        C("epi1-bf16-slots1", BF16, 2, 19, 70, 16, 16, bias=True, relu=True, stat_mode=1, stat_slots=1, min_tiles=9),
        C("epi1-bf16-slots2", BF16, 2, 19, 70, 32, 32, bias=True, relu=True, stat_mode=1, stat_slots=2, min_tiles=5),
        C("epi1-bf16-spare-slots", BF16, 2, 19, 70, 16, 32, bias=True, stat_mode=1, stat_slots=-1),
        C("epi1-f32-slots1", F32, 2, 19, 70, 16, 16, bias=True, relu=True, stat_mode=1, stat_slots=1, min_tiles=9),
        C("epi1-f32-slots2-cin32", F32, 2, 19, 70, 32, 40, bias=True, stat_mode=1, stat_slots=2, min_tiles=5),      # fp32 partly filled NT = 64
        C("epi1-bf16-s22-slots1", BF16, 2, 19, 135, 32, 32, stride=(2, 2), relu=True, stat_mode=1, stat_slots=1, min_tiles=9),
        C("epi1-bf16-norm-slots2", BF16, 2, 19, 70, 16, 16, norm=True, bias=True, stat_mode=1, stat_slots=2, min_tiles=5),
        C("epi3-elem-slots1", BF16, 2, 19, 70, 16, 16, bias=True, relu=True, drop="elem", stat_mode=1, stat_slots=1, min_tiles=9),
        C("epi3-elem-slots2-cout64", BF16, 2, 19, 70, 32, 64, bias=True, relu=True, drop="elem", stat_mode=1, stat_slots=2, min_tiles=5),
        C("epi3-chan-slots1", BF16, 2, 19, 70, 16, 32, bias=True, relu=True, drop="chan", stat_mode=1, stat_slots=1, min_tiles=9),
        C("epi3-chan-slots2-f32", F32, 2, 19, 70, 16, 16, bias=True, relu=True, drop="chan", stat_mode=1, stat_slots=2, min_tiles=5),
        C("epi3-elem-f32-slots1", F32, 2, 19, 70, 16, 16, relu=True, drop="elem", stat_mode=1, stat_slots=1, min_tiles=9),
        C("epi2-mode2-slots1", BF16, 2, 19, 70, 16, 16, stat_mode=2, stat_slots=1, min_tiles=9),
        C("epi2-mode2-slots2-cin64", BF16, 2, 19, 70, 64, 32, stat_mode=2, stat_slots=2, min_tiles=5),
        C("epi2-mode2-f32-slots1", F32, 2, 19, 70, 16, 16, stat_mode=2, stat_slots=1, min_tiles=9),
        C("epi2-mode2-s22-slots2", BF16, 2, 10, 35, 32, 32, dil=(2, 2), out=(19, 70), stat_mode=2, stat_slots=2, min_tiles=5),     # SUBPIX data gradient
        C("epi2-mode2-spare-slots", BF16, 2, 19, 70, 32, 16, stat_mode=2, stat_slots=-1),
        C("epi2-mode4-slots1", BF16, 2, 19, 70, 16, 16, stat_mode=4, stat_slots=1, min_tiles=9),
        C("epi2-mode4-slots2-f32", F32, 2, 19, 70, 16, 16, stat_mode=4, stat_slots=2, min_tiles=5),
        C("epi2-mode4-s21-slots1", BF16, 2, 10, 70, 32, 32, dil=(2, 1), out=(19, 70), stat_mode=4, stat_slots=1, min_tiles=9),
        # mode 5: integers up to the InstanceNorm-backward formula, which is bounded (a division by Ho * Wo)
        C("epi2-mode5-slots1", BF16, 2, 19, 70, 16, 16, relu=True, mask=2.0, stat_mode=5, stat_slots=1, min_tiles=9),
        C("epi2-mode5-slots2-f32", F32, 2, 19, 70, 16, 16, stat_mode=5, stat_slots=2, min_tiles=5),
    )
    # no statistics: only the batch brings the grid below the tile count.  gx <= ceil(256 * occupancy bound / (ny * B)).
    walk = (
        C("epi0-c16-single", BF16, 400, 25, 34, 16, 16, bias=True, relu=True, min_tiles=3),                   # SINGLE, CK = 16
        C("epi0-c32-single-mask", BF16, 300, 25, 34, 32, 32, mask=2.0, min_tiles=3),                          # SINGLE, CK = 32, out_mask
        C("epi0-c64-two-chunks", BF16, 128, 49, 34, 64, 32, bias=True, min_tiles=3),                           # !SINGLE, two chunks of 32
        C("epi0-c48-three-chunks", BF16, 128, 49, 34, 48, 48, bias=True, relu=True, min_tiles=3),              # CK = KS = 16, three chunks; NT = 64 with 48 couts
        C("epi0-c128-norm-max", BF16, 86, 49, 34, 128, 64, norm=True, min_tiles=3),                           # four chunks, CIN = NORM_MAX
        C("f32-c16-nostat", F32, 200, 25, 34, 16, 16, bias=True, relu=True, min_tiles=3),                     # fp32 has no EPI 0: EPI 1 with the features off
        C("f32-c32-two-chunks-cout40", F32, 128, 33, 34, 32, 40, bias=True, min_tiles=3),                      # fp32 CK = 16: two chunks
        # strides: odd and even H, W; the last output row / column of an even size sees one input row / column less
        C("s22-odd-c32-norm", BF16, 256, 27, 67, 32, 32, stride=(2, 2), norm=True, relu=True, min_tiles=3),
        C("s22-even-c64", BF16, 128, 40, 66, 64, 64, stride=(2, 2), bias=True, min_tiles=3),
        C("s21-odd-c32", BF16, 640, 19, 34, 32, 32, stride=(2, 1), min_tiles=3),
        C("s21-even-c128-norm", BF16, 64, 56, 34, 128, 128, stride=(2, 1), norm=True, min_tiles=3),
        C("s21-f32-odd", F32, 640, 19, 34, 16, 16, stride=(2, 1), bias=True, min_tiles=3),
        C("s22-f32-even", F32, 200, 40, 66, 16, 16, stride=(2, 2), min_tiles=3),
        # data gradients: dil = the conv's stride; (2, 2) stages the real pixels only (SUBPIX), (2, 1) skips dead tap rows (row_live)
        C("d22-odd-c32-mask", BF16, 200, 17, 17, 32, 32, dil=(2, 2), out=(33, 34), mask=2.0, min_tiles=3),
        C("d22-even-c64", BF16, 128, 25, 17, 64, 64, dil=(2, 2), out=(50, 34), min_tiles=3),
        C("d22-odd-in-c16", BF16, 400, 13, 17, 16, 16, dil=(2, 2), out=(25, 33), min_tiles=3),
        C("d21-odd-c32", BF16, 200, 17, 34, 32, 32, dil=(2, 1), out=(33, 34), min_tiles=3),
        C("d21-even-c128", BF16, 48, 25, 34, 128, 128, dil=(2, 1), out=(50, 34), min_tiles=3),
        C("d22-f32-even", F32, 200, 13, 17, 16, 16, dil=(2, 2), out=(26, 34), min_tiles=3),
        C("d21-f32-odd", F32, 200, 13, 34, 16, 16, dil=(2, 1), out=(25, 34), mask=2.0, min_tiles=3),
    )
    # channel counts that pass the guards (% VEC, % KS) and that the model does not use; one tile suffices
    width = (
        C("nt32-cout16", BF16, 2, 9, 33, 32, 16, bias=True, relu=True),
        C("nt64-cout48-bf16", BF16, 2, 9, 33, 32, 48, bias=True, relu=True, mask=2.0),
        C("nt64-cout40-f32", F32, 2, 9, 33, 16, 40, bias=True, relu=True, mask=2.0),
        C("norm-c128-f32", F32, 2, 9, 33, 128, 16, norm=True),
        C("cout8-bf16-drop", BF16, 3, 9, 33, 16, 8, relu=True, drop="elem"),
    )
    # real-valued operands, smallest multi-tile shape of the family
    real = (
        C("real-bf16-norm-mask", BF16, 2, 19, 70, 64, 32, norm=True, bias=True, relu=True, mask=1.25, stat_mode=1, stat_slots=1, min_tiles=9, real=True),
        C("real-bf16-mask", BF16, 2, 19, 70, 16, 16, bias=True, relu=True, mask=1.25, stat_mode=1, stat_slots=1, min_tiles=9, real=True),
        C("real-f32-bias", F32, 2, 19, 70, 32, 16, bias=True, stat_mode=1, stat_slots=1, min_tiles=9, real=True),
        C("real-bf16-d22", BF16, 2, 10, 35, 32, 32, dil=(2, 2), out=(19, 70), stat_mode=2, stat_slots=1, min_tiles=9, real=True),
    )
    return stat, walk, width, real


CONV_STAT_CASES, CONV_WALK_CASES, CONV_WIDTH_CASES, CONV_REAL_CASES = _conv_cases()
CONV_CASES = CONV_STAT_CASES + CONV_WALK_CASES + CONV_WIDTH_CASES + CONV_REAL_CASES


def conv_plan(c: ConvCase) -> dict:
    """Mirror of dispatch_conv / launch_conv3 (csrc/conv3x3_mfma.h:482-570): which instantiation a case reaches, its tile and an
    upper bound of its grid.  Resident workgroups per CU <= min(2048 / 256 threads, 160 KiB / dynamic LDS)."""
    vec = VEC[c.dtype]
    ks = 2 * vec                                                        # omr_common.h:48 KStep
    esz = 2 if c.dtype == BF16 else 4
    nt = 64 if c.cout > 32 else 32                                      # conv3x3_mfma.h:569
    strided = tuple(c.stride) != (1, 1)
    rpw = 1 if strided else 2                                           # :549-554
    ck = ks if strided or c.cin % (2 * ks) else 2 * ks
    single = c.cin == ck                                                # :540
    th = 4 * rpw
    subpix = tuple(c.dil) == (2, 2) and not strided and rpw == 2        # :40
    ih = ((th - 1) * c.stride[0] + 3 + 1) // 2 if subpix else (th - 1) * c.stride[0] + 3      # :41
    iw = ((TW - 1) * c.stride[1] + 3) // 2 if subpix else (TW - 1) * c.stride[1] + 3          # :42
    ckp, op = ck + vec, nt + vec
    xs = max(th * TW * op, ih * iw * ckp) if single else ih * iw * ckp                        # :488
    shm = (xs + nt * 9 * ckp) * esz                                                           # :491
    if not single:
        shm = max(shm, th * TW * op * esz)                                                    # :492
    Ho, Wo = c.out_hw
    tiles_h, tiles_w = cdiv(Ho, th), cdiv(Wo, TW)
    tiles = tiles_h * tiles_w
    epi = 2 if c.stat_mode in (2, 4, 5) else 3 if c.drop else 1 if c.stat_mode == 1 else 0    # :522
    if c.dtype == F32 and epi == 0:
        epi = 1 if tuple(c.dil) == (1, 1) else 2                                              # :523
    occ = min(2048 // 256, LDS_BYTES // shm)
    ny = cdiv(c.cout, nt)
    gx = min(cdiv(NUM_CU * occ, ny * c.B), tiles)                                             # :505-506
    slots = conv_slots(c, tiles)
    if c.stat_mode:
        gx = min(gx, slots)                                                                   # :509
    gx = max(gx, 1)
    return dict(nt=nt, ck=ck, single=single, th=th, subpix=subpix, shm=shm, tiles_h=tiles_h, tiles_w=tiles_w, tiles=tiles, epi=epi, gx_upper=gx,
                slots=slots, min_tiles=cdiv(tiles, gx), chunks=c.cin // ck)


def conv_slots(c: ConvCase, tiles: Optional[int] = None) -> int:
    """The stat_slots argument of a case.  0 in the table = omr_conv3x3_stat_slots (csrc/conv.hip:289)."""
    Ho, Wo = c.out_hw
    if c.stat_slots > 0:
        return c.stat_slots
    if c.stat_slots < 0:
        return (tiles if tiles is not None else conv_plan(c)["tiles"]) + 3
    return min(cdiv(Ho, 4) * cdiv(Wo, TW), cdiv(NUM_CU * 8, c.B))


@functools.lru_cache(maxsize=2)
def conv_inputs(c: ConvCase) -> Dict[str, torch.Tensor]:
    """CPU operands of a case in the compute dtype (cached, never modified)."""
    seed = 1000 + 17 * CONV_CASES.index(c)
    Ho, Wo = c.out_hw
    d: Dict[str, torch.Tensor] = {}
    if c.real:
        x = rnd((c.B, c.H, c.W, c.cin), seed)
        if c.norm:
            x = F.relu(x) * 3                                           # a ReLU output, as in the model; |xhat| of a few units
        w = rnd((c.cout, 3, 3, c.cin), seed + 1) * (2.0 / math.sqrt(9 * c.cin))
        bias = rnd((c.cout,), seed + 2)
        mean, rstd = 1.5 * rnd((c.B, c.cin), seed + 3, 0.2, 1.0), rnd((c.B, c.cin), seed + 4, 0.5, 2.0)
        d["mean"], d["rstd"] = guarded(mean), guarded(rstd)
    else:
        x = ints((c.B, c.H, c.W, c.cin), seed, -2, 2)
        w = ints((c.cout, 3, 3, c.cin), seed + 1, -1, 1)
        bias = ints((c.cout,), seed + 2, -3, 3)
        d["mean"], d["rstd"] = stats_pair(c.B, c.cin, seed + 3)
    d["x"], d["w"], d["bias"] = guarded(x, c.dtype), guarded(w, c.dtype), guarded(bias)
    d["mask"] = guarded(ints((c.B, Ho, Wo, c.cout), seed + 5, -1, 2), c.dtype)                 # kept where > 0: half of the elements
    d["stat_x"] = guarded(ints((c.B, Ho, Wo, c.cout), seed + 6, -2, 3), c.dtype)
    d["stat_mean"], d["stat_rstd"] = stats_pair(c.B, c.cout, seed + 7)
    # mode 5: the image's finished {sum g, sum g * xhat}, written by the test into the compact region behind the slots
    d["compact"] = (ints((c.B, c.cout, 2), seed + 9, -40, 40) * 7).double()
    return d


def _conv_common(c: ConvCase, inp, prec):
    """Operands in `prec` with the case's switches applied: (x or xhat, w, bias or None)."""
    x, w = inp["x"].to(prec), inp["w"].to(prec)
    if c.norm:
        x = normalised(x, inp["mean"], inp["rstd"])
    return x, w, (inp["bias"].to(prec) if c.bias else None)


def conv_ref(c: ConvCase) -> Dict[str, torch.Tensor]:
    """fp64 from the definition: y (before its rounding to the output type; for stat_mode 5 the applied InstanceNorm backward),
    sums [B, COUT, 2] of the statistics epilogue, and for the bounded cases the per-element bound of y."""
    inp = conv_inputs(c)
    x, w, bias = _conv_common(c, inp, torch.float64)
    B, (Ho, Wo) = c.B, c.out_hw
    acc = conv_def(x, w, c.stride, c.dil, c.out_hw)
    sum_abs = conv_def(x.abs(), w.abs(), c.stride, c.dil, c.out_hw)
    if bias is not None:
        acc, sum_abs = acc + bias, sum_abs + bias.abs()
    if not c.real:
        assert_sums_fit(sum_abs, c.name, 0.5 if c.norm else 1.0)        # rstd = 0.5: products are multiples of 1/2
    y = acc
    if c.relu and c.stat_mode < 4:
        y = y.clamp_min(0.0)
    scale = 1.0
    if c.mask and c.stat_mode < 4:
        scale *= float(f32_scalar(c.mask))
    shape = (B, Ho, Wo, c.cout)
    if c.drop:
        keep = keep_elem(shape) if c.drop == "elem" else keep_chan(shape)
        y = torch.where(keep, y * 2.0, 0.0)
    y = y * scale
    if c.mask and c.stat_mode < 4:
        y = torch.where(inp["mask"].double() > 0, y, 0.0)
    out = dict(y=y)
    K = 9 * c.cin + (1 if c.bias else 0)
    if c.real:
        extra = None
        if c.norm:                                                      # xhat is rounded to the operand type before the MFMA (conv3x3_mfma.h:265)
            u = U8 + 4 * U24 if c.dtype == BF16 else 2 * U24
            extra = u * conv_def(x.abs(), w.abs(), c.stride, c.dil, c.out_hw)
        assert not c.drop
        b = gemm_bound(K, sum_abs, acc, F32, extra)                     # the accumulator, then the epilogue's own roundings
        b = b * scale + (U24 * y.abs() if scale != 1.0 else 0.0)
        out["bound"] = b + (U8 * y.abs() if c.dtype == BF16 else 0.0)
    # the statistics epilogues sum the STORED output: exact cases round it first; a bounded case's stored value is within `bound` of y
    yr = y if c.real else y.to(c.dtype).double()
    n = Ho * Wo
    if c.stat_mode == 1:
        out["sums"] = torch.stack([yr.sum(dim=(1, 2)), (yr * yr).sum(dim=(1, 2))], dim=-1)
        if not c.real:
            assert_sums_fit(out["sums"].abs(), c.name + " statistics")
        else:
            bd = out["bound"]
            out["sums_bound"] = torch.stack([bd.sum(dim=(1, 2)) + 4 * (n + 2) * U24 * y.abs().sum(dim=(1, 2)),
                                             (2 * y.abs() * bd + bd * bd).sum(dim=(1, 2)) + 4 * (n + 2) * U24 * (y * y).sum(dim=(1, 2))], dim=-1)
    elif c.stat_mode in (2, 4):
        xh = normalised(inp["stat_x"].double(), inp["stat_mean"], inp["stat_rstd"])
        out["sums"] = torch.stack([yr.sum(dim=(1, 2)), (yr * xh).sum(dim=(1, 2))], dim=-1)
        if not c.real:
            assert_sums_fit(torch.stack([yr.abs().sum(dim=(1, 2)), (yr * xh).abs().sum(dim=(1, 2))]), c.name + " statistics", 0.5)
        else:
            bd = out["bound"]
            out["sums_bound"] = torch.stack([bd.sum(dim=(1, 2)) + 4 * (n + 2) * U24 * y.abs().sum(dim=(1, 2)),
                                             (bd * xh.abs()).sum(dim=(1, 2)) + 4 * (n + 2) * U24 * (y * xh).abs().sum(dim=(1, 2))], dim=-1)
    elif c.stat_mode == 5:
        # dx = rstd * (g - s1 - xhat * s2) [* (stat_x > 0) * mask_scale], s1 / s2 = the fp32 values of sums / (Ho * Wo) (conv3x3_mfma.h:199, :458)
        assert float(yr.abs().max()) <= 256, "mode 5 case: g must be exact in bf16"
        sx = inp["stat_x"].double()
        xh = normalised(sx, inp["stat_mean"], inp["stat_rstd"])
        s = (inp["compact"] * (1.0 / (Ho * Wo))).float().double().view(B, 1, 1, c.cout, 2)
        rs = inp["stat_rstd"].double().view(B, 1, 1, c.cout)
        d = rs * (yr - s[..., 0] - xh * s[..., 1])
        mag = rs * (yr.abs() + s[..., 0].abs() + (xh * s[..., 1]).abs())
        if c.relu:
            d = torch.where(sx > 0, d * c.mask, 0.0)
            mag = mag * c.mask
        out["y"] = d
        # four fp32 roundings (product, two differences, the ReLU scale), each of a value no larger than mag, then the output's own
        out["bound"] = 4 * U24 * mag + (U8 if c.dtype == BF16 else U24) * d.abs()
    return out


def conv_standin(c: ConvCase, variant: Optional[str] = None) -> Dict[str, Optional[torch.Tensor]]:
    """What a correct kernel computes, with torch CPU fp32 arithmetic and the kernel's roundings (the normalised operand and the output
    are rounded to the compute type; element-wise dropout and the mask act on the rounded value).  `variant` names a defect."""
    inp = conv_inputs(c)
    T = c.dtype
    B, (Ho, Wo) = c.B, c.out_hw
    p = conv_plan(c)
    x, w = inp["x"].float(), inp["w"].float()
    if c.norm:
        x = normalised(x, inp["mean"], inp["rstd"]).to(T).float()
    acc = conv_def(x, w, c.stride, c.dil, c.out_hw)
    if variant == "norm_padding":                                       # the halo outside the image is normalised too: (0 - mean) * rstd
        assert c.norm and tuple(c.dil) == (1, 1)
        xp = normalised(F.pad(inp["x"].float(), (0, 0, 1, 1, 1, 1)), inp["mean"], inp["rstd"]).to(T).float()
        acc = nhwc(F.conv2d(nchw(xp), nchw(w), stride=tuple(c.stride)))[:, :Ho, :Wo].contiguous()

    def with_tap_zeroed(kh, kw):
        w2 = w.clone()
        if kh is None:
            w2[:, :, kw, :] = 0
        else:
            w2[:, kh, kw, :] = 0
        return conv_def(x, w2, c.stride, c.dil, c.out_hw)

    if variant == "tap_border":                                         # tap (1, 2) dropped on the left border column
        acc[:, :, 0] = with_tap_zeroed(1, 2)[:, :, 0]
    if variant == "halo_column":                                        # the last halo column of every tile but the last is lost
        cols = [j for j in range(TW - 1, Wo - 1, TW)]
        assert cols, "halo_column needs two tile columns"
        acc[:, :, cols] = with_tap_zeroed(None, 2)[:, :, cols]
    if variant == "stale_tile":                                         # tile 1 computed from the data staged for tile 0
        assert p["tiles_w"] >= 2
        n = min(TW, Wo - TW)
        acc[:, :p["th"], TW:TW + n] = acc[:, :p["th"], :n].clone()
    if c.bias:
        acc = acc + inp["bias"]
    v = acc
    if c.relu and c.stat_mode < 4:
        v = v.clamp_min(0.0)
    shape = (B, Ho, Wo, c.cout)
    scale = f32_scalar(c.mask) if (c.mask and c.stat_mode < 4) else None
    if c.drop == "chan":
        v = torch.where(keep_chan(shape), v * 2.0, 0.0)
    if scale is not None:
        v = (v.to(T).float() * scale) if variant == "mask_double_round" else v * scale
    y = v.to(T)
    if c.drop == "elem":
        keep = keep_elem(shape, pitch=p["tiles_w"] * TW if variant == "drop_pitch" else None)
        y = torch.where(keep, (y.float() * 2.0).to(T), torch.zeros_like(y))
    if scale is not None:
        y = torch.where(inp["mask"].float() > 0, y, torch.zeros_like(y))
    if variant == "skip_last_tile":                                     # the last tile of workgroup 0's walk is never computed
        gx = p["gx_upper"]
        last = (p["tiles"] - 1) // gx * gx
        r0, c0 = last // p["tiles_w"] * p["th"], last % p["tiles_w"] * TW
        y[:, r0:r0 + p["th"], c0:c0 + TW] = 0
    out: Dict[str, Optional[torch.Tensor]] = dict(y=y)
    yf = y.float()
    if c.stat_mode == 1:
        out["sums"] = torch.stack([yf.double().sum(dim=(1, 2)), (yf * yf).double().sum(dim=(1, 2))], dim=-1)
    elif c.stat_mode in (2, 4, 5):
        sx = inp["stat_x"].float()
        xh = normalised(sx, inp["stat_mean"], inp["stat_rstd"])
        if c.stat_mode == 5:
            s = (inp["compact"] * (1.0 / (Ho * Wo))).float().view(B, 1, 1, c.cout, 2)
            rs = inp["stat_rstd"].view(B, 1, 1, c.cout)
            d = rs * (yf - s[..., 0] - xh * s[..., 1])
            if c.relu:
                d = torch.where(sx > 0, d * f32_scalar(c.mask), 0.0)
            out["y"] = d.to(T)
        else:
            out["sums"] = torch.stack([yf.double().sum(dim=(1, 2)), (yf * xh).double().sum(dim=(1, 2))], dim=-1)
            if c.stat_mode == 4:
                out["y"] = None
    return out


def conv_check(c: ConvCase, y: Optional[torch.Tensor], sums: Optional[torch.Tensor]) -> None:
    """y: the kernel's output (None for stat_mode 4); sums [B, COUT, 2]: the per-image sums of the slots it filled."""
    ref = conv_ref(c)
    p = conv_plan(c)
    if c.stat_mode == 4:
        assert y is None
    elif "bound" in ref:
        assert_bounded(y, ref["y"], ref["bound"], f"{c.name} output")
    else:
        assert_exact(y, ref["y"], c.dtype, f"{c.name} output", tile=(p["th"], TW))
    if "sums" in ref:
        assert sums is not None
        if c.real:
            # each stored element is within its bound of y; summing the stored values adds the fp32 partial sums' roundings
            assert_bounded(sums, ref["sums"], ref["sums_bound"], f"{c.name} statistics sums")
        else:
            assert_exact(sums, ref["sums"], torch.float64, f"{c.name} statistics sums")


# ================================================================================================ weight gradients (3x3 and the first layer)

@dataclass(frozen=True)
class WgradCase:
    """One omr_conv3x3_wgrad call: x [B, H, W, cin], dy [B, Ho, Wo, cout], dw / db accumulated in place."""
    name: str
    dtype: torch.dtype
    B: int
    H: int
    W: int
    cin: int
    cout: int
    stride: Tuple[int, int] = (1, 1)
    norm: bool = False
    kernel: str = "dma"                      # dma | generic | conv1_mfma | conv1: the kernel the dispatch must reach (asserted from wgrad_plan)
    min_tiles: int = 1
    cross: bool = False                      # the busiest workgroup must cross an image boundary
    dy_off: int = 0                          # bytes: dy starts this far into a 16-byte aligned buffer (omr_conv1_wgrad's fall-back)
    real: bool = False


# pick() of csrc/conv_wgrad_dma.hip:371-393: (stride, cn, cc) -> (TH, NW, NSTAGE)
DMA_PICK = {
    ((1, 1), 64, 64): (8, 8, 2), ((1, 1), 64, 32): (8, 8, 2), ((1, 1), 32, 64): (8, 8, 2), ((1, 1), 32, 32): (8, 4, 2),
    ((1, 1), 32, 16): (8, 4, 2), ((1, 1), 16, 16): (8, 8, 6),
    ((2, 2), 64, 64): (2, 8, 3), ((2, 2), 32, 32): (4, 8, 3), ((2, 2), 16, 16): (8, 8, 3),
    ((2, 1), 64, 64): (4, 8, 2), ((2, 1), 32, 32): (8, 8, 2),
}


def _wgrad_cases():
    C = WgradCase
    dma = (
        # every row of pick(): the busiest workgroup walks >= NSTAGE + 2 tiles and crosses an image boundary
        C("dma-s11-64x64", BF16, 48, 41, 34, 128, 128, min_tiles=4, cross=True),
        C("dma-s11-64x64-tail40", BF16, 44, 41, 34, 40, 128, min_tiles=4, cross=True),           # channel tail: cvalid = 40 of a 64-wide tile
        C("dma-s11-64x32", BF16, 96, 41, 34, 32, 128, min_tiles=4, cross=True),
        C("dma-s11-32x64", BF16, 96, 41, 34, 128, 32, min_tiles=4, cross=True),                 # two cin-block columns: db has one owner
        C("dma-s11-32x32", BF16, 220, 41, 34, 32, 32, min_tiles=4, cross=True),
        C("dma-s11-32x32-tail24", BF16, 220, 41, 34, 24, 32, min_tiles=4, cross=True),          # cvalid = 24 of a 32-wide tile
        C("dma-s11-32x16", BF16, 220, 41, 34, 16, 32, min_tiles=4, cross=True),
        C("dma-s11-16x16", BF16, 2100, 5, 20, 16, 16, min_tiles=8, cross=True),                 # NSTAGE 6, PAIR: one-tile images, every ring slot another image
        C("dma-s11-16x16-norm", BF16, 2100, 5, 20, 16, 16, norm=True, min_tiles=8, cross=True), # the 8-slot statistics ring turns over
        C("dma-s22-64x64", BF16, 28, 21, 68, 128, 128, stride=(2, 2), min_tiles=5, cross=True),
        C("dma-s22-64x64-norm", BF16, 54, 21, 68, 64, 128, stride=(2, 2), norm=True, min_tiles=5, cross=True),
        C("dma-s22-32x32", BF16, 110, 37, 68, 32, 32, stride=(2, 2), min_tiles=5, cross=True),
        C("dma-s22-32x32-norm", BF16, 110, 37, 68, 32, 32, stride=(2, 2), norm=True, min_tiles=5, cross=True),
        C("dma-s22-16x16", BF16, 1300, 9, 40, 16, 16, stride=(2, 2), min_tiles=5, cross=True),
        C("dma-s21-64x64", BF16, 24, 41, 34, 128, 128, stride=(2, 1), min_tiles=4, cross=True),
        C("dma-s21-64x64-norm", BF16, 24, 41, 34, 128, 128, stride=(2, 1), norm=True, min_tiles=4, cross=True),
        C("dma-s21-32x32", BF16, 110, 81, 34, 32, 32, stride=(2, 1), min_tiles=4, cross=True),
        # NORM on the remaining rows (the statistics fetch and the in-LDS pass differ with CBC and the thread count)
        C("dma-s11-64x64-norm", BF16, 48, 41, 34, 128, 128, norm=True, min_tiles=4, cross=True),
        C("dma-s11-64x32-norm", BF16, 96, 41, 34, 32, 128, norm=True, min_tiles=4, cross=True),
        C("dma-s11-32x64-norm", BF16, 96, 41, 34, 128, 32, norm=True, min_tiles=4, cross=True),
        C("dma-s11-32x32-norm", BF16, 220, 41, 34, 32, 32, norm=True, min_tiles=4, cross=True),
        C("dma-s11-32x32-tail24-norm", BF16, 220, 41, 34, 24, 32, norm=True, min_tiles=4, cross=True),
        C("dma-s11-32x16-norm", BF16, 220, 41, 34, 16, 32, norm=True, min_tiles=4, cross=True),
        C("dma-s22-16x16-norm", BF16, 1300, 9, 40, 16, 16, stride=(2, 2), norm=True, min_tiles=5, cross=True),
        C("dma-s21-32x32-norm", BF16, 110, 81, 34, 32, 32, stride=(2, 1), norm=True, min_tiles=4, cross=True),
    )
    generic = (
        C("gen-f32-s11", F32, 16, 25, 34, 128, 128, kernel="generic", min_tiles=3, cross=True),
        C("gen-f32-s22-norm", F32, 16, 25, 68, 128, 128, stride=(2, 2), norm=True, kernel="generic", min_tiles=3, cross=True),
        C("gen-f32-s21", F32, 28, 25, 34, 128, 128, stride=(2, 1), kernel="generic", min_tiles=3, cross=True),
        C("gen-f32-c40-c24", F32, 96, 25, 34, 24, 40, kernel="generic", min_tiles=3, cross=True),          # both channel tails of the 64 x 32 block
        C("gen-bf16-s22-16x128", BF16, 64, 33, 68, 16, 128, stride=(2, 2), kernel="generic", min_tiles=3, cross=True),   # pick() has no (64, 16) row
    )
    conv1 = (
        C("c1-mfma", BF16, 20, 125, 637, 1, 16, kernel="conv1_mfma", min_tiles=4, cross=True),              # 20 x 16 x 20 = 6400 tiles > 3 x 2048
        C("c1-bf16-unaligned-dy", BF16, 2, 35, 70, 1, 16, kernel="conv1", dy_off=8),
        C("c1-f32", F32, 2, 35, 70, 1, 16, kernel="conv1"),
        C("c1-f32-cout32", F32, 3, 35, 70, 1, 32, kernel="conv1"),
        C("c1-bf16-cout32", BF16, 3, 35, 70, 1, 32, kernel="conv1"),
    )
    real = (
        C("real-dma-s11-32x32-norm", BF16, 220, 41, 34, 32, 32, norm=True, min_tiles=4, cross=True, real=True),
        C("real-gen-f32-s11", F32, 16, 25, 34, 128, 128, kernel="generic", min_tiles=3, cross=True, real=True),
    )
    return dma, generic, conv1, real


WGRAD_DMA_CASES, WGRAD_GENERIC_CASES, WGRAD_CONV1_CASES, WGRAD_REAL_CASES = _wgrad_cases()
WGRAD_CASES = WGRAD_DMA_CASES + WGRAD_GENERIC_CASES + WGRAD_CONV1_CASES + WGRAD_REAL_CASES


def _tile_dma_elems(cb: int, npixt: int) -> int:
    """TileDma<CB, NPIXT, .>::ELEMS (csrc/conv_wgrad_dma.hip:67-71)."""
    nch = (round_up(npixt, 8) if cb == 16 else round_up(npixt, 2)) * (cb // 8)
    return round_up(nch, 64) * 8


def wgrad_plan(c: WgradCase) -> dict:
    """Mirror of omr_conv3x3_wgrad (csrc/conv.hip:324-343), omr_wgrad_dma_bf16 / pick / launch (csrc/conv_wgrad_dma.hip:346-405),
    launch_wgrad3 (csrc/conv.hip:217-249) and omr_conv1_wgrad (csrc/conv1.hip:270-288)."""
    Ho, Wo = out_hw(c.H, c.W, c.stride)
    if c.cin == 1:
        if c.dtype == BF16 and c.cout == 16 and c.dy_off % 16 == 0:
            tiles_h, tiles_w = cdiv(c.H, 8), cdiv(c.W, 32)
            ntiles = c.B * tiles_h * tiles_w
            gx = min(ntiles, NUM_CU * 8)                                # exact: conv1.hip:274
            return dict(kernel="conv1_mfma", th=8, tiles_h=tiles_h, tiles_w=tiles_w, tiles_per_img=tiles_h * tiles_w, ntiles=ntiles, gx_upper=gx,
                        min_tiles=cdiv(ntiles, gx), cross=ntiles - gx >= tiles_h * tiles_w, ncb=1)
        return dict(kernel="conv1", th=1, tiles_h=c.H, tiles_w=1, tiles_per_img=c.H, ntiles=c.B * c.H, gx_upper=min(c.B * c.H, 64), min_tiles=1, cross=False, ncb=1)
    vec = VEC[c.dtype]
    assert c.cin % vec == 0 and c.cout % vec == 0
    cn = 64 if c.cout > 32 else 32 if c.cout > 16 else 16
    cc = 64 if c.cin > 32 else 32 if c.cin > 16 else 16
    sh, sw = c.stride
    if c.dtype == BF16 and (tuple(c.stride), cn, cc) in DMA_PICK:
        th, nw, nstage = DMA_PICK[(tuple(c.stride), cn, cc)]
        ih, iw = (th - 1) * sh + 3, (TW - 1) * sw + 3
        shm = nstage * (_tile_dma_elems(cn, th * TW) + _tile_dma_elems(cc, ih * iw)) * 2 + 1024 + (8 * 512 if c.norm else 0)      # :353
        threads, kernel, cbn, cbc = nw * 64, "dma", cn, cc
    else:
        th = {BF16: (8, 4), F32: (4, 2)}[c.dtype][0 if tuple(c.stride) == (1, 1) else 1]                                          # conv.hip:340-342
        cbn, cbc = (64, 64) if c.cout > 32 and c.cin > 32 else (64, 32) if c.cout > 32 else (32, 32)                               # conv.hip:238-240
        pad = 8 if c.dtype == BF16 else 4
        ih, iw = (th - 1) * sh + 3, (TW - 1) * sw + 3
        shm = (th * TW * (cbn + pad) + ih * iw * (cbc + pad)) * (2 if c.dtype == BF16 else 4)                                     # conv.hip:223
        threads, kernel, nstage = 256, "generic", 1
    tiles_h, tiles_w = cdiv(Ho, th), cdiv(Wo, TW)
    ntiles = c.B * tiles_h * tiles_w
    occ = min(2048 // threads, LDS_BYTES // shm)
    gy = cdiv(c.cout, cbn) * cdiv(c.cin, cbc)
    gx = max(min(cdiv(NUM_CU * occ, gy), ntiles), 1)                                                                              # conv_wgrad_dma.hip:363, conv.hip:231
    return dict(kernel=kernel, th=th, nstage=nstage, shm=shm, tiles_h=tiles_h, tiles_w=tiles_w, tiles_per_img=tiles_h * tiles_w, ntiles=ntiles,
                gx_upper=gx, min_tiles=cdiv(ntiles, gx), cross=ntiles - gx >= tiles_h * tiles_w, ncb=cdiv(c.cin, cbc), cbc=cbc, cbn=cbn)


@functools.lru_cache(maxsize=2)
def wgrad_inputs(c: WgradCase) -> Dict[str, torch.Tensor]:
    seed = 5000 + 13 * WGRAD_CASES.index(c)
    Ho, Wo = out_hw(c.H, c.W, c.stride)
    d: Dict[str, torch.Tensor] = {}
    if c.real:
        x, dy = rnd((c.B, c.H, c.W, c.cin), seed), rnd((c.B, Ho, Wo, c.cout), seed + 1)
        if c.norm:
            x = F.relu(x) * 3
        d["mean"], d["rstd"] = guarded(1.5 * rnd((c.B, c.cin), seed + 3, 0.2, 1.0)), guarded(rnd((c.B, c.cin), seed + 4, 0.5, 2.0))
    else:
        x, dy = ints((c.B, c.H, c.W, c.cin), seed, -2, 2), ints((c.B, Ho, Wo, c.cout), seed + 1, -1, 1)
        d["mean"], d["rstd"] = stats_pair(c.B, c.cin, seed + 3)
    d["x"] = guarded(x, c.dtype)
    if c.dy_off:
        e = c.dy_off // (2 if c.dtype == BF16 else 4)
        buf = torch.full((dy.numel() + 128,), NAN, dtype=c.dtype)
        d["dy"] = buf[e:e + dy.numel()].view(dy.shape)
        d["dy"].copy_(dy)
    else:
        d["dy"] = guarded(dy, c.dtype)
    # both gradients accumulate: they start from non-zero integers
    d["dw0"], d["db0"] = guarded(ints((c.cout, 3, 3, c.cin), seed + 5, -5, 5)), guarded(ints((c.cout,), seed + 6, -5, 5))
    return d


def wgrad_ref(c: WgradCase) -> Dict[str, torch.Tensor]:
    inp = wgrad_inputs(c)
    x, dy = inp["x"].double(), inp["dy"].double()
    if c.norm:
        x = normalised(x, inp["mean"], inp["rstd"])
    dw0, db0 = inp["dw0"].double(), inp["db0"].double()
    dw, db = dw0 + wgrad_def(x, dy, c.stride), db0 + dy.sum(dim=(0, 1, 2))
    sum_abs = dw0.abs() + wgrad_def(x.abs(), dy.abs(), c.stride)
    out = dict(dw=dw, db=db)
    if c.real:
        K = c.B * dy.shape[1] * dy.shape[2] + 1
        extra = None
        if c.norm:                                                      # xhat rounded to bf16 in LDS (conv_wgrad_dma.hip:262) / to T in registers (conv.hip:126)
            extra = (U8 + 4 * U24 if c.dtype == BF16 else 2 * U24) * wgrad_def(x.abs(), dy.abs(), c.stride)
        out["dw_bound"] = gemm_bound(K, sum_abs, dw, F32, extra)
        out["db_bound"] = gemm_bound(K, db0.abs() + dy.abs().sum(dim=(0, 1, 2)), db, F32)
    else:
        assert_sums_fit(sum_abs, c.name, 0.5 if c.norm else 1.0)
    return out


def wgrad_standin(c: WgradCase, variant: Optional[str] = None):
    """torch CPU fp32 in the kernels' place: xhat rounded to the compute type, fp32 sums added to the pre-filled gradients."""
    inp = wgrad_inputs(c)
    p = wgrad_plan(c)
    x, dy = inp["x"].float(), inp["dy"].float().clone()
    th, tpi, tw_ = p["th"], p["tiles_per_img"], p["tiles_w"]
    sh, sw = c.stride

    def tile_box(t):                                                    # (image, dy rows, dy columns) of tile t
        b, rem = divmod(t, tpi)
        r0, c0 = rem // tw_ * th, rem % tw_ * TW
        return b, slice(r0, r0 + th), slice(c0, c0 + TW)

    if variant == "channel_tail":                                       # the last 8 channels of a pixel read from the next pixel's first 8
        flat = x.reshape(-1, c.cin).clone()
        flat[:-1, -8:] = x.reshape(-1, c.cin)[1:, :8]
        x = flat.view(x.shape)
    if c.norm:
        mean, rstd = inp["mean"], inp["rstd"]
        if variant == "prev_image_stats":                               # the statistics registers are not refreshed on the first image change
            mean, rstd = mean.clone(), rstd.clone()
            mean[1], rstd[1] = mean[0], rstd[0]
        x = normalised(x, mean, rstd).to(c.dtype).float()
    dyw = dy
    x2 = x
    if variant == "skip_last_tile":                                     # the last tile of workgroup 0's walk is never accumulated
        b, rs, cs = tile_box((p["ntiles"] - 1) // p["gx_upper"] * p["gx_upper"])
        dyw = dy.clone()
        dyw[b, rs, cs] = 0
    dw = wgrad_def(x2, dyw, c.stride)
    if variant == "stale_tile":                                         # workgroup 0's second tile is computed from the ring slot of its first
        t1 = p["gx_upper"]
        assert t1 < p["ntiles"]
        (b0, r0, c0), (b1, r1, c1) = tile_box(0), tile_box(t1)
        xp = F.pad(x, (0, 0, 1, sw + 1, 1, sh + 1))

        def patch(b, rs, cs):                                           # the halo tile of x and the dy tile, zero beyond the image
            hs = slice(rs.start * sh, rs.start * sh + (th - 1) * sh + 3)
            ws = slice(cs.start * sw, cs.start * sw + (TW - 1) * sw + 3)
            xt = torch.zeros((1, (th - 1) * sh + 3, (TW - 1) * sw + 3, c.cin))
            got = xp[b:b + 1, hs, ws]
            xt[:, :got.shape[1], :got.shape[2]] = got
            yt = torch.zeros((1, th, TW, c.cout))
            g = dy[b:b + 1, rs, cs]
            yt[:, :g.shape[1], :g.shape[2]] = g
            return xt, yt

        def contrib(xt, yt):
            g = torch.nn.grad.conv2d_weight(nchw(xt).contiguous(), (c.cout, c.cin, 3, 3), nchw(yt).contiguous(), stride=(sh, sw), padding=0)
            return g.permute(0, 2, 3, 1)

        dw = dw - contrib(*patch(b1, r1, c1)) + contrib(*patch(b0, r0, c0))
    if variant == "halo_row":                                           # the last halo row of every tile is lost: tap row 2 of a tile's last row
        rows = [r for r in range(th - 1, dy.shape[1], th)]
        dlast = torch.zeros_like(dy)
        dlast[:, rows] = dy[:, rows]
        dw = dw.clone()
        dw[:, 2] -= wgrad_def(x, dlast, c.stride)[:, 2]
    db = dy.sum(dim=(0, 1, 2))
    if variant == "bias_every_column":                                  # every cin-block column of the grid adds the bias sums
        db = db * p["ncb"]
    return inp["dw0"] + dw, inp["db0"] + db


def wgrad_check(c: WgradCase, dw: torch.Tensor, db: torch.Tensor) -> None:
    ref = wgrad_ref(c)
    if c.real:
        assert_bounded(dw, ref["dw"], ref["dw_bound"], f"{c.name} dw")
        assert_bounded(db, ref["db"], ref["db_bound"], f"{c.name} db")
    else:
        assert_exact(dw, ref["dw"], F32, f"{c.name} dw")
        assert_exact(db, ref["db"], F32, f"{c.name} db")


# ================================================================================================ first layer forward (CIN = 1)

@dataclass(frozen=True)
class Conv1Case:
    name: str
    dtype: torch.dtype
    B: int
    H: int
    W: int
    cout: int
    relu: bool = True


CONV1_CASES = (
    # conv1_direct_kernel: 256 columns per workgroup, 32 rows per chunk: W > 256 and H > 32 take a second workgroup each way
    Conv1Case("c1-fwd-bf16-cout32", BF16, 2, 35, 259, 32),
    Conv1Case("c1-fwd-f32-cout32", F32, 2, 35, 259, 32),
    Conv1Case("c1-fwd-bf16-cout16", BF16, 2, 35, 259, 16, relu=False),
)


@functools.lru_cache(maxsize=2)
def conv1_inputs(c: Conv1Case) -> Dict[str, torch.Tensor]:
    seed = 9000 + CONV1_CASES.index(c)
    return dict(x=guarded(ints((c.B, c.H, c.W, 1), seed, -3, 3), c.dtype), w=guarded(ints((c.cout, 3, 3, 1), seed + 1, -2, 2), c.dtype),
                bias=guarded(ints((c.cout,), seed + 2, -3, 3)))


def conv1_ref(c: Conv1Case) -> torch.Tensor:
    inp = conv1_inputs(c)
    y = conv_def(inp["x"].double(), inp["w"].double()) + inp["bias"].double()
    return y.clamp_min(0.0) if c.relu else y


def conv1_standin(c: Conv1Case) -> torch.Tensor:
    inp = conv1_inputs(c)
    y = conv_def(inp["x"].float(), inp["w"].float()) + inp["bias"]
    return (y.clamp_min(0.0) if c.relu else y).to(c.dtype)


# ================================================================================================ depthwise 3x3

@dataclass(frozen=True)
class DwCase:
    """omr_dwconv3x3 (op = fwd | flip) or omr_dwconv3x3_wgrad (op = wgrad) on x [B, H, W, C]."""
    name: str
    dtype: torch.dtype
    op: str
    B: int
    H: int
    W: int
    C: int
    norm: bool = False
    mask: float = 0.0
    w_off: int = 0                           # bytes: the weight starts this far into its buffer
    kernel: str = "tile"                     # forward: tile | walk | pixel; wgrad: tile12 | tile16 | wide | rows (asserted from dw_plan)
    min_tiles: int = 1
    real: bool = False
    rc: int = 8                              # walk: rows per thread the dispatch must choose


def _dw_cases():
    C = DwCase
    fwd = (
        # exact versions of DW_PATH_CASES (tests/test_kernels_gpu.py) and of test_dwconv3x3's shapes, forward and flipped
        C("dw-tile-bf16-c128", BF16, "fwd", 2, 11, 19, 128, norm=True, mask=2.0),
        C("dw-tile-f32-c256-flip", F32, "flip", 2, 11, 19, 256, mask=2.0),
        C("dw-tile-bf16-c256-flip", BF16, "flip", 2, 11, 19, 256),
        C("dw-walk-f32-c512", F32, "fwd", 2, 6, 19, 512, norm=True, mask=2.0, kernel="walk"),              # the tile is 80 KB > 64 KB
        C("dw-walk-bf16-unaligned-w", BF16, "flip", 2, 11, 19, 128, norm=True, w_off=8, kernel="walk"),    # RC = 8: H = 11 takes two row chunks
        # RC doubles while column blocks x images x row chunks > 4096: 1 x 2049 x 2 chunks of 8 rows -> RC = 16, one chunk of 9 rows
        C("dw-walk-bf16-rc16", BF16, "flip", 2049, 9, 3, 128, norm=True, mask=2.0, w_off=8, kernel="walk", rc=16),
        C("dw-pixel-bf16-h3", BF16, "fwd", 2, 3, 19, 128, norm=True, mask=2.0, kernel="pixel"),
        C("dw-pixel-f32-h3-flip", F32, "flip", 2, 3, 19, 128, kernel="pixel"),
    )
    wgrad = (
        # persistent tile kernel: one workgroup per CU, > 3 x 256 tiles, ragged both ways, across images
        C("dwg-tile12-bf16-c128", BF16, "wgrad", 8, 41, 259, 128, kernel="tile12", min_tiles=4),
        C("dwg-tile12-bf16-c128-norm", BF16, "wgrad", 8, 41, 259, 128, norm=True, kernel="tile12", min_tiles=4),
        C("dwg-tile16-bf16-c256", BF16, "wgrad", 8, 41, 131, 256, kernel="tile16", min_tiles=4),
        C("dwg-tile16-bf16-c256-norm", BF16, "wgrad", 8, 41, 131, 256, norm=True, kernel="tile16", min_tiles=4),
        C("dwg-wide-f32-c256", F32, "wgrad", 8, 41, 67, 256, kernel="wide", min_tiles=4),
        C("dwg-wide-f32-c256-norm", F32, "wgrad", 8, 41, 67, 256, norm=True, kernel="wide", min_tiles=4),
        C("dwg-rows-bf16-c64", BF16, "wgrad", 3, 11, 70, 64, norm=True, kernel="rows"),
        C("dwg-rows-bf16-h3", BF16, "wgrad", 2, 3, 19, 128, kernel="rows"),
    )
    real = (
        C("real-dw-tile-bf16-c128", BF16, "fwd", 2, 11, 19, 128, norm=True, mask=1.25, real=True),
        C("real-dw-walk-f32-c512-flip", F32, "flip", 2, 6, 19, 512, norm=True, mask=1.25, kernel="walk", real=True),
        C("real-dwg-tile12-bf16-c128-norm", BF16, "wgrad", 8, 41, 259, 128, norm=True, kernel="tile12", min_tiles=4, real=True),
    )
    return fwd, wgrad, real


DW_FWD_CASES, DW_WGRAD_CASES, DW_REAL_CASES = _dw_cases()
DW_CASES = DW_FWD_CASES + DW_WGRAD_CASES + DW_REAL_CASES


def dw_plan(c: DwCase) -> dict:
    """Mirror of DwTilePlan, omr_dwconv3x3 and omr_dwconv3x3_wgrad (csrc/dwconv.hip:438-520).  The grids are exact: no occupancy enters."""
    vec = VEC[c.dtype]
    esz = 2 if c.dtype == BF16 else 4
    cv = c.C // vec
    tc = 256 // cv if cv <= 256 and 256 % cv == 0 else 0                                      # :446
    nchunk = 10 * (tc + 2) * cv
    tile_bytes = 10 * (tc + 2) * c.C * esz
    wgrad = c.op == "wgrad"
    shape = tc >= 2
    if wgrad:
        tile_bytes = max(tile_bytes, (tc if cv >= 64 else 4) * cv * 10 * vec * 4)             # :451
        shape = (cv in (16, 32) or 64 <= cv <= 256) and tc >= 1
    fits = shape and c.H >= 4 and tile_bytes <= 64 * 1024 and nchunk <= 16 * 256              # :455
    if wgrad:
        if fits:
            ntiles = cdiv(c.W, tc) * c.B * cdiv(c.H, 8)
            gx = min(ntiles, NUM_CU)                                                          # :507
            kernel = "wide" if cv >= 64 else "tile12" if nchunk <= 12 * 256 else "tile16"     # :508
            return dict(kernel=kernel, tc=tc, ntiles=ntiles, gx=gx, min_tiles=cdiv(ntiles, gx), cross=ntiles - gx >= cdiv(c.W, tc) * cdiv(c.H, 8))
        assert cv <= 64 and 64 % cv == 0                                                      # :514
        return dict(kernel="rows", tc=256 // cv, ntiles=1, gx=1, min_tiles=1, cross=False)
    if fits and c.w_off % 16 == 0:
        return dict(kernel="tile", tc=tc, min_tiles=1)
    if tc >= 1 and c.H >= 4 and 10 * c.C * 4 <= 48 * 1024:                                     # :481
        rc = 8
        while rc < c.H and cdiv(c.W, tc) * c.B * cdiv(c.H, rc) > 4096:                        # :483: reached only by > 4096 column blocks x row chunks
            rc *= 2
        return dict(kernel="walk", tc=tc, rc=rc, min_tiles=1)
    return dict(kernel="pixel", tc=tc, min_tiles=1)


@functools.lru_cache(maxsize=2)
def dw_inputs(c: DwCase) -> Dict[str, torch.Tensor]:
    seed = 12000 + 11 * DW_CASES.index(c)
    shape = (c.B, c.H, c.W, c.C)
    d = dict(x=guarded(ints(shape, seed, -2, 2), c.dtype), dy=guarded(ints(shape, seed + 1, -1, 1), c.dtype), bias=guarded(ints((c.C,), seed + 2, -3, 3)),
             mask=guarded(ints(shape, seed + 3, -1, 2), c.dtype), dw0=guarded(ints((c.C, 9), seed + 4, -5, 5)), db0=guarded(ints((c.C,), seed + 5, -5, 5)))
    d["mean"], d["rstd"] = stats_pair(c.B, c.C, seed + 6)
    w = ints((c.C, 9), seed + 8, -2, 2).to(c.dtype)
    if c.real:
        d.update(x=guarded(F.relu(rnd(shape, seed)) * 3, c.dtype), dy=guarded(rnd(shape, seed + 1), c.dtype), bias=guarded(rnd((c.C,), seed + 2)),
                 mean=guarded(1.5 * rnd((c.B, c.C), seed + 6, 0.2, 1.0)), rstd=guarded(rnd((c.B, c.C), seed + 7, 0.5, 2.0)))
        w = (rnd((c.C, 9), seed + 8) / 3).to(c.dtype)
    e = c.w_off // (2 if c.dtype == BF16 else 4)
    buf = torch.full((w.numel() + 128,), NAN, dtype=c.dtype)
    d["w"] = buf[e:e + w.numel()].view(w.shape)
    d["w"].copy_(w)
    return d


def dw_compute(c: DwCase, prec) -> Dict[str, torch.Tensor]:
    """The operation from its definition in `prec` (fp64: the reference; fp32 with the output rounded: the CPU stand-in)."""
    inp = dw_inputs(c)
    x = inp["x"].to(prec)
    if c.norm:
        x = normalised(x, inp["mean"], inp["rstd"])
    ref = prec == torch.float64
    if not ref and c.norm:
        x = x.to(c.dtype).to(prec)                                      # the tile kernels keep xhat in an LDS tile of the compute type
    u_norm = (U8 + 4 * U24 if c.dtype == BF16 else 2 * U24) if c.norm else 0.0
    if c.op == "wgrad":
        dy = inp["dy"].to(prec)
        out = dict(dw=inp["dw0"].to(prec) + dw_wgrad_def(x, dy), db=inp["db0"].to(prec) + dy.sum(dim=(0, 1, 2)))
        if ref:
            sum_abs = dw_wgrad_def(x.abs(), dy.abs())
            if c.real:
                K = c.B * c.H * c.W + 1
                out["dw_bound"] = gemm_bound(K, inp["dw0"].abs().to(prec) + sum_abs, out["dw"], F32, u_norm * sum_abs)
                out["db_bound"] = gemm_bound(K, inp["db0"].abs().to(prec) + dy.abs().sum(dim=(0, 1, 2)), out["db"], F32)
            else:
                assert_sums_fit(inp["dw0"].abs().to(prec) + sum_abs, c.name, 0.5 if c.norm else 1.0)
        return out
    w = inp["w"].to(prec)
    acc = dw_def(x, w, flip=c.op == "flip") + inp["bias"].to(prec)
    scale = float(f32_scalar(c.mask)) if c.mask else 1.0
    y = torch.where(inp["mask"].to(prec) > 0, acc * scale, 0.0) if c.mask else acc
    out = dict(y=y)
    if ref and c.real:
        sum_abs = dw_def(x.abs(), w.abs(), flip=c.op == "flip")
        b = gemm_bound(10, sum_abs + inp["bias"].abs().to(prec), acc, F32, u_norm * sum_abs) * scale + (U24 * y.abs() if c.mask else 0.0)
        out["y_bound"] = b + (U8 * y.abs() if c.dtype == BF16 else 0.0)
    return out


def dw_check(c: DwCase, got: Dict[str, torch.Tensor]) -> None:
    ref = dw_compute(c, torch.float64)
    for k in ("y", "dw", "db"):
        if k not in ref:
            continue
        if c.real:
            assert_bounded(got[k], ref[k], ref[k + "_bound"], f"{c.name} {k}")
        else:
            assert_exact(got[k], ref[k], F32 if c.op == "wgrad" else c.dtype, f"{c.name} {k}")


# ================================================================================================ fused backward

@dataclass(frozen=True)
class FusedCase:
    """omr_conv3x3_bwd_fused (mode = plain | mask | norm | xnorm) or omr_conv3x3_bwd_fused_s2 (mode = s2); bf16."""
    name: str
    mode: str
    cout: int
    cin: int
    B: int
    H: int
    W: int
    slots: int = 0                           # xnorm / s2: stat_slots (0: omr_conv3x3_stat_slots)
    min_tiles: int = 1
    real: bool = False


# ring depth per instantiation: pick() and the xnorm launch of csrc/conv_bwd_fused.hip:517-523, :812; S2::NSLOT :542
FUSED_NSLOT = {("plain", 32, 32): 3, ("plain", 32, 16): 4, ("plain", 16, 16): 6, ("norm", 32, 32): 2, ("norm", 32, 16): 2, ("norm", 16, 16): 4,
               ("xnorm", 16, 16): 6, ("s2", 32, 32): 4}


def _fused_cases():
    C = FusedCase
    out = []
    # B images share the 256 workgroups: gx = ceil(256 / B) <= tiles / (NSLOT + 2); 3 x 3 or 4 x 3 tiles of 8 x 32 with overhang both ways
    for co, ci in ((32, 32), (32, 16), (16, 16)):
        for mode in ("plain", "mask", "norm"):
            ns = FUSED_NSLOT[("norm" if mode == "norm" else "plain", co, ci)]
            out.append(C(f"fused-{mode}-{co}x{ci}", mode, co, ci, 256, 19, 70, min_tiles=ns + 2))     # gx = 1: nine tiles, ring depth <= 6
    out.append(C("fused-xnorm-slots1", "xnorm", 16, 16, 2, 19, 70, slots=1, min_tiles=8))
    out.append(C("fused-xnorm-b256", "xnorm", 16, 16, 256, 19, 70, min_tiles=8))
    out.append(C("fused-s2-slots1", "s2", 32, 32, 2, 19, 70, slots=1, min_tiles=6))
    out.append(C("fused-s2-even-slots1", "s2", 32, 32, 2, 20, 72, slots=1, min_tiles=6))
    out.append(C("fused-plain-one-tile", "plain", 32, 32, 1, 8, 32))
    out.append(C("real-fused-mask-32x32", "mask", 32, 32, 256, 19, 70, min_tiles=5, real=True))
    out.append(C("real-fused-xnorm-slots1", "xnorm", 16, 16, 2, 19, 70, slots=1, min_tiles=8, real=True))
    out.append(C("real-fused-s2-slots1", "s2", 32, 32, 2, 19, 70, slots=1, min_tiles=6, real=True))
    return tuple(out)


FUSED_CASES = _fused_cases()


def fused_plan(c: FusedCase) -> dict:
    """Mirror of launch (csrc/conv_bwd_fused.hip:495-515) and omr_conv3x3_bwd_fused_s2 (:841-849): 1024-thread workgroups, one per CU;
    the grid is exact."""
    tiles_h, tiles_w = cdiv(c.H, 8), cdiv(c.W, 32)
    tiles = tiles_h * tiles_w
    gx = min(cdiv(NUM_CU, c.B), tiles)
    slots = fused_slots(c)
    if c.mode in ("xnorm", "s2"):
        gx = min(gx, slots)
    gx = max(gx, 1)
    key = ("plain" if c.mode == "mask" else c.mode, c.cout, c.cin)
    return dict(tiles_h=tiles_h, tiles_w=tiles_w, tiles=tiles, gx=gx, slots=slots, nslot=FUSED_NSLOT[key], min_tiles=cdiv(tiles, gx))


def fused_slots(c: FusedCase) -> int:
    return c.slots if c.slots > 0 else min(cdiv(c.H, 4) * cdiv(c.W, TW), cdiv(NUM_CU * 8, c.B))


FUSED_RELU_SCALE = 2.0


def fused_mask_scale(c: FusedCase) -> float:
    return 1.25 if c.real else 2.0


@functools.lru_cache(maxsize=2)
def fused_inputs(c: FusedCase) -> Dict[str, torch.Tensor]:
    seed = 20000 + 7 * FUSED_CASES.index(c)
    B, H, W = c.B, c.H, c.W
    gh, gw = ((H + 1) // 2, (W + 1) // 2) if c.mode == "s2" else (H, W)
    d = dict(x=guarded(ints((B, H, W, c.cin), seed, -1, 2), BF16), g=guarded(ints((B, gh, gw, c.cout), seed + 1, -2, 2), BF16),
             w=guarded(ints((c.cout, 3, 3, c.cin), seed + 2, -1, 1), BF16),
             dw0=guarded(ints((c.cout, 3, 3, c.cin), seed + 3, -5, 5)), db0=guarded(ints((c.cout,), seed + 4, -5, 5)))
    d["xmean"], d["xrstd"] = stats_pair(B, c.cin, seed + 5)
    if c.real:
        d.update(x=guarded(F.relu(rnd((B, H, W, c.cin), seed)) * 3, BF16), g=guarded(rnd((B, gh, gw, c.cout), seed + 1), BF16),
                 w=guarded(rnd((c.cout, 3, 3, c.cin), seed + 2) * 0.2, BF16),
                 xmean=guarded(1.5 * rnd((B, c.cin), seed + 5, 0.2, 1.0)), xrstd=guarded(rnd((B, c.cin), seed + 6, 0.5, 2.0)))
    d["wf"] = guarded(flip_weights(d["w"]), BF16)
    # norm: y of the layer above (a ReLU output: half zeros), its statistics, and the per-image means k1 = mean(ghat), k2 = mean(ghat * yhat)
    # the caller hands over as sums k * H * W: integers and halves, so G = relu_scale * rstd * (ghat - k1 - yhat * k2) is a multiple of 1/4
    d["y"] = guarded(ints((B, H, W, c.cout), seed + 7, -2, 3).clamp_min(0), BF16)
    d["ymean"], d["yrstd"] = stats_pair(B, c.cout, seed + 8)
    d["k"] = torch.stack([ints((B, c.cout), seed + 10, -1, 1), ints((B, c.cout), seed + 11, -2, 2) * 0.5], dim=-1).double()
    return d


def fused_g(c: FusedCase, inp) -> torch.Tensor:
    """fp64 gradient the conv backward starts from: g itself, or (norm) the InstanceNorm backward of the layer above with its ReLU mask."""
    g = inp["g"].double()
    if c.mode != "norm":
        return g
    B, C = c.B, c.cout
    y = inp["y"].double()
    k = inp["k"].view(B, 1, 1, C, 2)
    rs = inp["yrstd"].double().view(B, 1, 1, C)
    G = FUSED_RELU_SCALE * rs * (g - k[..., 0] - normalised(y, inp["ymean"], inp["yrstd"]) * k[..., 1])
    G = torch.where(y > 0, G, 0.0)
    assert bool((G * 4 == (G * 4).round()).all()) and float(G.abs().max()) * 4 < 256, "norm case: G must be exact in bf16"
    return G


def fused_ref(c: FusedCase) -> Dict[str, torch.Tensor]:
    """dx, dw, db (and for xnorm / s2 the InstanceNorm-backward sums [B, CIN, 2] of dx) in fp64 from the definitions."""
    inp = fused_inputs(c)
    x, w = inp["x"].double(), inp["w"].double()
    G = fused_g(c, inp)
    stride = (2, 2) if c.mode == "s2" else (1, 1)
    xh = normalised(x, inp["xmean"], inp["xrstd"]) if c.mode in ("xnorm", "s2") else x
    acc = conv_def(G, flip_weights(w), (1, 1), stride, (c.H, c.W))
    acc_abs = conv_def(G.abs(), flip_weights(w).abs(), (1, 1), stride, (c.H, c.W))
    unit = 0.125 if c.mode == "norm" else 0.5
    masked = c.mode in ("mask", "norm")
    scale = float(f32_scalar(fused_mask_scale(c))) if masked else 1.0
    dx = torch.where(x > 0, acc * scale, 0.0) if masked else acc
    dw_abs = inp["dw0"].double().abs() + wgrad_def(xh.abs(), G.abs(), stride)
    out = dict(dx=dx, dw=inp["dw0"].double() + wgrad_def(xh, G, stride), db=inp["db0"].double() + G.sum(dim=(0, 1, 2)))
    if c.real:
        K = c.B * G.shape[1] * G.shape[2] + 1
        u_norm = U8 + 4 * U24 if c.mode in ("xnorm", "s2") else 0.0     # xhat is rounded to bf16 in LDS
        out["dx_bound"] = gemm_bound(9 * c.cout, acc_abs, acc, F32) * scale + (U24 if masked else 0.0) * dx.abs() + U8 * dx.abs()
        out["dw_bound"] = gemm_bound(K, dw_abs, out["dw"], F32, u_norm * dw_abs)
        out["db_bound"] = gemm_bound(K, inp["db0"].double().abs() + G.abs().sum(dim=(0, 1, 2)), out["db"], F32)
    else:
        assert_sums_fit(acc_abs, c.name + " dx", unit)
        assert_sums_fit(dw_abs, c.name + " dw", unit)
    if c.mode in ("xnorm", "s2"):
        n = c.H * c.W
        if c.real:                                                      # the stored gradient is within dx_bound of dx, the bf16 xhat within 2^-8 of xhat
            bd = out["dx_bound"]
            out["sums"] = torch.stack([dx.sum(dim=(1, 2)), (dx * xh).sum(dim=(1, 2))], dim=-1)
            out["sums_bound"] = torch.stack([bd.sum(dim=(1, 2)) + 4 * (n + 2) * U24 * dx.abs().sum(dim=(1, 2)),
                                             ((bd + u_norm * dx.abs()) * xh.abs()).sum(dim=(1, 2)) + 4 * (n + 2) * U24 * (dx * xh).abs().sum(dim=(1, 2))], dim=-1)
        else:
            dxr = dx.to(BF16).double()                                  # the sums are taken over the stored gradient
            out["sums"] = torch.stack([dxr.sum(dim=(1, 2)), (dxr * xh).sum(dim=(1, 2))], dim=-1)
            assert_sums_fit(torch.stack([dxr.abs().sum(dim=(1, 2)), (dxr * xh).abs().sum(dim=(1, 2))]), c.name + " sums", 0.5)
    return out


def fused_standin(c: FusedCase, variant: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """torch CPU fp32 / bf16 in the kernel's place: G and xhat rounded to bf16 (they live in LDS), fp32 sums, dx rounded once."""
    inp = fused_inputs(c)
    p = fused_plan(c)
    x, w = inp["x"].float(), inp["w"].float()
    G = fused_g(c, inp).float().to(BF16).float()
    stride = (2, 2) if c.mode == "s2" else (1, 1)
    xh = normalised(x, inp["xmean"], inp["xrstd"]).to(BF16).float() if c.mode in ("xnorm", "s2") else x
    dx = conv_def(G, flip_weights(w), (1, 1), stride, (c.H, c.W))
    if c.mode in ("mask", "norm"):
        dx = torch.where(x > 0, dx * f32_scalar(fused_mask_scale(c)), 0.0)
    dx = dx.to(BF16)
    Gw = G
    if variant == "skip_last_tile":                                     # the last tile of workgroup 0's walk is left out of all three gradients
        last = (p["tiles"] - 1) // p["gx"] * p["gx"]
        r0, c0 = last // p["tiles_w"] * 8, last % p["tiles_w"] * 32
        dx[:, r0:r0 + 8, c0:c0 + 32] = 0
        # the weight gradient of a tile sums over the x pixels the tile owns
        xh = xh.clone()
        xh[:, r0:r0 + 8, c0:c0 + 32] = 0
    dw = inp["dw0"] + wgrad_def(xh, Gw, stride)
    db = inp["db0"] + G.sum(dim=(0, 1, 2))
    out = dict(dx=dx, dw=dw, db=db)
    if c.mode in ("xnorm", "s2"):
        xs = normalised(x, inp["xmean"], inp["xrstd"]).to(BF16).float()
        out["sums"] = torch.stack([dx.double().sum(dim=(1, 2)), (dx.float() * xs).double().sum(dim=(1, 2))], dim=-1)
    return out


def fused_check(c: FusedCase, got: Dict[str, torch.Tensor]) -> None:
    ref = fused_ref(c)
    if c.real:
        for k in ("dx", "dw", "db") + (("sums",) if "sums" in ref else ()):
            assert_bounded(got[k], ref[k], ref[k + "_bound"], f"{c.name} {k}")
        return
    assert_exact(got["dx"], ref["dx"], BF16, f"{c.name} dx", tile=(8, 32))
    assert_exact(got["dw"], ref["dw"], F32, f"{c.name} dw")
    assert_exact(got["db"], ref["db"], F32, f"{c.name} db")
    if "sums" in ref:
        assert_exact(got["sums"], ref["sums"], torch.float64, f"{c.name} InstanceNorm-backward sums")
