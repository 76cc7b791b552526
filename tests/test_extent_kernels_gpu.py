"""The ragged-batch kernels (csrc/extent.hip) one by one, fp32 and bf16, C in {1, 16, 128, 256}: B = 3 samples in a 64 x 96 plane
with sizes (64, 96) (full), (37, 50) (odd, no multiples of a tile) and (17, 9) (smaller than a tile).  Every input is NaN outside
the extents: a kernel that looks there fails.  References: tests/extent_refs.py (pinned by tests/test_extent_refs_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import extent_refs as E  # noqa: E402
from oracle.kernel_refs import assert_bit_equal, tol  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
WIDTHS = [1, 16, 128, 256]
# beyond the issue's widths: channel-group counts that do not divide the 256 threads of a workgroup (idle threads in the statistics and
# apply kernels: C = 24 is 6 groups in fp32 and 3 in bf16, C = 48 is 12 and 6) and an odd C on the element-wise path whose 2 C = 6 sums
# do not divide the 256 threads of the slot reduction either.  omr_instnorm_stats takes none of them, so their statistics are held
# to the fp64 reference (ODD_WIDTHS tests below).
ODD_WIDTHS = [3, 24, 48]
B = len(E.SIZES)
H, W = E.PLANE
EPS32 = float(np.float32(1e-3))          # the entry takes eps as a C float
NAN = float("nan")


def K():
    from omr_a2s_multimodal_transformer_amd import kernels
    return kernels


def ext_dev(ext=E.SIZES):
    return torch.tensor(list(ext), dtype=torch.int32, device=DEV)


def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def ints(shape, seed, bound=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-bound, bound + 1, shape, generator=g).float()


def outside(t, ext=E.SIZES):
    """The elements of an NHWC tensor outside the extents."""
    return t.detach().cpu()[~E.inside_mask(t.shape[1:3], ext)]


def assert_zero_bits(t, what):
    t = t.contiguous()
    assert not t.view({4: torch.int32, 2: torch.int16}[t.element_size()]).any(), f"{what}: not +0.0 everywhere outside the extents"


@functools.lru_cache(maxsize=None)
def int_input(C):
    """Small integers (|v| <= 8: exact in bf16, every sum and sum of squares exact in fp32 and fp64) inside, NaN outside."""
    return E.nan_outside_nhwc(ints((B, H, W, C), 70 + C), E.SIZES)


@functools.lru_cache(maxsize=None)
def int_norm_ref(C):
    return E.extent_norm_fwd_ref(int_input(C), E.SIZES, EPS32)


@functools.lru_cache(maxsize=None)
def bwd_input(C, dtype):
    """x a ReLU output, g in [-1, 1] like the existing InstanceNorm backward case (oracle.kernel_refs.in_inputs), NaN outside."""
    x = torch.relu(rnd((B, H, W, C), 51 + C) + 0.3).to(dtype)
    g = rnd((B, H, W, C), 52 + C).to(dtype)
    return E.nan_outside_nhwc(x, E.SIZES), E.nan_outside_nhwc(g, E.SIZES)


# ------------------------------------------------------------------------------------------------ 3. omr_extent_zero

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", WIDTHS + ODD_WIDTHS)
def test_extent_zero_is_torch_where(dtype, C):
    """Bit-equal to torch.where(inside, x, 0): zeros written over NaN (not multiplied in), the inside untouched (-0.0 and all)."""
    x = E.nan_outside_nhwc(rnd((B, H, W, C), 60 + C), E.SIZES).to(dtype)
    x[0, 0, 0, 0] = -0.0
    want = E.zero_outside_nhwc(x, E.SIZES)
    xd = x.to(DEV)
    out = K().extent_zero(xd, ext_dev())
    assert out.data_ptr() == xd.data_ptr(), "omr_extent_zero works in place"
    assert_bit_equal(xd, want, f"extent_zero C={C} {dtype}")
    again = K().extent_zero(xd, ext_dev())                      # its own adjoint / idempotent
    assert_bit_equal(again, want, f"extent_zero twice C={C} {dtype}")


def test_extent_zero_on_a_plane_that_is_all_inside_or_all_outside():
    """Extent = the plane: nothing is stored.  Extent 0 x 0 (and one clamped from beyond the plane): everything / nothing is zeroed."""
    x = rnd((3, 5, 7, 16), 5)
    xd = x.to(DEV)
    K().extent_zero(xd, torch.tensor([[5, 7], [0, 0], [9, 99]], dtype=torch.int32, device=DEV))
    assert torch.equal(xd[0].cpu(), x[0]) and not xd[1].any() and torch.equal(xd[2].cpu(), x[2])


# ------------------------------------------------------------------------------------------------ 4. omr_instnorm_extent_fwd

def _stats_of_crop(crop):
    """K.instnorm_stats of one cropped sample [1, h, w, C].  It takes C a multiple of 8 / 4 only: the 1-channel crop goes in as 8 equal
    channels (a channel's statistics do not depend on its neighbours) and channel 0 comes back."""
    if crop.shape[-1] == 1:
        mean, rstd = K().instnorm_stats(crop.expand(-1, -1, -1, 8).contiguous(), eps=EPS32)
        return mean[:, :1], rstd[:, :1]
    return K().instnorm_stats(crop.contiguous(), eps=EPS32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", WIDTHS)
def test_instnorm_extent_fwd(dtype, C):
    """Small-integer inputs: all fp32 / fp64 sums are exact, so mean and rstd are bit-equal to omr_instnorm_stats of each crop.

    Output bound, from the fp64 reference yref = (x - mu) * rho (u = 2^-24): the kernel computes fl(fl(x - mean) * rstd) in fp32 with
    mean = mu (1 + d1), rstd = rho (1 + d2) (the fp32 roundings of statistics that are exact to fp64 rounding), |d| <= u each:
      x - mean is off by u |mu|, its rounding adds u |x - mu|; times rho: u (rho |mu| + |yref|);
      rstd's rounding and the product's rounding add u |yref| each
    => |y - yref| <= u (rho |mu| + 3 |yref|), times 1.001 for the second-order terms and the fp64 roundings of mu and rho.
    bf16 stores round once more: the bound times (1 + 2^-8), plus 2^-8 |yref|.  Outside the extents: +0.0."""
    x = int_input(C).to(dtype)
    y64, mean64, rstd64 = int_norm_ref(C)
    xd = x.to(DEV)
    y, mean, rstd = K().instnorm_extent_fwd(xd, ext_dev(), eps=EPS32)
    assert y.dtype == dtype and mean.dtype == rstd.dtype == torch.float32 and tuple(mean.shape) == (B, C)
    for b, (h, w) in enumerate(E.SIZES):
        m1, r1 = _stats_of_crop(xd[b:b + 1, :h, :w])
        assert_bit_equal(mean[b:b + 1], m1.cpu(), f"mean of sample {b} C={C} {dtype}")
        assert_bit_equal(rstd[b:b + 1], r1.cpu(), f"rstd of sample {b} C={C} {dtype}")
    _check_norm_output(y, y64, mean64, rstd64, dtype, C)


def _check_norm_output(y, y64, mean64, rstd64, dtype, C):
    """The output bound derived in test_instnorm_extent_fwd's docstring, and +0.0 outside the extents."""
    u = 2.0 ** -24
    bound = u * ((rstd64 * mean64.abs())[:, None, None, :] + 3 * y64.abs()) * 1.001
    if dtype == torch.bfloat16:
        bound = bound * (1 + 2.0 ** -8) + 2.0 ** -8 * y64.abs()
    got = y.cpu().double()
    inside = E.inside_mask((H, W), E.SIZES)
    err = (got - y64).abs()[inside]
    print(f"instnorm_extent_fwd C={C} {dtype}: max err / bound = {float((err / bound[inside].clamp_min(1e-300)).max()):.3f}")
    assert torch.isfinite(got).all() and bool((err <= bound[inside]).all()), f"max err / bound = {float((err / bound[inside].clamp_min(1e-300)).max()):.3f}"
    assert_zero_bits(outside(y), f"instnorm_extent_fwd C={C} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", ODD_WIDTHS)
def test_instnorm_extent_fwd_odd_widths(dtype, C):
    """The widths omr_instnorm_stats does not take (idle threads, a slot-reduction round that 256 is no multiple of).  Small integers:
    the sums are exact, so mean and rstd are the fp64 reference's rounded to fp32, up to the kernel's own fp64 roundings (sum * (1 / n)
    instead of sum / n; E[x^2] - mean^2 with |x| <= 8 and variance >= 1: a few 2^-53 relative, amplified at most 64-fold in the
    variance): within 2^-24 (1 + 2^-20) relative of the fp64 value.  Output: the same derived bound as for the issue's widths."""
    x = int_input(C).to(dtype)
    y64, mean64, rstd64 = int_norm_ref(C)
    y, mean, rstd = K().instnorm_extent_fwd(x.to(DEV), ext_dev(), eps=EPS32)
    one_rounding = 2.0 ** -24 * (1 + 2.0 ** -20)
    assert bool((1.0 / rstd64 ** 2 - EPS32 >= 1.0).all()), "the derivation assumes a variance of at least 1"
    assert bool(((mean.cpu().double() - mean64).abs() <= one_rounding * mean64.abs()).all()), f"mean C={C} {dtype}"
    assert bool(((rstd.cpu().double() - rstd64).abs() <= one_rounding * rstd64).all()), f"rstd C={C} {dtype}"
    _check_norm_output(y, y64, mean64, rstd64, dtype, C)


# ------------------------------------------------------------------------------------------------ 5. omr_instnorm_extent_bwd

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", WIDTHS + ODD_WIDTHS)
def test_instnorm_extent_bwd(dtype, C):
    """Against fp64 with the saved mean / rstd and the tolerances of the existing InstanceNorm backward case (oracle.kernel_refs.in_check:
    tol(dtype, 3), and tol(dtype, 6) with the ReLU factor at scale 2), same input distributions.  x and g are NaN outside; dx is +0.0 there."""
    x, g = bwd_input(C, dtype)
    xd, gd, ext = x.to(DEV), g.to(DEV), ext_dev()
    _, mean, rstd = K().instnorm_extent_fwd(xd, ext, eps=EPS32)
    for relu_mask, relu_scale, scale in ((False, 1.0, 3.0), (True, 2.0, 6.0)):
        dx = K().instnorm_extent_bwd(gd, xd, mean, rstd, ext, relu_mask=relu_mask, relu_scale=relu_scale)
        ref = E.extent_norm_bwd_ref(g, x, mean.cpu(), rstd.cpu(), E.SIZES, relu_mask, relu_scale)
        got = dx.cpu().double()
        assert torch.isfinite(got).all(), f"non-finite dx C={C} {dtype} relu={relu_mask}"
        torch.testing.assert_close(got, ref, **tol(dtype, scale), msg=lambda m: f"instnorm_extent_bwd C={C} {dtype} relu={relu_mask}: {m}")
        assert_zero_bits(outside(dx), f"instnorm_extent_bwd C={C} {dtype} relu={relu_mask}")


# ------------------------------------------------------------------------------------------------ 6. omr_pack_memory_fwd / _bwd

GRID_PLANE = (5, 13)                                  # one row / column more than the largest feature grid
GRID_EXT = ((4, 12), (3, 7), (2, 2))                  # the feature grids of E.SIZES
SMAX = 50                                             # > 48: the longest sample has zero rows behind it too


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", WIDTHS + ODD_WIDTHS)
def test_pack_memory_fwd_and_its_adjoint(dtype, C):
    assert list(GRID_EXT) == E.extent_levels(E.SIZES)[-1]
    x = E.nan_outside_nhwc(ints((B,) + GRID_PLANE + (C,), 80 + C), GRID_EXT).to(dtype)
    ext = ext_dev(GRID_EXT)
    packed = K().pack_memory_fwd(x.to(DEV), ext, SMAX)
    assert_bit_equal(packed, E.pack_rows(E.zero_outside_nhwc(x, GRID_EXT), GRID_EXT, SMAX), f"pack fwd C={C} {dtype}")
    for b, (h, w) in enumerate(GRID_EXT):
        assert_zero_bits(packed[b, h * w:].cpu(), f"pack fwd rows >= S_b of sample {b}")
    # backward: rows >= S_b of the incoming gradient are NaN (ignored), the result is zero outside the extents
    g = ints((B, SMAX, C), 90 + C).to(dtype)
    for b, (h, w) in enumerate(GRID_EXT):
        g[b, h * w:] = NAN
    dx = K().pack_memory_bwd(g.to(DEV), ext, *GRID_PLANE)
    assert tuple(dx.shape) == (B,) + GRID_PLANE + (C,) and torch.isfinite(dx).all()
    assert_zero_bits(outside(dx, GRID_EXT), f"pack bwd C={C} {dtype}")
    g0 = torch.nan_to_num(g.double(), nan=0.0)
    x0 = E.zero_outside_nhwc(x, GRID_EXT).double()
    lhs = float((packed.cpu().double() * g0).sum())           # small integers: both sums are exact
    rhs = float((x0 * dx.cpu().double()).sum())
    assert lhs == rhs and lhs != 0.0, (lhs, rhs)
    assert_bit_equal(K().pack_memory_fwd(dx, ext, SMAX), E.pack_rows(dx.cpu(), GRID_EXT, SMAX), "pack(pack_bwd(g))")
    for b, (h, w) in enumerate(GRID_EXT):                      # and the scatter itself
        assert_bit_equal(dx[b, :h, :w].cpu().reshape(h * w, C), g[b, :h * w], f"pack bwd sample {b}")
