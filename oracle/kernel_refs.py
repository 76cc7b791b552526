"""Float64 references, error bounds and the shared case table for the kernel-branch tests.

tests/test_kernel_branches_gpu.py runs every case below through the HIP kernels; tests/test_kernel_refs_cpu.py runs the same
cases with torch CPU fp32 / bf16 arithmetic standing in for the kernels, which shows without a GPU that a correct
implementation passes each check and (for the GEMMs) that a subtly wrong one does not.  Every `*_inputs` function builds the
quantised CPU tensors a case feeds the kernel (cached, never modified: callers clone what a kernel writes into), every
`*_ref` function restates the operation in plain fp64 arithmetic on those tensors, and every `*_check` function holds the
assertions both test files share.

Test infrastructure only: nothing here is imported by the package.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = (F32, BF16)
VEC = {F32: 4, BF16: 8}                     # elements per 16-byte fragment
TAG = {F32: "f32", BF16: "bf16"}
U24 = 2.0 ** -24                            # fp32 unit roundoff
EW_CAP = 2048 * 256                         # threads of a capped element-wise launch (ew_grid of elementwise.hip)
SENTINEL = 1234.5                           # fill of everything a kernel must not write


def rnd(shape, seed: int, lo: float = -1.0, hi: float = 1.0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def bits(t: torch.Tensor) -> torch.Tensor:
    """The storage bits of a tensor as integers (bit-equality that also holds for NaN, and tells -0 from +0)."""
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def assert_bit_equal(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{tuple(got.shape)} vs {want.dtype}{tuple(want.shape)}"
    bad = bits(got) != bits(want)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits, first at flat index {i}: "
                             f"{got.detach().cpu().flatten()[i].item()!r} vs {want.flatten()[i].item()!r}")


def tol(dtype, scale: float = 1.0) -> dict:
    """The project's per-kernel tolerance (tests/test_kernels_gpu.py): 2e-4 for fp32, 3e-2 for bf16."""
    return dict(rtol=2e-4, atol=2e-4 * scale) if dtype == F32 else dict(rtol=3e-2, atol=3e-2 * scale)


def check_close(got: torch.Tensor, ref64: torch.Tensor, dtype, scale: float = 1.0, what: str = "") -> None:
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    torch.testing.assert_close(got, ref64, **tol(dtype, scale), msg=lambda m: f"{what}: {m}")


def check_rounded_once(got: torch.Tensor, ref64: torch.Tensor, dtype, scale: float, what: str) -> None:
    """A kernel that computes in fp32 and rounds once to `dtype`: the fp32 tolerance on the value before the rounding plus, for
    bf16, that one rounding (unit roundoff 2^-8).  For bf16 this is far tighter than tol(bf16, scale)."""
    got = got.detach().cpu().double()
    t = tol(F32, scale)
    allowed = (t["atol"] + t["rtol"] * ref64.abs()) * (1 + 2.0 ** -8) + (2.0 ** -8 * ref64.abs() if dtype == BF16 else 0.0)
    err = (got - ref64).abs()
    assert bool((err <= allowed).all()), f"{what}: max error / allowed = {float((err / allowed).max()):.3f}"


def padded(rows: int, cols: int, dtype, fill: float, extra_rows: int = 2, ld: Optional[int] = None) -> torch.Tensor:
    """A [rows + extra_rows, ld] buffer full of `fill`; ld defaults to cols rounded up to the 16-byte vector width."""
    ld = round_up(cols, VEC[dtype]) if ld is None else ld
    return torch.full((rows + extra_rows, ld), fill, dtype=dtype)


# ================================================================================================ GEMM

@dataclass(frozen=True)
class GemmCase:
    name: str
    dtype: torch.dtype                       # operands
    cdtype: torch.dtype                      # C
    M: int = 130                             # two M tiles with a 2-row tail
    N: int = 70                              # one ragged N tile
    K: int = 45                              # 45: FULLK with a partial 16-byte chunk; 301: the pipelined loop, again partial
    ta: bool = False
    tb: bool = False
    bias: bool = False
    relu: bool = False
    accumulate: bool = False
    split_k: int = 1
    colsum: bool = False
    ldc: int = 0                             # 0: N + 7 (odd: scalar stores only)
    drop: Optional[Tuple[float, int]] = None

    @property
    def ld_c(self) -> int:
        return self.ldc or self.N + 7


TYPE_PAIRS = ((F32, F32), (BF16, BF16), (BF16, F32))


def _pair_tag(dt, cdt) -> str:
    return f"{TAG[dt]}-{TAG[cdt]}"


def _gemm_cases():
    prod, epi, split, colsum, drop = [], [], [], [], []
    for dt, cdt in TYPE_PAIRS:
        t = _pair_tag(dt, cdt)
        for ta in (False, True):
            for tb in (False, True):
                for K in (45, 301):
                    prod.append(GemmCase(f"{t}-{'t' if ta else 'n'}{'t' if tb else 'n'}-k{K}", dt, cdt, K=K, ta=ta, tb=tb))
        epi.append(GemmCase(f"{t}-bias-relu", dt, cdt, K=45, bias=True, relu=True))
        epi.append(GemmCase(f"{t}-accumulate", dt, cdt, K=301, accumulate=True))
        epi.append(GemmCase(f"{t}-ldc80", dt, cdt, K=45, ldc=80))            # ldc % 8 == 0, N % 8 != 0: vector stores + a scalar tail
        drop.append(GemmCase(f"{t}-dropout", dt, cdt, K=45, bias=True, relu=True, drop=(0.25, 4242)))
    for dt in DTYPES:
        for s in (2, 4):
            # K = 100: fp32 splits 64 + 36 (s = 2) or 32 + 32 + 32 + 4 (s = 4); bf16 gets 64 + 36 for both (fewer than requested)
            split.append(GemmCase(f"{TAG[dt]}-f32-split{s}", dt, F32, K=100, bias=True, accumulate=True, split_k=s))
        for tb in (False, True):
            for s in (1, 3):
                # the column sums run over the 130 side; N = 150 is two N tiles, of which only the first may add them
                colsum.append(GemmCase(f"{TAG[dt]}-f32-t{'t' if tb else 'n'}-colsum-split{s}", dt, F32, N=150, K=301, ta=True, tb=tb,
                                       accumulate=True, split_k=s, colsum=True))
    return tuple(prod), tuple(epi), tuple(split), tuple(colsum), tuple(drop)


GEMM_PRODUCT_CASES, GEMM_EPILOGUE_CASES, GEMM_SPLIT_CASES, GEMM_COLSUM_CASES, GEMM_DROPOUT_CASES = _gemm_cases()
GEMM_BOUND_CASES = GEMM_PRODUCT_CASES + GEMM_EPILOGUE_CASES + GEMM_SPLIT_CASES + GEMM_COLSUM_CASES
GEMM_FACTOR = 4.0                            # see gemm_bound


def view2d(buf: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    return buf[:rows, :cols]


@functools.lru_cache(maxsize=None)
def gemm_inputs(case: GemmCase) -> dict:
    """Operands as views into NaN-filled buffers (row padding up to the vector width and two rows past the logical extent), C
    as a view into a sentinel-filled buffer with ldc > N.  For a transposed operand the padded dimension is the M / N side."""
    M, N, K, dt = case.M, case.N, case.K, case.dtype
    seed = 1000 + 7 * sum(map(ord, case.name))
    a_shape = (K, M) if case.ta else (M, K)
    b_shape = (K, N) if case.tb else (N, K)
    a_buf, b_buf = padded(*a_shape, dt, float("nan")), padded(*b_shape, dt, float("nan"))
    view2d(a_buf, *a_shape).copy_(rnd(a_shape, seed))
    view2d(b_buf, *b_shape).copy_(rnd(b_shape, seed + 1))
    bias = rnd((N,), seed + 2) if case.bias else None
    c_buf = padded(M, N, case.cdtype, SENTINEL, ld=case.ld_c)
    inp = dict(a_buf=a_buf, b_buf=b_buf, a_shape=a_shape, b_shape=b_shape, bias=bias, c_buf=c_buf)
    if case.accumulate:
        # |c0| in [0.5, 1.5) with the sign of the product, so nothing cancels: the two roundings of an accumulate into a bf16 C
        # (the product, then the sum) are then both relative to at most |ref|, which is what the 2 x 2^-8 |ref| term allows
        A, B = _gemm_ab64(case, inp)
        prod = A @ B.t() + (bias.double() if bias is not None else 0.0)
        c0 = torch.where(prod < 0, -1.0, 1.0) * (0.5 + rnd((M, N), seed + 3, 0.0, 1.0).double())
        view2d(c_buf, M, N).copy_(c0)
    if case.colsum:
        inp["colsum0"] = rnd((M,), seed + 4) + 2.0
    return inp


def _gemm_ab64(case: GemmCase, inp: dict):
    a = view2d(inp["a_buf"], *inp["a_shape"]).double()
    b = view2d(inp["b_buf"], *inp["b_shape"]).double()
    return (a.t() if case.ta else a), (b.t() if case.tb else b)          # A [M, K], B [N, K]


@functools.lru_cache(maxsize=None)
def gemm_ref(case: GemmCase):
    """(ref, bound) of C, and (ref, bound) of the fused column sums or None, all fp64.

    Bound per element: GEMM_FACTOR * (K + 2) * 2^-24 * sum_k |a_ik| |b_kj|  (+ 2^-8 |ref| per rounding to a bf16 C).
    (K + 2) * 2^-24 * sum |a||b| is the order-independent worst case of an fp32 summation of K products plus the bias and the
    accumulate add (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5 with gamma_n ~ n u); the factor 4 covers
    the MFMA's internal summation tree; split-K and its atomics only reorder the sum.  2^-8 is the unit roundoff of bf16 (8
    significant bits): a bf16 C is rounded once, or twice with accumulate (the product, then the sum; see gemm_inputs)."""
    inp = gemm_inputs(case)
    A, B = _gemm_ab64(case, inp)
    ref = A @ B.t()
    sabs = A.abs() @ B.abs().t()
    if inp["bias"] is not None:
        ref = ref + inp["bias"].double()
    if case.relu:
        ref = ref.clamp_min(0.0)
    if case.accumulate:
        ref = ref + view2d(inp["c_buf"], case.M, case.N).double()
    bound = GEMM_FACTOR * (case.K + 2) * U24 * sabs
    if case.cdtype == BF16:
        bound = bound + (2 if case.accumulate else 1) * 2.0 ** -8 * ref.abs()
    cs = None
    if case.colsum:
        # db[m] += sum_k a[k][m]: K + 1 fp32 terms in an arbitrary order (per-thread partials, LDS and global atomics)
        c0 = inp["colsum0"].double()
        cs = (c0 + A.sum(1), (case.K + 2) * U24 * (c0.abs() + A.abs().sum(1)))
    return ref, bound, cs


def gemm_standin(case: GemmCase, drop_k: bool = False, drop_row: bool = False):
    """torch CPU arithmetic in the kernel's formats: fp32 accumulation, one rounding to the C type (two with accumulate).
    drop_k leaves the last k index out (a guard that cuts the partial chunk short); drop_row leaves the last row of C unwritten."""
    inp = gemm_inputs(case)
    a = view2d(inp["a_buf"], *inp["a_shape"]).float()
    b = view2d(inp["b_buf"], *inp["b_shape"]).float()
    A, B = (a.t() if case.ta else a), (b.t() if case.tb else b)
    if drop_k:
        A = A[:, :-1]
        B = B[:, :-1]
    v = A @ B.t()
    if inp["bias"] is not None:
        v = v + inp["bias"]
    if case.relu:
        v = v.clamp_min(0.0)
    c_buf = inp["c_buf"].clone()
    c = view2d(c_buf, case.M, case.N)
    rows = case.M - 1 if drop_row else case.M
    if case.accumulate:
        c[:rows] = (c[:rows].float() + v[:rows].to(case.cdtype).float()).to(case.cdtype)
    else:
        c[:rows] = v[:rows].to(case.cdtype)
    cs = None
    if case.colsum:
        cs = inp["colsum0"] + A.sum(1)
        if drop_row:
            cs[-1] = inp["colsum0"][-1]
    return c_buf, cs


def gemm_ratio(case: GemmCase, c_buf_after: torch.Tensor) -> float:
    """max over the logical [M, N] of |got - ref| / bound."""
    ref, bound, _ = gemm_ref(case)
    got = view2d(c_buf_after.detach().cpu(), case.M, case.N).double()
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float((err / bound).max())


def colsum_ratio(case: GemmCase, colsum_after: torch.Tensor) -> float:
    ref, bound = gemm_ref(case)[2]
    err = (colsum_after.detach().cpu().double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float((err / bound).max())


def assert_outside_untouched(buf_after: torch.Tensor, buf_before: torch.Tensor, rows: int, cols: int, what: str) -> None:
    """Everything outside the logical [rows, cols] of a padded buffer is bit-equal to what it held before the call."""
    after, before = bits(buf_after), bits(buf_before)
    mask = torch.ones_like(before, dtype=torch.bool)
    mask[:rows, :cols] = False
    bad = (after != before) & mask
    if bad.any():
        r, c = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the logical [{rows}, {cols}] were written, first at row {r}, column {c}")


def gemm_check(case: GemmCase, c_buf_after: torch.Tensor, colsum_after: Optional[torch.Tensor] = None) -> float:
    inp = gemm_inputs(case)
    r = gemm_ratio(case, c_buf_after)
    print(f"gemm {case.name}: max |err| / bound = {r:.4f}")
    assert r <= 1.0, f"gemm {case.name}: error is {r:.3f} x the bound"
    assert_outside_untouched(c_buf_after, inp["c_buf"], case.M, case.N, f"gemm {case.name}")
    if case.colsum:
        rc = colsum_ratio(case, colsum_after)
        print(f"gemm {case.name}: fused column sums, max |err| / bound = {rc:.4f}")
        assert rc <= 1.0, f"gemm {case.name}: column-sum error is {rc:.3f} x the bound"
    return r


# ================================================================================================ element-wise

EW_EXTRA_VECS = 37                          # 16-byte vectors past one capped launch: 37 threads take the second sweep


def ew_n(dtype) -> int:
    """Past the 2048-block cap of the vectorised grid-stride loops with a scalar tail of 5.  The loops run over n / VEC vectors
    with 2048 * 256 threads, so 2048 * 256 * VEC + 5 alone reaches the second iteration only where 5 >= VEC (fp32: one thread,
    bf16: none); EW_EXTRA_VECS more vectors give both types a second sweep of several threads."""
    return (EW_CAP + EW_EXTRA_VECS) * VEC[dtype] + 5


def f32_scalar(x: float) -> torch.Tensor:
    return torch.tensor(x, dtype=F32)


@functools.lru_cache(maxsize=None)
def add_relu_inputs(dtype) -> dict:
    n = ew_n(dtype)
    a, b = rnd((n,), 11).to(dtype), rnd((n,), 12).to(dtype)
    scale = 0.37
    return dict(a=a, b=b, scale=scale,
                add=(a.float() + b.float()).to(dtype),                                                   # fp32 add, rounded once
                relu_bwd=torch.where(b.float() > 0, a.float() * f32_scalar(scale), f32_scalar(0.0)).to(dtype),
                add64=a.double() + b.double(), relu_bwd64=torch.where(b.double() > 0, a.double() * float(np.float32(scale)), 0.0))


def assert_rounded_once(got: torch.Tensor, ref64: torch.Tensor, dtype, what: str) -> None:
    """got is within half an ulp of the exact result: |got - ref| <= u |ref| with u = 2^-24 (fp32) or 2^-8 (bf16), plus the
    smallest subnormal for results that underflow."""
    u = U24 if dtype == F32 else 2.0 ** -8
    err = (got.double() - ref64).abs()
    assert bool((err <= u * ref64.abs() + 2.0 ** -149).all()), f"{what}: not a correctly rounded result"


@functools.lru_cache(maxsize=None)
def cast_inputs() -> dict:
    """fp32 values whose rounding to bf16 is decided by the rule, not the magnitude, at both ends of a buffer that is longer than
    one capped launch."""
    special_bits = [
        0x00000000, 0x80000000,              # +0, -0
        0x7F7F0000, 0xFF7F0000,              # the largest finite bf16
        0x3F808000, 0x3F818000,              # exactly halfway: ties to even go down (0x3F80) and up (0x3F82)
        0x3F808001, 0x3F807FFF,              # just above / below halfway
        0xBF808000, 0xBF818000,              # the same ties, negative
        0x7F7F8000,                          # halfway between the largest finite bf16 and 2^128: rounds to +inf
        0x7F7F7FFF,                          # just below: stays finite
        0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF,      # fp32 subnormals (ties among them too)
        0x00800000, 0x00FF8000,              # smallest normal; a tie that carries into the exponent
        0x7F800000, 0xFF800000,              # infinities
    ]
    sp = torch.tensor(np.array(special_bits, dtype=np.uint32).view(np.int32)).view(F32)
    n = ew_n(F32)
    x = rnd((n,), 13, -3.0, 3.0)
    x[:sp.numel()] = sp
    x[-sp.numel():] = sp
    return dict(x=x, nspecial=sp.numel())


@dataclass(frozen=True)
class DropCase:
    dtype: torch.dtype
    p: float = 0.25
    seed: int = 20240229


def drop_keep_np(seed: int, idx: np.ndarray, p: float) -> np.ndarray:
    """The library's keep decision for element indices `idx` (drop_keep of csrc/omr_common.h): one 32-bit hash per element
    pair, 16 bits each, keep iff bits >= round(p * 2^16).  Used by the CPU stand-in only."""
    idx = idx.astype(np.uint64)
    pair = idx >> np.uint64(1)
    x = (pair & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ ((pair >> np.uint64(32)).astype(np.uint32) * np.uint32(0x27D4EB2F))
    h = x * np.uint32(0x9E3779B1) + np.uint32(seed & 0xFFFFFFFF)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h += np.uint32((seed >> 32) & 0xFFFFFFFF)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    b = np.where((idx & np.uint64(1)).astype(bool), h >> np.uint32(16), h & np.uint32(0xFFFF))
    return b >= np.uint32(int(p * 65536.0 + 0.5))


def drop_scaled(x: torch.Tensor, p: float) -> torch.Tensor:
    """x / (1 - p) the way every dropout site computes it: an fp32 multiply by the fp32 value 1 / (1 - p), rounded once."""
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return (x.float() * f32_scalar(float(scale))).to(x.dtype)


@functools.lru_cache(maxsize=None)
def dropout_flat_input(dtype) -> torch.Tensor:
    return rnd((ew_n(dtype),), 14, 0.5, 1.5).to(dtype)          # no zeros: a dropped element is told from a kept one by its value


def dropout_flat_check(case: DropCase, x: torch.Tensor, out: torch.Tensor, out_again: torch.Tensor, out_prefix: torch.Tensor) -> None:
    """out, out_again = two calls on x; out_prefix = a call on x[:n0], n0 = the vector-loop part of one capped launch."""
    n, n0 = x.numel(), EW_CAP * VEC[case.dtype]
    out, out_again, out_prefix = out.cpu(), out_again.cpu(), out_prefix.cpu()
    assert_bit_equal(out_again, out, "dropout: second call")
    keep = out != 0
    want = torch.where(keep, drop_scaled(x, case.p), torch.zeros_like(x))
    assert_bit_equal(out, want, "dropout: kept values are x / (1 - p) rounded once, dropped ones +0")
    assert out_prefix.numel() == n0 and torch.equal(out_prefix != 0, keep[:n0]), "dropout: the mask of a prefix depends on the launch size"
    # the number of kept elements is Binomial(n, 1 - p): 4 standard deviations
    rate, sd = keep.double().mean().item(), math.sqrt(case.p * (1 - case.p) / n)
    print(f"dropout {TAG[case.dtype]}: keep rate {rate:.6f}, expected {1 - case.p} +- {sd:.2e}")
    assert abs(rate - (1 - case.p)) <= 4 * sd, f"dropout keep rate {rate} is {(rate - (1 - case.p)) / sd:.1f} standard deviations off"


def dropout_channel_shape(dtype):
    return (3, 7, 5, 24 if dtype == F32 else 40)


@functools.lru_cache(maxsize=None)
def dropout_channel_input(dtype) -> torch.Tensor:
    return rnd(dropout_channel_shape(dtype), 15, 0.5, 1.5).to(dtype)


def dropout_channel_check(x: torch.Tensor, out: torch.Tensor, p: float) -> None:
    out = out.cpu()
    keep = out != 0                                                   # [B, H, W, C]
    assert bool((keep == keep[:, :1, :1, :]).all()), "channel dropout: the mask changes over the pixels of a channel"
    per = keep[:, 0, 0, :]
    assert not bool((per == per[:1]).all()), "channel dropout: every sample has the same mask"
    assert 0 < int(per.sum()) < per.numel(), "channel dropout: nothing or everything dropped"
    assert_bit_equal(out, torch.where(keep, drop_scaled(x, p), torch.zeros_like(x)), "channel dropout: kept values")


def dropout_standin(x: torch.Tensor, p: float, seed: int, channel_mode: bool = False) -> torch.Tensor:
    if channel_mode:
        B, C = x.shape[0], x.shape[-1]
        keep = torch.from_numpy(drop_keep_np(seed, np.arange(B * C), p)).view(B, 1, 1, C).expand(x.shape)
    else:
        keep = torch.from_numpy(drop_keep_np(seed, np.arange(x.numel()), p)).view(x.shape)
    return torch.where(keep, drop_scaled(x, p), torch.zeros_like(x))


# ---- Adam
ADAM_N = EW_CAP + 77
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, grad_scale=0.5, steps=3)


@functools.lru_cache(maxsize=None)
def adam_inputs() -> dict:
    return dict(p=rnd((ADAM_N,), 16), grads=tuple(rnd((ADAM_N,), 17 + s) for s in range(ADAM["steps"])))


@functools.lru_cache(maxsize=None)
def adam_ref() -> torch.Tensor:
    """torch.optim.Adam's single-tensor recurrence in fp64 on grad_scale * g."""
    inp, h = adam_inputs(), ADAM
    p = inp["p"].double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step, g in enumerate(inp["grads"], start=1):
        g = g.double() * h["grad_scale"]
        m = h["b1"] * m + (1 - h["b1"]) * g
        v = h["b2"] * v + (1 - h["b2"]) * g * g
        bc1, bc2 = 1 - h["b1"] ** step, 1 - h["b2"] ** step
        p = p - (h["lr"] / bc1) * m / (v.sqrt() / math.sqrt(bc2) + h["eps"])
    return p


def adam_standin() -> torch.Tensor:
    inp, h = adam_inputs(), ADAM
    p = inp["p"].clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step, g in enumerate(inp["grads"], start=1):
        g = g * f32_scalar(h["grad_scale"])
        m = f32_scalar(h["b1"]) * m + (1 - f32_scalar(h["b1"])) * g
        v = f32_scalar(h["b2"]) * v + (1 - f32_scalar(h["b2"])) * g * g
        bc1, bc2 = 1 - h["b1"] ** step, 1 - h["b2"] ** step
        p = p - f32_scalar(h["lr"] / bc1) * (m / (v.sqrt() * f32_scalar(1 / math.sqrt(bc2)) + f32_scalar(h["eps"])))
    return p


def adam_check(p: torch.Tensor, p_lowp: Optional[torch.Tensor]) -> None:
    torch.testing.assert_close(p.cpu().double(), adam_ref(), rtol=1e-5, atol=1e-7)
    if p_lowp is not None:
        assert_bit_equal(p_lowp.cpu(), p.cpu().to(BF16), "adam: the bf16 copy is the rounded fp32 parameter")


# ---- column sums
COLSUM_M, COLSUM_N = 300, 70                 # three 128-row slabs, the last one short


@functools.lru_cache(maxsize=None)
def colsum_inputs(dtype) -> dict:
    buf = padded(COLSUM_M, COLSUM_N, dtype, float("nan"), ld=round_up(COLSUM_N, 8))
    view2d(buf, COLSUM_M, COLSUM_N).copy_(rnd((COLSUM_M, COLSUM_N), 21))
    return dict(buf=buf, db0=rnd((COLSUM_N,), 22) + 3.0)


def colsum_check(dtype, db: torch.Tensor) -> None:
    """db0 + column sums: M + 1 fp32 terms in an arbitrary order -> (M + 1) 2^-24 (|db0| + sum |x|) per column."""
    inp = colsum_inputs(dtype)
    x = view2d(inp["buf"], COLSUM_M, COLSUM_N).double()
    ref = inp["db0"].double() + x.sum(0)
    bound = (COLSUM_M + 1) * U24 * (inp["db0"].double().abs() + x.abs().sum(0))
    got = db.cpu().double()
    assert torch.isfinite(got).all(), "colsum: non-finite (the NaN padding was read)"
    r = float(((got - ref).abs() / bound).max())
    print(f"colsum {TAG[dtype]}: max |err| / bound = {r:.4f}")
    assert r <= 1.0, f"colsum: error is {r:.3f} x the bound"


# ---- argmax
NEG_INF, NAN = float("-inf"), float("nan")


@functools.lru_cache(maxsize=None)
def argmax_inputs(n: int) -> dict:
    """[5, ld] buffers, logical width n.  expect[i] = the required index, finite[i] = row i has a finite maximum."""
    assert n in (30, 600)
    ld = n + 10 if n == 30 else 640
    buf = rnd((5, ld), 23 + n)
    buf[:, n:] = rnd((5, ld - n), 24 + n) - 2.0                    # the padding holds ordinary, smaller values ...
    if n == 30:
        buf[0, 29] = 5.0                                           # a unique maximum in the last column
        buf[1, 3] = buf[1, 17] = 5.0                               # a tie: the first index wins
        buf[2, :n] = NEG_INF                                       # all -inf: index 0
        buf[3, 11] = 5.0
        buf[3, n:] = 100.0                                         # ... except here: larger values right behind the row
        buf[4, :n] = NAN                                           # all NaN: index 0, as torch.argmax
        expect = [29, 3, 0, 11, 0]
    else:
        buf[0, 3] = buf[0, 259] = buf[0, 515] = 5.0                # a tie inside one thread, across its loop iterations
        buf[1, 260] = buf[1, 7] = 5.0                              # a tie across threads: the later thread holds the smaller index
        buf[2, 515] = buf[2, 258] = 5.0                            # across threads and iterations
        buf[3, 599] = 5.0                                          # the last column
        buf[3, n:] = 100.0
        buf[4, :n] = NAN
        expect = [3, 7, 258, 599, 0]
    finite = [bool(torch.isfinite(buf[i, :n]).all()) for i in range(5)]
    return dict(buf=buf, n=n, expect=expect, finite=finite)


def argmax_standin(x: torch.Tensor):
    idx = torch.argmax(x, dim=1)
    return idx, x.gather(1, idx[:, None])[:, 0]


def argmax_check(n: int, idx: torch.Tensor, val: torch.Tensor) -> None:
    inp = argmax_inputs(n)
    idx, val = idx.cpu(), val.cpu()
    assert idx.dtype == torch.int64 and idx.tolist() == inp["expect"], f"argmax n={n}: indices {idx.tolist()}, expected {inp['expect']}"
    for i in range(5):
        if inp["finite"][i]:
            assert float(val[i]) == 5.0, f"argmax n={n}: row {i} value {float(val[i])}"


# ---- embedding
EMB_V, EMB_D, EMB_PAD = 50, 64, 0


@functools.lru_cache(maxsize=None)
def embed_fwd_inputs(dtype) -> dict:
    B, T = 2, 4100                                                # B T d = 524 800: past one capped launch
    table = rnd((EMB_V, EMB_D), 31).to(dtype)
    pe = rnd((T, EMB_D), 32)
    tok = torch.randint(0, EMB_V, (B, T), generator=torch.Generator().manual_seed(33))
    tok[0, 5] = tok[1, 4099] = -1
    tok[0, 4098] = tok[1, 0] = EMB_V
    valid = (tok >= 0) & (tok < EMB_V)
    e = torch.where(valid[..., None], table.float()[tok.clamp(0, EMB_V - 1)], f32_scalar(0.0))
    return dict(tok=tok, table=table, pe=pe, want=(e + pe[None]).to(dtype))        # out-of-range tokens: pe alone


@functools.lru_cache(maxsize=None)
def embed_bwd_inputs(dtype) -> dict:
    M = 4096
    choices = torch.tensor([3, 7, 11, 19, 42, EMB_PAD, -1, EMB_V])
    tok = choices[torch.randint(0, 8, (M,), generator=torch.Generator().manual_seed(34))]
    return dict(tok=tok, dout=rnd((M, EMB_D), 35).to(dtype))


def embed_bwd_standin(dtype) -> torch.Tensor:
    inp = embed_bwd_inputs(dtype)
    ok = (inp["tok"] > 0) & (inp["tok"] < EMB_V)
    return torch.zeros(EMB_V, EMB_D).index_add_(0, inp["tok"][ok], inp["dout"].float()[ok])


def embed_bwd_check(dtype, dtable: torch.Tensor) -> None:
    """dtable (zero before the call) against an fp64 index_add.  A row that `count` tokens hit is a sum of `count` fp32 atomics in
    an arbitrary order: (count + 1) 2^-24 sum |dout| per element."""
    inp = embed_bwd_inputs(dtype)
    tok, dout = inp["tok"], inp["dout"].double()
    ok = (tok != EMB_PAD) & (tok >= 0) & (tok < EMB_V)
    ref = torch.zeros(EMB_V, EMB_D, dtype=torch.float64).index_add_(0, tok[ok], dout[ok])
    sabs = torch.zeros(EMB_V, EMB_D, dtype=torch.float64).index_add_(0, tok[ok], dout[ok].abs())
    count = torch.bincount(tok[ok], minlength=EMB_V).double()[:, None]
    got = dtable.cpu().double()
    assert bool((bits(dtable[EMB_PAD]) == 0).all()), "embed bwd: the pad row received a gradient"
    bound = (count + 1) * U24 * sabs
    assert bool(((got - ref).abs() <= bound).all()), f"embed bwd: max error {float((got - ref).abs().max()):.3e} exceeds (count + 1) 2^-24 sum |dout|"
    assert int(count.max()) > 400                                     # heavy duplicates


# (dtype, C).  C = 12 in bf16 and C = 18 in fp32 are no multiple of the vector width: the scalar kernel.  C = 20 in fp32 is a multiple
# of 4 and takes the vector kernel with an odd number of fragments per pixel.
ADD_PE2D_CASES = ((F32, 20), (BF16, 12), (F32, 18))


@functools.lru_cache(maxsize=None)
def add_pe2d_inputs(dtype, C: int) -> dict:
    B, h, w, maxh, maxw = 2, 3, 5, 4, 7
    x, pe = rnd((B, h, w, C), 36).to(dtype), rnd((maxh, maxw, C), 37)
    return dict(x=x, pe=pe, want=(x.float() + pe[:h, :w]).to(dtype))


# ================================================================================================ LayerNorm

LN_EPS = 1e-5


@dataclass(frozen=True)
class LnCase:
    d: int
    M: int
    dtype: torch.dtype
    res: bool

    @property
    def name(self) -> str:
        return f"d{self.d}-M{self.M}-{TAG[self.dtype]}-{'res' if self.res else 'nores'}"

    @property
    def spread(self) -> float:
        # rows are 100 + spread * u.  bf16 cannot hold 100 + 0.1 u in ONE tensor (its spacing at 100 is 0.5), so without a
        # residual the bf16 rows are 100 + 2 u: still a mean ~90 standard deviations from 0.  With a residual x = 100 and
        # res = 0.1 u, and the fp32 sum x + res is exact.
        return 2.0 if (self.dtype == BF16 and not self.res) else 0.1

    @property
    def scale(self) -> float:
        """|gamma| / std: the size of one unit of the normalised row (what `scale` is in tests/test_kernels_gpu.py)."""
        return 2.5 * math.sqrt(3.0) / self.spread


LN_CASES = tuple(LnCase(d, M, dt, res) for d in (128, 256, 512) for M in (1, 3, 65) for dt in DTYPES for res in (True, False))


@functools.lru_cache(maxsize=None)
def ln_inputs(case: LnCase) -> dict:
    M, d = case.M, case.d
    u = rnd((M, d), 41 + d + M)
    if case.res:
        if case.dtype == BF16:
            x, res = torch.full((M, d), 100.0), case.spread * u
        else:
            x, res = 100.0 + case.spread * u, 0.01 * rnd((M, d), 42)
    else:
        x, res = 100.0 + case.spread * u, None
    flat = 1 if M >= 3 else None                                    # one all-equal row: out = beta, rstd = 1 / sqrt(eps)
    if flat is not None:
        x[flat] = 100.0
        if res is not None:
            res[flat] = 0.0
    x = x.to(case.dtype)
    res = None if res is None else res.to(case.dtype)
    gamma, beta = rnd((d,), 43) + 1.5, rnd((d,), 44)
    return dict(x=x, res=res, gamma=gamma, beta=beta, dy=rnd((M, d), 45).to(case.dtype), dgamma0=rnd((d,), 46) + 1.0, dbeta0=rnd((d,), 47) - 1.0,
                flat=flat)


def ln_fwd_ref(case: LnCase):
    inp = ln_inputs(case)
    s = inp["x"].double() + (inp["res"].double() if inp["res"] is not None else 0.0)
    mean = s.mean(1)
    var = ((s - mean[:, None]) ** 2).mean(1)                         # two passes
    rstd = 1.0 / torch.sqrt(var + float(np.float32(LN_EPS)))
    out = (s - mean[:, None]) * rstd[:, None] * inp["gamma"].double() + inp["beta"].double()
    return out, mean, rstd


def ln_bwd_ref(case: LnCase, mean: torch.Tensor, rstd: torch.Tensor):
    """The closed form in fp64 on what the backward entry is given: dy, x, res, gamma and the SAVED mean / rstd."""
    inp = ln_inputs(case)
    s = inp["x"].double() + (inp["res"].double() if inp["res"] is not None else 0.0)
    dy = inp["dy"].double()
    xhat = (s - mean.cpu().double()[:, None]) * rstd.cpu().double()[:, None]
    gh = dy * inp["gamma"].double()
    ds = rstd.cpu().double()[:, None] * (gh - gh.mean(1, keepdim=True) - xhat * (gh * xhat).mean(1, keepdim=True))
    return ds, inp["dgamma0"].double() + (dy * xhat).sum(0), inp["dbeta0"].double() + dy.sum(0)


def ln_standin(case: LnCase):
    inp = ln_inputs(case)
    s = inp["x"].float() + (inp["res"].float() if inp["res"] is not None else 0.0)
    mean = s.mean(1)
    t = s - mean[:, None]
    rstd = torch.rsqrt((t * t).mean(1) + LN_EPS)
    out = (t * rstd[:, None] * inp["gamma"] + inp["beta"]).to(case.dtype)
    dy = inp["dy"].float()
    xhat, gh = t * rstd[:, None], dy * inp["gamma"]
    ds = (rstd[:, None] * (gh - gh.mean(1, keepdim=True) - xhat * (gh * xhat).mean(1, keepdim=True))).to(case.dtype)
    return out, mean, rstd, ds, inp["dgamma0"] + (dy * xhat).sum(0), inp["dbeta0"] + dy.sum(0)


def ln_check(case: LnCase, out, mean, rstd, ds, dgamma, dbeta) -> None:
    inp = ln_inputs(case)
    out64, mean64, rstd64 = ln_fwd_ref(case)
    n = case.name
    check_close(out, out64, case.dtype, case.scale, f"ln {n} out")
    # the kernel normalises in fp32 and rounds once: hold bf16 rows to that too (3e-2 * scale is ~1.3 on outputs below 4)
    check_rounded_once(out, out64, case.dtype, case.scale, f"ln {n} out, fp32 value rounded once")
    check_close(mean, mean64, F32, 1.0, f"ln {n} mean")
    check_close(rstd, rstd64, F32, math.sqrt(3.0) / case.spread, f"ln {n} rstd")
    if inp["flat"] is not None:
        f = inp["flat"]
        check_close(out[f], inp["beta"].double(), case.dtype, 1.0, f"ln {n} all-equal row = beta")
        check_close(rstd[f], torch.tensor(1.0 / math.sqrt(float(np.float32(LN_EPS))), dtype=torch.float64), F32, 1.0, f"ln {n} all-equal row rstd")
    ds64, dg64, db64 = ln_bwd_ref(case, mean, rstd)
    check_close(ds, ds64, case.dtype, case.scale, f"ln {n} ds")
    check_rounded_once(ds, ds64, case.dtype, case.scale, f"ln {n} ds, fp32 value rounded once")
    check_close(dgamma, dg64, case.dtype, 8.0, f"ln {n} dgamma")      # 8: the scale tests/test_kernels_gpu.py gives sums over ~70 rows
    check_close(dbeta, db64, case.dtype, 8.0, f"ln {n} dbeta")


# ================================================================================================ InstanceNorm

IN_EPS = 1e-3


@dataclass(frozen=True)
class InCase:
    C: int
    dtype: torch.dtype
    HW: int
    const: bool = False

    @property
    def name(self) -> str:
        return f"C{self.C}-{TAG[self.dtype]}-HW{self.HW}" + ("-const" if self.const else "")


IN_WIDTHS = ((32, F32), (64, F32), (32, BF16), (64, BF16), (8, BF16), (4, F32))          # 8 / 4: the narrowest the entry accepts
IN_CASES = tuple(InCase(C, dt, HW) for C, dt in IN_WIDTHS for HW in (1, 3, 333))
IN_CONST_CASES = tuple(InCase(C, dt, 333, True) for C, dt in IN_WIDTHS)
IN_B = 2


@functools.lru_cache(maxsize=None)
def in_inputs(case: InCase) -> dict:
    shape = (IN_B, 1, case.HW, case.C)                               # NHWC
    x = torch.full(shape, 0.7) if case.const else torch.relu(rnd(shape, 51 + case.C) + 0.3)
    return dict(x=x.to(case.dtype), g=rnd(shape, 52 + case.C).to(case.dtype))


def in_stats_ref(case: InCase):
    x = in_inputs(case)["x"].double()
    mean = x.mean((1, 2))
    var = ((x - mean[:, None, None, :]) ** 2).mean((1, 2))
    return mean, 1.0 / torch.sqrt(var + float(np.float32(IN_EPS)))


def in_bwd_ref(case: InCase, mean, rstd, relu_mask: bool, relu_scale: float):
    """dx = rstd (g - mean_hw(g) - xhat mean_hw(g xhat)) in fp64 with the SAVED mean / rstd the entry is given."""
    inp = in_inputs(case)
    x, g = inp["x"].double(), inp["g"].double()
    mu, rs = mean.cpu().double()[:, None, None, :], rstd.cpu().double()[:, None, None, :]
    xhat = (x - mu) * rs
    dx = rs * (g - g.mean((1, 2), keepdim=True) - xhat * (g * xhat).mean((1, 2), keepdim=True))
    return torch.where(x > 0, dx * relu_scale, torch.zeros_like(dx)) if relu_mask else dx


def in_standin(case: InCase, mean=None, rstd=None, relu_mask: bool = False, relu_scale: float = 1.0):
    """One-pass statistics on fp32 squares summed in fp64, as the kernel has them; the backward in fp32."""
    inp = in_inputs(case)
    x, g = inp["x"].float(), inp["g"].float()
    if mean is None:
        m = x.double().mean((1, 2))
        var = ((x * x).double().mean((1, 2)) - m * m).clamp_min(0.0)
        return m.float(), (1.0 / torch.sqrt(var + float(np.float32(IN_EPS)))).float()
    mu, rs = mean[:, None, None, :], rstd[:, None, None, :]
    xhat = (x - mu) * rs
    dx = rs * (g - g.mean((1, 2), keepdim=True) - xhat * (g * xhat).mean((1, 2), keepdim=True))
    if relu_mask:
        dx = torch.where(x > 0, dx * relu_scale, torch.zeros_like(dx))
    return dx.to(case.dtype)


def in_check(case: InCase, mean, rstd, dx, dx_masked) -> None:
    n = case.name
    mean64, rstd64 = in_stats_ref(case)
    if case.const:
        x0 = float(in_inputs(case)["x"].flatten()[0])
        # a thread adds at most 4 pixels in fp32 at these sizes (3 roundings) and the mean is rounded to fp32 once: 4 x 2^-24
        assert bool(((mean.cpu().double() - x0).abs() <= 4 * U24 * x0).all()), f"in {n}: mean of a constant image {mean.flatten()[0].item()!r} vs {x0!r}"
        r0 = 1.0 / math.sqrt(float(np.float32(IN_EPS)))
        assert bool(((rstd.cpu().double() - r0).abs() <= 1e-6 * r0).all()), f"in {n}: rstd of a constant image {rstd.flatten()[0].item()!r} vs {r0!r}"
        assert torch.isfinite(dx.float()).all() and torch.isfinite(dx_masked.float()).all(), f"in {n}: non-finite backward"
    check_close(mean, mean64, F32, 1.0, f"in {n} mean")
    check_close(rstd, rstd64, F32, 5.0, f"in {n} rstd")
    check_close(dx, in_bwd_ref(case, mean, rstd, False, 1.0), case.dtype, 3.0, f"in {n} dx")
    check_close(dx_masked, in_bwd_ref(case, mean, rstd, True, 2.0), case.dtype, 6.0, f"in {n} dx masked")


# ================================================================================================ cross-entropy

CE_PAD = 0
CE_GRAD_SCALE, CE_GRAD_OUT = 0.5, 3.0


@dataclass(frozen=True)
class CeCase:
    dtype: torch.dtype
    V: int
    padded: bool                             # True: ldv = V rounded up to 8 (the vector path), NaN in the padding; False: ldv = V
    M: int = 1030                            # past the finalize kernel's 1024 threads
    inf: bool = False

    @property
    def name(self) -> str:
        return f"{TAG[self.dtype]}-V{self.V}-{'padded' if self.padded else 'contiguous'}" + ("-inf" if self.inf else "")

    @property
    def ldv(self) -> int:
        return round_up(self.V, 8) if self.padded else self.V


CE_CASES = tuple(CeCase(dt, 6997, pad) for dt in DTYPES for pad in (False, True)) + tuple(CeCase(dt, 30, True) for dt in DTYPES)
# 301 columns: one past 256 for every thread 0..44, and ldv = 301 is odd (the scalar path)
# 2101 columns in a padded buffer: every thread of the vector path gets a second 16-byte chunk (at column 1024 in fp32, 2048 in bf16),
# so thread 0 goes from a chunk of nothing but -inf to finite values -- with 301 columns it has that one chunk only
CE_INF_CASES = tuple(CeCase(dt, 301, pad, M=3, inf=True) for dt in DTYPES for pad in (False, True)) + \
    tuple(CeCase(dt, 2101, True, M=3, inf=True) for dt in DTYPES)


@functools.lru_cache(maxsize=None)
def ce_inputs(case: CeCase) -> dict:
    M, V = case.M, case.V
    lo, amp = (80.0, 30.0) if case.dtype == F32 else (20.0, 8.0)
    logits = lo + amp * rnd((M, V), 61 + V)
    tgt = torch.randint(1, V, (M,), generator=torch.Generator().manual_seed(62))
    if case.inf:
        logits[0, :16] = NEG_INF                                    # whole 16-byte chunks of -inf at the start of the row ...
        logits[0, 270] = NEG_INF                                    # ... and one in the second sweep
        logits[1, :] = NEG_INF                                      # a single finite entry
        logits[1, 100] = lo
        tgt[0], tgt[1] = 20, 100
    else:
        logits[7, 11] = logits[7].max() + 60.0                      # a lone spike 60 above the rest of its row
        tgt[3], tgt[4], tgt[5], tgt[M - 1] = CE_PAD, -1, V, CE_PAD  # all three count as ignored
    buf = torch.full((M, case.ldv), NAN, dtype=case.dtype)
    buf[:, :V] = logits
    return dict(buf=buf, tgt=tgt)


@functools.lru_cache(maxsize=None)
def ce_ref(case: CeCase) -> dict:
    inp = ce_inputs(case)
    x, tgt = inp["buf"][:, :case.V].double(), inp["tgt"]
    mx = x.max(1, keepdim=True).values
    lse = (mx + torch.log(torch.exp(x - mx).sum(1, keepdim=True)))[:, 0]
    live = (tgt != CE_PAD) & (tgt >= 0) & (tgt < case.V)
    t = tgt.clamp(0, case.V - 1)
    count = int(live.sum())
    loss = float(((lse - x.gather(1, t[:, None])[:, 0]) * live).sum() / count)
    soft = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(x).scatter_(1, t[:, None], 1.0)
    dl = (soft - onehot) * (CE_GRAD_SCALE * CE_GRAD_OUT / count) * live[:, None]
    return dict(lse=lse, loss=loss, count=count, live=live, dlogits=dl)


def ce_standin(case: CeCase):
    inp = ce_inputs(case)
    x, tgt = inp["buf"][:, :case.V].float(), inp["tgt"]
    lse = torch.logsumexp(x, 1)
    live = (tgt != CE_PAD) & (tgt >= 0) & (tgt < case.V)
    t = tgt.clamp(0, case.V - 1)
    count = float(live.sum())
    loss = ((lse - x.gather(1, t[:, None])[:, 0]).double() * live).sum() / count
    onehot = torch.zeros_like(x).scatter_(1, t[:, None], 1.0)
    dl = torch.zeros((case.M, case.ldv), dtype=case.dtype)
    d = (torch.exp(x - lse[:, None]) - onehot) * f32_scalar(CE_GRAD_SCALE * CE_GRAD_OUT / count)
    dl[:, :case.V] = torch.where(live[:, None], d, f32_scalar(0.0)).to(case.dtype)
    return loss.float().view(1), lse, torch.tensor([float(loss) * count, count], dtype=torch.float64), dl


def ce_check(case: CeCase, loss, lse, acc2, dl_full) -> None:
    """dl_full: the whole [M, ldv] gradient buffer, padding columns included."""
    ref, n = ce_ref(case), case.name
    inp = ce_inputs(case)
    check_close(lse, ref["lse"], F32, 1.0, f"ce {n} lse")
    rel = abs(float(loss.cpu()[0]) - ref["loss"]) / abs(ref["loss"])
    print(f"ce {n}: loss {float(loss.cpu()[0])!r} vs {ref['loss']!r} (relative {rel:.2e})")
    assert rel <= (1e-4 if case.dtype == F32 else 1e-2), f"ce {n}: loss off by {rel:.2e} relative"
    assert float(acc2.cpu()[1]) == float(ref["count"]), f"ce {n}: live-row count {float(acc2.cpu()[1])} vs {ref['count']}"
    dl_full = dl_full.detach().cpu()
    assert tuple(dl_full.shape) == (case.M, case.ldv)
    # |dlogits| <= grad_scale grad_out / count: that is the size the absolute tolerance is scaled to
    check_close(dl_full[:, :case.V], ref["dlogits"], case.dtype, CE_GRAD_SCALE * CE_GRAD_OUT / ref["count"], f"ce {n} dlogits")
    assert bool((bits(dl_full[:, case.V:]) == 0).all()), f"ce {n}: dlogits padding columns are not +0"
    assert bool((bits(dl_full[~ref["live"]]) == 0).all()), f"ce {n}: ignored rows have a gradient"
    if case.inf:
        neg = torch.isinf(inp["buf"][:, :case.V].float())
        assert bool((dl_full[:, :case.V][neg] == 0).all()), f"ce {n}: -inf columns have a gradient"
