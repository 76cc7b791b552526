"""Float64 references, the exact-sum argument, mirrors of the launch arithmetic and the shared case table for the specialised
GEMMs: the panel kernel (csrc/gemm_panel.hip), the DMA-fed tall kernel (csrc/gemm_tall.hip), the grouped weight gradient
(gemm_dw_grouped_kernel of csrc/gemm.hip) and the row-group views of omr_gemm that feed all three from the packed in_proj
parameters.

tests/test_gemm_branches_gpu.py runs every case below through the HIP kernels; tests/test_gemm_refs_cpu.py runs the same cases
with torch CPU arithmetic in the kernels' formats standing in for them, which shows without a GPU that a correct implementation
passes every check and that a list of subtly wrong ones does not.

Most cases are EXACT: A holds {-1, 0, 1}, B integers of [-2, 2], the bias and an accumulate target small integers, so every
product and every partial sum is an integer below 2^24 and fp32 accumulation is exact in ANY order (MFMA chains, split-K,
atomics).  For a bf16 C the ranges keep every |ref| <= 256: an integer of that size IS a bf16 number, so the rounding of the
output cannot hide an error of one unit and the output must equal the fp64 reference bit for bit, at every element.  Both
conditions belong to a case and are asserted (`check`), not assumed.  One BOUNDED case per kernel, with real-valued operands,
checks what integers cannot -- fp32 accumulation across k-tiles and a single rounding to bf16 -- per element against the bound of
oracle/kernel_refs.gemm_ref.

Operands are views into NaN-filled buffers (ld > width, guard rows in front and behind; in a grouped operand every row outside
the view -- the Q rows of [Wq;Wk;Wv] -- is NaN too), C is a view into a sentinel-filled buffer with ldc > N and rows past M, and
the whole buffer is compared, so a read or a write outside the logical extent shows.  No rows are sampled anywhere.

The library does not report which kernel ran.  `gemm_route`, `tall_plan` and `dw_plan` restate the acceptance conditions and
the grid arithmetic of the launchers, so a test can assert that its case meets the conditions of the branch it is named for
instead of passing for the wrong reason; that is all a route named here claims.

Test infrastructure only: nothing here is imported by the package.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from oracle.conv_refs import ints, on_device
from oracle.kernel_refs import (BF16, F32, GEMM_FACTOR, SENTINEL, TAG, U24, VEC, assert_bit_equal, assert_outside_untouched, padded, rnd,
                                round_up)

NAN = float("nan")
GUARD = 2                                    # NaN rows in front of and behind every operand
NUM_CU = 256                                 # csrc/launch_setup.h: OMR_NUM_CU, the cap of the tall kernel's persistent grid
TALL_TM, TALL_N, TALL_BK, TALL_MIN_TILES, TALL_NST = 256, 256, 64, 192, 2      # csrc/gemm_tall.hip
PANEL_PM, PANEL_PN, PANEL_MIN_M, PANEL_MIN_N = 256, 64, 200 * 256, 8 * 64      # csrc/gemm_panel.hip
TILE = 128                                   # BM = BN of the tile kernel (csrc/gemm.hip)
DW_MAX = 24                                  # problems per kernel-argument table (csrc/gemm.hip)


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def bk_of(dtype) -> int:
    return 64 if dtype == BF16 else 32       # GemmCfg<T>::BK


# ================================================================================================ cases of omr_gemm

@dataclass(frozen=True)
class Case:
    """One omr_gemm call: C[M, N] (+)= act(opA(A) . opB(B)^T + bias).  group = (rows per group, physical stride, first row inside
    a group, operand) is the row-group view; `route` the kernel whose acceptance conditions the case is built to meet."""
    name: str
    route: str                               # "tall" | "panel" | "tile"
    dtype: torch.dtype
    cdtype: torch.dtype
    M: int
    N: int
    K: int
    ta: bool = False
    tb: bool = False
    bias: bool = False
    relu: bool = False
    accumulate: bool = False
    split_k: int = 1
    colsum: bool = False
    group: Optional[Tuple[int, int, int, int]] = None
    exact: bool = True
    fullk: Optional[bool] = None             # tile kernel: whether the case must take the FULLK branch (None: not part of the case)

    @property
    def a_shape(self) -> Tuple[int, int]:
        return (self.K, self.M) if self.ta else (self.M, self.K)

    @property
    def b_shape(self) -> Tuple[int, int]:
        """The LOGICAL B as stored: [N, K], or [K, N] with tb."""
        return (self.K, self.N) if self.tb else (self.N, self.K)

    @property
    def lda(self) -> int:
        return round_up(self.a_shape[1], VEC[self.dtype]) + VEC[self.dtype]

    @property
    def ldb(self) -> int:
        return round_up(self.b_shape[1], VEC[self.dtype]) + VEC[self.dtype]

    @property
    def ldc(self) -> int:
        return round_up(self.N, 8) + 8

    @property
    def operand(self) -> int:
        return self.group[3] if self.group else 0

    @property
    def splits(self) -> int:
        """omr_gemm: the k range is cut into pieces of whole k-tiles, which may give fewer splits than asked for."""
        bk = bk_of(self.dtype)
        return cdiv(self.K, cdiv(cdiv(self.K, self.split_k), bk) * bk)


def group_rows(n: int, group) -> torch.Tensor:
    """Physical row of each of the n logical rows of a row-group view (csrc/gemm_args.h)."""
    grp, stride, base = group[:3]
    i = torch.arange(n)
    return (i // grp) * stride + base + i % grp


def phys_rows(n: int, group) -> int:
    """Rows of the physical block behind n logical rows: whole [Wq;Wk;Wv] blocks."""
    return (n // group[0]) * group[1]


T2_M = 257 * 256 + 37                        # 258 row tiles: two workgroups of the 256 walk a second tile, one of them the ragged one
TALL = dict(dtype=BF16, cdtype=BF16, N=256, tb=True)
TALL_CASES = (
    Case("T1-192tiles-k64", "tall", M=192 * 256, K=64, **TALL),                                   # fewest tiles, prologue only
    Case("T2-258tiles-ragged-k192", "tall", M=T2_M, K=192, **TALL),                               # second sweep, three k-tiles in two stages
    Case("T3-258tiles-rowgroups-k384", "tall", M=T2_M, K=384, group=(128, 192, 64, 2), **TALL),   # d = 64, L = 3: two k-tiles per group
    Case("T4-bounded-k640", "tall", M=192 * 256 + 5, K=640, exact=False, **TALL),
)
TALL_NEIGHBOURS = (
    Case("T-neighbour-k96", "tile", M=192 * 256, K=96, **TALL),                                   # K % 64 != 0
    Case("T-neighbour-191tiles", "tile", M=191 * 256, K=64, **TALL),                              # fewer row tiles than the kernel takes
)
PANEL = dict(dtype=BF16, cdtype=BF16)
PANEL_CASES = (
    Case("P1-smallest-nobias", "panel", M=200 * 256, N=512, K=128, **PANEL),
    Case("P2-ragged-9tiles-bias", "panel", M=200 * 256 + 77, N=576, K=256, bias=True, **PANEL),   # nine column tiles: the last one in buffer 0
    Case("P3-rowgroups", "panel", M=200 * 256, N=512, K=128, bias=True, group=(256, 384, 128, 1), **PANEL),      # d = 128, L = 2
    Case("P4-bounded-k256", "panel", M=200 * 256, N=512, K=256, bias=True, exact=False, **PANEL),
)
PANEL_NEIGHBOURS = (
    Case("P-neighbour-m-1", "tile", M=200 * 256 - 1, N=512, K=128, bias=True, **PANEL),
    Case("P-neighbour-n520", "tile", M=200 * 256, N=520, K=128, bias=True, **PANEL),
    Case("P-neighbour-relu", "tile", M=200 * 256, N=512, K=128, bias=True, relu=True, **PANEL),
)


def _tile_group_cases():
    """The tile kernel through the three row-group operands at GemmCase's ragged sizes, d = 64 (groups of 2d = 128 rows in blocks
    of 3d = 192), fp32 and bf16."""
    out = []
    for dt in (F32, BF16):
        t, g = TAG[dt], (128, 192, 64)
        # operand 1: the forward, N = L 2d = 384 over the K|V rows of B and of the bias; K = 70 ends in a partial 16-byte chunk
        out.append(Case(f"G1-{t}-operand1", "tile", dt, dt, M=130, N=384, K=70, bias=True, group=g + (1,), fullk=True))
        # operand 2, K = L 2d = 256: in bf16 the FULLK branch, which resolves the group per 64-wide slab
        out.append(Case(f"G2-{t}-operand2-k256", "tile", dt, dt, M=130, N=70, K=256, tb=True, group=g + (2,), fullk=dt == BF16))
        # operand 2, K = 384: the pipelined loop for both types
        out.append(Case(f"G2-{t}-operand2-k384", "tile", dt, dt, M=130, N=70, K=384, tb=True, group=g + (2,), fullk=False))
        # operand 3: the weight gradient with split-K and fused column sums, M = L 2d = 384 rows of dW / entries of db
        out.append(Case(f"G3-{t}-operand3-split3-colsum", "tile", dt, F32, M=384, N=70, K=301, ta=True, tb=True, accumulate=True, split_k=3,
                        colsum=True, group=g + (3,), fullk=False))
    return tuple(out)


TILE_GROUP_CASES = _tile_group_cases()
CASES = TALL_CASES + TALL_NEIGHBOURS + PANEL_CASES + PANEL_NEIGHBOURS + TILE_GROUP_CASES
BOUNDED_CASES = tuple(c for c in CASES if not c.exact)


def case(name: str) -> Case:
    return next(c for c in CASES if c.name.startswith(name))


# ------------------------------------------------------------------------------------------------ mirrors of the launch arithmetic

def gemm_route(c: Case, aligned: bool = True) -> str:
    """The kernel omr_gemm hands the case to: the acceptance conditions of omr_gemm, omr_gemm_panel_bf16 and omr_gemm_tall_bf16,
    restated.  `aligned`: A, B and C start on 16 bytes (the GPU test asserts it of its pointers)."""
    bf = c.dtype == BF16 and c.cdtype == BF16
    ld8 = c.lda % 8 == 0 and c.ldb % 8 == 0
    if (bf and not c.ta and not c.tb and not c.relu and not c.accumulate and c.splits == 1 and not c.colsum and ld8
            and c.K in (128, 256) and c.N % PANEL_PN == 0 and c.M >= PANEL_MIN_M and c.N >= PANEL_MIN_N and c.ldc % 8 == 0 and aligned
            and c.operand in (0, 1)):
        return "panel"
    if (bf and not c.ta and c.tb and c.splits == 1
            and c.N == TALL_N and c.K % TALL_BK == 0 and c.K >= TALL_BK and not (c.bias or c.relu or c.accumulate or c.colsum)
            and ld8 and c.ldc % 8 == 0 and aligned and (c.operand == 0 or (c.operand == 2 and c.group[0] % TALL_BK == 0))
            and cdiv(c.M, TALL_TM) >= TALL_MIN_TILES):
        return "tall"
    return "tile"


def tile_fullk(c: Case) -> bool:
    """launch<T, TC> of csrc/gemm.hip: all k-slabs requested up front."""
    return not c.ta and c.splits == 1 and c.K <= 4 * bk_of(c.dtype)


def tall_plan(M: int) -> dict:
    """Row tiles, grid (min(mt, OMR_NUM_CU)) and the walk of the busiest workgroup of gemm_tall_kernel (tile += gridDim.x)."""
    mt = cdiv(M, TALL_TM)
    grid = min(mt, NUM_CU)
    return dict(tiles=mt, grid=grid, busiest=cdiv(mt, grid), second_sweep=max(mt - grid, 0), last_rows=M - (mt - 1) * TALL_TM,
                last_tile_owner=(mt - 1) % grid)


def dw_plan(problems, dtype) -> List[dict]:
    """omr_linear_wgrad_grouped, per problem (rows, n_out, n_in): the split factor (the call's problems together should give ~2048
    workgroups, none reducing fewer than 512 rows), the k range of a split, the first block and the argument table (DW_MAX
    problems each, block numbering restarts per table)."""
    bk = bk_of(dtype)
    tiles_total = sum(cdiv(n_out, TILE) * cdiv(n_in, TILE) for _, n_out, n_in in problems)
    out, block0 = [], 0
    for i, (rows, n_out, n_in) in enumerate(problems):
        if i % DW_MAX == 0:
            block0 = 0
        mt, nt = cdiv(n_out, TILE), cdiv(n_in, TILE)
        want = max(1, min(cdiv(2048, tiles_total), cdiv(rows, 512)))
        ksplit_len = cdiv(cdiv(rows, want), bk) * bk
        splits = cdiv(rows, ksplit_len)
        total = nt * mt * splits
        chunk = nt * mt if splits > 1 else nt
        blocks = cdiv(total // chunk, 8) * 8 * chunk
        out.append(dict(table=i // DW_MAX, block0=block0, blocks=blocks, splits=splits, ksplit_len=ksplit_len, mt=mt, nt=nt,
                        last_split_rows=rows - (splits - 1) * ksplit_len))
        block0 += blocks
    return out


# ------------------------------------------------------------------------------------------------ inputs

def guarded2d(t: torch.Tensor, dtype, ld: int) -> torch.Tensor:
    """`t` [rows, cols] as a view into a NaN-filled [GUARD + rows + GUARD, ld] buffer (ld a multiple of the 16-byte vector, so the
    view starts on 16 bytes)."""
    rows, cols = t.shape
    assert ld > cols and ld % VEC[dtype] == 0
    buf = torch.full((rows + 2 * GUARD, ld), NAN, dtype=dtype)
    view = buf[GUARD:GUARD + rows, :cols]
    view.copy_(t)
    return view


def scattered(t: torch.Tensor, group, fill: float) -> torch.Tensor:
    """The logical rows (or entries) `t` at their physical places in a block full of `fill`."""
    full = torch.full((phys_rows(t.shape[0], group),) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    full[group_rows(t.shape[0], group)] = t
    return full


def _seed(name: str) -> int:
    return 5000 + 13 * sum((i + 1) * ord(ch) for i, ch in enumerate(name))


@functools.lru_cache(maxsize=None)
def inputs(c: Case) -> dict:
    """CPU tensors of a case, never modified (callers clone what a kernel writes into): a, b = operand views (b the PHYSICAL block for
    operands 1 / 2), bias (fp32, physical for operand 1) or None, c_buf = the whole C buffer (physical rows for operand 3), colsum0
    (physical) or None."""
    s, dt = _seed(c.name), c.dtype
    if c.exact:
        a, b = ints(c.a_shape, s, -1, 1), ints(c.b_shape, s + 1, -2, 2)
        bias = ints((c.N,), s + 2, -3, 3) if c.bias else None
    else:
        a, b = rnd(c.a_shape, s), rnd(c.b_shape, s + 1)
        bias = rnd((c.N,), s + 2) if c.bias else None
    if c.operand == 1:
        b = scattered(b, c.group, NAN)
        bias = scattered(bias, c.group, NAN) if bias is not None else None
    elif c.operand == 2:
        b = scattered(b, c.group, NAN)
    c_rows = phys_rows(c.M, c.group) if c.operand == 3 else c.M
    c_buf = padded(c_rows, c.N, c.cdtype, SENTINEL, ld=c.ldc)
    out = dict(a=guarded2d(a, dt, c.lda), b=guarded2d(b, dt, c.ldb), bias=bias, c_buf=c_buf, colsum0=None)
    if c.accumulate:
        assert c.exact
        c_buf[c_rows_of(c), :c.N] = ints((c.M, c.N), s + 3, -3, 3).to(c.cdtype)
    if c.colsum:
        cs = ints((c.M,), s + 4, -3, 3)
        out["colsum0"] = scattered(cs, c.group, SENTINEL) if c.operand == 3 else cs
    return out


def c_rows_of(c: Case) -> torch.Tensor:
    """Rows of c_buf that hold the logical C."""
    return group_rows(c.M, c.group) if c.operand == 3 else torch.arange(c.M)


def logical(c: Case, inp: Optional[dict] = None, device="cpu", base_ignored: bool = False):
    """(A [M, K], B [N, K], bias [N] or None) as stored, in fp64 on `device`.  base_ignored: the view read from the first row of every
    group (a kernel that drops grp_base), which brings in the NaN of the Q rows."""
    inp = inp or inputs(c)
    a, b, bias = inp["a"].to(device).double(), inp["b"].to(device).double(), inp["bias"]
    bias = None if bias is None else bias.to(device).double()
    g = c.group[:2] + (0,) if (c.group and base_ignored) else c.group
    if c.operand == 1:
        rows = group_rows(c.N, g).to(device)
        b, bias = b[rows], (None if bias is None else bias[rows])
    elif c.operand == 2:
        b = b[group_rows(c.K, g).to(device)]
    return (a.t() if c.ta else a), (b.t() if c.tb else b), bias


def expected(c: Case, device="cpu") -> dict:
    """fp64 on `device`: ref [M, N], sabs = sum_k |a||b| [M, N], bound (kernel_refs.gemm_ref's) and, with column sums, cs_ref [M] and
    cs_abs = sum_k |a| [M].  torch's own float64 matmul: independent of the code under test."""
    inp = inputs(c)
    A, B, bias = logical(c, inp, device)
    ref, sabs = A @ B.t(), A.abs() @ B.abs().t()
    extra = torch.zeros((), dtype=torch.float64, device=device)          # |bias| + |c0|: the other addends of an element's sum
    if bias is not None:
        ref, extra = ref + bias, extra + bias.abs().max()
    if c.relu:
        ref = ref.clamp_min(0.0)
    if c.accumulate:
        c0 = inp["c_buf"][c_rows_of(c), :c.N].to(device).double()
        ref, extra = ref + c0, extra + c0.abs().max()
    bound = GEMM_FACTOR * (c.K + 2) * U24 * sabs
    if c.cdtype == BF16:
        bound = bound + 2.0 ** -8 * ref.abs()
    out = dict(ref=ref, sabs=sabs, bound=bound, extra=float(extra))
    if c.colsum:
        cs0 = inp["colsum0"][c_rows_of(c)] if c.operand == 3 else inp["colsum0"]
        out["cs_ref"], out["cs_abs"] = cs0.to(device).double() + A.sum(1), cs0.to(device).double().abs() + A.abs().sum(1)
    return out


@functools.lru_cache(maxsize=None)
def summary(c: Case, device: str = "cpu") -> dict:
    """What `check` keeps of `expected` (cached: the CPU twin checks a case many times).  top = the largest sum of |products| plus
    |bias| and |accumulate target|, max_ref = max |ref|; EXACT: want = the reference in the C type (on the host; exact, the
    conditions hold) and cs_want; BOUNDED: ref and bound."""
    exp = expected(c, torch.device(device))
    out = dict(top=float(exp["sabs"].max()) + exp["extra"], max_ref=float(exp["ref"].abs().max()))
    if c.exact:
        out["want"] = exp["ref"].to(c.cdtype).cpu()
        if c.colsum:
            out["cs_top"], out["cs_want"] = float(exp["cs_abs"].max()), exp["cs_ref"].float().cpu()
    else:
        out["ref"], out["bound"] = exp["ref"], exp["bound"]
    return out


def assert_exact_conditions(c: Case, device: str = "cpu") -> None:
    """What the exactness argument rests on, per case: every sum of |products| (plus bias and accumulate target) below 2^24, and for
    a bf16 C every |ref| <= 256."""
    s = summary(c, device)
    assert s["top"] < 2.0 ** 24, f"{c.name}: partial sums reach {s['top']:.3g}, not below 2^24: the case is not exact in fp32"
    if c.cdtype == BF16:
        assert s["max_ref"] <= 256.0, f"{c.name}: max |ref| = {s['max_ref']} > 256: a bf16 C could round an error away"
    if c.colsum:
        assert s["cs_top"] < 2.0 ** 24


def check(c: Case, c_buf_after: torch.Tensor, colsum_after: Optional[torch.Tensor] = None) -> Optional[float]:
    """EXACT: the whole C buffer (padding, rows past M, Q rows) equals, bit for bit, the buffer before the call with the fp64
    reference at the logical elements; the same for the column sums.  BOUNDED: per element within the bound, C's surroundings
    untouched; returns max |err| / bound.  The reference is formed on the device the output lives on."""
    inp, dev = inputs(c), str(c_buf_after.device)
    exp = summary(c, dev)
    rows = c_rows_of(c)
    if c.exact:
        assert_exact_conditions(c, dev)
        want = inp["c_buf"].clone()
        want[rows, :c.N] = exp["want"]
        got = c_buf_after.detach().cpu()
        if c.operand != 3:
            assert_bit_equal(got[:c.M, :c.N], want[:c.M, :c.N], f"gemm {c.name}: C")
            assert_outside_untouched(got, inp["c_buf"], c.M, c.N, f"gemm {c.name}")
        assert_bit_equal(got, want, f"gemm {c.name}: the whole C buffer")
        if c.colsum:
            want_cs = inp["colsum0"].clone()
            want_cs[rows] = exp["cs_want"]
            assert_bit_equal(colsum_after.detach().cpu(), want_cs, f"gemm {c.name}: fused column sums")
        return None
    got = c_buf_after.detach()[:c.M, :c.N].double()
    err = (got - exp["ref"]).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = float((err / exp["bound"]).max())
    print(f"gemm {c.name}: max |err| / bound = {r:.4f}")
    assert r <= 1.0, f"gemm {c.name}: error is {r:.3f} x the bound"
    assert_outside_untouched(c_buf_after, inp["c_buf"], c.M, c.N, f"gemm {c.name}")
    return r


# ------------------------------------------------------------------------------------------------ stand-ins

TALL_FAULTS = ("drop_last_ktile", "stale_ktile", "second_sweep_repeats", "chunk_permute", "ignore_group_base", "write_past_M",
               "round_between_ktiles")
PANEL_FAULTS = ("bias_next_tile", "garbage_no_bias", "skip_last_tile", "stale_c_image")


def standin(c: Case, fault: Optional[str] = None):
    """torch CPU arithmetic in the kernels' formats -- fp32 products and sums, one rounding to the C type (an accumulate target is
    fp32 here) -- -> (C buffer, column sums or None).  fp32 is exact for the integer cases, whatever torch's summation order.
    `fault` makes it one of the wrong implementations of TALL_FAULTS / PANEL_FAULTS."""
    inp = inputs(c)
    A, B, bias = (None if t is None else t.float() for t in logical(c, inp, base_ignored=fault == "ignore_group_base"))
    A, B = A.contiguous(), B.contiguous()
    bk = TALL_BK
    if fault == "drop_last_ktile":                                        # the wait in front of the last k-tile lets nothing land
        A[:, c.K - bk:] = 0
    elif fault == "stale_ktile":                                          # k-tile 2 computed on what its stage held before: k-tile 0
        A[:, 2 * bk:3 * bk], B[:, 2 * bk:3 * bk] = A[:, :bk].clone(), B[:, :bk].clone()
    elif fault == "chunk_permute":                                        # rows of one swizzle class: 16-byte chunks 0 and 1 of k-tile 0 swapped
        m = torch.arange(c.M)
        sel = ((m >> 1) & 7) == 5
        A[sel, 0:16] = torch.cat([A[sel, 8:16], A[sel, 0:8]], dim=1)
    if fault == "round_between_ktiles":                                   # the accumulator kept in bf16 from one k-tile to the next
        v = torch.zeros((c.M, c.N))
        for k0 in range(0, c.K, bk):
            v = (v + A[:, k0:k0 + bk] @ B[:, k0:k0 + bk].t()).to(BF16).float()
    else:
        v = A @ B.t()
    if bias is not None:
        if fault == "bias_next_tile":                                     # the bias image of the other buffer
            bias = bias.roll(-PANEL_PN)
        v = v + bias
    if fault == "garbage_no_bias":                                        # the zero array indexed like a real bias: whatever lies behind it
        assert bias is None
        v[:, PANEL_PN:] += 1.0
    if c.relu:
        v = v.clamp_min(0.0)
    if fault == "second_sweep_repeats":                                   # the row base not advanced with the tile
        p = tall_plan(c.M)
        for t in range(p["grid"], p["tiles"]):
            n = min(TALL_TM, c.M - t * TALL_TM)
            v[t * TALL_TM:t * TALL_TM + n] = v[(t - p["grid"]) * TALL_TM:(t - p["grid"]) * TALL_TM + n].clone()
    if fault == "stale_c_image":                                          # the last column tile stored from the image of two tiles earlier
        nt = c.N // PANEL_PN
        v[:, (nt - 1) * PANEL_PN:] = v[:, (nt - 3) * PANEL_PN:(nt - 2) * PANEL_PN].clone()
    c_buf = inp["c_buf"].clone()
    rows = c_rows_of(c)
    ncols = c.N - PANEL_PN if fault == "skip_last_tile" else c.N
    if c.accumulate:
        c_buf[rows, :ncols] = (c_buf[rows, :ncols].float() + v[:, :ncols]).to(c.cdtype)
    else:
        c_buf[rows, :ncols] = v[:, :ncols].to(c.cdtype)
    if fault == "write_past_M":                                           # the row guard of the store off by one
        c_buf[c.M, :c.N] = c_buf[c.M - 1, :c.N]
    cs = None
    if c.colsum:
        cs = inp["colsum0"].clone()
        cs[rows] += A.sum(1)
    return c_buf, cs


# ================================================================================================ grouped weight gradient

@dataclass(frozen=True)
class DwProblem:
    """dW[n_out, n_in] += dY^T X, db[n_out] += column sums of dY, reduced over `rows`."""
    rows: int
    n_out: int
    n_in: int
    db: bool = True
    pad: bool = True                         # dY and X in rows longer than their width (a strided dY: logit rows with a padded pitch)
    ld_dw: int = 0                           # 0: n_in (contiguous dW); else a pitch whose padding must stay bit-equal
    group: Optional[Tuple[int, int, int]] = None

    @property
    def shape(self) -> Tuple[int, int, int]:
        return self.rows, self.n_out, self.n_in


def _dw_problems():
    base = [
        DwProblem(300, 128, 128, ld_dw=136),                              # one split (rows <= 512), one tile
        DwProblem(1000, 256, 256),                                        # split-K, 2 x 2 tiles
        DwProblem(77, 200, 136, pad=False),                               # rows no multiple of 64 or 32; n_out and n_in tails; contiguous operands
        DwProblem(513, 50, 256, ld_dw=264),                               # n_out tail; the second split reduces 193 / 225 rows: a tail of 1; two N tiles
        DwProblem(2048, 256, 128, db=False),                              # four splits; no bias gradient
        DwProblem(640, 256, 64, group=(128, 384, 128)),                   # rows [128, 256) of two 384-row blocks: the Q rows must stay as they were
    ]
    probs = [base[i % len(base)] for i in range(24)]
    probs.append(DwProblem(1100, 136, 200, ld_dw=208))                    # the 25th: first of the second argument table; 2 x 2 ragged tiles, 3 splits
    return tuple(probs)


DW_CALLS: Dict[str, Tuple[Tuple[DwProblem, ...], bool]] = {
    "25-problems": (_dw_problems(), True),
    "single-problem": ((DwProblem(4096, 256, 256, ld_dw=272),), True),   # alone in its call: 8 splits of 512 rows
    "single-bounded": ((DwProblem(4096, 256, 256),), False),             # real-valued
}


@functools.lru_cache(maxsize=None)
def dw_inputs(call: str, dtype) -> Tuple[dict, ...]:
    """Per problem: dy [rows, n_out], x [rows, n_in] (views into NaN-filled buffers), dw_buf = the whole fp32 buffer (sentinel in the
    padding, the rows past the end and the rows outside a row-group view; prior integers elsewhere), db0 (the same) or None."""
    probs, exact = DW_CALLS[call]
    out = []
    for i, q in enumerate(probs):
        s = _seed(f"{call}-{TAG[dtype]}-{i}")
        if exact:
            dy, x = ints((q.rows, q.n_out), s, -1, 1), ints((q.rows, q.n_in), s + 1, -2, 2)
            dw0, db0 = ints((q.n_out, q.n_in), s + 2, -3, 3), ints((q.n_out,), s + 3, -3, 3)
        else:
            dy, x = rnd((q.rows, q.n_out), s), rnd((q.rows, q.n_in), s + 1)
            dw0, db0 = rnd((q.n_out, q.n_in), s + 2), rnd((q.n_out,), s + 3)
        v = VEC[dtype]
        if q.pad:
            dy, x = guarded2d(dy, dtype, round_up(q.n_out, v) + v), guarded2d(x, dtype, round_up(q.n_in, v) + v)
        else:
            assert q.n_out % v == 0 and q.n_in % v == 0
            dy, x = dy.to(dtype), x.to(dtype)
        n_phys = phys_rows(q.n_out, q.group) if q.group else q.n_out
        rows = group_rows(q.n_out, q.group) if q.group else torch.arange(q.n_out)
        dw_buf = padded(n_phys, q.n_in, F32, SENTINEL, ld=q.ld_dw or q.n_in)
        dw_buf[rows, :q.n_in] = dw0
        db = None
        if q.db:
            db = torch.full((n_phys,), SENTINEL)
            db[rows] = db0
        out.append(dict(dy=dy, x=x, dw_buf=dw_buf, db0=db, rows=rows, n_phys=n_phys))
    return tuple(out)


def dw_standin(call: str, dtype, fault: Optional[str] = None):
    """fp32 CPU arithmetic (exact for the integer calls) -> per problem (dW buffer, db or None).  Faults: skip_25th, missing_last_tile,
    split_k_tail, db_two_n_tiles, ignore_group_base."""
    probs, _ = DW_CALLS[call]
    plan = dw_plan([q.shape for q in probs], dtype)
    out = []
    for i, (q, inp, p) in enumerate(zip(probs, dw_inputs(call, dtype), plan)):
        dw, db = inp["dw_buf"].clone(), (None if inp["db0"] is None else inp["db0"].clone())
        if fault == "skip_25th" and i == DW_MAX:                          # the loop over the argument tables stops after the first
            out.append((dw, db))
            continue
        dy, x = inp["dy"].float(), inp["x"].float()
        if fault == "split_k_tail" and p["last_split_rows"] % bk_of(dtype):      # the last split stops at its last whole k-tile
            keep = q.rows - p["last_split_rows"] % bk_of(dtype)
            dy, x = dy[:keep], x[:keep]
        add = dy.t() @ x
        if fault == "missing_last_tile" and p["mt"] * p["nt"] > 1:       # a grid one tile short
            add[(p["mt"] - 1) * TILE:, (p["nt"] - 1) * TILE:] = 0
        rows = inp["rows"]
        if fault == "ignore_group_base" and q.group:
            rows = group_rows(q.n_out, q.group[:2] + (0,))
        dw[rows, :q.n_in] += add
        if db is not None:
            db[rows] += dy.sum(0) * (2 if (fault == "db_two_n_tiles" and p["nt"] > 1) else 1)
        out.append((dw, db))
    return out


def dw_check(call: str, dtype, results) -> Optional[float]:
    """results: per problem (dW buffer after the call, db after the call or None).  EXACT: both whole buffers bit-equal to the prior
    contents plus the fp64 products (exact sums, so also with atomics); BOUNDED: (rows + 2) 2^-24 GEMM_FACTOR sum |dy||x| per element."""
    probs, exact = DW_CALLS[call]
    worst = 0.0
    for i, (q, inp, (dw, db)) in enumerate(zip(probs, dw_inputs(call, dtype), results)):
        what = f"dw {call} {TAG[dtype]} problem {i} {q.shape}"
        dev = dw.device
        dy, x = inp["dy"].to(dev).double(), inp["x"].to(dev).double()
        rows = inp["rows"]
        ref = dy.t() @ x + inp["dw_buf"][rows, :q.n_in].to(dev).double()
        sabs = dy.abs().t() @ x.abs() + inp["dw_buf"][rows, :q.n_in].to(dev).double().abs()
        assert (db is None) == (inp["db0"] is None)
        if exact:
            assert float(sabs.max()) < 2.0 ** 24, f"{what}: not exact in fp32"
            want = inp["dw_buf"].clone()
            want[rows, :q.n_in] = ref.float().cpu()
            assert_bit_equal(dw.detach().cpu(), want, f"{what}: dW, its padding and the rows outside the view")
            if db is not None:
                want_b = inp["db0"].clone()
                want_b[rows] = (inp["db0"][rows].to(dev).double() + dy.sum(0)).float().cpu()
                assert_bit_equal(db.detach().cpu(), want_b, f"{what}: db")
            continue
        bound = GEMM_FACTOR * (q.rows + 2) * U24 * sabs
        got = dw.detach()[rows.to(dev), :q.n_in].double()
        r = float(((got - ref).abs() / bound).max())
        if db is not None:
            b0 = inp["db0"][rows].to(dev).double()
            rb = ((db.detach()[rows.to(dev)].double() - (b0 + dy.sum(0))).abs() / ((q.rows + 2) * U24 * (b0.abs() + dy.abs().sum(0)))).max()
            r = max(r, float(rb))
        assert r == r, f"{what}: non-finite output"
        worst = max(worst, r)
        assert_outside_untouched(dw, inp["dw_buf"], q.n_out, q.n_in, what)
    if exact:
        return None
    print(f"dw {call} {TAG[dtype]}: max |err| / bound = {worst:.3g}")
    assert worst <= 1.0, f"dw {call} {TAG[dtype]}: error is {worst:.3f} x the bound"
    return worst


def dw_device_problems(call: str, dtype, device):
    """The problems of a call as kernels.linear_wgrad_grouped takes them, on `device`, and the buffers to hand to dw_check."""
    probs, _ = DW_CALLS[call]
    args, results = [], []
    for q, inp in zip(probs, dw_inputs(call, dtype)):
        dw_buf = inp["dw_buf"].to(device)
        db = None if inp["db0"] is None else inp["db0"].to(device)
        args.append((on_device(inp["dy"], device), on_device(inp["x"], device), dw_buf[:inp["n_phys"], :q.n_in], db, q.group))
        results.append((dw_buf, db))
    return args, results
