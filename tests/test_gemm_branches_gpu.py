"""Branch-level tests of the specialised GEMMs -- the panel kernel (gemm_panel.hip), the DMA-fed tall kernel (gemm_tall.hip), the
grouped weight gradient (gemm_dw_grouped_kernel of gemm.hip) and the row-group views of omr_gemm -- against the fp64 references of
oracle/gemm_refs.py, and of functional.FusedCrossKVFn / KVGradSink at node level.  Most cases are EXACT: small-integer operands
make every fp32 sum exact in any order and keep every |ref| <= 256, so a bf16 output must equal the reference bit for bit, at
EVERY element of buffers of 50 000 - 66 000 rows (no sampling), with everything around C untouched -- a stale stage in the second
tile of a workgroup, a swizzle that is wrong for some in-tile rows, a lost k-tile, column tile or argument table cannot hide in
a tolerance.  One BOUNDED case per kernel checks fp32 accumulation and the single rounding.  The case table is shared with
tests/test_gemm_refs_cpu.py, which shows on the CPU that a correct implementation passes each check and a list of wrong ones does
not.  The library does not report which kernel ran: a case asserts, through the mirrors of the launchers in oracle/gemm_refs.py,
that it meets the acceptance conditions of the kernel it is named for, and claims no more.  DESIGN.md ("GEMM family branch
coverage") maps each branch to the case that reaches it."""
import ctypes

import pytest
import torch

from oracle import gemm_refs as R
from oracle.conv_refs import ints, on_device
from oracle.kernel_refs import SENTINEL, assert_bit_equal

pytestmark = pytest.mark.gpu

F32, BF16 = R.F32, R.BF16
ERR_ARG = -1                                 # OMR_ERR_ARG of include/omr_hip.h


def dev():
    return torch.device("cuda:0")


def K():
    from omr_a2s_multimodal_transformer_amd import kernels
    return kernels


def ids(cases):
    return [c.name for c in cases]


def D(t):
    return None if t is None else on_device(t, dev())


def run(c):
    """The case through kernels.gemm / kernels.gemm_row_groups -> (C buffer, column sums or None)."""
    inp = R.inputs(c)
    a, b, c_buf = D(inp["a"]), D(inp["b"]), inp["c_buf"].to(dev())
    bias = None if inp["bias"] is None else inp["bias"].to(dev())
    cs = None if inp["colsum0"] is None else inp["colsum0"].to(dev())
    aligned = all(t.data_ptr() % 16 == 0 for t in (a, b, c_buf))
    assert (a.stride(0), b.stride(0), c_buf.stride(0)) == (c.lda, c.ldb, c.ldc)
    route = R.gemm_route(c, aligned)
    print(f"gemm {c.name}: meets the conditions of the {route} kernel" + (f", {R.tall_plan(c.M)}" if route == "tall" else ""))
    assert route == c.route
    if c.group is None:
        K().gemm(a, b, trans_a=c.ta, trans_b=c.tb, bias=bias, relu=c.relu, out=c_buf[:c.M, :c.N])
    else:
        assert not c.relu
        K().gemm_row_groups(a, b, c_buf, c.M, c.N, c.K, trans_a=c.ta, trans_b=c.tb, bias=bias, accumulate=c.accumulate, split_k=c.split_k,
                            colsum_a=cs, group=c.group)
    torch.cuda.synchronize()
    return c_buf, cs


# ------------------------------------------------------------------------------------------------ gemm_tall.hip

@pytest.mark.parametrize("c", R.TALL_CASES[:3], ids=ids(R.TALL_CASES[:3]))
def test_tall_gemm_is_exact_at_every_element(c):
    """T1: the fewest tiles, one k-tile (prologue only).  T2: 258 tiles on 256 workgroups -- workgroups 0 and 1 walk a second tile,
    the ragged 37-row one among them -- three k-tiles through the two-stage ring, lda / ldb / ldc past the widths.  T3: the same
    walk through the reduction-side row groups, two k-tiles per group, NaN in the Q rows."""
    if c.name[:2] in ("T2", "T3"):
        assert R.tall_plan(c.M)["busiest"] >= 2
    R.check(c, *run(c))


def test_tall_gemm_real_valued_within_the_derived_bound():
    """T4, ten k-tiles: fp32 accumulation across k-tiles and ONE rounding to bf16 (an accumulator kept in bf16 between k-tiles passes
    every exact case; tests/test_gemm_refs_cpu.py shows this case catching it)."""
    c = R.TALL_CASES[3]
    R.check(c, *run(c))


@pytest.mark.parametrize("c", R.TALL_NEIGHBOURS, ids=ids(R.TALL_NEIGHBOURS))
def test_tall_gemm_neighbours_fall_through_exactly(c):
    """One acceptance condition missed each (K % 64, 191 row tiles): the tile kernel, the same exact result."""
    R.check(c, *run(c))


# ------------------------------------------------------------------------------------------------ gemm_panel.hip

@pytest.mark.parametrize("c", R.PANEL_CASES[:3], ids=ids(R.PANEL_CASES[:3]))
def test_panel_gemm_is_exact_at_every_element(c):
    """P1: the smallest sizes, NO bias (the zero array and the index mask).  P2: a ragged last panel, nine column tiles (the last
    one back in buffer 0 of the W / C / bias images), K = 256, a bias, lda > K, ldc > N.  P3: the row-group view, NaN in the Q rows
    of the weight block and of the bias."""
    R.check(c, *run(c))


def test_panel_gemm_real_valued_within_the_derived_bound():
    c = R.PANEL_CASES[3]
    R.check(c, *run(c))


@pytest.mark.parametrize("c", R.PANEL_NEIGHBOURS, ids=ids(R.PANEL_NEIGHBOURS))
def test_panel_gemm_neighbours_fall_through_exactly(c):
    """M one row short, N no multiple of 64, a ReLU: the tile kernel, the same exact result."""
    R.check(c, *run(c))


# ------------------------------------------------------------------------------------------------ the tile kernel through row groups

@pytest.mark.parametrize("c", R.TILE_GROUP_CASES, ids=ids(R.TILE_GROUP_CASES))
def test_tile_gemm_through_row_groups_is_exact(c):
    """Operands 1, 2 and 3 at ragged small sizes in fp32 and bf16: the FULLK branch (the group resolved per slab), the pipelined
    loop, split-K with fused column sums into the K|V rows of dW / db -- whose Q rows stay bit-equal."""
    R.check(c, *run(c))


# ------------------------------------------------------------------------------------------------ gemm_dw_grouped_kernel

@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("call", list(R.DW_CALLS))
def test_grouped_weight_gradients(call, dtype):
    """25 problems in one call (the 25th in a second argument table): one split and split-K, rows no multiple of the k-tile, n_out
    and n_in tails, no db, strided dY, ld_dw > n_in, a row-group view; then one problem alone, and one with real values.  Exact calls:
    every element of every dW buffer and db bit-equal, padding and Q rows included -- exact sums make that hold with atomics."""
    args, results = R.dw_device_problems(call, dtype, dev())
    K().linear_wgrad_grouped(args)
    torch.cuda.synchronize()
    R.dw_check(call, dtype, results)


# ------------------------------------------------------------------------------------------------ refusals

def _gemm_args(a, b, c, bias, M, N, Kd, tb, group):
    code = {F32: 0, BF16: 1}
    return [code[a.dtype], code[c.dtype], 0, int(tb), M, N, Kd, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0),
            None if bias is None else bias.data_ptr(), 0, 0, 1, None, 0.0, 0, *group, None]


def test_row_group_arguments_are_refused():
    """Each bad row-group argument returns OMR_ERR_ARG from the raw entry and C keeps its sentinel.  Every operand is the interior of
    a larger buffer."""
    from omr_a2s_multimodal_transformer_amd._lib import lib
    M, N, Kd = 130, 384, 64
    big_a = torch.zeros((1024, 72), dtype=BF16, device=dev())
    big_b = torch.zeros((2048, 72), dtype=BF16, device=dev())
    bias = torch.zeros(2048, device=dev())
    c_buf = torch.full((1024, 392), SENTINEL, dtype=BF16, device=dev())
    a, b, c = big_a[256:256 + M, :Kd], big_b[512:512 + 576, :Kd], c_buf[256:256 + M, :N]
    before = c_buf.clone()
    good = (128, 192, 64, 1)
    assert lib().query("omr_gemm", *_gemm_args(a, b, c, bias[512:], M, N, Kd, False, good)) == 0          # the call the refusals vary
    torch.cuda.synchronize()
    assert not torch.equal(c_buf, before)
    c_buf.copy_(before)
    bad = {
        "row_group % 128": ((64, 192, 64, 1), False), "stride < group": ((128, 127, 64, 1), False), "base < 0": ((128, 192, -64, 1), False),
        "operand 4": ((128, 192, 64, 4), False), "operand -1": ((128, 192, 64, -1), False), "row_group 0": ((0, 192, 64, 1), False),
        "operand 2 without transB": ((128, 192, 64, 2), False), "operand 1 with transB": ((128, 192, 64, 1), True),
    }
    for what, (group, tb) in bad.items():
        rc = lib().query("omr_gemm", *_gemm_args(a, b, c, bias[512:], M, N, Kd, tb, group))
        assert rc == ERR_ARG, f"{what}: returned {rc}"
    torch.cuda.synchronize()
    assert_bit_equal(c_buf, before.cpu(), "refused calls: C")


def test_grouped_weight_gradient_arguments_are_refused():
    from omr_a2s_multimodal_transformer_amd._lib import lib
    P = K()._DwProblem
    rows, n_out, n_in = 300, 128, 64
    dy = torch.ones((1024, n_out + 8), dtype=BF16, device=dev())[256:256 + rows]
    x = torch.ones((1024, n_in + 8), dtype=BF16, device=dev())[256:256 + rows]
    dw = torch.full((1024, n_in), SENTINEL, device=dev())
    db = torch.full((1024,), SENTINEL, device=dev())

    def prob(**kw):
        q = (P * 1)()
        q[0].dy, q[0].x, q[0].dw, q[0].db = dy.data_ptr(), x.data_ptr(), dw[256:].data_ptr(), db[256:].data_ptr()
        q[0].rows, q[0].n_out, q[0].n_in, q[0].row_group = rows, n_out, n_in, 0
        q[0].ld_dy, q[0].ld_x, q[0].ld_dw, q[0].row_group_stride, q[0].row_group_base = dy.stride(0), x.stride(0), n_in, 0, 0
        for k, v in kw.items():
            setattr(q[0], k, v)
        return q

    call = lambda nprob, q: lib().query("omr_linear_wgrad_grouped", 1, nprob, None if q is None else ctypes.byref(q), None)
    assert call(0, prob()) == ERR_ARG and call(-3, prob()) == ERR_ARG
    assert call(1, None) == ERR_ARG
    for field in ("dy", "x", "dw"):
        assert call(1, prob(**{field: None})) == ERR_ARG, field
    assert call(1, prob(ld_dy=n_out + 9)) == ERR_ARG                      # rows of dY off the 16-byte grid
    assert call(1, prob(row_group=100, row_group_stride=192, row_group_base=0)) == ERR_ARG
    assert call(1, prob(row_group=128, row_group_stride=64, row_group_base=0)) == ERR_ARG
    assert call(1, prob(row_group=128, row_group_stride=192, row_group_base=-1)) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all())
    assert call(1, prob()) == 0                                           # the call the refusals vary
    torch.cuda.synchronize()
    assert bool((dw[256:256 + n_out] == SENTINEL + rows).all()) and bool((db[256:256 + n_out] == SENTINEL + rows).all())
    assert bool((dw[:256] == SENTINEL).all()) and bool((dw[256 + n_out:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ FusedCrossKVFn / KVGradSink

KV_B, KV_S, KV_D, KV_L = 2, 37, 64, 3


def _kv_rows(l):
    return slice(l * 3 * KV_D + KV_D, (l + 1) * 3 * KV_D)


def _kv_setup(dtype):
    d, L = KV_D, KV_L
    cpu = dict(w=ints((L * 3 * d, d), 71, -2, 2), b=ints((L * 3 * d,), 72, -3, 3), gw=ints((L * 3 * d, d), 73, -3, 3), gb=ints((L * 3 * d,), 74, -3, 3),
               mem=ints((KV_B, KV_S, d), 75, -1, 1), g=[ints((KV_B, KV_S, 2 * d), 76 + l, -1, 1) for l in range(L)])
    pack = dict(L=L, d=d, w=cpu["w"].to(dev(), dtype), b=cpu["b"].to(dev()), gw=cpu["gw"].to(dev()), gb=cpu["gb"].to(dev()))
    return cpu, pack


def _kv_reference(cpu, used, mem_grad):
    """torch float64 autograd of memory @ w[kv rows].T + b[kv rows] per layer, the layers of `used` weighted by their gradients."""
    w, b = cpu["w"].double().requires_grad_(), cpu["b"].double().requires_grad_()
    mem = cpu["mem"].double().requires_grad_(mem_grad)
    outs = [mem @ w[_kv_rows(l)].t() + b[_kv_rows(l)] for l in range(KV_L)]
    sum((outs[l] * cpu["g"][l].double()).sum() for l in used).backward()
    return [o.detach() for o in outs], cpu["gw"].double() + w.grad, cpu["gb"].double() + b.grad, mem.grad


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("situation", ["a-sink", "b-copied", "c-one-unused", "d-memory-without-grad"])
def test_fused_cross_kv_node(situation, dtype):
    """Outputs, dmem, gw and gb (after WgradStream.join) against float64 autograd, bit for bit on integer operands: (a) every layer's
    gradient written into its KVGradSink slot; (b) gradients from ordinary torch ops, copied in (no sink buffer); (c) layer 0 through
    its slot, layer 1 unused -- its slab of the (NaN-filled) sink buffer must be zeroed, its K|V rows of gw / gb keep their values,
    dmem lacks its term -- layer 2 copied; (d) a memory that needs no gradient.  The Q rows of gw / gb stay bit-equal in all four."""
    from omr_a2s_multimodal_transformer_amd import functional as Fn
    from omr_a2s_multimodal_transformer_amd.runtime import WgradStream
    cpu, pack = _kv_setup(dtype)
    mem_grad = situation != "d-memory-without-grad"
    used = (0, 2) if situation == "c-one-unused" else (0, 1, 2)
    outs64, gw64, gb64, dmem64 = _kv_reference(cpu, used, mem_grad)
    if dtype == BF16:                                                      # the exactness conditions of a bf16 output
        assert max(float(o.abs().max()) for o in outs64) <= 256 and (dmem64 is None or float(dmem64.abs().max()) <= 256)
    memory = cpu["mem"].to(dev(), dtype).requires_grad_(mem_grad)
    anchor = torch.zeros((), device=dev(), requires_grad=True)
    sink = Fn.KVGradSink()
    kvs = Fn.FusedCrossKVFn.apply(memory, pack, sink, anchor)
    g = [t.to(dev(), dtype) for t in cpu["g"]]
    for l in range(KV_L):
        assert_bit_equal(kvs[l].detach().cpu(), outs64[l].to(dtype), f"{situation}: K|V of layer {l}")
    if situation == "a-sink":
        slots = [sink.slot(kvs[l], l) for l in range(KV_L)]
        for s, t in zip(slots, g):
            s.copy_(t)
        torch.autograd.backward(list(kvs), slots)
    elif situation == "c-one-unused":
        slot0 = sink.slot(kvs[0], 0)
        sink.buf.fill_(float("nan"))
        slot0.copy_(g[0])
        torch.autograd.backward([kvs[0], (kvs[2].float() * g[2].float()).sum()], [slot0, None])
    else:
        sum((kvs[l].float() * g[l].float()).sum() for l in range(KV_L)).backward()
    WgradStream.join()
    torch.cuda.synchronize()
    assert sink.buf is None and anchor.grad is None
    assert_bit_equal(pack["gw"].cpu(), gw64.float(), f"{situation}: gw (Q rows and unused layers as they were)")
    assert_bit_equal(pack["gb"].cpu(), gb64.float(), f"{situation}: gb")
    q_rows = torch.cat([torch.arange(l * 3 * KV_D, l * 3 * KV_D + KV_D) for l in range(KV_L)])
    assert_bit_equal(pack["gw"].cpu()[q_rows], cpu["gw"][q_rows], f"{situation}: Q rows of gw")
    assert_bit_equal(pack["gb"].cpu()[q_rows], cpu["gb"][q_rows], f"{situation}: Q rows of gb")
    if situation == "c-one-unused":
        assert_bit_equal(pack["gw"].cpu()[_kv_rows(1)], cpu["gw"][_kv_rows(1)], "c: K|V rows of the unused layer")
    if mem_grad:
        assert_bit_equal(memory.grad.cpu(), dmem64.to(dtype), f"{situation}: dmem")
    else:
        assert memory.grad is None
