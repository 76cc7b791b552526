"""omr_concat_memory_fwd / _bwd (csrc/extent.hip), fp32 and bf16, C in {128, 20, 3}: 128 takes the 16-byte path in both types, 20 the
fp32 16-byte path and the bf16 element path, 3 the element path.  The kernel only copies, so everything is BIT-equal to
multimodal_ragged_refs.concat_rows and its adjoint (pinned by tests/test_multimodal_ragged_refs_cpu.py).  B = 3, La = 48, Lb = 15,
lengths a = (48, 21, 4), b = (9, 15, 0); every input is NaN at and past its length: a kernel that looks there fails."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import multimodal_ragged_refs as M  # noqa: E402
from oracle.kernel_refs import assert_bit_equal  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
WIDTHS = [128, 20, 3]
B, LA, LB = 3, 48, 15
LEN_A, LEN_B = (48, 21, 4), (9, 15, 0)
SMAX = 57
NAN = float("nan")


def K():
    from omr_a2s_multimodal_transformer_amd import kernels
    return kernels


def lens_dev(lens):
    return torch.tensor(list(lens), dtype=torch.int32, device=DEV)


def ints(shape, seed, bound=8):
    """Small integers: exact in bf16."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-bound, bound + 1, shape, generator=g).float()


def nan_past(x, lens):
    x = x.clone()
    for i, n in enumerate(lens):
        x[i, n:] = NAN
    return x


@functools.lru_cache(maxsize=None)
def inputs(C, dtype):
    """(a, b, g) on the host in `dtype`: NaN at and past the lengths of a and b, and at and past la + lb in the gradient g."""
    a = nan_past(ints((B, LA, C), 10 + C), LEN_A).to(dtype)
    b = nan_past(ints((B, LB, C), 20 + C), LEN_B).to(dtype)
    g = nan_past(ints((B, SMAX, C), 30 + C), [x + y for x, y in zip(LEN_A, LEN_B)]).to(dtype)
    return a, b, g


def offset_by_one(t):
    """The same values at a base address one element past a 16-byte boundary (contiguous)."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_concat_of_two_memories_and_its_adjoint(dtype, C):
    a, b, g = inputs(C, dtype)
    la, lb = lens_dev(LEN_A), lens_dev(LEN_B)
    out = K().concat_memory_fwd(a.to(DEV), la, b.to(DEV), lb, SMAX)
    assert_bit_equal(out, M.concat_rows(a, LEN_A, b, LEN_B, SMAX), "concat")
    da, db = K().concat_memory_bwd(g.to(DEV), la, LA, lb, LB)
    rda, rdb = M.concat_rows_adjoint(g, LEN_A, LA, LEN_B, LB)
    assert_bit_equal(da, rda, "da")
    assert_bit_equal(db, rdb, "db")
    # concat(bwd(g)) = g with its tails zeroed
    g0 = g.clone()
    for i, (x, y) in enumerate(zip(LEN_A, LEN_B)):
        g0[i, x + y:] = 0
    assert_bit_equal(K().concat_memory_fwd(da, la, db, lb, SMAX), g0, "concat(bwd(g))")


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_tail_zeroing_form(dtype, C):
    """b = NULL, Lb = 0: the first la rows, zeros behind them; the backward returns no db."""
    a, _, g = inputs(C, dtype)
    la = lens_dev(LEN_A)
    g = nan_past(torch.nan_to_num(g[:, :LA].float()), LEN_A).to(dtype)
    assert_bit_equal(K().concat_memory_fwd(a.to(DEV), la, None, None, LA), M.concat_rows(a, LEN_A, None, None, LA), "tail zeroing")
    da, db = K().concat_memory_bwd(g.to(DEV), la, LA, None, 0)
    assert db is None
    assert_bit_equal(da, M.concat_rows_adjoint(g, LEN_A, LA, None, 0)[0], "tail zeroing, da")


@pytest.mark.parametrize("C", [128, 20])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_base_pointer_off_by_one_element_takes_the_element_path_with_the_same_bits(dtype, C):
    a, b, g = inputs(C, dtype)
    la, lb = lens_dev(LEN_A), lens_dev(LEN_B)
    want = M.concat_rows(a, LEN_A, b, LEN_B, SMAX)
    ad, bd = a.to(DEV), b.to(DEV)
    assert_bit_equal(K().concat_memory_fwd(offset_by_one(ad), la, bd, lb, SMAX), want, "a off by one element")
    assert_bit_equal(K().concat_memory_fwd(ad, la, offset_by_one(bd), lb, SMAX), want, "b off by one element")
    out = offset_by_one(torch.zeros((B, SMAX, C), dtype=dtype, device=DEV))
    assert_bit_equal(K().concat_memory_fwd(ad, la, bd, lb, SMAX, out=out), want, "out off by one element")
    da, db = K().concat_memory_bwd(offset_by_one(g.to(DEV)), la, LA, lb, LB)
    rda, rdb = M.concat_rows_adjoint(g, LEN_A, LA, LEN_B, LB)
    assert_bit_equal(da, rda, "da, dout off by one element")
    assert_bit_equal(db, rdb, "db, dout off by one element")


@pytest.mark.parametrize("smax", [50, 30])
@pytest.mark.parametrize("dtype", DTYPES)
def test_smax_below_la_plus_lb_truncates_and_writes_nothing_past_it(dtype, smax):
    """B = 1, la + lb = 57 > Smax (50: b cut short; 30: a cut short, b absent), the output inside a larger buffer full of a sentinel."""
    C = 128
    a, b, g = (t[:1] for t in inputs(C, dtype))
    la, lb = lens_dev(LEN_A[:1]), lens_dev(LEN_B[:1])
    guard = 64 * C
    buf = torch.full((guard + smax * C + guard,), 7.0, dtype=dtype, device=DEV)
    out = buf[guard:guard + smax * C].view(1, smax, C)
    K().concat_memory_fwd(a.to(DEV), la, b.to(DEV), lb, smax, out=out)
    assert_bit_equal(out, M.concat_rows(a, LEN_A[:1], b, LEN_B[:1], smax), f"Smax {smax}")
    assert bool((buf[:guard] == 7.0).all()) and bool((buf[guard + smax * C:] == 7.0).all()), "the sentinel around the output"
    gs = torch.nan_to_num(g[:, :smax].float()).to(dtype)
    da, db = K().concat_memory_bwd(gs.to(DEV), la, LA, lb, LB)
    rda, rdb = M.concat_rows_adjoint(gs, LEN_A[:1], LA, LEN_B[:1], LB)
    assert_bit_equal(da, rda, f"da, Smax {smax}")
    assert_bit_equal(db, rdb, f"db, Smax {smax}")


def test_more_than_one_trip_through_the_grid_stride_loop():
    """B = 2, La = 600, Lb = 8, C = 1024, fp32: 608 * 256 = 155 648 output fragments per sample against 256 * 256 = 65 536 threads."""
    Bb, La, Lb, C = 2, 600, 8, 1024
    len_a, len_b = (600, 333), (8, 5)
    a = nan_past(ints((Bb, La, C), 41), len_a)
    b = nan_past(ints((Bb, Lb, C), 42), len_b)
    g = nan_past(ints((Bb, La + Lb, C), 43), [x + y for x, y in zip(len_a, len_b)])
    la, lb = lens_dev(len_a), lens_dev(len_b)
    assert_bit_equal(K().concat_memory_fwd(a.to(DEV), la, b.to(DEV), lb, La + Lb), M.concat_rows(a, len_a, b, len_b, La + Lb), "concat, long")
    da, db = K().concat_memory_bwd(g.to(DEV), la, La, lb, Lb)
    rda, rdb = M.concat_rows_adjoint(g, len_a, La, len_b, Lb)
    assert_bit_equal(da, rda, "da, long")
    assert_bit_equal(db, rdb, "db, long")


def test_arguments_are_checked():
    """B = 0 -> OMR_ERR_ARG (-1); a float64 dtype code -> OMR_ERR_UNSUPPORTED (-3); b without Lb or Lb without b -> OMR_ERR_ARG."""
    from omr_a2s_multimodal_transformer_amd._lib import lib
    a, b, _ = inputs(128, torch.float32)
    a, b = a.to(DEV), b.to(DEV)
    la, lb = lens_dev(LEN_A), lens_dev(LEN_B)
    out = torch.zeros((B, SMAX, 128), device=DEV)
    p = lambda t: t.data_ptr()  # noqa: E731
    q = lib().query
    assert q("omr_concat_memory_fwd", 0, p(a), p(la), LA, p(b), p(lb), LB, p(out), B, 128, SMAX, None) == 0
    assert q("omr_concat_memory_fwd", 0, p(a), p(la), LA, p(b), p(lb), LB, p(out), 0, 128, SMAX, None) == -1
    assert q("omr_concat_memory_fwd", 0, p(a), p(la), LA, p(b), p(lb), LB, p(out), 65536, 128, SMAX, None) == -1
    assert q("omr_concat_memory_fwd", 0, p(a), p(la), LA, None, None, LB, p(out), B, 128, SMAX, None) == -1
    assert q("omr_concat_memory_fwd", 0, p(a), p(la), 1 << 24, p(b), p(lb), LB, p(out), B, 128, SMAX, None) == -1       # La * C = 2^31
    assert q("omr_concat_memory_fwd", 7, p(a), p(la), LA, p(b), p(lb), LB, p(out), B, 128, SMAX, None) == -3
    assert q("omr_concat_memory_bwd", 0, p(out), p(la), LA, p(lb), LB, p(a), p(b), 0, 128, SMAX, None) == -1
    assert q("omr_concat_memory_bwd", 0, p(out), p(la), LA, p(lb), LB, p(a), None, B, 128, SMAX, None) == -1
    assert q("omr_concat_memory_bwd", 7, p(out), p(la), LA, p(lb), LB, p(a), p(b), B, 128, SMAX, None) == -3
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="invalid argument"):
        K().concat_memory_fwd(a[:0], la[:0], b[:0], lb[:0], SMAX)


def test_autograd_function_keeps_only_the_lengths():
    from omr_a2s_multimodal_transformer_amd import functional as Fn
    a, b, g = inputs(128, torch.float32)
    la, lb = lens_dev(LEN_A), lens_dev(LEN_B)
    ad, bd = torch.nan_to_num(a).to(DEV).requires_grad_(), torch.nan_to_num(b).to(DEV).requires_grad_()
    out = Fn.ConcatMemoryFn.apply(ad, la, bd, lb, SMAX)
    assert out.grad_fn.saved_tensors == ()                   # the lengths ride on the context, no activation is kept
    out.backward(torch.nan_to_num(g).to(DEV))
    rda, rdb = M.concat_rows_adjoint(torch.nan_to_num(g), LEN_A, LA, LEN_B, LB)
    assert_bit_equal(ad.grad, rda, "autograd da")
    assert_bit_equal(bd.grad, rdb, "autograd db")
    t = Fn.ConcatMemoryFn.apply(ad, la, None, None, LA)
    t.backward(torch.ones_like(t))
