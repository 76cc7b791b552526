"""omr_ctc_frames_fwd / _bwd: the packed (ragged) and the dense memory -> time-ordered frames, bit for bit against the numpy restatement of the
documented order (tests/ctc_refs.py), pool = 1 a transposing copy, the backward the exact adjoint, +0 outside."""
import itertools

import pytest
import torch

import ctc_refs as R
from oracle import kernel_refs as KR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 72                                       # not a multiple of 64: the channel loop's tail
GRIDS = list(itertools.product((1, 5, 16), (1, 7)))


def K():
    from omr_a2s_multimodal_transformer_amd import kernels
    return kernels


def packed(grids, S, dtype, seed):
    mem = torch.zeros((len(grids), S, D), dtype=dtype)
    for b, (gh, gw) in enumerate(grids):
        mem[b, :gh * gw] = (KR.rnd((gh * gw, D), seed + b) * 3).to(dtype)
    return mem


@pytest.mark.parametrize("dtype", KR.DTYPES, ids=lambda d: KR.TAG[d])
@pytest.mark.parametrize("pool", [1, 2, 4, 32])
def test_ragged_batch_of_every_grid(pool, dtype):
    S = max(gh * gw for gh, gw in GRIDS) + 3
    mem = packed(GRIDS, S, dtype, 40)
    fmax = max(R.frame_count(gh, gw, pool) for gh, gw in GRIDS) + 2
    grid = torch.tensor(GRIDS, dtype=torch.int32, device=DEV)
    frames, flen = K().ctc_frames_fwd(mem.to(DEV), grid, 0, 0, pool, fmax)
    want, lens = R.frames_ref(mem, GRIDS, pool, fmax)
    assert flen.cpu().tolist() == lens
    KR.assert_bit_equal(frames.cpu(), want, f"frames pool {pool}")                    # zeros behind F_b included: +0 bits
    if pool == 1:
        for b, (gh, gw) in enumerate(GRIDS):
            KR.assert_bit_equal(frames[b, :gh * gw].cpu(), mem[b, :gh * gw].view(gh, gw, D).permute(1, 0, 2).reshape(-1, D).contiguous(), "transposed copy")
    g = (KR.rnd((len(GRIDS), fmax, D), 9) * 2).to(dtype)
    dmem = K().ctc_frames_bwd(g.to(DEV), grid, 0, 0, pool, S)
    KR.assert_bit_equal(dmem.cpu(), R.frames_bwd_ref(g, GRIDS, pool, S), f"frames backward pool {pool}")
    again, _ = K().ctc_frames_fwd(mem.to(DEV), grid, 0, 0, pool, fmax)
    KR.assert_bit_equal(again.cpu(), frames.cpu(), "two runs")


@pytest.mark.parametrize("dtype", KR.DTYPES, ids=lambda d: KR.TAG[d])
@pytest.mark.parametrize("gh,gw", GRIDS)
def test_dense_memory(gh, gw, dtype):
    B, S = 3, gh * gw
    mem = (KR.rnd((B, S, D), 70 + gh + gw) * 3).to(dtype)
    for pool in (1, 2, 4, 32):
        fmax = R.frame_count(gh, gw, pool)
        frames, flen = K().ctc_frames_fwd(mem.to(DEV), None, gh, gw, pool, fmax)
        want, lens = R.frames_ref(mem, [(gh, gw)] * B, pool, fmax)
        assert flen.cpu().tolist() == lens == [fmax] * B
        KR.assert_bit_equal(frames.cpu(), want, f"dense frames {gh}x{gw} pool {pool}")
        g = (KR.rnd((B, fmax, D), 3) * 2).to(dtype)
        KR.assert_bit_equal(K().ctc_frames_bwd(g.to(DEV), None, gh, gw, pool, S).cpu(), R.frames_bwd_ref(g, [(gh, gw)] * B, pool, S), "dense backward")


def test_autograd_node_is_the_adjoint():
    from omr_a2s_multimodal_transformer_amd import functional as Fn
    grids = [(5, 7), (16, 1)]
    S, pool = 40, 4
    mem = packed(grids, S, torch.float32, 5).to(DEV).requires_grad_(True)
    grid = torch.tensor(grids, dtype=torch.int32, device=DEV)
    fmax = max(R.frame_count(gh, gw, pool) for gh, gw in grids)
    frames, flen = Fn.CTCFramesFn.apply(mem, grid, 0, 0, pool, fmax)
    g = KR.rnd(tuple(frames.shape), 8).to(DEV)
    (dm,) = torch.autograd.grad(frames, mem, g)
    lhs = float((frames.detach().double() * g.double()).sum())
    rhs = float((mem.detach().double() * dm.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(lhs)) and not flen.requires_grad


def test_bad_arguments_and_grids_that_do_not_fit():
    from omr_a2s_multimodal_transformer_amd._lib import lib
    mem = torch.ones((2, 12, 8), device=DEV)
    out = torch.full((2, 6, 8), KR.SENTINEL, device=DEV)
    flen = torch.full((2,), 99, dtype=torch.int32, device=DEV)
    call = lambda **kw: lib().fns["omr_ctc_frames_fwd"](0, kw.get("mem", mem.data_ptr()), None, out.data_ptr(), flen.data_ptr(), kw.get("B", 2), 12, 8,  # noqa: E731
                                                        kw.get("gh", 3), kw.get("gw", 4), kw.get("pool", 2), 6, None)
    for rc in (call(B=0), call(pool=0), call(gh=0), call(gh=4), call(mem=None)):       # 4 x 4 cells do not fit 12 rows
        assert rc == -1
    torch.cuda.synchronize()
    assert bool((out == KR.SENTINEL).all()) and flen.cpu().tolist() == [99, 99]
    # a device-side grid that does not fit S or Fmax is the empty sample: no frame, zeros, nothing read out of bounds
    grid = torch.tensor([[3, 4], [5, 4]], dtype=torch.int32, device=DEV)               # 20 cells > 12 rows
    frames, fl = K().ctc_frames_fwd(mem, grid, 0, 0, 2, 8)
    assert fl.cpu().tolist() == [8, 0] and bool((KR.bits(frames[1]) == 0).all())
