"""Branch-level tests of the convolution kernels (conv3x3_mfma.h, conv.hip, conv_wgrad_dma.hip, conv_bwd_fused.hip, conv1.hip,
dwconv.hip) against the fp64 references of oracle/conv_refs.py.  Most cases are EXACT: small-integer operands make every fp32 sum
exact in any order, so the output must equal the reference rounded once, bit for bit -- a lost tile, halo row, tap or ring slot
cannot hide in a tolerance.  Every multi-tile case first asserts, from the mirror of its launcher's grid arithmetic, that its
busiest workgroup walks the stated number of tiles (and, for the weight gradients, crosses an image boundary).  The case table
is shared with tests/test_conv_refs_cpu.py, which shows on the CPU that a correct implementation passes each check and a list of
wrong ones does not.  DESIGN.md ("Convolution branch coverage") maps each branch to the test id here that reaches it."""
import numpy as np
import pytest
import torch

from oracle import conv_refs as R

pytestmark = pytest.mark.gpu

F32, BF16 = R.F32, R.BF16
IN_EPS = 1e-3


def dev():
    return torch.device("cuda:0")


def K():
    from omr_a2s_multimodal_transformer_amd import kernels
    return kernels


def ids(cases):
    return [c.name for c in cases]


def D(t):
    return R.on_device(t, dev())


def announce(name, plan, want, cross=None):
    print(f"{name}: busiest workgroup walks >= {plan['min_tiles']} tiles (asked: {want})" + ("" if cross is None else f", crosses an image: {cross}"))
    assert plan["min_tiles"] >= want, plan


# ------------------------------------------------------------------------------------------------ conv3x3_mfma_kernel

def run_conv(c):
    """-> (y or None, per-image sums [B, COUT, 2] or None); every property of the slot workspace is asserted on the way."""
    k, inp, p = K(), R.conv_inputs(c), R.conv_plan(c)
    B, (Ho, Wo), C = c.B, c.out_hw, c.cout
    kw = dict(stride=c.stride, dil=c.dil, out_hw=c.out_hw, relu=c.relu)
    if c.norm:
        kw["in_stats"] = (D(inp["mean"]), D(inp["rstd"]))
    if c.mask:
        kw["mask_scale"] = c.mask
        if c.stat_mode < 4:
            kw["out_mask"] = D(inp["mask"])
    if c.drop:
        kw["drop"] = (R.DROP_P, R.DROP_SEED, c.drop == "chan")
    ws = None
    slots = p["slots"]
    if c.stat_mode:
        n = B * slots * C * 2
        ws = torch.full((n + B * C * 2,), R.NAN, dtype=torch.float64, device=dev())      # every slot must be written
        if c.stat_mode == 5:
            ws[n:] = inp["compact"].to(dev()).flatten()
        kw.update(stat_mode=c.stat_mode, stat_ws=ws, stat_slots=slots)
        if c.stat_mode >= 2:
            kw.update(stat_x=D(inp["stat_x"]), stat_stats=(D(inp["stat_mean"]), D(inp["stat_rstd"])))
    y = k.conv3x3(D(inp["x"]), D(inp["w"]), D(inp["bias"]) if c.bias else None, **kw)
    torch.cuda.synchronize()
    sums = None
    if c.stat_mode in (1, 2, 4):
        sl = ws[:n].view(B, slots, C, 2).cpu()
        assert bool(torch.isfinite(sl).all()), f"{c.name}: a statistics slot was not written"
        assert bool((sl[:, p["tiles"]:] == 0).all()), f"{c.name}: a slot no workgroup owns is not zero"
        sums = sl.sum(dim=1)
        k.instnorm_reduce_sums(ws, slots, B, C)
        torch.cuda.synchronize()
        compact = ws[n:].view(B, C, 2).cpu()
        if not c.real:
            assert torch.equal(compact, sums), f"{c.name}: omr_instnorm_reduce_sums differs from the sum of the slots"
        if c.stat_mode == 1 and not c.real:
            mean, rstd = k.instnorm_finalize(ws, slots, B, C, Ho * Wo, IN_EPS)
            m = sums[..., 0] / (Ho * Wo)
            var = (sums[..., 1] / (Ho * Wo) - m * m).clamp_min(0)
            r = 1.0 / torch.sqrt(var + float(np.float32(IN_EPS)))
            assert bool(((mean.cpu().double() - m).abs() <= 2.0 ** -23 * m.abs()).all()), f"{c.name}: finalised mean"
            assert bool(((rstd.cpu().double() - r).abs() <= 2.0 ** -23 * r).all()), f"{c.name}: finalised rstd"
    return y, sums


def check_conv(c):
    announce(c.name, R.conv_plan(c), c.min_tiles)
    R.conv_check(c, *run_conv(c))


@pytest.mark.parametrize("c", R.CONV_STAT_CASES, ids=ids(R.CONV_STAT_CASES))
def test_conv3x3_fused_epilogues_through_the_tile_loop(c):
    """EPI 1 / 2 / 3 with the grid clamped to 1 or 2 workgroups per image by stat_slots: 3 x 3 tiles ragged both ways, two images;
    prefetch across tiles, the output staging tile over the halo, weights staged once (SINGLE), statistics partials carried over
    the tiles.  Output, slot sums (every slot written, spare slots zero), omr_instnorm_reduce_sums and omr_instnorm_finalize."""
    check_conv(c)


@pytest.mark.parametrize("c", R.CONV_WALK_CASES, ids=ids(R.CONV_WALK_CASES))
def test_conv3x3_walks_three_tiles(c):
    """No statistics, so only the batch brings the grid below the tile count: >= 3 tiles per workgroup for EPI 0, fp32, one / two /
    three / four channel chunks (the prefetch wrap from the last chunk to chunk 0 of the next tile), every stride and dilation
    with odd and even sizes."""
    check_conv(c)


@pytest.mark.parametrize("c", R.CONV_WIDTH_CASES, ids=ids(R.CONV_WIDTH_CASES))
def test_conv3x3_channel_counts_the_model_does_not_use(c):
    check_conv(c)


@pytest.mark.parametrize("c", R.CONV_REAL_CASES, ids=ids(R.CONV_REAL_CASES))
def test_conv3x3_real_valued_within_the_derived_bound(c):
    """Real operands: fp32 accumulation, the rounding of the normalised operand and ONE rounding of the output; prints error / bound."""
    check_conv(c)


def test_conv3x3_refuses_what_it_does_not_cover():
    """CIN % KS != 0, COUT % VEC != 0, CIN > NORM_MAX with statistics, stride together with dilation."""
    k = K()
    x = torch.zeros((1, 8, 32, 24), dtype=BF16, device=dev())
    with pytest.raises(RuntimeError, match="unsupported"):
        k.conv3x3(x, torch.zeros((16, 3, 3, 24), dtype=BF16, device=dev()), None)
    x = torch.zeros((1, 8, 32, 16), dtype=BF16, device=dev())
    with pytest.raises(RuntimeError, match="unsupported"):
        k.conv3x3(x, torch.zeros((12, 3, 3, 16), dtype=BF16, device=dev()), None)
    with pytest.raises(RuntimeError, match="unsupported"):
        k.conv3x3(x, torch.zeros((16, 3, 3, 16), dtype=BF16, device=dev()), None, stride=(2, 2), dil=(2, 2), out_hw=(8, 32))
    x = torch.zeros((1, 8, 32, 256), dtype=BF16, device=dev())
    st = (torch.zeros((1, 256), device=dev()), torch.ones((1, 256), device=dev()))
    with pytest.raises(RuntimeError, match="unsupported"):
        k.conv3x3(x, torch.zeros((16, 3, 3, 256), dtype=BF16, device=dev()), None, in_stats=st)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ weight gradients

def run_wgrad(c):
    inp = R.wgrad_inputs(c)
    dw, db = D(inp["dw0"]), D(inp["db0"])
    st = (D(inp["mean"]), D(inp["rstd"])) if c.norm else None
    dy = D(inp["dy"])
    assert dy.data_ptr() % 16 == c.dy_off % 16
    K().conv3x3_wgrad(D(inp["x"]), dy, dw, stride=c.stride, in_stats=st, db=db)
    torch.cuda.synchronize()
    return dw, db


def check_wgrad(c):
    p = R.wgrad_plan(c)
    assert p["kernel"] == c.kernel
    announce(c.name, p, c.min_tiles, p["cross"])
    assert p["cross"] or not c.cross
    R.wgrad_check(c, *run_wgrad(c))


@pytest.mark.parametrize("c", R.WGRAD_DMA_CASES, ids=ids(R.WGRAD_DMA_CASES))
def test_wgrad_dma_ring_wraps_across_images(c):
    """Every row of pick(): the busiest workgroup walks >= NSTAGE + 2 tiles across an image boundary, so the ring wraps, the dummy
    issues past the last tile run, and (NORM) the statistics registers and the 8-slot statistics ring turn over.  Channel tails
    (CIN = 24 / 40), db with two cin-block columns, dw / db accumulated onto non-zero integers."""
    check_wgrad(c)


@pytest.mark.parametrize("c", R.WGRAD_GENERIC_CASES, ids=ids(R.WGRAD_GENERIC_CASES))
def test_wgrad_generic_walks_tiles_across_images(c):
    check_wgrad(c)


@pytest.mark.parametrize("c", R.WGRAD_CONV1_CASES, ids=ids(R.WGRAD_CONV1_CASES))
def test_conv1_wgrad_every_kernel(c):
    """conv1_wgrad_mfma_kernel over > 3 x 2048 ragged tiles; conv1_wgrad_kernel for fp32, COUT = 32 and a dy 8 bytes into its buffer."""
    check_wgrad(c)


@pytest.mark.parametrize("c", R.WGRAD_REAL_CASES, ids=ids(R.WGRAD_REAL_CASES))
def test_wgrad_real_valued_within_the_derived_bound(c):
    check_wgrad(c)


@pytest.mark.parametrize("c", R.CONV1_CASES, ids=ids(R.CONV1_CASES))
def test_conv1_forward(c):
    """conv1_direct_kernel<T, 32> and <T, 16>: two row chunks (H > 32) and two column blocks (W > 256)."""
    inp = R.conv1_inputs(c)
    y = K().conv3x3(D(inp["x"]), D(inp["w"]), D(inp["bias"]), relu=c.relu)
    torch.cuda.synchronize()
    R.assert_exact(y, R.conv1_ref(c), c.dtype, c.name, tile=(32, 256))


# ------------------------------------------------------------------------------------------------ depthwise

@pytest.mark.parametrize("c", R.DW_CASES, ids=ids(R.DW_CASES))
def test_depthwise_every_kernel(c):
    """Exact versions of the depthwise path cases (tile / walk / per-pixel forward and flipped data gradient, with normalise-on-load
    and the producer's mask) and the persistent weight-gradient tile kernels <T, 12>, <T, 16> and the wide fold over > 3 x 256
    tiles across images, with and without in_stats."""
    k, inp, p = K(), R.dw_inputs(c), R.dw_plan(c)
    assert p["kernel"] == c.kernel and p.get("rc", c.rc) == c.rc
    announce(c.name, p, c.min_tiles)
    st = (D(inp["mean"]), D(inp["rstd"])) if c.norm else None
    if c.op == "wgrad":
        dw, db = D(inp["dw0"]), D(inp["db0"])
        k.dwconv3x3_wgrad(D(inp["x"]), D(inp["dy"]), dw, db, in_stats=st)
        got = dict(dw=dw, db=db)
    else:
        w = D(inp["w"])
        assert w.data_ptr() % 16 == c.w_off % 16
        y = k.dwconv3x3(D(inp["x"]), w, D(inp["bias"]), in_stats=st, out_mask=D(inp["mask"]) if c.mask else None, mask_scale=c.mask or 1.0,
                        flip=c.op == "flip")
        got = dict(y=y)
    torch.cuda.synchronize()
    R.dw_check(c, got)


# ------------------------------------------------------------------------------------------------ fused backward

@pytest.mark.parametrize("c", R.FUSED_CASES, ids=ids(R.FUSED_CASES))
def test_fused_backward_against_the_reference(c):
    """omr_conv3x3_bwd_fused / _s2 with the ring turned over (>= NSLOT + 2 tiles per workgroup, 3 x 3 tiles with overhang): dx, dw, db
    and the InstanceNorm-backward slots each against the fp64 reference, not against the separate kernels."""
    k, inp, p = K(), R.fused_inputs(c), R.fused_plan(c)
    announce(c.name, p, c.min_tiles)
    B, H, W = c.B, c.H, c.W
    dw, db = D(inp["dw0"]), D(inp["db0"])
    g, x, wf = D(inp["g"]), D(inp["x"]), D(inp["wf"])
    got = dict(dw=dw, db=db)
    ws = None
    if c.mode in ("xnorm", "s2"):
        n = B * p["slots"] * c.cin * 2
        ws = torch.full((n + B * c.cin * 2,), R.NAN, dtype=torch.float64, device=dev())
        xm, xr = D(inp["xmean"]), D(inp["xrstd"])
    if c.mode == "s2":
        got["dx"] = k.conv3x3_bwd_fused_s2(g, x, wf, dw, db, xm, xr, ws, p["slots"])
    elif c.mode == "xnorm":
        got["dx"] = k.conv3x3_bwd_fused(g, x, wf, dw, db, False, 1.0, xnorm=(xm, xr, ws, p["slots"]))
    elif c.mode == "norm":
        # the caller's protocol: the image sums sit in slot 0 of a zeroed workspace and omr_instnorm_reduce_sums compacts them
        nws, nslots = k.conv_stat_ws(B, H, W, c.cout, dev())
        nws.zero_()
        nws[: B * nslots * c.cout * 2].view(B, nslots, c.cout, 2)[:, 0] = (inp["k"] * (H * W)).to(dev())
        k.instnorm_reduce_sums(nws, nslots, B, c.cout)
        got["dx"] = k.conv3x3_bwd_fused(g, x, wf, dw, db, True, R.fused_mask_scale(c),
                                        norm=(D(inp["y"]), D(inp["ymean"]), D(inp["yrstd"]), nws, nslots, True, R.FUSED_RELU_SCALE))
    else:
        got["dx"] = k.conv3x3_bwd_fused(g, x, wf, dw, db, c.mode == "mask", R.fused_mask_scale(c) if c.mode == "mask" else 1.0)
    torch.cuda.synchronize()
    if ws is not None:
        sl = ws[:n].view(B, p["slots"], c.cin, 2).cpu()
        assert bool(torch.isfinite(sl).all()), f"{c.name}: a statistics slot was not written"
        got["sums"] = sl.sum(dim=1)
    R.fused_check(c, got)


def test_weight_flip_kernel_is_the_reference_flip():
    """omr_conv3x3_weight_flip (the fused and data-gradient cases above are fed flip_weights() from the CPU)."""
    w = R.ints((48, 3, 3, 40), 77, -100, 100).to(BF16)
    assert torch.equal(K().conv3x3_weight_flip(w.to(dev())).cpu(), R.flip_weights(w))
