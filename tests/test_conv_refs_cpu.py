"""The convolution case table of oracle/conv_refs.py without a GPU: torch CPU fp32 / bf16 arithmetic (with the kernels' roundings: the
normalised operand and the output in the compute type, fp32 sums) stands in for the kernels.  A correct implementation is exact on
every exact case -- including the < 2^24 condition the exactness argument rests on, which the references assert -- and within
every bound; each of a list of subtly wrong implementations fails the case built for it, which is what shows that the checks
tests/test_conv_branches_gpu.py shares with this file can see them.  The plan mirror is checked too: every multi-tile case
reaches the tile loop it names for any occupancy the hardware allows."""
import pytest
import torch
import torch.nn.functional as F

from oracle import conv_refs as R


def ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------ the plan mirror

@pytest.mark.parametrize("c", R.CONV_CASES, ids=ids(R.CONV_CASES))
def test_conv_case_reaches_its_tile_loop(c):
    p = R.conv_plan(c)
    assert p["shm"] <= R.LDS_BYTES
    assert p["min_tiles"] >= c.min_tiles, p
    if c.stat_slots < 0:
        assert p["slots"] > p["tiles"]                                   # spare slots the launch must zero
    if c.stat_mode and c.stat_slots > 0:
        assert p["tiles_h"] >= 3 and p["tiles_w"] >= 3 and c.out_hw[0] % p["th"] and c.out_hw[1] % R.TW and c.B == 2


@pytest.mark.parametrize("c", R.WGRAD_CASES, ids=ids(R.WGRAD_CASES))
def test_wgrad_case_reaches_its_kernel_and_ring(c):
    p = R.wgrad_plan(c)
    assert p["kernel"] == c.kernel, p
    assert p["min_tiles"] >= c.min_tiles and (p["cross"] or not c.cross), p
    if c.kernel == "dma":
        assert c.min_tiles >= p["nstage"] + 2 and p["shm"] <= R.LDS_BYTES


def test_every_row_of_the_dma_table_has_a_case():
    seen = set()
    for c in R.WGRAD_DMA_CASES:
        cn = 64 if c.cout > 32 else 32 if c.cout > 16 else 16
        cc = 64 if c.cin > 32 else 32 if c.cin > 16 else 16
        seen.add((tuple(c.stride), cn, cc))
    assert seen == set(R.DMA_PICK)


@pytest.mark.parametrize("c", R.DW_CASES, ids=ids(R.DW_CASES))
def test_depthwise_case_reaches_its_kernel(c):
    p = R.dw_plan(c)
    assert p["kernel"] == c.kernel and p["min_tiles"] >= c.min_tiles, p
    if c.min_tiles > 1:
        assert p["cross"]
    if p["kernel"] == "walk":
        assert p["rc"] == c.rc


@pytest.mark.parametrize("c", R.FUSED_CASES, ids=ids(R.FUSED_CASES))
def test_fused_case_turns_its_ring_over(c):
    p = R.fused_plan(c)
    assert p["min_tiles"] >= c.min_tiles, p
    if c.min_tiles > 1:
        assert c.min_tiles >= p["nslot"] + 2 and p["tiles_h"] >= 2 and p["tiles_w"] >= 2 and c.H % 8 and c.W % 32


# ------------------------------------------------------------------------------------------------ a correct implementation passes

@pytest.mark.parametrize("c", R.CONV_CASES, ids=ids(R.CONV_CASES))
def test_conv_standin_meets_every_check(c):
    out = R.conv_standin(c)
    R.conv_check(c, out["y"], out.get("sums"))


DGRAD_CASES = [c for c in R.CONV_STAT_CASES + R.CONV_WIDTH_CASES if tuple(c.dil) != (1, 1)] + [R.CONV_WALK_CASES[-1]]


@pytest.mark.parametrize("c", DGRAD_CASES, ids=ids(DGRAD_CASES))
def test_dilated_conv_with_flipped_weights_is_the_transposed_conv(c):
    """The reference of a data-gradient case (a conv over the zero-dilated operand) against autograd's input gradient of the strided conv."""
    inp = R.conv_inputs(c)
    g, wd = inp["x"].double(), inp["w"].double()                          # wd = flip_weights(w): [CIN of the conv = cout here][3][3][cin here]
    w = R.flip_weights(wd)                                                # the flip is an involution
    xin = torch.zeros((c.B, c.cout, *c.out_hw), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xin, R.nchw(w), stride=c.dil, padding=1)
    assert tuple(y.shape[2:]) == (c.H, c.W)
    y.backward(R.nchw(g))
    assert torch.equal(R.nhwc(xin.grad), R.conv_def(g, wd, (1, 1), c.dil, c.out_hw))


@pytest.mark.parametrize("c", R.WGRAD_CASES, ids=ids(R.WGRAD_CASES))
def test_wgrad_standin_meets_every_check(c):
    R.wgrad_check(c, *R.wgrad_standin(c))


@pytest.mark.parametrize("c", R.CONV1_CASES, ids=ids(R.CONV1_CASES))
def test_conv1_standin_is_exact(c):
    R.assert_exact(R.conv1_standin(c), R.conv1_ref(c), c.dtype, c.name)


@pytest.mark.parametrize("c", R.DW_CASES, ids=ids(R.DW_CASES))
def test_depthwise_standin_is_exact(c):
    out = R.dw_compute(c, torch.float32)
    R.dw_check(c, {k: v.to(torch.float32 if c.op == "wgrad" else c.dtype) for k, v in out.items()})


@pytest.mark.parametrize("c", R.FUSED_CASES, ids=ids(R.FUSED_CASES))
def test_fused_standin_is_exact(c):
    R.fused_check(c, R.fused_standin(c))


# ------------------------------------------------------------------------------------------------ wrong implementations do not

def conv_case(name):
    return next(c for c in R.CONV_CASES if c.name == name)


def wgrad_case(name):
    return next(c for c in R.WGRAD_CASES if c.name == name)


CONV_VARIANTS = [
    ("tap_border", "epi1-bf16-slots1"),              # one tap dropped on one border
    ("halo_column", "epi1-bf16-slots2"),             # the last halo column of a tile lost
    ("halo_column", "epi2-mode4-slots1"),            # ... seen through the sums alone (mode 4 stores nothing)
    ("skip_last_tile", "epi0-c16-single"),           # the last tile of a workgroup's walk skipped
    ("skip_last_tile", "epi3-chan-slots1"),
    ("stale_tile", "epi0-c64-two-chunks"),           # tile t computed from tile t - 1's staged data
    ("stale_tile", "epi2-mode2-s22-slots2"),
    ("norm_padding", "epi1-bf16-norm-slots2"),       # normalisation applied to the zero padding
    ("norm_padding", "epi0-c128-norm-max"),
    ("drop_pitch", "epi3-elem-slots1"),              # the dropout index formed with the wrong row pitch
    ("mask_double_round", "real-bf16-mask"),         # the mask's scale applied after the output was rounded
]


@pytest.mark.parametrize("variant,name", CONV_VARIANTS, ids=[f"{v}-{n}" for v, n in CONV_VARIANTS])
def test_wrong_conv_is_rejected(variant, name):
    c = conv_case(name)
    out = R.conv_standin(c, variant)
    with pytest.raises(AssertionError):
        R.conv_check(c, out["y"], out.get("sums"))


WGRAD_VARIANTS = [
    ("skip_last_tile", "dma-s11-32x32"),
    ("skip_last_tile", "c1-mfma"),
    ("stale_tile", "dma-s11-16x16"),                 # a stale ring slot: every slot of the 6-deep ring holds another image
    ("stale_tile", "dma-s22-32x32"),
    ("prev_image_stats", "dma-s11-16x16-norm"),      # the statistics of the previous image used after an image change
    ("prev_image_stats", "gen-f32-s22-norm"),
    ("channel_tail", "dma-s11-32x32-tail24"),        # a channel tail read from the neighbouring pixel
    ("channel_tail", "dma-s11-64x64-tail40"),
    ("bias_every_column", "dma-s11-32x64"),          # bias added by every cin-block column
    ("bias_every_column", "gen-f32-s11"),
    ("halo_row", "gen-f32-s21"),                     # the last halo row of a tile lost
    ("halo_row", "dma-s21-32x32"),
    # (the bounded weight-gradient cases do not see a lost row: over 3e5 terms the worst-case bound is 7 % of sum |dy| |x|.  That
    # is what the exact cases are for; the bounded ones check the roundings integers cannot.)
]


@pytest.mark.parametrize("variant,name", WGRAD_VARIANTS, ids=[f"{v}-{n}" for v, n in WGRAD_VARIANTS])
def test_wrong_wgrad_is_rejected(variant, name):
    c = wgrad_case(name)
    with pytest.raises(AssertionError):
        R.wgrad_check(c, *R.wgrad_standin(c, variant))


@pytest.mark.parametrize("name", ["fused-plain-32x32", "fused-xnorm-slots1", "fused-s2-slots1"])
def test_wrong_fused_backward_is_rejected(name):
    c = next(k for k in R.FUSED_CASES if k.name == name)
    with pytest.raises(AssertionError):
        R.fused_check(c, R.fused_standin(c, "skip_last_tile"))


def test_a_case_that_is_not_exact_is_refused():
    with pytest.raises(AssertionError, match="2\\^24"):
        R.assert_sums_fit(torch.tensor([2.0 ** 24]), "too large")
    with pytest.raises(AssertionError, match="2\\^24"):
        R.assert_sums_fit(torch.tensor([2.0 ** 23]), "halves", unit=0.5)
    R.assert_sums_fit(torch.tensor([2.0 ** 23]), "integers")
