"""CPU only: the extent arithmetic of the ragged-batch path and the invariant it rests on, in fp64 torch.  Pins tests/extent_refs.py
(the reference of the GPU tests) against the oracle encoder run on each cropped sample."""
import pytest
import torch

import extent_refs as E
from omr_a2s_multimodal_transformer_amd import synthetic as syn
from omr_a2s_multimodal_transformer_amd.encoder import Encoder
from omr_a2s_multimodal_transformer_amd.image import collate_ragged
from omr_a2s_multimodal_transformer_amd.kernels import conv_out_hw
from oracle import ref_cpu as R


def rnd(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo


def test_extent_levels_against_brute_force():
    """Every level of every size 1..70 x 1..40: ceil(previous / stride) = the number of windows a k=3 / pad=1 conv of that stride places
    (enumerated), = kernels.conv_out_hw; Encoder.extent_levels returns the same table; the last level is (ceil(h/16), ceil(w/8))."""
    sizes = [(h, w) for h in range(1, 71) for w in (1, 2, 7, 8, 9, 16, 17, 39, 40)]
    levels = E.extent_levels(sizes)
    assert len(levels) == 6
    for lv, nxt, (sh, sw) in zip(levels, levels[1:], R.CONV_STRIDES):
        for (h, w), (h2, w2) in zip(lv, nxt):
            assert (h2, w2) == (E.conv_out_brute(h, sh), E.conv_out_brute(w, sw)) == conv_out_hw(h, w, (sh, sw))
    assert levels[-1] == [(-(-h // 16), -(-w // 8)) for h, w in sizes]
    table = Encoder(1).extent_levels(torch.tensor(sizes))
    assert table.dtype == torch.int32 and table.tolist() == [[list(e) for e in lv] for lv in levels]
    with pytest.raises(ValueError):
        Encoder(1).extent_levels(torch.tensor([[0, 5]]))


def test_issue_shapes_cover_the_cases_they_name():
    lv = E.extent_levels(E.SIZES)
    assert lv[0][0] == E.PLANE and lv[-1] == [(4, 12), (3, 7), (2, 2)]
    assert E.SIZES[1][0] % 16 and E.SIZES[1][1] % 8 and E.SIZES[1][0] % 2 and max(E.SIZES[2]) < 32


def test_pack_row_map_against_brute_force():
    ext = [(4, 12), (3, 7), (2, 2), (1, 1)]
    smax = 50
    x = torch.arange(4 * 5 * 13 * 2, dtype=torch.float64).view(4, 5, 13, 2)
    packed = E.pack_rows(x, ext, smax)
    for b, e in enumerate(ext):
        rows = E.pack_row_map_brute(e)
        assert len(rows) == e[0] * e[1]
        for r, (i, j) in rows.items():
            assert r == i * e[1] + j and torch.equal(packed[b, r], x[b, i, j])
        assert not packed[b, len(rows):].any()
        # the packed rows are the sample's own grid flattened like model.py:147
        assert torch.equal(packed[b, :len(rows)], x[b, :e[0], :e[1]].permute(2, 0, 1).flatten(1).t())


def test_collate_ragged_pads_with_zeros_and_reports_sizes():
    imgs = [torch.full((1, h, w), float(k + 1)) for k, (h, w) in enumerate(E.SIZES)]
    x, sizes = collate_ragged(imgs)
    assert tuple(x.shape) == (3, 1) + E.PLANE and sizes.tolist() == [list(s) for s in E.SIZES]
    for b, (h, w) in enumerate(E.SIZES):
        assert bool((x[b, :, :h, :w] == b + 1).all()) and float(x[b].sum()) == (b + 1) * h * w
    x2, _ = collate_ragged([im[0] for im in imgs])            # [h, w] samples
    assert torch.equal(x, x2)


@pytest.fixture(scope="module")
def oracle_encoder():
    sd = {k: v.double() for k, v in syn.seeded_state_dict(syn.encoder_shapes("encoder."), 13).items()}
    crops = [rnd((1, 1, h, w), 300 + b) for b, (h, w) in enumerate(E.SIZES)]
    with torch.no_grad():
        alone = [R.encoder(sd, "encoder.", c) for c in crops]
    x = torch.full((len(crops), 1) + E.PLANE, float("nan"), dtype=torch.float64)      # the collate pad value is the caller's
    for b, c in enumerate(crops):
        x[b, :, :c.shape[2], :c.shape[3]] = c[0]
    return sd, x, alone


def test_masked_encoder_on_the_padded_batch_equals_the_oracle_on_each_crop(oracle_encoder):
    """THE invariant (activations zero outside each extent => sample b's features are those of b alone), fp64, <= 1e-12."""
    sd, x, alone = oracle_encoder
    with torch.no_grad():
        got = E.masked_encoder(sd, "encoder.", x, E.SIZES)
    grid = E.extent_levels(E.SIZES)[-1]
    assert tuple(got.shape[2:]) == grid[0]
    for b, ((h, w), ref) in enumerate(zip(grid, alone)):
        assert tuple(ref.shape[2:]) == (h, w)
        err = float((got[b:b + 1, :, :h, :w] - ref).abs().max())
        assert err <= 1e-12 * max(1.0, float(ref.abs().max())), (b, err)
        outside = got[b].clone()
        outside[:, :h, :w] = 0
        assert not outside.any(), f"sample {b}: features outside its extent"


def test_an_extent_rule_that_is_off_by_one_breaks_it(oracle_encoder):
    """floor(h / s) instead of ceil(h / s) zeroes the last row / column of an odd extent: the test above can see a wrong stride rule."""
    sd, x, alone = oracle_encoder
    with torch.no_grad():
        got = E.masked_encoder(sd, "encoder.", x, E.SIZES, out_extent_of=lambda n, s: max(1, n // s))
    h, w = E.extent_levels(E.SIZES)[-1][1]
    err = float((got[1:2, :, :h, :w] - alone[1]).abs().max())
    assert err > 1e-6, err
