"""CPU only: the fp64 reference of the attention map (tests/attention_map_refs.py) against torch's own nn.MultiheadAttention and
against oracle/attention_refs.py, what its bound sees, and the host arithmetic of evaluation.cells_and_boxes."""
import numpy as np
import pytest
import torch

import attention_map_refs as M
from omr_a2s_multimodal_transformer_amd.evaluation import cells_and_boxes, grid_of, plan_align_groups
from oracle import attention_refs as R

F64 = torch.float64
C = R.AttnCase
MHA_CASES = (
    C("mha-none", "fwd", 3, 4, 9, 11, 32),
    C("mha-boolmask", "fwd", 3, 4, 9, 11, 32),              # the bool key mask is built in the test: keys 10 - 2 b .. of row b hidden
    C("mha-blk", "fwd", 3, 4, 9, 11, 32, blk=((5, 3, 2), (7, 4, 2))),
)


@pytest.mark.parametrize("case", MHA_CASES, ids=lambda c: c.name)
def test_reference_equals_torch_multihead_attention(case):
    """B 3, H 4, hd 32, T 9, S 11 in fp64: nn.MultiheadAttention(batch_first=True)(need_weights=True) with identity projections,
    the -inf key mask as key_padding_mask, the block mask tiled the way the reference tiles it (.repeat(num_heads, 1, 1))."""
    inp = R.attn_inputs(case, F64)
    B, H, T, S, d = case.B, case.H, case.T, case.S, case.d
    kpm = None
    if case.name == "mha-boolmask":
        kpm = torch.arange(S)[None, :] >= torch.tensor([10, 8, 6])[:, None]
    bias = None if kpm is None else torch.zeros(B, S).masked_fill(kpm, float("-inf"))
    w_ref, bound = M.weights_ref(inp["q"], inp["k"], H, case=case, dtype=F64, key_bias=bias)
    mha = torch.nn.MultiheadAttention(d, H, batch_first=True, dtype=F64).eval()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(d, dtype=F64).repeat(3, 1))
        mha.in_proj_bias.zero_()
        am = None
        if case.blk is not None:
            m = torch.zeros(B, T, S, dtype=torch.bool)
            for b, (lq, lkv) in enumerate(zip(*case.blk)):
                m[b, lq:, lkv:] = True
            am = m.repeat(H, 1, 1)
        _, w = mha(inp["q"].contiguous(), inp["k"].contiguous(), inp["v"].contiguous(), key_padding_mask=kpm, attn_mask=am, need_weights=True)
    err = float((w - w_ref).abs().max())
    print(f"{case.name}: max |reference - nn.MultiheadAttention| {err:.3e}")
    assert err <= 1e-12
    assert float((w_ref.sum(dim=-1) - 1.0).abs().max()) <= 1e-12            # no dropout: rows sum to 1
    if kpm is not None:
        assert float(w_ref.masked_select(kpm[:, None, :].expand(B, T, S)).abs().max()) == 0.0
    assert bool(torch.isfinite(bound).all()) and float(bound.min()) >= 0.0


def test_plus_one_bias_is_added_and_rows_sum_to_one():
    case = M.MAP_CASE["map-t33-s65-hd32-plus1"]
    inp = R.attn_inputs(case, torch.float32)
    w_ref, _ = M.map_case_ref(case, torch.float32)
    hd, H = case.hd, case.H
    q, k = inp["q"].double().view(case.B, case.T, H, hd), inp["k"].double().view(case.B, case.S, H, hd)
    s = torch.einsum("bthd,bshd->bhts", q, k) / hd ** 0.5 + inp["bias"].double()[:, None, None, :]
    assert float((torch.softmax(s, dim=-1).mean(dim=1) - w_ref).abs().max()) <= 1e-12
    assert float((w_ref.sum(dim=-1) - 1.0).abs().max()) <= 1e-12


@pytest.mark.parametrize("name", ["mha-h1-needles", "mha-h1-drop"])
def test_single_head_weights_times_v_is_the_attention_output(name):
    """H = 1: out_scale = 1 and w is the (post-dropout) probability matrix itself, so w @ V is attention_ref's O."""
    case = C(name, "fwd", 2, 1, 33, 65, 32, family="needles", drop=(0.25, 5) if name.endswith("drop") else None)
    inp = R.attn_inputs(case, torch.float32)
    w_ref, _ = M.weights_ref(inp["q"], inp["k"], 1, case=case, dtype=torch.float32, key_bias=inp["bias"], keep=inp["keep"])
    o_ref = R.attention_ref(inp["q"], inp["k"], inp["v"], 1, case=case, dtype=torch.float32, key_bias=inp["bias"], keep=inp["keep"])["o"][0]
    assert float((w_ref @ inp["v"].double() - o_ref).abs().max()) <= 1e-12


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.case_id)
def test_inf_row_and_hidden_keys_are_exact_zeros(dtype):
    case = M.MAP_CASE["map-t33-s129-hd64-infrow"]
    w_ref, bound = M.map_case_ref(case, dtype)
    assert float(w_ref[case.B - 1].abs().max()) == 0.0 and float(bound[case.B - 1].max()) == 0.0
    for b in range(case.B - 1):
        cut = R.inf_cut(case, b)
        assert float(w_ref[b, :, cut:].abs().max()) == 0.0 and float(bound[b, :, cut:].max()) == 0.0
        assert float(bound[b, :, :cut].min()) > 0.0


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.case_id)
@pytest.mark.parametrize("name", ["map-t40-s300-hd32-inftail", "map-kvlen-t20-s300-hd64"])
def test_a_dropped_tile_is_outside_the_bound(name, dtype):
    """The reference itself sits at ratio 0; with one 64-key tile of a needles case zeroed -- the tile of the needles at keys 64
    and 127 -- the ratio is far above 1, and so is a map that keeps every key but forgets the head average."""
    case = M.MAP_CASE[name]
    w_ref, bound = M.map_case_ref(case, dtype)
    assert R.ratio(w_ref.clone(), w_ref, bound) == 0.0
    wrong = w_ref.clone()
    wrong[:, :, 64:128] = 0.0
    r = R.ratio(wrong, w_ref, bound)
    print(f"{name}-{R.case_id(dtype)}: tile 1 dropped: ratio {r:.1f}")
    assert r > 1.0
    assert R.ratio(w_ref * case.H, w_ref, bound) > 1.0
    inside = w_ref * (1.0 + 2.0 ** -24)                                     # one fp32 rounding is inside
    assert R.ratio(inside, w_ref, bound) <= 1.0


def test_cells_and_boxes_single_grid_clips_the_last_row_and_column():
    # 37 x 50 pixels -> grid 3 x 7; the last row covers pixels 32 .. 36, the last column 48 .. 49
    assert grid_of(37, 50) == (3, 7) and grid_of(64, 96) == (4, 12) and grid_of(17, 9) == (2, 2)
    cell, box, source = cells_and_boxes([0, 6, 7, 20, 14], (("image", 37, 50),))
    assert cell.tolist() == [[0, 0], [0, 6], [1, 0], [2, 6], [2, 0]]
    assert box.tolist() == [[0, 0, 16, 8], [0, 48, 16, 50], [16, 0, 32, 8], [32, 48, 37, 50], [32, 0, 37, 8]]
    assert source == ["image"] * 5
    assert cell.dtype == np.int64 and box.dtype == np.int64 and box.shape == (5, 4)
    with pytest.raises(ValueError):
        cells_and_boxes([21], (("image", 37, 50),))
    with pytest.raises(ValueError):
        cells_and_boxes([0], (("image", 37, 50),), split=3)
    cell, box, source = cells_and_boxes([], (("audio", 37, 50),))
    assert cell.shape == (0, 2) and box.shape == (0, 4) and source == []


def test_cells_and_boxes_concat_splits_at_the_image_length():
    # image 17 x 9 -> 2 x 2 = 4 rows; audio 33 x 20 -> 3 x 3 = 9 rows, in spectrogram coordinates
    sizes = (("image", 17, 9), ("audio", 33, 20))
    cell, box, source = cells_and_boxes([0, 3, 4, 12, 8], sizes, split=4)
    assert source == ["image", "image", "audio", "audio", "audio"]
    assert cell.tolist() == [[0, 0], [1, 1], [0, 0], [2, 2], [1, 1]]
    assert box.tolist() == [[0, 0, 16, 8], [16, 8, 17, 9], [0, 0, 16, 8], [32, 16, 33, 20], [16, 8, 32, 16]]
    assert cells_and_boxes([4], sizes)[2] == ["audio"]                      # split defaults to the first grid's length
    with pytest.raises(ValueError):
        cells_and_boxes([0], sizes, split=5)
    with pytest.raises(ValueError):
        cells_and_boxes([13], sizes, split=4)


def test_cells_and_boxes_attention_mixers_name_the_query_grid():
    # attn_img: queries = audio, the memory lives on the audio grid; attn_audio: the image grid
    assert cells_and_boxes([8], (("audio", 33, 20),))[2] == ["audio"]
    cell, box, source = cells_and_boxes([3], (("image", 17, 9),))
    assert source == ["image"] and cell.tolist() == [[1, 1]] and box.tolist() == [[16, 8, 17, 9]]


def test_plan_align_groups_cuts_by_rows_and_by_bytes():
    assert plan_align_groups([5, 6, 7], [10, 20, 30], 2) == [[0, 1], [2]]
    assert plan_align_groups([5, 6, 7], [10, 20, 30], 8) == [[0, 1, 2]]
    # 2 rows x 6 x 20 x 4 bytes = 960 > 900: every input alone, also the one that exceeds the limit by itself
    assert plan_align_groups([5, 6, 7], [10, 20, 30], 8, limit_bytes=900) == [[0], [1], [2]]
    assert plan_align_groups([5, 6, 7], [10, 20, 30], 8, limit_bytes=100) == [[0], [1], [2]]
    assert plan_align_groups([5, 6, 7], [10, 20, 30], 8, limit_bytes=960) == [[0, 1], [2]]
    assert plan_align_groups([], [], 4) == []
    with pytest.raises(ValueError):
        plan_align_groups([1], [1], 0)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.case_id)
@pytest.mark.parametrize("name", ["map-t33-s129-hd64-infrow", "map-drop-causal-t129-hd32", "map-blk-b3-h4-t40-s100-hd32"])
def test_lse_and_its_bound_are_the_oracles(name, dtype):
    """This file's per-head routine restates oracle.attention_refs' score error and lse bound; the two must not drift apart: lse and
    bound(lse) equal attention_ref's, to the last bit of the same fp64 expressions."""
    case = M.MAP_CASE[name]
    inp = R.attn_inputs(case, dtype)
    lse_ref, blse_ref = R.attention_ref(inp["q"], inp["k"], inp["v"], case.H, case=case, dtype=dtype, key_bias=inp["bias"], keep=inp["keep"])["lse"]
    q, k, hd = inp["q"].double(), inp["k"].double(), case.hd
    for b in range(case.B):
        bias = None if inp["bias"] is None else inp["bias"][b].double()
        for h in range(case.H):
            ch = slice(h * hd, (h + 1) * hd)
            vis = R.visibility(case, b, h, case.S, bias)
            _, _, lse, blse = M._p_and_rel(q[b, :, ch], k[b, :, ch], bias, vis, R.unit(dtype), hd)
            dead = ~vis.any(dim=1)
            assert bool((lse_ref[b, h][dead] == float("-inf")).all()) and bool((lse[dead] == 0).all())
            assert torch.equal(lse[~dead], lse_ref[b, h][~dead]) and torch.equal(blse, blse_ref[b, h])


def test_range_plan_restated():
    """choose_range restated (tests/attention_map_refs.expected_range): the tiny cases get one tile per workgroup, the range cases
    two, the C2 cross-attention shape eight; the GPU tests hold omr_attn_weights_range to this."""
    assert all(M.expected_range(c.B, c.T, c.S) == 64 for c in M.MAP_CASES)
    assert all(M.expected_range(c.B, c.T, c.S) == 128 < c.S for c in M.RANGE_CASES)
    assert M.expected_range(32, 512, 4096) == 512
    assert M.expected_range(2, 40, 300, min_wg=2) == 320 and M.expected_range(2, 40, 300, min_wg=4) == 192
