"""CPU only: the reference of the ragged multimodal route (tests/multimodal_ragged_refs.py) in fp64.  Pins concat_rows and its adjoint,
and shows that the written-out route (masked encoders -> pack -> mixer with exact key masks -> decoder with the bool mask) on the
padded batch gives, for every pair, the logits of oracle.ref_cpu.multimodal_forward of that pair alone (lengths None) -- and that a
wrong concat offset, a missing key mask or the reference's block mask do not.  Shapes: the issue's (multimodal_ragged_refs)."""
import functools

import pytest
import torch

import multimodal_ragged_refs as M
from omr_a2s_multimodal_transformer_amd import synthetic as syn
from oracle import ref_cpu as R

TOL = 1e-10
CFG = R.OracleCfg(d_model=M.D, nhead=4, ff_dim=M.D, num_layers=M.LAYERS)


# ------------------------------------------------------------------------------------------------ 1. concat_rows

def test_issue_shapes_cover_the_cases_they_name():
    assert tuple(M.memory_lengths(M.IMG_SIZES)) == M.IMG_LENS == (48, 21, 4)
    assert tuple(M.memory_lengths(M.AUD_SIZES)) == M.AUD_LENS == (9, 15, 4)
    both = [a + b for a, b in zip(M.IMG_LENS, M.AUD_LENS)]
    assert both == [57, 36, 8] and max(both) != max(M.IMG_LENS) + max(M.AUD_LENS)
    assert M.IMG_LENS.index(max(M.IMG_LENS)) != M.AUD_LENS.index(max(M.AUD_LENS))


@pytest.mark.parametrize("smax", [57, 63, 30, 5])
def test_concat_rows_against_a_brute_force_row_map(smax):
    """Also with smax below a sample's la + lb (rows dropped) and below la (b absent), and with NaN past every length."""
    la, lb = (48, 21, 4, 0), (9, 15, 0, 3)
    a = torch.arange(4 * 48 * 2, dtype=torch.float64).view(4, 48, 2) + 1
    b = -(torch.arange(4 * 15 * 2, dtype=torch.float64).view(4, 15, 2) + 1)
    for i in range(4):
        a[i, la[i]:] = float("nan")
        b[i, lb[i]:] = float("nan")
    out = M.concat_rows(a, la, b, lb, smax)
    assert tuple(out.shape) == (4, smax, 2)
    for i in range(4):
        rows = M.concat_row_map_brute(la[i], lb[i], smax)
        assert len(rows) == min(la[i] + lb[i], smax)
        for r in range(smax):
            if r in rows:
                which, k = rows[r]
                assert torch.equal(out[i, r], (a if which == "a" else b)[i, k]), (i, r)
            else:
                assert not out[i, r].any(), (i, r)
    tail = M.concat_rows(a, la, None, None, 48)                # the tail-zeroing form
    for i in range(4):
        assert torch.equal(tail[i, :la[i]], a[i, :la[i]]) and not tail[i, la[i]:].any()


@pytest.mark.parametrize("smax", [57, 30])
def test_concat_rows_adjoint_is_the_transpose_exactly(smax):
    """<concat(a, b), g> = <a, da> + <b, db> on small integers in fp64: every product and sum is exact."""
    la, lb = (48, 21, 4), (9, 15, 0)
    gen = torch.Generator().manual_seed(5)
    a, b, g = (torch.randint(-8, 9, s, generator=gen).double() for s in ((3, 48, 3), (3, 15, 3), (3, smax, 3)))
    da, db = M.concat_rows_adjoint(g, la, 48, lb, 15)
    lhs = float((M.concat_rows(a, la, b, lb, smax) * g).sum())
    assert lhs == float((a * da).sum() + (b * db).sum()) and lhs != 0.0
    for i in range(3):
        assert not da[i, la[i]:].any() and not db[i, lb[i]:].any()
    da1, none = M.concat_rows_adjoint(g, la, 48, None, 0)                     # the tail-zeroing form
    assert none is None and float((M.concat_rows(a, la, None, None, smax) * g).sum()) == float((a * da1).sum())


# ------------------------------------------------------------------------------------------------ 2. the route, fp64

@functools.lru_cache(maxsize=None)
def setup(mixer: str):
    w2i, _ = syn.make_vocab(M.V)
    sd = {k: v.double() for k, v in syn.seeded_state_dict(syn.multimodal_shapes(M.V, mixer, M.D, M.D, M.LAYERS), 23).items()}
    ci, ca, xi, si, xa, sa = M.make_pairs(dtype=torch.float64, pad=float("nan"))      # the collate pad value is the caller's
    y_in, _, counts = M.make_targets(w2i)
    return sd, ci, ca, xi, si, xa, sa, y_in, counts


@functools.lru_cache(maxsize=None)
def alone(mixer: str, modality: str):
    """Logits [V, n_b] of every pair alone, at its non-pad positions: multimodal_forward with xli = xla = None."""
    sd, ci, ca, _, _, _, _, y_in, counts = setup(mixer)
    with torch.no_grad():
        return [R.multimodal_forward(sd, ci[b], None, ca[b], None, y_in[b:b + 1], CFG, mixer, M.IMG_PLANE, M.AUD_PLANE, modality)[0, :, :n]
                for b, n in enumerate(counts)]


def errors(mixer: str, modality: str = "both", **kw):
    """Per sample: max |ragged - alone| over the logits of its non-pad positions, relative to the largest |logit| of the sample alone."""
    sd, _, _, xi, si, xa, sa, y_in, counts = setup(mixer)
    with torch.no_grad():
        got = M.ragged_multimodal_ref(sd, xi, si, xa, sa, y_in, CFG, mixer, M.IMG_PLANE, M.AUD_PLANE, modality, **kw)
    assert torch.isfinite(got).all()
    return [float((got[b, :, :n] - ref).abs().max() / ref.abs().max()) for b, (n, ref) in enumerate(zip(counts, alone(mixer, modality)))]


@pytest.mark.parametrize("mixer", M.MIXERS)
def test_ragged_reference_equals_every_pair_alone_fp64(mixer):
    err = errors(mixer)
    print(f"{mixer}: {err}")
    assert max(err) <= TOL, err


@pytest.mark.parametrize("modality", ["image", "audio"])
def test_ragged_reference_with_a_dropped_modality_equals_every_pair_alone_fp64(modality):
    err = errors("concat", modality)
    print(f"{modality}: {err}")
    assert max(err) <= TOL, err


# ------------------------------------------------------------------------------------------------ 3. negative controls

@pytest.mark.parametrize("mixer", ["concat", "attn_both"])
@pytest.mark.parametrize("shift", [1, -1])
def test_a_concat_offset_off_by_one_row_breaks_it(mixer, shift):
    err = errors(mixer, concat_shift=shift)
    print(f"{mixer} shift {shift}: {err}")
    assert min(err) > 1e3 * TOL, err                        # every sample has audio rows to misplace


@pytest.mark.parametrize("mixer", ["attn_img", "attn_audio", "attn_both"])
@pytest.mark.parametrize("key_mask", ["none", "block"])
def test_leaving_the_key_mask_out_or_using_the_block_mask_breaks_it(mixer, key_mask):
    """Without a key mask the zero rows behind a shorter memory are keys (their K is the bias); the quirk-2 block mask only covers query
    rows past lq, so every real query row still sees them, and head h of sample b gets the lengths of sample (4 b + h) % 3."""
    err = errors(mixer, key_mask=key_mask)
    print(f"{mixer} key mask {key_mask}: {err}")
    # the sample whose key memory is the longest of the batch has no padded keys: attn_img sample 0, attn_audio sample 1
    padded = {"attn_img": (1, 2), "attn_audio": (0, 2), "attn_both": (0, 1, 2)}[mixer]
    assert min(err[b] for b in padded) > 1e3 * TOL, err


# ------------------------------------------------------------------------------------------------ 4. route detection

def test_route_detection():
    from omr_a2s_multimodal_transformer_amd.model import MultimodalTransformer, Transformer, _pair_route
    B = 3
    px = torch.tensor([[64, 96], [37, 50], [17, 9]])
    for dt in (torch.int64, torch.int32):
        assert _pair_route(px.to(dt), px.to(dt)) == "ragged"
    lens = torch.tensor([48, 21, 4])
    assert _pair_route(lens, lens) == "dense" and _pair_route(None, None) == "dense"
    assert _pair_route(torch.zeros((B, 48), dtype=torch.bool), torch.zeros((B, 15), dtype=torch.bool)) == "dense"
    assert _pair_route(torch.zeros((B, 2), dtype=torch.bool), torch.zeros((B, 2), dtype=torch.bool)) == "dense"     # S == 2 masks
    assert _pair_route(px.float(), px.float()) == "dense"
    for other in (None, lens, torch.zeros((B, 48), dtype=torch.bool), px.float()):
        with pytest.raises(ValueError):
            _pair_route(px, other)
        with pytest.raises(ValueError):
            _pair_route(other, px)
    assert Transformer._is_pixel_sizes(px) and not Transformer._is_pixel_sizes(lens)      # the unimodal rule, where it was
    # the model asks the same rule before it touches an encoder
    w2i, i2w = syn.make_vocab(M.V)
    m = MultimodalTransformer(64, 96, 35, 40, 16, w2i, i2w)
    with pytest.raises(ValueError):
        m.encoder_forward(torch.zeros(B, 1, 64, 96), torch.zeros(B, 1, 35, 40), px, lens)


def test_collate_ragged_pairs_is_two_collate_ragged_calls():
    from omr_a2s_multimodal_transformer_amd.image import collate_ragged, collate_ragged_pairs
    ci, ca, xi, si, xa, sa = M.make_pairs()
    got = collate_ragged_pairs([c[0] for c in ci], [c[0] for c in ca])
    for g, r in zip(got, collate_ragged([c[0] for c in ci]) + collate_ragged([c[0] for c in ca])):
        assert torch.equal(g, r)
    assert torch.equal(got[0], xi) and torch.equal(got[1], si) and torch.equal(got[2], xa) and torch.equal(got[3], sa)
    with pytest.raises(ValueError):
        collate_ragged_pairs([c[0] for c in ci], [c[0] for c in ca][:2])
