"""CPU-only checks of the batched beam search: the host backtrack over the history tables against a brute-force replay, the
argument checks that run before anything is encoded or launched, and the new entry points of the C ABI."""
import ctypes
import random
import subprocess

import pytest
import torch

from omr_a2s_multimodal_transformer_amd import _lib
from omr_a2s_multimodal_transformer_amd import synthetic as syn
from omr_a2s_multimodal_transformer_amd.config import ModelConfig
from omr_a2s_multimodal_transformer_amd.decoder import MAX_BEAM, _BeamDesc
from omr_a2s_multimodal_transformer_amd.evaluation import beam_backtrack, beam_results

NEW = ("omr_beam_select", "omr_beam_decode_steps", "omr_beam_workspace_bytes")


def test_new_entry_points_are_declared_and_exported():
    protos = _lib.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T omr_" in line}
    for name in NEW:
        assert name in protos, name
        assert name in exported, name
    assert protos["omr_beam_decode_steps"][1][:3] == ["const omr_decode_desc* desc", "const omr_beam_desc* beam_desc", "const int* mem_len"]
    assert protos["omr_beam_workspace_bytes"][0] == "long"


def test_beam_desc_mirror_has_the_c_layout_and_the_library_carves_it():
    assert ctypes.sizeof(_BeamDesc) == 4 * 4 + 2 * 8 + 12 * 8
    bd = _BeamDesc()
    bd.beam, bd.N, bd.max_len, bd.state = 4, 3, 16, None
    n = _lib.lib().query("omr_beam_workspace_bytes", ctypes.byref(bd))
    offs = [int(getattr(bd, f) or 0) for f in _BeamDesc.STATE_FIELDS]
    sizes = [12 * 8, 3 * 8, 12 * 8, 3 * 4, 3 * 4, 3 * 4, 3 * 4, 12 * 4, 16 * 12 * 4, 16 * 12 * 4]
    assert offs[0] == 0 and all(o % 256 == 0 for o in offs)
    assert all(offs[i] + sizes[i] <= offs[i + 1] for i in range(9)) and offs[9] + sizes[9] <= n
    for beam in (0, MAX_BEAM + 1):                         # refused: beam outside 1..8
        bd.beam = beam
        assert _lib.lib().query("omr_beam_workspace_bytes", ctypes.byref(bd)) < 0


def _replay(beam, positions, rng, vocab=9):
    """A random beam-search history of one input, carried the slow way: every row holds its whole token list."""
    seqs = [[] for _ in range(beam)]
    hp, ht, snaps = [], [], [list(map(list, seqs))]
    for _ in range(positions):
        parents = [rng.randrange(beam) for _ in range(beam)]
        toks = [rng.randrange(vocab) for _ in range(beam)]
        seqs = [seqs[p] + [t] for p, t in zip(parents, toks)]
        hp.append(parents)
        ht.append(toks)
        snaps.append(list(map(list, seqs)))
    return hp, ht, snaps


@pytest.mark.parametrize("beam", [1, 2, 3, 4, 8])
def test_beam_backtrack_equals_a_brute_force_replay(beam):
    rng = random.Random(100 + beam)
    for positions in (1, 2, 7, 24):
        hp, ht, snaps = _replay(beam, positions, rng)
        for pos in range(positions + 1):                   # position 0 (empty prefix) .. the last position
            for row in range(beam):
                assert beam_backtrack(hp, ht, row, pos) == snaps[pos][row], (positions, pos, row)
    assert beam_backtrack([], [], 0, 0) == []


def test_beam_results_assembles_finished_and_exhausted_inputs():
    rng = random.Random(7)
    beam, positions, eos = 3, 6, 1
    tables = [_replay(beam, positions, rng) for _ in range(4)]
    hp = [sum((tables[n][0][p] for n in range(4)), []) for p in range(positions)]          # [positions][rows], rows = 4 * beam
    ht = [sum((tables[n][1][p] for n in range(4)), []) for p in range(positions)]
    ninf = float("-inf")
    scores = [-5.0, -6.0, ninf, -1.0, -2.0, -3.0, -9.0, ninf, ninf, -4.0, -4.5, -4.75]
    # input 0: finished at position 0 (just <eos>), done.  1: finished at the last position, done.  2: ran out of positions,
    # its finished hypothesis still leads.  3: ran out of positions with nothing finished.
    best_score, best_row, best_pos, done = [-0.5, -0.25, -8.0, ninf], [0, 2, 1, 0], [0, positions - 1, 3, 0], [1, 1, 0, 0]
    got = beam_results(beam, positions, eos, scores, best_score, best_row, best_pos, done, hp, ht)
    assert got[0] == ([eos], -0.5)
    assert got[1] == (tables[1][2][positions - 1][2] + [eos], -0.25)
    assert got[2] == (tables[2][2][3][1] + [eos], -8.0)
    assert got[3] == (tables[3][2][positions][0], -4.0)
    scores[6] = -7.0                                       # ... and now input 2's live hypothesis overtakes the finished one
    assert beam_results(beam, positions, eos, scores, best_score, best_row, best_pos, done, hp, ht)[2] == (tables[2][2][positions][0], -7.0)


def _cpu_model(cls="Transformer"):
    from omr_a2s_multimodal_transformer_amd import model as M
    w2i, i2w = syn.make_vocab(30)
    cfg = ModelConfig(num_layers=1)
    if cls == "Transformer":
        return M.Transformer(64, 256, 16, w2i, i2w, config=cfg)
    return M.MultimodalTransformer(64, 256, 64, 256, 16, w2i, i2w, config=cfg)


@pytest.mark.parametrize("cls", ["Transformer", "MultimodalTransformer"])
@pytest.mark.parametrize("beam", [0, 9, -1])
def test_predict_and_evaluate_refuse_a_bad_beam_before_encoding(cls, beam):
    m = _cpu_model(cls)

    def no_encode(*a, **k):
        pytest.fail("an input was encoded before the beam width was checked")

    m._encode_input = no_encode
    m.encode = no_encode
    m.encoder_forward = no_encode
    x = torch.zeros(1, 1, 32, 32)
    item = x if cls == "Transformer" else (x, x)
    y = torch.tensor([[2, 5, 1]])
    batch = (x, y) if cls == "Transformer" else (x, x, y)
    with pytest.raises(ValueError, match="beam"):
        m.predict([item], beam=beam)
    with pytest.raises(ValueError, match="beam"):
        m.evaluate([batch], beam=beam)


def test_beam_search_batch_refuses_bad_arguments_before_launching():
    m = _cpu_model()
    with pytest.raises(ValueError, match="no memories given"):
        m.beam_search_batch([])
    with pytest.raises(ValueError, match="beam"):
        m.beam_search_batch([torch.zeros(100, 256)], beam=9)
    with pytest.raises(ValueError, match="empty"):
        m.beam_search_batch([torch.zeros(100, 256), torch.zeros(0, 256)])
    with pytest.raises(ValueError, match="beam"):
        m.decoder.init_beam_decode([torch.zeros(100, 256)], 0)
