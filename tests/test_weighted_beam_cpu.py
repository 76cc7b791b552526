"""CPU-only checks of the beam search over the weighted late fusion: the three entry points of the C ABI, and the `beam`
keyword of weighted_predict / weighted_evaluate -- checked before anything is encoded, the parameter lists unchanged."""
import inspect
import subprocess

import pytest
import torch

from omr_a2s_multimodal_transformer_amd import _lib
from omr_a2s_multimodal_transformer_amd import synthetic as syn
from omr_a2s_multimodal_transformer_amd.config import ModelConfig
from omr_a2s_multimodal_transformer_amd.weighted_fusion import weighted_evaluate, weighted_predict

ENTRY_POINTS = {
    "omr_weighted_topk_logprob": ["const float* logits_a", "long", "const float* logits_b", "long", "int", "int", "float", "int",
                                  "long* idx_out", "float* val_out", "void* stream"],
    "omr_weighted_beam_select": ["const float* logits_a", "long", "const float* logits_b", "long", "int", "float",
                                 "const omr_beam_desc* beam_desc", "int", "void* stream"],
    "omr_weighted_beam_decode_steps": ["const omr_decode_desc* desc_a", "const int* mem_len_a", "const omr_decode_desc* desc_b",
                                       "const int* mem_len_b", "const omr_beam_desc* beam_desc", "void* self_kv2_b", "float", "int", "int",
                                       "void* stream"],
}


def test_the_three_entry_points_are_declared_and_exported():
    protos = _lib.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T omr_" in line}
    for name, args in ENTRY_POINTS.items():
        assert name in protos and name in exported, name
        assert protos[name] == ("int", args), name


def _cpu_models():
    from omr_a2s_multimodal_transformer_amd import model as M
    w2i, i2w = syn.make_vocab(30)
    models = [M.Transformer(64, 256, 16, w2i, i2w, config=ModelConfig(num_layers=1)) for _ in range(2)]

    def no_encode(*a, **k):
        pytest.fail("an input was encoded before the arguments were checked")

    for m in models:
        m.encode = no_encode
    return models


def _inputs():
    x = torch.zeros(1, 1, 32, 32)
    return [(x, x)], [(x, x, torch.tensor([[2, 5, 1]]))]


@pytest.mark.parametrize("beam", [0, 9, 2.0])
def test_a_bad_beam_is_refused_before_anything_is_encoded(beam):
    img, aud = _cpu_models()
    pairs, batches = _inputs()
    with pytest.raises(ValueError, match="beam"):
        weighted_predict(pairs, img, aud, beam=beam)
    with pytest.raises(ValueError, match="beam"):
        weighted_evaluate(batches, img, aud, alpha=[0.3, 0.7], beam=beam)


def test_a_beam_with_refill_is_refused():
    img, aud = _cpu_models()
    pairs, batches = _inputs()
    with pytest.raises(ValueError, match="refill"):
        weighted_predict(pairs, img, aud, beam=2, refill=True)
    with pytest.raises(ValueError, match="refill"):
        weighted_evaluate(batches, img, aud, beam=2, refill=True)


def test_the_parameter_lists_are_unchanged():
    assert list(inspect.signature(weighted_predict).parameters) == ["pairs", "img_model", "audio_model", "alpha", "batch_size", "sync_every"]
    assert list(inspect.signature(weighted_evaluate).parameters) == ["batches", "img_model", "audio_model", "alpha", "batch_size"]
