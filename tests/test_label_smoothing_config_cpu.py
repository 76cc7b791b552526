"""CPU-only: ModelConfig.label_smoothing through to_dict / from_dict / save_pretrained, model construction and checkpoints."""
import pytest
import torch

from omr_a2s_multimodal_transformer_amd import synthetic as syn
from omr_a2s_multimodal_transformer_amd.config import ModelConfig

V = 40


def small(**kw) -> ModelConfig:
    return ModelConfig(d_model=128, ff_dim=128, num_layers=1, **kw)


def make(config):
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    w2i, i2w = syn.make_vocab(V)
    return Transformer(32, 64, 16, w2i, i2w, config=config)


def test_config_round_trips_the_field(tmp_path):
    c = small(label_smoothing=0.1)
    assert c.to_dict()["label_smoothing"] == 0.1
    assert ModelConfig.from_dict(c.to_dict()) == c
    p = str(tmp_path / "config.json")
    c.save_pretrained(p)
    assert ModelConfig.from_pretrained(p) == c and ModelConfig.from_pretrained(p).label_smoothing == 0.1


def test_a_dictionary_from_before_the_field_gives_0():
    d = small(label_smoothing=0.3).to_dict()
    del d["label_smoothing"]
    assert ModelConfig.from_dict(d).label_smoothing == 0.0 and ModelConfig().label_smoothing == 0.0


def test_the_model_hands_it_to_the_loss():
    assert make(small(label_smoothing=0.1)).compute_loss.label_smoothing == 0.1
    m = make(None)
    assert m.compute_loss.label_smoothing == 0.0 and m.compute_loss.last_nll is None
    assert make(small(label_smoothing=1.0)).compute_loss.label_smoothing == 1.0


@pytest.mark.parametrize("eps", [-0.1, 1.5, float("nan")])
def test_out_of_range_is_a_value_error_at_construction(eps):
    from omr_a2s_multimodal_transformer_amd.model import CrossEntropyLoss
    with pytest.raises(ValueError):
        make(small(label_smoothing=eps))
    with pytest.raises(ValueError):
        make(dict(small().to_dict(), label_smoothing=eps))
    with pytest.raises(ValueError):
        CrossEntropyLoss(ignore_index=0, label_smoothing=eps)


def test_checkpoint_round_trip_keeps_it_and_an_old_checkpoint_loads_with_0(tmp_path):
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    m = make(small(label_smoothing=0.1))
    p = str(tmp_path / "m.ckpt")
    m.save_checkpoint(p)
    m2 = Transformer.load_from_checkpoint(p)
    assert m2.config.label_smoothing == 0.1 and m2.compute_loss.label_smoothing == 0.1
    ck = torch.load(p, map_location="cpu", weights_only=True)
    del ck["hyper_parameters"]["config"]["label_smoothing"]           # as written before the field existed
    old = str(tmp_path / "old.ckpt")
    torch.save(ck, old)
    m3 = Transformer.load_from_checkpoint(old)
    assert m3.config.label_smoothing == 0.0 and m3.compute_loss.label_smoothing == 0.0 and m3.config.d_model == 128
