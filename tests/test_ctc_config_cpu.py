"""CPU-only: ModelConfig.ctc_weight / ctc_pool through to_dict / from_dict / save_pretrained, model construction and checkpoints."""
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


def test_config_round_trips_the_fields(tmp_path):
    c = small(ctc_weight=0.3, ctc_pool=4)
    assert c.to_dict()["ctc_weight"] == 0.3 and c.to_dict()["ctc_pool"] == 4
    assert ModelConfig.from_dict(c.to_dict()) == c
    p = str(tmp_path / "config.json")
    c.save_pretrained(p)
    assert ModelConfig.from_pretrained(p) == c and ModelConfig.from_pretrained(p).ctc_pool == 4


def test_a_dictionary_from_before_the_fields_gives_0_and_1():
    d = small(ctc_weight=0.3, ctc_pool=2).to_dict()
    del d["ctc_weight"], d["ctc_pool"]
    c = ModelConfig.from_dict(d)
    assert (c.ctc_weight, c.ctc_pool) == (0.0, 1) and (ModelConfig().ctc_weight, ModelConfig().ctc_pool) == (0.0, 1)


def test_the_head_exists_only_with_a_weight():
    m = make(small(ctc_weight=0.3, ctc_pool=2))
    assert (m.ctc_weight, m.ctc_pool) == (0.3, 2)
    assert tuple(m.ctc_head.weight.shape) == (V, 128) and tuple(m.ctc_head.bias.shape) == (V,)
    keys = list(m.state_dict().keys())
    assert keys[-2:] == ["ctc_head.weight", "ctc_head.bias"]                   # behind the decoder: the decoder-side range stays contiguous
    plain = make(small())
    assert make(None).ctc_weight == 0.0 and plain.ctc_weight == 0.0 and not hasattr(plain, "ctc_head")
    assert list(plain.state_dict().keys()) == keys[:-2] and not any("ctc" in k for k in plain.state_dict())
    with pytest.raises(ValueError):
        plain.predict_ctc([torch.zeros(1, 1, 32, 64)])
    with pytest.raises(ValueError):
        plain.evaluate_ctc([])


@pytest.mark.parametrize("kw", [dict(ctc_weight=-0.1), dict(ctc_weight=1.5), dict(ctc_weight=float("nan")), dict(ctc_weight="0.3"),
                                dict(ctc_pool=0), dict(ctc_pool=-2), dict(ctc_pool=1.5), dict(ctc_pool=True)])
def test_out_of_range_is_a_value_error_at_construction(kw):
    with pytest.raises(ValueError):
        small(**kw)
    with pytest.raises(ValueError):
        make(dict(small().to_dict(), **kw))


def test_the_multimodal_model_and_distillation_refuse_it():
    from omr_a2s_multimodal_transformer_amd.model import MultimodalTransformer
    w2i, i2w = syn.make_vocab(V)
    with pytest.raises(ValueError):
        MultimodalTransformer(32, 64, 32, 64, 16, w2i, i2w, config=small(ctc_weight=0.3))
    MultimodalTransformer(32, 64, 32, 64, 16, w2i, i2w, config=small())
    with pytest.raises(ValueError):
        make(small(ctc_weight=0.3)).set_distillation(object())


def test_checkpoint_round_trip_keeps_the_head_and_an_old_checkpoint_loads_without(tmp_path):
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    m = make(small(ctc_weight=0.3, ctc_pool=2))
    p = str(tmp_path / "m.ckpt")
    m.save_checkpoint(p)
    m2 = Transformer.load_from_checkpoint(p)
    assert (m2.config.ctc_weight, m2.config.ctc_pool) == (0.3, 2)
    assert torch.equal(m2.ctc_head.weight.detach().cpu(), m.ctc_head.weight.detach().cpu())
    plain = make(small())
    q = str(tmp_path / "plain.ckpt")
    plain.save_checkpoint(q)
    ck = torch.load(q, map_location="cpu", weights_only=True)
    del ck["hyper_parameters"]["config"]["ctc_weight"], ck["hyper_parameters"]["config"]["ctc_pool"]      # as written before the fields existed
    old = str(tmp_path / "old.ckpt")
    torch.save(ck, old)
    m3 = Transformer.load_from_checkpoint(old)
    assert (m3.config.ctc_weight, m3.config.ctc_pool) == (0.0, 1) and not hasattr(m3, "ctc_head") and m3.config.d_model == 128
