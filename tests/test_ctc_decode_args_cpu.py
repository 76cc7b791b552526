"""CPU-only: every refusal of `ctc_decode=` is a ValueError raised before anything is encoded -- the inputs handed in raise AssertionError
the moment they are touched."""
import pytest

from omr_a2s_multimodal_transformer_amd import kernels as K
from omr_a2s_multimodal_transformer_amd import synthetic as syn
from omr_a2s_multimodal_transformer_amd.config import ModelConfig

V = 40


class Untouchable:
    """Stands for a memory or a list of inputs: any use is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"the input was touched ({name}) before the arguments were refused")

    def __iter__(self):
        raise AssertionError("the inputs were iterated before the arguments were refused")


def small(**kw) -> ModelConfig:
    return ModelConfig(d_model=128, ff_dim=128, num_layers=1, **kw)


def transformer(config):
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    w2i, i2w = syn.make_vocab(V)
    return Transformer(32, 64, 16, w2i, i2w, config=config)


def multimodal():
    from omr_a2s_multimodal_transformer_amd.model import MultimodalTransformer
    w2i, i2w = syn.make_vocab(V)
    return MultimodalTransformer(32, 64, 32, 64, 16, w2i, i2w, mixer_type="concat", config=small())


@pytest.fixture(scope="module")
def with_head():
    return transformer(small(ctc_weight=0.3))


def calls(m, **kw):
    """The four entry points with the keywords `kw` on inputs that must not be touched."""
    x = Untouchable()
    beam = kw.pop("beam", 4)
    return [lambda: m.beam_search(x, beam, **kw), lambda: m.beam_search(x, beam=beam, **kw), lambda: m.beam_search_batch(x, beam, **kw),
            lambda: m.predict(x, beam=beam, **kw), lambda: m.evaluate(x, beam=beam, **kw)]


def refused(fns, match):
    for fn in fns:
        with pytest.raises(ValueError, match=match):
            fn()


def test_a_model_without_the_head_is_refused():
    refused(calls(transformer(small()), ctc_decode=0.3), "CTC head")


def test_a_multimodal_model_is_refused():
    refused(calls(multimodal(), ctc_decode=0.3), "Transformer")


@pytest.mark.parametrize("beam", [1, 0, 9, 2.0, True])
def test_a_beam_below_2_is_refused(with_head, beam):
    refused(calls(with_head, ctc_decode=0.3, beam=beam), "beam")


def test_the_default_beam_of_predict_and_evaluate_is_1_and_refused(with_head):
    refused([lambda: with_head.predict(Untouchable(), ctc_decode=0.3), lambda: with_head.evaluate(Untouchable(), ctc_decode=0.3)], "beam")


@pytest.mark.parametrize("lam", [0.0, 1.0, -0.2, 1.5, float("nan"), "0.3", True, 1e-60])
def test_a_weight_outside_0_1_is_refused(with_head, lam):
    refused(calls(with_head, ctc_decode=lam), "ctc_decode")
    with pytest.raises(ValueError, match="ctc_decode"):
        K.check_ctc_decode(lam)


def test_combinations_are_refused(with_head):
    g = object()                                   # any grammar: the combination is refused before the object is looked at
    refused(calls(with_head, ctc_decode=0.3, grammar=g), "grammar")
    x = Untouchable()
    refused([lambda: with_head.predict(x, beam=4, ctc_decode=0.3, refill=True), lambda: with_head.evaluate(x, beam=4, ctc_decode=0.3, refill=True)],
            "refill")
    refused([lambda: with_head.predict(x, beam=4, ctc_decode=0.3, draft=with_head), lambda: with_head.evaluate(x, beam=4, ctc_decode=0.3, draft=with_head)],
            "draft")
    with_head.decode_grammar = g                   # the model's own grammar counts like the keyword
    try:
        refused(calls(with_head, ctc_decode=0.3), "grammar")
    finally:
        with_head.decode_grammar = None


def test_the_late_fusion_calls_are_refused(with_head):
    from omr_a2s_multimodal_transformer_amd.late_fusion import sw_evaluate, sw_predict
    from omr_a2s_multimodal_transformer_amd.weighted_fusion import weighted_evaluate, weighted_predict
    x = Untouchable()
    refused([lambda: sw_predict(x, with_head, with_head, ctc_decode=0.3), lambda: sw_evaluate(x, with_head, with_head, ctc_decode=0.3),
             lambda: weighted_predict(x, with_head, with_head, ctc_decode=0.3), lambda: weighted_evaluate(x, with_head, with_head, ctc_decode=0.3)],
            "ctc_decode")


def test_none_is_the_absent_keyword(with_head):
    """ctc_decode=None goes the parent's way: the call reaches the inputs."""
    with pytest.raises(AssertionError, match="touched|iterated"):
        with_head.predict(Untouchable(), beam=4, ctc_decode=None)


def test_the_mix_weights_are_the_kernels():
    import numpy as np
    wa, wc = K.ctc_mix_weights(0.3)
    assert wc == float(np.float32(0.3)) and wa == float(np.float32(1.0 - float(np.float32(0.3))))
    assert float(np.float32(wa)) == wa and float(np.float32(wc)) == wc
