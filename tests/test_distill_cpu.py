"""DistillConfig and the batch routing of distill.Distillation, without a GPU: stub teachers record what they are called with."""
import json

import pytest
import torch

from omr_a2s_multimodal_transformer_amd.config import DistillConfig
from omr_a2s_multimodal_transformer_amd.distill import Distillation


def test_defaults_and_round_trip():
    c = DistillConfig()
    assert (c.weight, c.temperature, c.alpha) == (0.5, 2.0, 0.5)
    full = DistillConfig(weight=1, temperature=4, alpha=0)
    assert all(isinstance(v, float) for v in full.to_dict().values())
    d = json.loads(json.dumps(full.to_dict()))
    assert DistillConfig.from_dict(dict(d, unknown_key=1)) == full
    assert DistillConfig.from_dict(c.to_dict()) == c
    assert Distillation(Stub(), full.to_dict()).config == full


@pytest.mark.parametrize("bad", [dict(weight=-0.1), dict(weight=1.1), dict(weight=float("nan")), dict(temperature=0.0), dict(temperature=-2.0),
                                 dict(temperature=float("inf")), dict(temperature=float("nan")), dict(alpha=-0.1), dict(alpha=1.5),
                                 dict(alpha=float("nan")), dict(weight="0.5"), dict(alpha=None), dict(temperature=True)])
def test_bad_values_are_refused(bad):
    with pytest.raises(ValueError):
        DistillConfig(**bad)


class Stub:
    """A teacher as far as Distillation is concerned: a vocabulary, eval() and a call that returns logits."""

    def __init__(self, w2i=None, tag=0.0):
        self.w2i = w2i if w2i is not None else {"<PAD>": 0, "a": 1}
        self.training = True
        self.calls = []
        self.tag = tag

    def eval(self):
        self.training = False
        return self

    def __call__(self, *args):
        assert not torch.is_grad_enabled(), "teachers run under no_grad"
        self.calls.append(args)
        return torch.full((1, 2, 3), self.tag, requires_grad=True)


class Student:
    def __init__(self, w2i=None, label_smoothing=0.0):
        self.w2i = w2i if w2i is not None else {"<PAD>": 0, "a": 1}
        self.padding_idx = 0
        self.config = type("C", (), {"label_smoothing": label_smoothing})()


X, XL, XI, XLI, XA, XLA, Y_IN, Y_OUT = (object() for _ in range(8))


def test_teachers_are_put_in_eval():
    a, b = Stub(), Stub()
    Distillation([a, b])
    assert not a.training and not b.training


@pytest.mark.parametrize("n", [1, 2])
def test_same_input_routing(n):
    ts = [Stub(tag=float(i)) for i in range(n)]
    d = Distillation(ts, DistillConfig(alpha=0.3))
    assert d.alpha == (0.3 if n == 2 else 1.0)
    own, y_in, y_out, calls = d.split((X, XL, Y_IN, Y_OUT))
    assert own == (X, XL) and y_in is Y_IN and y_out is Y_OUT
    assert [(t, args) for t, args in calls] == [(t, (X, XL)) for t in ts]
    noised = object()
    ts[0].training = True                                    # someone called train() on it: put back before it runs
    out = d.teacher_logits(calls, noised)
    assert [t.calls for t in ts] == [[(X, XL, noised)]] * n and not ts[0].training
    assert [float(o[0, 0, 0]) for o in out] == [float(i) for i in range(n)] and not any(o.requires_grad for o in out)
    with pytest.raises(ValueError):
        d.split((XI, XLI, XA, XLA, Y_IN, Y_OUT))


@pytest.mark.parametrize("student_input", ["image", "audio"])
def test_cross_modal_pair_routing(student_input):
    ti, ta = Stub(), Stub()
    d = Distillation((ti, ta), student_input=student_input)
    own, y_in, y_out, calls = d.split((XI, XLI, XA, XLA, Y_IN, Y_OUT))
    assert own == ((XI, XLI) if student_input == "image" else (XA, XLA)) and y_in is Y_IN and y_out is Y_OUT
    assert calls == [(ti, (XI, XLI)), (ta, (XA, XLA))] and d.alpha == 0.5
    with pytest.raises(ValueError):
        d.split((X, XL, Y_IN, Y_OUT))


def test_cross_modal_multimodal_routing():
    t = Stub()
    d = Distillation(t, student_input="audio")
    own, _, _, calls = d.split((XI, XLI, XA, XLA, Y_IN, Y_OUT))
    assert own == (XA, XLA) and calls == [(t, (XI, XLI, XA, XLA))] and d.alpha == 1.0


def test_construction_and_attachment_refusals():
    with pytest.raises(ValueError):
        Distillation([])
    with pytest.raises(ValueError):
        Distillation([Stub(), Stub(), Stub()])
    with pytest.raises(ValueError):
        Distillation(Stub(), student_input="both")
    with pytest.raises(ValueError, match="vocabulary"):
        Distillation(Stub(w2i={"<PAD>": 0, "b": 1})).attach(Student())
    with pytest.raises(ValueError, match="label_smoothing"):
        Distillation(Stub()).attach(Student(label_smoothing=0.1))
    d = Distillation(Stub(), DistillConfig(weight=0.25))
    d.attach(Student())
    assert d.loss.config.weight == 0.25 and d.loss.ignore_index == 0 and d.loss.last_nll is None and d.loss.last_kd is None
