"""Knowledge distillation of a unimodal `Transformer` (an extension: the reference trains from hard labels alone).

A `Distillation` names the teachers, the `DistillConfig` and how a training batch is shared between the student and the teachers;
`Transformer.set_distillation(d)` attaches it and `set_distillation(None)` detaches it.  The teachers are NOT sub-modules of the
student: they stay out of `parameters()`, `state_dict()`, checkpoints, the flat parameter store and the DDP reducer, are put in `eval()`
and run under `no_grad`.  The loss is functional.cross_entropy_distill: (1 - weight) nll + weight tau^2 KL(q || softmax(student / tau)),
q = alpha softmax(a / tau) + (1 - alpha) softmax(b / tau) -- with two teachers the distribution the weighted late fusion decodes from.

Two recipes, told apart by `student_input`:
  same input (student_input = None)     batch (x, xl, y_in, y_out); one or two teachers read the same (x, xl).
  cross-modal ("image" or "audio")      batch (xi, xli, xa, xla, y_in, y_out) (image.collate_ragged_pairs or the multimodal collate); the
                                        student reads the half named; the teachers are a pair (image Transformer, audio Transformer), each
                                        on its own half, or one MultimodalTransformer on both halves.
Lengths pass through unchanged, so the ragged [B, 2] forms work as they do without a distillation.  With one set of teacher logits alpha is
taken as 1.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from .config import DistillConfig

STUDENT_INPUTS = ("image", "audio")


class Distillation:
    def __init__(self, teachers, config: Optional[DistillConfig] = None, student_input: Optional[str] = None) -> None:
        if isinstance(config, dict):
            config = DistillConfig.from_dict(config)
        self.config = config if config is not None else DistillConfig()
        if student_input is not None and student_input not in STUDENT_INPUTS:
            raise ValueError(f"student_input must be None or one of {STUDENT_INPUTS}, got {student_input!r}")
        self.student_input = student_input
        self.teachers: Tuple = tuple(teachers) if isinstance(teachers, (list, tuple)) else (teachers,)
        if len(self.teachers) not in (1, 2):
            raise ValueError(f"a distillation takes one or two teachers, got {len(self.teachers)}")
        for t in self.teachers:
            t.eval()
        self.loss = None             # model.DistillationLoss, made when a student attaches

    @property
    def alpha(self) -> float:
        return self.config.alpha if len(self.teachers) == 2 else 1.0

    def attach(self, student) -> None:
        """Checks the student against the teachers and makes the loss module (Transformer.set_distillation)."""
        from .model import DistillationLoss
        if getattr(student.config, "label_smoothing", 0.0) > 0:
            raise ValueError("label_smoothing > 0 together with a distillation is not supported")
        for i, t in enumerate(self.teachers):
            if t is student:
                raise ValueError("a model cannot be its own teacher")
            if dict(t.w2i) != dict(student.w2i):
                raise ValueError(f"teacher {i} has another vocabulary than the student: distillation compares logits token by token")
        self.loss = DistillationLoss(ignore_index=student.padding_idx, config=self.config)

    def split(self, batch: Sequence):
        """batch -> ((x, xl) of the student, y_in, y_out, [(teacher, its positional inputs)])."""
        if self.student_input is None:
            if len(batch) != 4:
                raise ValueError(f"a same-input distillation takes batches (x, xl, y_in, y_out), got {len(batch)} items")
            x, xl, y_in, y_out = batch
            return (x, xl), y_in, y_out, [(t, (x, xl)) for t in self.teachers]
        if len(batch) != 6:
            raise ValueError(f"a cross-modal distillation takes batches (xi, xli, xa, xla, y_in, y_out), got {len(batch)} items")
        xi, xli, xa, xla, y_in, y_out = batch
        own = (xi, xli) if self.student_input == "image" else (xa, xla)
        if len(self.teachers) == 2:
            calls = [(self.teachers[0], (xi, xli)), (self.teachers[1], (xa, xla))]
        else:
            calls = [(self.teachers[0], (xi, xli, xa, xla))]
        return own, y_in, y_out, calls

    def teacher_logits(self, calls, y_in) -> List[torch.Tensor]:
        """Every teacher on its inputs and the student's (already noised) y_in, in eval() and without a graph."""
        out = []
        with torch.no_grad():
            for t, args in calls:
                if t.training:
                    t.eval()
                out.append(t(*args, y_in).detach())
        return out
