"""Distillation through the model: Transformer.set_distillation + training_step with one or two teachers on the same input, and cross-modal
with a pair (image Transformer, audio Transformer) or one MultimodalTransformer as the teacher.  Tiny fp32 models (d_model 128, two decoder
layers, 64 tokens, T = 12, dropout 0) on a batch of two: images 32 x 64, spectrograms 195 x 32, targets of 11 and 7 tokens."""
import functools
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

import multimodal_ragged_refs as M  # noqa: E402
from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import DistillConfig, ModelConfig  # noqa: E402
from oracle import kernel_refs as KR  # noqa: E402

DEV = "cuda:0"
V, T, D, LAYERS, B = 64, 12, 128, 2, 2
IMG, AUD = (32, 64), (195, 32)
TARGET_LENS = (11, 7)
PAD = 0
CFG = DistillConfig(weight=0.5, temperature=2.0, alpha=0.3)
LOSS_RTOL = 1e-4                                   # the project's model-level bound on a loss


def _config(**kw):
    return ModelConfig(d_model=D, ff_dim=D, num_layers=LAYERS, dropout=0.0, encoder_dropout=0.0, compute_dtype="fp32", **kw)


def transformer(plane, seed, vocab=V, **kw):
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    w2i, i2w = syn.make_vocab(vocab)
    m = Transformer(plane[0], plane[1], T + 4, w2i, i2w, config=_config(**kw))
    m.load_state_dict(syn.seeded_state_dict(syn.transformer_shapes(vocab, D, D, LAYERS), seed), strict=False)
    m.flatten_parameters()
    m.teacher_forcing_prob = 0.0
    m.eval()                                       # gradients stay enabled; no dropout anywhere (the config has none either)
    return m


def multimodal(seed):
    from omr_a2s_multimodal_transformer_amd.model import MultimodalTransformer
    w2i, i2w = syn.make_vocab(V)
    m = MultimodalTransformer(IMG[0], IMG[1], AUD[0], AUD[1], T + 4, w2i, i2w, mixer_type="concat", config=_config())
    m.load_state_dict(syn.seeded_state_dict(syn.multimodal_shapes(V, "concat", D, D, LAYERS), seed), strict=False)
    m.flatten_parameters()
    m.teacher_forcing_prob = 0.0
    m.eval()
    return m


@functools.lru_cache(maxsize=None)
def data():
    w2i, _ = syn.make_vocab(V)
    assert w2i["<PAD>"] == PAD
    xi = KR.rnd((B, 1) + IMG, 701).to(DEV)
    xa = KR.rnd((B, 1) + AUD, 702).to(DEV)
    y_in, y_out, counts = M.make_targets(w2i, TARGET_LENS, V, T)
    return xi, xa, y_in, y_out, counts


def ref64(student_bvt, teachers_bvt, y_out, cfg, alpha):
    """(loss, nll, kd) of the definition in fp64 (torch ops on the CPU) on the logits given."""
    F = torch.nn.functional
    rows = lambda t: t.detach().double().cpu().permute(0, 2, 1).reshape(-1, t.shape[1])  # noqa: E731
    x, tgt = rows(student_bvt), y_out.reshape(-1).cpu()
    live = tgt != PAD
    tau = cfg.temperature
    q = F.softmax(rows(teachers_bvt[0]) / tau, 1)
    if len(teachers_bvt) == 2:
        q = alpha * q + (1 - alpha) * F.softmax(rows(teachers_bvt[1]) / tau, 1)
    nll = F.cross_entropy(x, tgt, ignore_index=PAD)
    kd = tau * tau * F.kl_div(F.log_softmax(x / tau, 1)[live], q[live], reduction="sum") / int(live.sum())
    return float((1 - cfg.weight) * nll + cfg.weight * kd), float(nll), float(kd)


def rel(a, b):
    return abs(a - b) / abs(b)


def no_gradient_reached(t):
    """A flattened model's parameters carry views of its zero-initialised flat gradient buffer as .grad: no .grad, or one that is all zeros."""
    return all(p.grad is None or not bool(p.grad.any()) for p in t.parameters())


def step_and_check(student, distillation, batch, student_args, teacher_calls, alpha):
    """One training_step; the logged loss, nll and kd against ref64 on the logits `forward` returns for the same inputs."""
    from omr_a2s_multimodal_transformer_amd.runtime import WgradStream
    student.set_distillation(distillation)
    try:
        student.zero_grad()
        student.logged_metrics.clear()
        loss = student.training_step(batch, 0)
        loss.backward()
        WgradStream.join()
        torch.cuda.synchronize()
        logged = {k: float(student.logged_metrics[k].detach()) for k in ("train_loss", "train_nll", "train_kd")}
        assert student.logged_metrics["train_loss"] is loss
        assert student.logged_metrics["train_nll"] is distillation.loss.last_nll and student.logged_metrics["train_kd"] is distillation.loss.last_kd
        assert not distillation.loss.last_nll.requires_grad and not distillation.loss.last_kd.requires_grad
        y_in, y_out = batch[-2], batch[-1]
        with torch.no_grad():
            s = student(*student_args, y_in)
            ts = [t(*args, y_in) for t, args in teacher_calls]
        want = ref64(s, ts, y_out, distillation.config, alpha)
        print(f"logged {logged} vs fp64 (loss, nll, kd) {want}")
        assert rel(logged["train_loss"], want[0]) <= LOSS_RTOL and rel(logged["train_nll"], want[1]) <= LOSS_RTOL
        assert abs(logged["train_kd"] - want[2]) <= LOSS_RTOL * max(abs(want[2]), abs(want[1]))
        assert want[2] > 1e-3, "the teachers must differ from the student for this check to see the kd term"
        g = student._flat.grad
        assert g is not None and torch.isfinite(g).all() and float(g.double().norm()) > 0.0
        for t, _ in teacher_calls:
            assert not t.training and no_gradient_reached(t)
        return logged
    finally:
        student.set_distillation(None)


@pytest.mark.parametrize("n_teachers", [1, 2])
def test_same_input_distillation_matches_the_fp64_reference(n_teachers):
    from omr_a2s_multimodal_transformer_amd.distill import Distillation
    xi, _, y_in, y_out, _ = data()
    student = transformer(IMG, 31)
    teachers = [transformer(IMG, 32 + i) for i in range(n_teachers)]
    d = Distillation(teachers, CFG)
    assert d.alpha == (CFG.alpha if n_teachers == 2 else 1.0)
    step_and_check(student, d, (xi, None, y_in, y_out), (xi, None), [(t, (xi, None)) for t in teachers], d.alpha)


@pytest.mark.parametrize("student_input", ["image", "audio"])
def test_cross_modal_pair_of_teachers(student_input):
    """The weighted late fusion (image model, audio model) as the teacher of an image-only or an audio-only student."""
    from omr_a2s_multimodal_transformer_amd.distill import Distillation
    xi, xa, y_in, y_out, _ = data()
    own = (xi, None) if student_input == "image" else (xa, None)
    student = transformer(IMG if student_input == "image" else AUD, 41)
    ti, ta = transformer(IMG, 42), transformer(AUD, 43)
    d = Distillation((ti, ta), CFG, student_input=student_input)
    step_and_check(student, d, (xi, None, xa, None, y_in, y_out), own, [(ti, (xi, None)), (ta, (xa, None))], CFG.alpha)


def test_cross_modal_multimodal_teacher():
    from omr_a2s_multimodal_transformer_amd.distill import Distillation
    xi, xa, y_in, y_out, _ = data()
    student, teacher = transformer(IMG, 51), multimodal(52)
    d = Distillation(teacher, CFG, student_input="image")
    assert d.alpha == 1.0
    step_and_check(student, d, (xi, None, xa, None, y_in, y_out), (xi, None), [(teacher, (xi, None, xa, None))], 1.0)


def test_teachers_stay_out_of_the_student_and_unchanged_by_its_optimizer():
    from omr_a2s_multimodal_transformer_amd.distill import Distillation
    from omr_a2s_multimodal_transformer_amd.runtime import WgradStream
    xi, _, y_in, y_out, _ = data()
    student, teacher = transformer(IMG, 61), transformer(IMG, 62)
    names, n_params, flat_size = list(student.state_dict()), len(list(student.parameters())), student._flat.master.numel()
    before_t = {k: v.detach().clone() for k, v in teacher.state_dict().items()}
    flat_t = teacher._flat.master.detach().clone()
    start = student._flat.master.detach().clone()
    student.set_distillation(Distillation(teacher, CFG))
    opt = student.make_optimizer(lr=1e-2)
    assert list(student.state_dict()) == names and len(list(student.parameters())) == n_params and student._flat.master.numel() == flat_size
    assert all(m is not teacher for m in student.modules())
    ids = {id(p) for p in student.parameters()}
    assert not any(id(p) in ids for p in teacher.parameters())
    random.seed(0)
    opt.zero_grad()
    student.training_step((xi, None, y_in, y_out), 0).backward()
    WgradStream.join()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(student._flat.master, start), "the student did not move"
    assert no_gradient_reached(teacher)
    KR.assert_bit_equal(teacher._flat.master, flat_t.cpu(), "teacher's flat parameters")
    for k, v in teacher.state_dict().items():
        KR.assert_bit_equal(v, before_t[k].cpu(), k)
    student.set_distillation(None)


def test_a_copy_of_the_single_teacher_has_kd_0():
    from omr_a2s_multimodal_transformer_amd.distill import Distillation
    xi, _, y_in, y_out, _ = data()
    student, teacher = transformer(IMG, 71), transformer(IMG, 71)
    student.set_distillation(Distillation(teacher, CFG))
    student.logged_metrics.clear()
    student.training_step((xi, None, y_in, y_out), 0)
    kd, nll = float(student.logged_metrics["train_kd"]), float(student.logged_metrics["train_nll"])
    print(f"kd {kd!r} at nll {nll!r}")
    # equal models give equal logits bit for bit, and the kernel's two row constants then come from the same arithmetic
    assert abs(kd) <= 1e-6 * nll
    student.set_distillation(None)


def test_detaching_restores_the_plain_steps_loss_bits():
    from omr_a2s_multimodal_transformer_amd.distill import Distillation
    xi, _, y_in, y_out, _ = data()
    student, teacher = transformer(IMG, 81), transformer(IMG, 82)
    batch = (xi, None, y_in, y_out)
    plain = student.training_step(batch, 0).detach().clone()
    student.set_distillation(Distillation(teacher, CFG))
    distilled = student.training_step(batch, 0).detach().clone()
    student.set_distillation(None)
    student.logged_metrics.clear()
    again = student.training_step(batch, 0).detach()
    assert float(distilled) != float(plain)
    KR.assert_bit_equal(again.view(1), plain.view(1).cpu(), "plain loss after detaching")
    assert "train_kd" not in student.logged_metrics and "train_nll" not in student.logged_metrics


def test_vocabulary_mismatch_and_label_smoothing_raise():
    from omr_a2s_multimodal_transformer_amd.distill import Distillation
    student = transformer(IMG, 91)
    with pytest.raises(ValueError, match="vocabulary"):
        student.set_distillation(Distillation(transformer(IMG, 92, vocab=V + 1), CFG))
    assert student._distillation is None
    smoothing = transformer(IMG, 93, label_smoothing=0.1)
    with pytest.raises(ValueError, match="label_smoothing"):
        smoothing.set_distillation(Distillation(transformer(IMG, 94), CFG))


def test_ragged_batch_runs():
    """Per-sample pixel sizes [B, 2] pass through to the student and the teachers unchanged."""
    from omr_a2s_multimodal_transformer_amd.distill import Distillation
    xi, xa, y_in, y_out, _ = data()
    si = torch.tensor([[32, 64], [20, 40]], dtype=torch.int64)
    sa = torch.tensor([[195, 32], [100, 24]], dtype=torch.int64)
    student, ti, ta = transformer(IMG, 101), transformer(IMG, 102), transformer(AUD, 103)
    d = Distillation((ti, ta), CFG, student_input="image")
    step_and_check(student, d, (xi, si, xa, sa, y_in, y_out), (xi, si), [(ti, (xi, si)), (ta, (xa, sa))], CFG.alpha)
