"""The guarded optimizer step behind the data-parallel path, with RCCL in the loop: a one-rank "nccl" group and a reducer told it
has two ranks (as tests/test_rccl_single_rank_gpu.py sets it up), one step through Trainer.fit with the reducer attached and the
guard on.  grad_scale = 1/2 has to reach BOTH kernels of the guarded step: the result must be, bit for bit, the plain guarded
step (no reducer) on the same gradient bits with grad_scale = 0.5."""
import random

import pytest
import torch
import torch.distributed as dist

pytestmark = pytest.mark.gpu

from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402
from omr_a2s_multimodal_transformer_amd.lightning_shim import Trainer  # noqa: E402
from test_model_gpu import DEV, NO_DROP, make_transformer  # noqa: E402

V = 50
CLIP = 1e-2


@pytest.fixture()
def one_rank_group():
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29733", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        yield
    finally:
        dist.destroy_process_group()


def _model():
    m, w2i = make_transformer(V, ModelConfig(num_layers=2, compute_dtype="bf16", **NO_DROP), 47, hw=(64, 96), max_seq=16)
    m.train()
    m.teacher_forcing_prob = 0.0
    return m, w2i


def _bits(t):
    return t.detach().cpu().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def test_guarded_step_under_a_reducer_equals_the_plain_guarded_step(one_rank_group):
    m, w2i = _model()
    batch = syn.synthetic_unimodal_batch(3, 64, 96, 12, V, w2i["<sos>"], w2i["<eos>"], seed=8)
    start = m._flat.master.clone()
    red = m.attach_reducer()
    assert red.world == 1
    red.world = 2                          # pretend: the collective still runs over the one real rank
    random.seed(0)
    trainer = Trainer(max_epochs=1, reducer=red, gradient_clip_val=CLIP, skip_nonfinite=True)
    trainer.fit(m, [batch])
    torch.cuda.synchronize()
    grad = m._flat.grad.clone()            # the all-reduced SUM the step saw (nothing touches it after the step)
    assert trainer.callback_metrics["skipped_steps"] == 0 and not torch.equal(m._flat.master, start)
    norm = m.logged_metrics["grad_norm"]
    want = 0.5 * float(grad.double().norm())
    assert abs(norm - want) <= 1e-5 * want                  # the norm of the MEAN gradient: 1/world reached omr_grad_norm

    plain, _ = _model()
    assert torch.equal(plain._flat.master, start)
    opt = plain.configure_optimizers()
    opt.enable_guard(max_norm=CLIP)
    plain._flat.grad.copy_(grad)
    opt.step(grad_scale=0.5)
    assert opt.last_grad_norm == norm and opt.skipped == 0
    for name in ("master", "exp_avg", "exp_avg_sq", "lowp"):
        assert torch.equal(_bits(getattr(m._flat, name)), _bits(getattr(plain._flat, name))), name
