"""N>1 path on CPU: world_size-2 gloo processes exercise the flat-bucket gradient reducer, the backward-triggered
bucket boundary and the DistributedSampler-equivalent sharding (no HIP kernels involved: pure host logic)."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from omr_a2s_multimodal_transformer_amd.ddp import GradBoundary, GradReducer, shard_indices
from omr_a2s_multimodal_transformer_amd.params import FlatParams


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.enc = nn.Linear(5, 7)
        self.dec = nn.Linear(7, 3)
        self.conv = nn.Conv2d(2, 4, 3)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    m = Tiny()
    flat = FlatParams(list(m.named_parameters()), torch.device("cpu"), torch.float32)
    # parameters are views of the flat buffer and keep their logical shapes; conv weights are stored channels-last
    assert m.conv.weight.shape == (4, 2, 3, 3) and m.conv.weight.omr_phys.shape == (4, 3, 3, 2)
    assert m.conv.weight.data_ptr() == m.conv.weight.omr_phys.data_ptr()
    enc_b, dec_b = flat.slice_of(["enc.weight", "enc.bias"]), flat.slice_of(["dec.weight", "dec.bias", "conv.weight", "conv.bias"])
    red = GradReducer(flat, None, [enc_b, dec_b])
    assert red.grad_scale == 1.0 / world

    # 1) plain finish(): every bucket summed over ranks
    flat.grad.fill_(float(rank + 1))
    red.finish()
    assert torch.allclose(flat.grad, torch.full_like(flat.grad, float(sum(range(1, world + 1)))))
    assert torch.equal(m.enc.weight.grad, flat.grad[: 35].view(7, 5))

    # 2) boundary fired from backward reduces ONLY its bucket; finish() does the rest exactly once
    flat.grad.fill_(float(rank + 1))
    x = torch.ones(2, requires_grad=True)
    y = GradBoundary.apply(red, (1,), x * 2.0)
    y.sum().backward()
    for h in red.handles:
        h.wait()
    total = float(sum(range(1, world + 1)))
    assert torch.allclose(flat.grad[dec_b[0]:dec_b[1]], torch.full((dec_b[1] - dec_b[0],), total))
    assert torch.allclose(flat.grad[enc_b[0]:enc_b[1]], torch.full((enc_b[1] - enc_b[0],), float(rank + 1)))
    red.finish()
    assert torch.allclose(flat.grad, torch.full_like(flat.grad, total))

    # 3) an "unused" bucket (all zeros on every rank) reduces to zeros: no negotiation, no hang
    flat.zero_grad()
    flat.grad[dec_b[0]:dec_b[1]].fill_(1.0)
    red.finish()
    assert float(flat.grad[enc_b[0]:enc_b[1]].abs().sum()) == 0.0
    dist.barrier()
    dist.destroy_process_group()
    q.put(rank)


def test_grad_reducer_world2_gloo():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert sorted(q.get() for _ in range(world)) == [0, 1]


def test_shard_indices_matches_distributed_sampler():
    from torch.utils.data.distributed import DistributedSampler
    data = list(range(23))
    for world in (2, 8):
        for epoch in (0, 3):
            got = [shard_indices(len(data), r, world, epoch=epoch, shuffle=True, seed=0) for r in range(world)]
            for r in range(world):
                s = DistributedSampler(data, num_replicas=world, rank=r, shuffle=True, seed=0)
                s.set_epoch(epoch)
                assert list(s) == got[r]
            assert sorted(set(sum(got, []))) == data


# ---------------------------------------------------------------------------------------------------------------------
# The drop-in Trainer under world_size 2 (gloo): rank-0 parameter broadcast, sample sharding (DistributedSampler
# semantics), MEAN gradient in the optimizer step, sharded evaluation with all-reduced metric counts.  The HIP kernels have
# no CPU path, so the toy module below does its arithmetic with torch CPU ops and a plain-SGD optimizer that honours the
# step(grad_scale=...) contract; everything else (FlatParams, GradReducer, GradBoundary, ShardedLoader, Trainer,
# compute_metrics_sharded) is the product's own host code.

N_TRAIN, N_VAL, BS, EPOCHS, LR = 13, 7, 2, 2, 0.1


def _toy_classes():
    from omr_a2s_multimodal_transformer_amd.lightning_shim import LightningModule
    from omr_a2s_multimodal_transformer_amd.metrics import compute_metrics, compute_metrics_sharded
    from omr_a2s_multimodal_transformer_amd.model import _Base
    from omr_a2s_multimodal_transformer_amd.runtime import FlatModuleMixin

    class FlatSGD:
        def __init__(self, flat):
            self.flat = flat

        def zero_grad(self, set_to_none=False):
            self.flat.grad.zero_()

        def step(self, grad_scale=1.0):
            self.flat.master.sub_(LR * grad_scale * self.flat.grad)

    class Toy(FlatModuleMixin, LightningModule):
        attach_reducer = _Base.attach_reducer
        _boundary = _Base._boundary
        _reducer = None

        def __init__(self, seed):
            super().__init__()
            torch.manual_seed(seed)
            self.encoder = nn.Linear(5, 7)
            self.decoder = nn.Linear(7, 3)
            self.Y, self.YHat = [], []

        def configure_optimizers(self):
            return FlatSGD(self.ensure_flat())

        def training_step(self, batch, i):
            x, y = batch
            return ((self.decoder(self._boundary(torch.tanh(self.encoder(x)))) - y) ** 2).mean()

        def validation_step(self, batch, i):
            x, y = batch
            self.Y.append([str(int(v)) for v in y])
            self.YHat.append([str(int(v)) for v in x])

        def on_validation_epoch_end(self, name="val"):
            m = compute_metrics_sharded(self.Y, self.YHat) if self._reducer is not None else compute_metrics(self.Y, self.YHat)
            self.Y.clear(); self.YHat.clear()
            return m

    return Toy


def _toy_data():
    g = torch.Generator().manual_seed(5)
    train = [(torch.randn(5, generator=g), torch.randn(3, generator=g)) for _ in range(N_TRAIN)]
    val = [(torch.randint(0, 4, (6,), generator=g), torch.randint(0, 4, (5,), generator=g)) for _ in range(N_VAL)]
    return train, val


def _collate(items):
    return torch.stack([a for a, _ in items]), torch.stack([b for _, b in items])


def _trainer_worker(rank, world, port, q):
    from omr_a2s_multimodal_transformer_amd.ddp import ShardedLoader
    from omr_a2s_multimodal_transformer_amd.lightning_shim import Trainer
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    Toy = _toy_classes()
    m = Toy(seed=100 + rank)                   # ranks start from DIFFERENT parameters: the reducer must broadcast rank 0's
    m.flatten_parameters(device="cpu")
    train, val = _toy_data()
    tr = Trainer(max_epochs=EPOCHS, check_val_every_n_epoch=1)
    tr.fit(m, ShardedLoader(train, BS, _collate, shuffle=True, seed=3), val)
    assert m._reducer is not None and tr.reducer is m._reducer
    q.put((rank, m._flat.master.clone().numpy(), dict(tr.callback_metrics)))
    dist.barrier()
    dist.destroy_process_group()


def test_trainer_world2_gloo_equals_single_process_mean_gradient_training():
    from omr_a2s_multimodal_transformer_amd.metrics import compute_metrics
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_trainer_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    # single-process emulation: same shards, gradient = mean over ranks of the per-rank mean-loss gradients
    Toy = _toy_classes()
    ref = Toy(seed=100)
    ref.flatten_parameters(device="cpu")
    train, val = _toy_data()
    for epoch in range(EPOCHS):
        shards = [shard_indices(len(train), r, world, epoch=epoch, shuffle=True, seed=3) for r in range(world)]
        for s in range(0, len(shards[0]), BS):
            ref._flat.grad.zero_()
            for r in range(world):
                ref.training_step(_collate([train[j] for j in shards[r][s:s + BS]]), 0).backward()
            ref._flat.master.sub_(LR * (1.0 / world) * ref._flat.grad)
    for rank, master, metrics in got:
        assert torch.allclose(torch.from_numpy(master), ref._flat.master, rtol=1e-5, atol=1e-6), rank
        want = compute_metrics([[str(int(v)) for v in y] for _, y in val], [[str(int(v)) for v in x] for x, _ in val])
        assert metrics == {f"val_{k}": v for k, v in want.items()}, (rank, metrics, want)
    assert (got[0][1] == got[1][1]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# Modality drop under data parallelism (model.py:510-519,561-575): the ranks seed Python's `random` DIFFERENTLY and must
# still drop the same modality in every step -- the all-reduced buckets carry every rank's gradients, so FusedAdam has to
# skip the same sub-modules everywhere.  The toy borrows MultimodalTransformer's own decision code (_draw_modality /
# apply_teacher_forcing_modality), _Base.attach_reducer / _boundary and the real FusedAdam host logic; only the Adam kernel
# launch is replaced by the same arithmetic in torch (there is no CPU kernel path).

MM_STEPS = 12


def _cpu_adam_step(p, g, m, v, step, lr, betas, eps, grad_scale, p_lowp=None, *, weight_decay=0.0, decay_blocks=None, ema=None,
                   ema_decay=0.0, ctl=None):
    assert weight_decay == 0 and decay_blocks is None and ema is None and ema_decay == 0 and ctl is None      # plain Adam is all this stands in for
    b1, b2 = betas
    g = g * grad_scale
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    p.sub_((lr / (1 - b1 ** step)) * m / ((v / (1 - b2 ** step)).sqrt() + eps))


def _mm_toy_class():
    from omr_a2s_multimodal_transformer_amd.lightning_shim import LightningModule
    from omr_a2s_multimodal_transformer_amd.model import MultimodalTransformer, _Base
    from omr_a2s_multimodal_transformer_amd.runtime import FlatModuleMixin

    class MMToy(FlatModuleMixin, LightningModule):
        attach_reducer = _Base.attach_reducer
        _boundary = _Base._boundary
        _reducer = None
        _touched = None
        _draw_modality = MultimodalTransformer._draw_modality
        apply_teacher_forcing_modality = MultimodalTransformer.apply_teacher_forcing_modality
        teacher_forcing_modality_prob = 0.6

        def __init__(self, seed):
            super().__init__()
            torch.manual_seed(seed)
            self.image_encoder = nn.Linear(5, 7)
            self.audio_encoder = nn.Linear(4, 7)
            self.decoder = nn.Linear(7, 3)
            self.drawn = []

        def training_step(self, batch, i):
            xi, xa, y = batch
            mi, ma = self._boundary(torch.tanh(self.image_encoder(xi)), torch.tanh(self.audio_encoder(xa)))
            modality = self._draw_modality()
            self.drawn.append(modality)
            self._touched = {"image": ("image_encoder", "decoder"), "audio": ("audio_encoder", "decoder"), "both": None}[modality]
            mem = mi if modality == "image" else ma if modality == "audio" else mi + ma
            return ((self.decoder(mem) - y) ** 2).mean()

    return MMToy


def _mm_worker(rank, world, port, q):
    import random
    from omr_a2s_multimodal_transformer_amd import kernels as K
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    K.adam_step = _cpu_adam_step
    random.seed(1000 + 17 * rank)              # different Python streams on purpose
    m = _mm_toy_class()(seed=50 + rank)
    m.flatten_parameters(device="cpu")
    opt = m.configure_optimizers() if hasattr(m, "configure_optimizers") else m.make_optimizer(lr=1e-2)
    red = m.attach_reducer()
    g = torch.Generator().manual_seed(7 + rank)
    local_draws = []
    for i in range(MM_STEPS):
        st = random.getstate()
        local_draws.append(m.apply_teacher_forcing_modality())      # what this rank's own stream would have decided
        random.setstate(st)
        batch = (torch.randn(2, 5, generator=g), torch.randn(2, 4, generator=g), torch.randn(2, 3, generator=g))
        opt.zero_grad()
        m.training_step(batch, i).backward()
        red.finish()
        opt.step(grad_scale=red.grad_scale)
    q.put((rank, m.drawn, local_draws, m._flat.master.clone().numpy(), m._flat.exp_avg.clone().numpy(), m._flat.exp_avg_sq.clone().numpy(),
           dict(opt.steps)))
    dist.barrier()
    dist.destroy_process_group()


def test_modality_drop_world2_ranks_seeded_differently_stay_identical():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_mm_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    (_, d0, l0, p0, m0, v0, s0), (_, d1, l1, p1, m1, v1, s1) = got
    assert l0 != l1, "the test is vacuous unless the ranks' own streams disagree somewhere"
    assert d0 == d1 and len(set(d0)) == 3, d0          # same decision everywhere; all three branches seen
    assert s0 == s1 and s0["decoder"] == MM_STEPS and s0["image_encoder"] < MM_STEPS and s0["audio_encoder"] < MM_STEPS
    assert (p0 == p1).all() and (m0 == m1).all() and (v0 == v1).all()
