"""resident.ResidentLoader(augment=..., augment2=...) on the GPU: the samples and the small models of tests/test_resident_loader_gpu.py
(three image / audio pairs in a 64 x 96 and a 35 x 40 plane, targets of 11 / 7 / 4 tokens; 2 decoder layers, d_model 128).  A batch has
to be tests/augment_refs.py applied to the records the loader drew, bit for bit; the draws depend on (seed, epoch, sample) alone; and
the extents handed on are the right ones: each sample's share of a ragged training step's loss is what the sample gives alone, at
batch size 1, on its own augmented plane -- the ragged route's guarantee, with the project's model-level bound on the loss."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_refs as AR  # noqa: E402
import multimodal_ragged_refs as M  # noqa: E402
import test_resident_loader_gpu as L  # noqa: E402
from omr_a2s_multimodal_transformer_amd import augment as A  # noqa: E402
from oracle.kernel_refs import assert_bit_equal  # noqa: E402

DEV = L.DEV
LOSS_RTOL = 1e-4                     # the project's model-level bound on a loss (tests/test_ragged_training_gpu.py)
SEED = 5


def image_augment():
    return A.ImageAugment(scale=(0.8, 1.2), aspect=(0.9, 1.1), rotate_deg=2.0, shear=0.05, gain=(0.8, 1.2), bias=(-20.0, 20.0), noise=8.0, fill=255.0,
                          limit=M.IMG_PLANE)


def spec_augment():
    return A.SpecAugment(time_masks=2, max_time=6, freq_masks=2, max_freq=4, time_stretch=(0.8, 1.2), gain=(0.9, 1.1), fill=0.0, limit=M.AUD_PLANE)


@functools.lru_cache(maxsize=None)
def data():
    """(image samples as uint8 [h, w], audio samples as float32 [h, w], targets, the paired data set, the image-only data set)."""
    ci, ca, _, _, targets = L.samples()
    qi = L.quantised(ci)
    img_u8 = [(c[0, 0] * 255).round().to(torch.uint8) for c in qi]
    aud = [c[0, 0].clone() for c in ca]
    pairs = L.R().ResidentDataset(images=L.store_of(qi, "u8"), audios=L.store_of(ca, "f32"), targets=targets)
    images = L.R().ResidentDataset(images=L.store_of(qi, "u8"), targets=targets)
    return img_u8, aud, targets, pairs, images


def pair_loader(epoch=0, dtype=torch.float32, batch_size=2, **kw):
    loader = L.R().ResidentLoader(data()[3], batch_size, dtype, augment=image_augment(), augment2=spec_augment(), seed=SEED, rank=0, world=1, **kw)
    loader.set_epoch(epoch)
    return loader


def planes_by_sample(loader):
    """{sample: (its image extent's pixels, its audio extent's pixels)} over one pass."""
    out = {}
    for indices, (xi, si, xa, sa, _, _) in zip(loader.plan(), loader):
        for b, n in enumerate(indices):
            out[n] = (xi[b, 0, :si[b, 0], :si[b, 1]].cpu().clone(), xa[b, 0, :sa[b, 0], :sa[b, 1]].cpu().clone())
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_loader_batches_are_the_reference_applied_to_the_records_it_drew(dtype):
    img_u8, aud, targets, _, _ = data()
    loader = pair_loader(epoch=1, dtype=dtype)
    ri, ra = loader.records()
    assert ri.dtype == ra.dtype == A.AUG_DTYPE and ri.shape == ra.shape == (3,)
    for n in range(3):
        assert ri[n].tobytes() == image_augment().draw(SEED, 1, n, *img_u8[n].shape).tobytes()
        assert ra[n].tobytes() == spec_augment().draw(SEED, 1, n, *aud[n].shape).tobytes()
    plan = loader.plan()
    assert sorted(n for b in plan for n in b) == [0, 1, 2] and len(plan) == 2
    batches = list(loader)
    assert len(batches) == len(plan)
    for indices, (xi, si, xa, sa, y_in, y_out) in zip(plan, batches):
        assert xi.is_cuda and xa.is_cuda and xi.dtype == xa.dtype == dtype and not si.is_cuda and si.dtype == sa.dtype == torch.int64
        assert si.tolist() == A.extents(ri[indices]).tolist() and sa.tolist() == A.extents(ra[indices]).tolist()
        assert tuple(xi.shape) == (len(indices), 1, int(si[:, 0].max()), int(si[:, 1].max()))
        assert tuple(xa.shape) == (len(indices), 1, int(sa[:, 0].max()), int(sa[:, 1].max()))
        assert xi.shape[2] <= M.IMG_PLANE[0] and xi.shape[3] <= M.IMG_PLANE[1] and xa.shape[2] <= M.AUD_PLANE[0] and xa.shape[3] <= M.AUD_PLANE[1]
        assert_bit_equal(xi.cpu(), AR.gather_augmented_ref(img_u8, indices, ri[indices], xi.shape[2], xi.shape[3], 0.0, dtype), f"images {indices}")
        assert_bit_equal(xa.cpu(), AR.gather_augmented_ref(aud, indices, ra[indices], xa.shape[2], xa.shape[3], 0.0, dtype), f"audios {indices}")
        T = max(targets[n].numel() for n in indices) - 1
        assert y_in.shape == y_out.shape == (len(indices), T)
        for b, n in enumerate(indices):
            k = targets[n].numel() - 1
            assert torch.equal(y_in[b, :k], targets[n][:-1]) and torch.equal(y_out[b, :k], targets[n][1:])


def test_same_seed_and_epoch_same_batches_and_the_next_epoch_differs():
    first, again, other = planes_by_sample(pair_loader(0)), planes_by_sample(pair_loader(0, batch_size=3)), planes_by_sample(pair_loader(1))
    assert sorted(first) == sorted(again) == sorted(other) == [0, 1, 2]
    for n in range(3):
        for k in (0, 1):
            assert_bit_equal(first[n][k], again[n][k], f"sample {n}, store {k}: the same (seed, epoch) in batches of another size")
            assert first[n][k].shape != other[n][k].shape or not torch.equal(first[n][k], other[n][k]), f"sample {n}, store {k}: the next epoch"
    a, b = list(pair_loader(0)), list(pair_loader(0))
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        for t, u in zip(x, y):
            assert_bit_equal(t.cpu(), u.cpu(), "the same loader twice")
    loader = pair_loader(0)                                              # set_epoch on ONE loader: its own records follow
    e0 = planes_by_sample(loader)
    loader.set_epoch(1)
    e1 = planes_by_sample(loader)
    for n in range(3):
        assert_bit_equal(e0[n][0], first[n][0], "epoch 0")
        assert_bit_equal(e1[n][0], other[n][0], "epoch 1")


def test_without_augmentation_the_loader_is_the_plain_one_to_the_bit():
    from omr_a2s_multimodal_transformer_amd.image import collate_ragged_pairs
    ci, ca, _, _, targets = L.samples()
    qi = L.quantised(ci)
    ds = data()[3]
    loader = L.R().ResidentLoader(ds, 2, torch.float32, augment=None, augment2=None, seed=SEED, rank=0, world=1)
    plan = L.R().plan_batches(ds.stores[0].sizes, 2, sizes2=ds.stores[1].sizes, target_lens=ds.target_lens(), seed=SEED, epoch=0)
    assert loader.plan() == plan and loader.records() == [None, None]
    for indices, got in zip(plan, loader):
        want = collate_ragged_pairs([qi[n][0] for n in indices], [ca[n][0] for n in indices])
        assert_bit_equal(got[0].cpu(), want[0], "xi")
        assert_bit_equal(got[2].cpu(), want[2], "xa")
        assert torch.equal(got[1], want[1]) and torch.equal(got[3], want[3])
        for t, u in zip(got, ds.batch(indices, torch.float32)):
            assert_bit_equal(t.cpu(), u.cpu(), "dataset.batch without records")
    one = L.R().ResidentLoader(ds, 2, torch.float32, augment=image_augment(), seed=SEED, rank=0, world=1)      # only the first store
    for indices, got in zip(one.plan(), one):
        plain = ds.stores[1].gather(indices, torch.float32)
        assert_bit_equal(got[2].cpu(), plain[0].cpu(), "the store without an augmentation")
        assert torch.equal(got[3], plain[1])


def counts_of(y_out):
    return [int((y_out[b] != 0).sum()) for b in range(y_out.shape[0])]


def finite_step(m, batch):
    m.zero_grad()
    loss = m.training_step(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    grad = m._flat.grad.detach()
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all() and float(grad.abs().max()) > 0
    return float(loss.detach().double())


def test_training_step_on_an_augmented_unimodal_batch_equals_the_batch_size_1_runs():
    ds = data()[4]
    loader = L.R().ResidentLoader(ds, 3, torch.float32, augment=image_augment(), seed=SEED, rank=0, world=1)
    (batch,) = list(loader)
    x, sizes, y_in, y_out = batch
    assert x.shape[0] == 3 and len({tuple(s) for s in sizes.tolist()}) == 3
    m = L.make_unimodal("fp32")
    loss = finite_step(m, batch)
    counts = counts_of(y_out)
    alone = 0.0
    for b in range(3):
        crop = x[b:b + 1, :, :sizes[b, 0], :sizes[b, 1]].contiguous()
        alone += counts[b] / sum(counts) * finite_step(m, (crop, None, y_in[b:b + 1], y_out[b:b + 1]))
    print(f"augmented unimodal batch: loss {loss:.8f} vs the batch-size-1 runs {alone:.8f} (rel {abs(loss - alone) / abs(alone):.3e})")
    assert abs(loss - alone) <= LOSS_RTOL * abs(alone), (loss, alone)


def test_training_step_on_an_augmented_pair_batch_equals_the_batch_size_1_runs():
    loader = pair_loader(0, batch_size=3)
    (batch,) = list(loader)
    xi, si, xa, sa, y_in, y_out = batch
    assert xi.shape[0] == 3
    m = L.make_multimodal()
    loss = finite_step(m, batch)
    counts = counts_of(y_out)
    alone = 0.0
    for b in range(3):
        ci = xi[b:b + 1, :, :si[b, 0], :si[b, 1]].contiguous()
        ca = xa[b:b + 1, :, :sa[b, 0], :sa[b, 1]].contiguous()
        alone += counts[b] / sum(counts) * finite_step(m, (ci, None, ca, None, y_in[b:b + 1], y_out[b:b + 1]))
    print(f"augmented pair batch: loss {loss:.8f} vs the batch-size-1 runs {alone:.8f} (rel {abs(loss - alone) / abs(alone):.3e})")
    assert abs(loss - alone) <= LOSS_RTOL * abs(alone), (loss, alone)


def test_trainer_fit_takes_the_augmented_loader_for_two_steps():
    from omr_a2s_multimodal_transformer_amd.lightning_shim import Trainer
    ds = data()[4]
    loader = L.R().ResidentLoader(ds, 2, torch.bfloat16, augment=image_augment(), seed=SEED, rank=0, world=1)
    assert len(loader) == 2
    m = L.make_unimodal("bf16")
    seen = []
    step = m.training_step

    def counting_step(batch, i):
        x, xl, y_in, y_out = batch
        assert x.is_cuda and x.dtype == torch.bfloat16 and not xl.is_cuda and xl.shape == (x.shape[0], 2)
        assert x.shape[2] == int(xl[:, 0].max()) and x.shape[3] == int(xl[:, 1].max())
        seen.append(x.shape[0])
        return step(batch, i)

    m.training_step = counting_step
    before = m._flat.master.clone()
    Trainer(max_epochs=1).fit(m, loader)
    torch.cuda.synchronize()
    assert sorted(seen) == [1, 2]
    assert torch.isfinite(m.logged_metrics["train_loss"]).all()
    assert torch.isfinite(m._flat.master).all() and not torch.equal(m._flat.master, before)
