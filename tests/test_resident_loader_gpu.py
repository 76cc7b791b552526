"""resident.ResidentStore / ResidentDataset / ResidentLoader on the GPU against the host collate they replace.  The samples are those of
tests/test_ragged_training_gpu.py (64 x 96, 37 x 50, 17 x 9) and the three pairs of tests/test_multimodal_ragged_gpu.py, with their
targets of 11 / 7 / 4 tokens: a batch from the resident set has to be `image.collate_ragged` / `collate_ragged_pairs` of the same
tensors to the bit, and the models must not see a difference.  Small models (2 decoder layers, d_model 128, 30 tokens)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import multimodal_ragged_refs as M  # noqa: E402
from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402
from oracle.kernel_refs import assert_bit_equal  # noqa: E402

DEV = "cuda:0"


def R():
    from omr_a2s_multimodal_transformer_amd import resident
    return resident


def vocab():
    return syn.make_vocab(M.V)


def make_unimodal(dtype: str):
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    w2i, i2w = vocab()
    cfg = ModelConfig(d_model=M.D, ff_dim=M.D, num_layers=M.LAYERS, dropout=0.0, encoder_dropout=0.0, compute_dtype=dtype)
    m = Transformer(M.IMG_PLANE[0], M.IMG_PLANE[1], M.T + 4, w2i, i2w, config=cfg)
    m.load_state_dict(syn.seeded_state_dict(syn.transformer_shapes(M.V, M.D, M.D, M.LAYERS), 23), strict=False)
    m.flatten_parameters()
    m.teacher_forcing_prob = 0.0
    m.eval()
    return m


def make_multimodal():
    from omr_a2s_multimodal_transformer_amd.model import MultimodalTransformer
    w2i, i2w = vocab()
    cfg = ModelConfig(d_model=M.D, ff_dim=M.D, num_layers=M.LAYERS, dropout=0.0, encoder_dropout=0.0, compute_dtype="fp32")
    m = MultimodalTransformer(M.IMG_PLANE[0], M.IMG_PLANE[1], M.AUD_PLANE[0], M.AUD_PLANE[1], M.T + 4, w2i, i2w, mixer_type="concat", config=cfg)
    m.load_state_dict(syn.seeded_state_dict(syn.multimodal_shapes(M.V, "concat", M.D, M.D, M.LAYERS), 23), strict=False)
    m.flatten_parameters()
    m.teacher_forcing_prob = 0.0
    m.apply_teacher_forcing_modality = lambda: "both"
    m.eval()
    return m


@functools.lru_cache(maxsize=None)
def samples():
    """(image crops [1, 1, h, w], audio crops, y_in, y_out [3, 12] padded by hand, the targets as token lists with <sos> and <eos>)."""
    ci, ca, *_ = M.make_pairs()
    y_in, y_out, counts = M.make_targets(vocab()[0])
    targets = [torch.cat([y_in[b, :n], y_out[b, n - 1:n]]) for b, n in enumerate(counts)]
    assert [t.numel() for t in targets] == [n + 2 for n in M.TARGET_LENS]
    return ci, ca, y_in, y_out, targets


def store_of(crops, kind="f32"):
    s = R().ResidentStore(kind, DEV)
    for c in crops:
        s.append(c[0])
    return s


def quantised(crops):
    """The crops rounded to k / 255: what a score image is after preprocess_image."""
    return [(c * 255).round() / 255 for c in crops]


# ------------------------------------------------------------------------------------------------ the store

def test_store_round_trip_of_a_preprocessed_image():
    """A 45 x 83 RGB image resized to height 32 (width int(32 * 83 / 45) = 59) by image.preprocess_image: append + gather gives that
    tensor's bits, in fp32 and (through kernels.cast) in bf16."""
    from omr_a2s_multimodal_transformer_amd import image, kernels
    g = torch.Generator().manual_seed(8)
    raws = [torch.randint(0, 256, (45, 83, 3), generator=g).to(torch.uint8), torch.randint(0, 256, (20, 31, 3), generator=g).to(torch.uint8)]
    want = [image.preprocess_image(r, 32, torch.float32, DEV) for r in raws]
    assert tuple(want[0].shape) == (1, 32, 59)
    ds = R().ResidentDataset.from_raw_images(raws, 32, [torch.tensor([1, 2, 3]), torch.tensor([1, 3])], DEV)
    store = ds.stores[0]
    assert store.kind == "u8" and store.buf.dtype == torch.uint8 and store.sizes.tolist() == [[32, 59], [32, 49]]
    for n, w in enumerate(want):
        x, sizes = store.gather([n], torch.float32)
        assert sizes.tolist() == [list(w.shape[1:])] and sizes.dtype == torch.int64 and not sizes.is_cuda
        assert_bit_equal(x[0].cpu(), w.cpu(), f"sample {n}, fp32")
        assert_bit_equal(store.gather([n], torch.bfloat16)[0][0].cpu(), kernels.cast(w, torch.bfloat16).cpu(), f"sample {n}, bf16")
    x, sizes = store.gather([1, 0], torch.float32, pad_value=1.0)              # the dense collate's white background
    assert_bit_equal(x.cpu(), image.pad_batch_inputs([want[1], want[0]], pad_value=1.0).cpu(), "pad 1.0")


def test_a_u8_store_refuses_what_it_cannot_reproduce():
    store = R().ResidentStore("u8", DEV)
    ok = torch.tensor([[0.0, 255.0, 128.0], [3.0, 254.0, 77.0]]) / 255
    assert store.append(ok) == 0
    for bad in (torch.tensor([[0.5, 0.25]]), torch.tensor([[float("nan")]]), torch.tensor([[2.0]]), torch.tensor([[1 / 255 + 1e-8, 0.7]])):
        with pytest.raises(ValueError, match="lossless"):
            store.append(bad)
    assert len(store) == 1 and store.used == 6                              # a refused sample leaves no trace
    assert store.append(ok[:1].to(DEV)) == 1                                # host or device tensors
    assert_bit_equal(store.gather([1, 0], torch.float32)[0].cpu(), torch.stack([torch.cat([ok[:1], torch.zeros(1, 3)]), ok]).unsqueeze(1), "after a refusal")
    assert R().ResidentStore("f32", DEV).append(torch.tensor([[0.5, 0.25]])) == 0
    with pytest.raises(ValueError):
        R().ResidentStore("bf16", DEV)


def test_the_buffer_grows_geometrically_and_never_holds_twice_its_content():
    store = R().ResidentStore("f32", DEV)
    g = torch.Generator().manual_seed(1)
    allocations, kept = set(), []
    for n in range(40):
        s = torch.rand((3 + n % 5, 7 + n % 3), generator=g)
        kept.append(s)
        store.append(s)
        allocations.add(store.buf.data_ptr())
        assert store.used <= store.buf.numel() <= 2 * store.used
    assert len(allocations) <= 8                                            # 40 samples, a handful of doublings
    x, sizes = store.gather(list(range(40)), torch.float32)
    from omr_a2s_multimodal_transformer_amd.image import collate_ragged
    want, want_sizes = collate_ragged(kept)
    assert torch.equal(sizes, want_sizes)
    assert_bit_equal(x.cpu(), want, "40 samples")


# ------------------------------------------------------------------------------------------------ batches equal the host collate

@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_unimodal_batch_equals_collate_ragged_and_the_model_agrees(kind):
    from omr_a2s_multimodal_transformer_amd.image import collate_ragged
    ci, _, y_in, y_out, targets = samples()
    crops = quantised(ci) if kind == "u8" else ci
    ds = R().ResidentDataset(images=store_of(crops, kind), targets=targets)
    want_x, want_sizes = collate_ragged([c[0] for c in crops])
    for order in ([0, 1, 2], [2, 0]):
        x, sizes, yi, yo = ds.batch(order, torch.float32)
        wx, ws = collate_ragged([crops[n][0] for n in order])
        assert x.is_cuda and not sizes.is_cuda and not yi.is_cuda and not yo.is_cuda
        assert sizes.dtype == yi.dtype == yo.dtype == torch.int64 and torch.equal(sizes, ws)
        assert_bit_equal(x.cpu(), wx, f"x, samples {order}")
        T = max(targets[n].numel() for n in order) - 1
        assert torch.equal(yi, y_in[order, :T]) and torch.equal(yo, y_out[order, :T]) and yi.shape == (len(order), T)
    x, sizes, yi, yo = ds.batch([0, 1, 2], torch.float32)
    assert tuple(x.shape) == (3, 1) + M.IMG_PLANE and torch.equal(yi, y_in) and torch.equal(yo, y_out)
    m = make_unimodal("fp32")
    with torch.no_grad():
        got = m(x, sizes, yi)
        ref = m(want_x.to(DEV), want_sizes, y_in)
    assert_bit_equal(got.cpu(), ref.cpu(), "logits")
    assert torch.isfinite(got).all()
    xb = ds.batch([0, 1, 2], torch.bfloat16)[0]
    assert_bit_equal(xb.cpu(), want_x.to(torch.bfloat16), "bf16 batch")


def test_multimodal_batch_equals_collate_ragged_pairs_and_the_model_agrees():
    from omr_a2s_multimodal_transformer_amd.image import collate_ragged_pairs
    ci, ca, y_in, y_out, targets = samples()
    qi = quantised(ci)
    ds = R().ResidentDataset(images=store_of(qi, "u8"), audios=store_of(ca, "f32"), targets=targets)
    want = collate_ragged_pairs([c[0] for c in qi], [c[0] for c in ca])
    xi, si, xa, sa, yi, yo = ds.batch([0, 1, 2], torch.float32)
    assert tuple(xi.shape) == (3, 1) + M.IMG_PLANE and tuple(xa.shape) == (3, 1) + M.AUD_PLANE
    assert_bit_equal(xi.cpu(), want[0], "xi")
    assert_bit_equal(xa.cpu(), want[2], "xa")
    assert torch.equal(si, want[1]) and torch.equal(sa, want[3]) and torch.equal(yi, y_in) and torch.equal(yo, y_out)
    m = make_multimodal()
    with torch.no_grad():
        got = m(xi, si, xa, sa, yi, apply_teacher_forcing_modality=True)
        ref = m(want[0].to(DEV), want[1], want[2].to(DEV), want[3], y_in, apply_teacher_forcing_modality=True)
    assert_bit_equal(got.cpu(), ref.cpu(), "logits")
    items = list(ds.eval_batches())
    assert len(items) == 3
    for b, (xi1, xa1, y) in enumerate(items):
        assert_bit_equal(xi1.cpu(), qi[b], f"eval image {b}")
        assert_bit_equal(xa1.cpu(), ca[b], f"eval audio {b}")
        assert torch.equal(y, targets[b].unsqueeze(0))
    assert m.evaluate(items) == m.evaluate([(qi[b].to(DEV), ca[b].to(DEV), targets[b].unsqueeze(0)) for b in range(3)])
    with pytest.raises(ValueError):
        R().ResidentDataset(images=store_of(qi[:2], "u8"), audios=store_of(ca, "f32"), targets=targets)


def test_eval_batches_are_the_samples_unpadded_and_evaluate_takes_them():
    ci, _, _, _, targets = samples()
    ds = R().ResidentDataset(images=store_of(ci), targets=targets)
    items = list(ds.eval_batches())
    assert len(items) == 3
    for b, (x, y) in enumerate(items):
        assert_bit_equal(x.cpu(), ci[b], f"eval sample {b}")
        assert torch.equal(y, targets[b].unsqueeze(0)) and not y.is_cuda
    m = make_unimodal("fp32")
    got = m.evaluate(ds.eval_batches(), batch_size=2)
    assert got == m.evaluate([(ci[b].to(DEV), targets[b].unsqueeze(0)) for b in range(3)])
    assert set(got) and all(v == v for v in got.values())


# ------------------------------------------------------------------------------------------------ the loader under Trainer.fit

def test_trainer_fit_runs_the_loader_for_two_epochs_with_batches_of_different_size():
    """7 images in the 64 x 96 plane, batch_size 3, at most 2 * 64 * 96 padded pixels per batch: the plans hold batches of 1, 2 and 3."""
    from omr_a2s_multimodal_transformer_amd.lightning_shim import Trainer
    sizes = [(64, 96), (37, 50), (17, 9), (20, 30), (33, 64), (48, 80), (10, 90)]
    w2i, _ = vocab()
    g = torch.Generator().manual_seed(12)
    store = R().ResidentStore("u8", DEV)
    targets = []
    for n, (h, w) in enumerate(sizes):
        store.append(torch.randint(0, 256, (h, w), generator=g).float() / 255)
        toks = torch.randint(3, M.V, (3 + n,), generator=g)
        targets.append(torch.cat([torch.tensor([w2i["<sos>"]]), toks, torch.tensor([w2i["<eos>"]])]))
    ds = R().ResidentDataset(images=store, targets=targets)
    loader = R().ResidentLoader(ds, 3, torch.bfloat16, max_padded_pixels=2 * 64 * 96, chunk_batches=4, seed=1)
    plans = []
    for e in (0, 1):
        loader.set_epoch(e)
        plans.append([list(b) for b in loader.plan()])
        assert sorted(n for b in plans[e] for n in b) == list(range(7)) and len(loader) == len(plans[e])
    assert plans[0] != plans[1]
    assert all(len({len(b) for b in p}) > 1 for p in plans)

    m = make_unimodal("bf16")
    seen = []
    step = m.training_step

    def counting_step(batch, i):
        x, xl, y_in, y_out = batch
        assert x.is_cuda and x.dtype == torch.bfloat16 and not xl.is_cuda and not y_in.is_cuda and xl.shape == (x.shape[0], 2)
        seen.append(x.shape[0])
        return step(batch, i)

    m.training_step = counting_step
    before = m._flat.master.clone()
    Trainer(max_epochs=2).fit(m, loader)
    torch.cuda.synchronize()
    assert seen == [len(b) for b in plans[0]] + [len(b) for b in plans[1]]
    assert len(set(seen)) > 1
    loss = m.logged_metrics["train_loss"]
    assert torch.isfinite(loss).all(), loss
    assert torch.isfinite(m._flat.master).all() and not torch.equal(m._flat.master, before)
