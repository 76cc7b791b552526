"""The CTC auxiliary head through Transformer: ctc_weight = 0 is the parent (no head, no omr_ctc_* entry), ctc_weight > 0 trains
(1 - w) CE + w CTC on both routes, the encoder-only transcript, and the head's gradient inside the decoder-side bucket of the reducer."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_refs as R
import spec_refs
from oracle import kernel_refs as KR

pytestmark = pytest.mark.gpu

from omr_a2s_multimodal_transformer_amd import functional as Fn  # noqa: E402
from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402

DEV = "cuda:0"
V = 40
W = 0.3


def cfg(**kw) -> ModelConfig:
    return ModelConfig(d_model=128, ff_dim=128, num_layers=1, dropout=0.0, encoder_dropout=0.0, **kw)


def build(config, seed=3, state=None, hw=(48, 160)):
    """A small Transformer on the GPU; `state`: the weights of another one (its head, if it has one, is left out where this one has none)."""
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    w2i, i2w = syn.make_vocab(V)
    torch.manual_seed(seed)
    m = Transformer(hw[0], hw[1], 16, w2i, i2w, config=config)
    if state is not None:
        m.load_state_dict({k: v for k, v in state.items() if k in m.state_dict()})
    m.flatten_parameters()
    m.train()
    m.teacher_forcing_prob = 0.0
    return m, w2i


def dense_batch(w2i, B=3):
    return tuple(t.to(DEV) for t in syn.synthetic_unimodal_batch(B, 32, 96, 8, V, w2i["<sos>"], w2i["<eos>"], seed=8))


SIZES = [[32, 96], [48, 160], [40, 120]]


def ragged_batch(w2i):
    _, _, y_in, y_out = syn.synthetic_unimodal_batch(3, 32, 96, 8, V, w2i["<sos>"], w2i["<eos>"], seed=9)
    x = torch.zeros((3, 1, 48, 160))
    for b, (h, w) in enumerate(SIZES):
        x[b, :, :h, :w] = KR.rnd((1, h, w), 20 + b, 0.0, 1.0)
    return x.to(DEV), torch.tensor(SIZES, dtype=torch.int64), y_in.to(DEV), y_out.to(DEV)


def step(m, batch):
    random.seed(0)
    m.zero_grad()
    loss = m.training_step(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    return loss, m._flat.grad.clone()


def by_name(m, flat_grad):
    return {n: flat_grad[o:o + c] for n, (o, c) in m._flat.offsets.items()}


def labels_of_batch(y_out, w2i):
    return [tuple(R.labels_of(row, blank=w2i["<PAD>"], eos=w2i["<eos>"])) for row in y_out.cpu().tolist()]


def test_weight_0_is_the_parent():
    m, w2i = build(cfg())
    assert not any("ctc" in k for k in m.state_dict()) and not hasattr(m, "ctc_head")
    batch = dense_batch(w2i)
    called = spec_refs.record_entries(lambda: step(m, batch))
    assert called and not [n for n in called if n.startswith("omr_ctc")]
    assert set(m.logged_metrics) == {"train_loss"}
    with_head, _ = build(cfg(ctc_weight=W))
    assert [n for n in spec_refs.record_entries(lambda: step(with_head, batch)) if n.startswith("omr_ctc")] == \
        ["omr_ctc_frames_fwd", "omr_ctc_workspace_bytes", "omr_ctc_fwd", "omr_ctc_bwd", "omr_ctc_frames_bwd"]


@pytest.mark.parametrize("pool", [1, 2])
def test_joint_loss_and_its_gradient(pool):
    m, w2i = build(cfg(ctc_weight=W, ctc_pool=pool))
    m0, _ = build(cfg(), state=m.state_dict())
    batch = dense_batch(w2i)
    x, xl, y_in, y_out = batch
    loss, g = step(m, batch)
    log = {k: v.detach().cpu() for k, v in m.logged_metrics.items()}
    loss0, g0 = step(m0, batch)
    # the CE part is the parent's loss of the same weights, bit for bit
    KR.assert_bit_equal(log["train_ce"].view(1), loss0.detach().cpu().view(1), "train_ce")
    assert int(log["ctc_infeasible"]) == 0 and set(log) == {"train_loss", "train_ce", "train_ctc", "ctc_infeasible"}
    want = (1.0 - W) * log["train_ce"] + W * log["train_ctc"]                        # the stated combination, in fp32 like the step's
    KR.assert_bit_equal(log["train_loss"].view(1), want.view(1), "train_loss")
    KR.assert_bit_equal(loss.detach().cpu().view(1), log["train_loss"].view(1), "returned loss")

    # the CTC part alone, on the memory the decoder read: the head's logits, its loss, and the gradients of the head and of the memory
    m.zero_grad()
    with torch.no_grad():
        _, mem = m._forward_memory(x, xl, y_in)
    mem = mem.detach().clone().requires_grad_(True)
    logits, flen = m._ctc_logits(mem)
    ctc, rows, infeasible = Fn.ctc_loss(logits, flen, y_out, w2i["<PAD>"], w2i["<eos>"])
    ctc.backward()
    torch.cuda.synchronize()
    KR.assert_bit_equal(ctc.detach().cpu().view(1), log["train_ctc"].view(1), "train_ctc")
    g_ctc = by_name(m, m._flat.grad.clone())
    gh, gw = 2, 12
    frames = [R.frame_count(gh, gw, pool)] * 3
    assert flen.cpu().tolist() == frames and tuple(logits.shape) == (3, frames[0], V) and logits.stride(1) == 40
    labels = labels_of_batch(y_out, w2i)
    lg = logits.detach().cpu()
    ref = R.reference_of(lg, frames, labels)
    bd = R.bounds_of(lg, frames, labels, ref)
    assert ref["feasible"].all()
    print(f"train_ctc {float(ctc)!r} vs fp64 {ref['loss']!r}, bound {bd['loss']:.3e}; rows error / bound "
          f"{(np.abs(rows.cpu().double().numpy() - ref['rows']) / bd['rows']).max():.3g}")
    assert abs(float(ctc) - ref["loss"]) <= bd["loss"]
    assert np.all(np.abs(rows.cpu().double().numpy() - ref["rows"]) <= bd["rows"])

    # torch autograd in fp64 from the same memory and head
    mem64 = mem.detach().cpu().double().requires_grad_(True)
    w64 = m.ctc_head.weight.detach().cpu().double().requires_grad_(True)
    b64 = m.ctc_head.bias.detach().cpu().double().requires_grad_(True)
    fr = torch.stack([R.frames_torch(mem64[b], gh, gw, pool) for b in range(3)])
    lp = F.log_softmax(fr @ w64.t() + b64, dim=2).permute(1, 0, 2)
    tg = torch.zeros((3, max(len(lb) for lb in labels)), dtype=torch.int64)
    for b, lb in enumerate(labels):
        tg[b, :len(lb)] = torch.tensor(lb)
    want_ctc = F.ctc_loss(lp, tg, torch.tensor(frames), torch.tensor([len(lb) for lb in labels]), blank=w2i["<PAD>"], reduction="mean", zero_infinity=True)
    gm, gw_, gb_ = torch.autograd.grad(want_ctc, (mem64, w64, b64))

    def close(got, ref64, what):
        t = KR.tol(KR.F32, float(ref64.abs().max()))
        err = (got.detach().cpu().double() - ref64).abs()
        allowed = t["atol"] + t["rtol"] * ref64.abs()
        assert bool((err <= allowed).all()), f"{what}: max error / allowed {float((err / allowed).max()):.3g}"

    close(mem.grad, gm, "CTC gradient of the memory")
    close(g_ctc["ctc_head.weight"].view(V, 128), gw_, "CTC gradient of the head weight")
    close(g_ctc["ctc_head.bias"], gb_, "CTC gradient of the head bias")

    # the whole CTC-only step (through the encoder) and the combination of the two
    random.seed(0)
    m.zero_grad()
    yhat, mem2 = m._forward_memory(x, xl, y_in)
    Fn.ctc_loss(*m._ctc_logits(mem2), y_out, w2i["<PAD>"], w2i["<eos>"])[0].backward()
    torch.cuda.synchronize()
    g_only = by_name(m, m._flat.grad.clone())
    g, g0 = by_name(m, g), by_name(m0, g0)
    for n, got in g.items():
        mix = W * g_only[n] + ((1.0 - W) * g0[n] if n in g0 else 0.0)
        if float(mix.norm()) == 0:
            assert float(got.norm()) == 0, n
            continue
        assert float((got - mix).norm() / mix.norm()) < 2e-4, n          # weight-gradient sums use fp32 atomics: noise, not bits
    assert float(g["ctc_head.weight"].norm()) > 0 and float(g_only["encoder.conv_blocks.0.conv1.weight"].norm()) > 0


def test_label_smoothing_applies_to_the_ce_part_only():
    m, w2i = build(cfg(ctc_weight=W, label_smoothing=0.1))
    m1, _ = build(cfg(ctc_weight=W), state=m.state_dict())
    batch = dense_batch(w2i)
    step(m, batch), step(m1, batch)
    a, b = m.logged_metrics, m1.logged_metrics
    KR.assert_bit_equal(a["train_ctc"].cpu().view(1), b["train_ctc"].cpu().view(1), "train_ctc")
    KR.assert_bit_equal(a["train_nll"].cpu().view(1), b["train_ce"].cpu().view(1), "un-smoothed CE")
    assert float(a["train_ce"]) != float(b["train_ce"])


def test_ragged_rows_equal_the_samples_alone():
    m, w2i = build(cfg(ctc_weight=W, ctc_pool=2))
    x, xl, y_in, y_out = ragged_batch(w2i)
    step(m, (x, xl, y_in, y_out))
    _, rows, infeasible = m.last_ctc
    rows = rows.cpu().tolist()
    assert int(infeasible.cpu()) == 0 and all(r > 0 for r in rows)
    for b, (h, w) in enumerate(SIZES):
        step(m, (x[b:b + 1, :, :h, :w].contiguous(), xl[b:b + 1], y_in[b:b + 1], y_out[b:b + 1]))
        alone = float(m.last_ctc[1].cpu()[0])
        assert abs(alone - rows[b]) <= 2e-4 * (1.0 + abs(rows[b])), (b, alone, rows[b])      # the InstanceNorm sums are added in another order


def test_a_target_that_does_not_fit_is_counted_and_adds_nothing():
    m, w2i = build(cfg(ctc_weight=W, ctc_pool=2), hw=(32, 64))
    x = KR.rnd((2, 1, 32, 16), 4, 0.0, 1.0).to(DEV)
    y_in = torch.tensor([[w2i["<sos>"], 5, 6, 7, 8, 0, 0, 0]] * 2, device=DEV)
    y_out = torch.tensor([[5, 6, 7, 8, w2i["<eos>"], 0, 0, 0]] * 2, device=DEV)
    loss, g = step(m, (x, None, y_in, y_out))                               # a 2 x 2 grid pooled by 2: 2 frames for 4 labels
    assert int(m.logged_metrics["ctc_infeasible"].cpu()) == 2 and float(m.logged_metrics["train_ctc"]) == 0.0
    assert torch.isfinite(loss).all() and float(by_name(m, g)["ctc_head.weight"].norm()) == 0


def test_predict_ctc_is_the_collapsed_arg_max_of_the_heads_logits():
    from omr_a2s_multimodal_transformer_amd.image import collate_ragged
    m, w2i = build(cfg(ctc_weight=W, ctc_pool=1))
    xs = [KR.rnd((1, 1, h, w), 60 + i, 0.0, 1.0) for i, (h, w) in enumerate(SIZES + [[32, 64], [48, 96]])]
    got = m.predict_ctc(xs, batch_size=3)
    assert m.training                                                      # the mode is put back
    want = []
    m.eval()
    with torch.no_grad():
        for group in (xs[:3], xs[3:]):
            x, sizes = collate_ragged([t[0] for t in group])
            mem, _, _ = m._encode_packed(x, sizes)
            logits, flen = m._ctc_logits(mem)
            toks, _ = R.greedy_ref(logits.cpu().double().numpy(), flen.cpu().tolist(), blank=w2i["<PAD>"])
            want.extend([[m.i2w[t] for t in seq] for seq in toks])
    assert got == want and len(got) == 5 and any(len(w) > 0 for w in got)
    metrics = m.evaluate_ctc([(x, torch.tensor([[w2i["<sos>"], 5, 6, w2i["<eos>"]]])) for x in xs], batch_size=2)
    assert set(metrics) >= {"sym-er", "seq-er"}
    plain, _ = build(cfg())
    with pytest.raises(ValueError):
        plain.predict_ctc(xs)
    with pytest.raises(ValueError):
        plain.evaluate_ctc([])


def test_checkpoint_round_trip_keeps_the_head(tmp_path):
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    m, _ = build(cfg(ctc_weight=W, ctc_pool=2))
    p = str(tmp_path / "m.ckpt")
    m.save_checkpoint(p)
    m2 = Transformer.load_from_checkpoint(p)
    assert (m2.ctc_weight, m2.ctc_pool) == (W, 2)
    for k, v in m.state_dict().items():
        assert torch.equal(v.detach().cpu(), m2.state_dict()[k].detach().cpu()), k


def test_single_rank_reducer_holds_the_head_in_the_decoder_bucket():
    import torch.distributed as dist
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29733", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        results = []
        state = None
        for with_reducer in (False, True):
            m, w2i = build(cfg(ctc_weight=W, ctc_pool=2), state=state)
            state = {k: v.detach().clone() for k, v in m.state_dict().items()} if state is None else state      # a copy: the step below moves the weights
            batch = dense_batch(w2i)
            opt = m.configure_optimizers()
            red = None
            if with_reducer:
                red = m.attach_reducer()
                red.world = 2                                              # pretend: the collective still runs over the one real rank
                flat = m._flat
                enc = [n for n in flat.names if n.startswith("encoder.")]
                b, e = flat.slice_of([n for n in flat.names if n not in set(enc)])
                for n in ("ctc_head.weight", "ctc_head.bias"):
                    o, c = flat.offsets[n]
                    assert b <= o and o + c <= e, n
                assert all(not (b <= flat.offsets[n][0] < e) for n in enc)  # the decoder-side range holds no encoder parameter
            random.seed(0)
            opt.zero_grad()
            m.training_step(batch, 0).backward()
            if red is not None:
                assert red.done[1] and not red.done[0]                     # the head's gradient was final at the memory boundary
                red.finish()
            torch.cuda.synchronize()
            grad = m._flat.grad.clone()
            opt.step(grad_scale=red.grad_scale if red is not None else 0.5)
            torch.cuda.synchronize()
            results.append((by_name(m, grad), m._flat.master.clone()))
        (g0, p0), (g1, p1) = results
        for n, r in g0.items():
            if float(r.abs().max()) == 0:
                continue
            assert float((g1[n] - r).norm() / r.norm()) < 1e-5, n
        assert float(g1["ctc_head.weight"].norm()) > 0 and float((p1 - p0).abs().max()) < 2.5e-4
    finally:
        dist.destroy_process_group()
