"""The optimizer recipe's references (tests/optim_refs.py) against torch on the CPU, and the host-side pieces of the recipe:
config.OptimConfig, config.lr_at, params.decay_block_map, FusedAdam's state.  No GPU."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import optim_refs as R
from omr_a2s_multimodal_transformer_amd.config import OptimConfig, lr_at
from omr_a2s_multimodal_transformer_amd.params import ALIGN, FlatParams, FusedAdam, decay_block_map, decays

SIZES = [1, 3, 4, 63, 64, 65, 4 * 1024 + 1, 2048 * 256 * 4 + 4 * 256 + 3]          # tests/test_optim_recipe_gpu.py's sizes


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


# ------------------------------------------------------------------------------------------------ restatement == torch, fp64
@pytest.mark.parametrize("wd", [0.0, 0.1], ids=["no-decay", "decay"])
def test_restatement_agrees_with_torch_adamw_fp64(wd):
    """Three steps; a second param group with weight_decay=0 plays the no-decay blocks."""
    n, lr, b1, b2, eps = 257, 1e-3, 0.9, 0.999, 1e-8
    p0, _, _, _, grads = R.inputs(2 * n, seed=5, steps=3)
    a, b = nn.Parameter(torch.tensor(p0[:n], dtype=torch.float64)), nn.Parameter(torch.tensor(p0[n:], dtype=torch.float64))
    opt = torch.optim.AdamW([dict(params=[a], weight_decay=wd), dict(params=[b], weight_decay=0.0)], lr=lr, betas=(b1, b2), eps=eps)
    mask = np.arange(2 * n) < n
    state = (p0.astype(np.float64), np.zeros(2 * n), np.zeros(2 * n), None)
    for j, g in enumerate(grads):
        a.grad, b.grad = torch.tensor(g[:n], dtype=torch.float64), torch.tensor(g[n:], dtype=torch.float64)
        opt.step()
        state, _ = R.ref_step(state, g, j + 1, lr, b1, b2, eps, wd=wd, decay_mask=mask)
        want = torch.cat([a.detach(), b.detach()]).numpy()
        assert rel(state[0], want) <= 1e-12, (j, rel(state[0], want))
    if wd:
        plain, _ = R.ref_step((p0.astype(np.float64), np.zeros(2 * n), np.zeros(2 * n), None), grads[0], 1, lr, b1, b2, eps)
        first, _ = R.ref_step((p0.astype(np.float64), np.zeros(2 * n), np.zeros(2 * n), None), grads[0], 1, lr, b1, b2, eps, wd=wd, decay_mask=mask)
        assert np.array_equal(first[0][n:], plain[0][n:]) and not np.array_equal(first[0][:n], plain[0][:n])


def test_restatement_clip_scale_and_skip():
    p0, m0, v0, e0, grads = R.inputs(100, seed=6, steps=1)
    st = tuple(x.astype(np.float64) for x in (p0, m0, v0, e0))
    a, _ = R.ref_step(st, grads[0], 2, 1e-3, 0.9, 0.999, 1e-8, grad_scale=0.5, clip=0.25)
    b, _ = R.ref_step(st, grads[0] * np.float32(0.125), 2, 1e-3, 0.9, 0.999, 1e-8)              # 0.125 g is exact in fp32
    assert rel(a[0], b[0]) <= 1e-15
    s, t = R.ref_step(st, grads[0], 2, 1e-3, 0.9, 0.999, 1e-8, wd=0.1, ema_decay=0.9, apply=False)
    assert all(x is y for x, y in zip(s, st)) and not t.any()


@pytest.mark.parametrize("d", [0.0, 0.9, 0.999, 1.0])
def test_restatement_ema_agrees_with_averaged_model(d):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    n, lr = 64, 1e-2
    p0, _, _, _, grads = R.inputs(n, seed=7, steps=4)
    lin = nn.Linear(n, 1, bias=False).double()
    with torch.no_grad():
        lin.weight.copy_(torch.tensor(p0, dtype=torch.float64).view(1, n))
    avg = AveragedModel(lin, multi_avg_fn=get_ema_multi_avg_fn(d))
    avg.update_parameters(lin)                                   # the first update copies: FusedAdam.enable_ema's initial state
    opt = torch.optim.AdamW(lin.parameters(), lr=lr, weight_decay=0.0)
    state = (p0.astype(np.float64), np.zeros(n), np.zeros(n), p0.astype(np.float64))
    for j, g in enumerate(grads):
        lin.weight.grad = torch.tensor(g, dtype=torch.float64).view(1, n)
        opt.step()
        avg.update_parameters(lin)
        state, _ = R.ref_step(state, g, j + 1, lr, 0.9, 0.999, 1e-8, ema_decay=d)
    want = avg.module.weight.detach().numpy().ravel()
    assert rel(state[3], want) <= 1e-12
    if d == 1.0:
        assert np.array_equal(state[3], p0.astype(np.float64))
    if d == 0.0:
        assert np.array_equal(state[3], state[0])
    snaps = []
    st = (p0.astype(np.float64), np.zeros(n), np.zeros(n), None)
    for j, g in enumerate(grads):
        st, _ = R.ref_step(st, g, j + 1, lr, 0.9, 0.999, 1e-8)
        snaps.append(st[0])
    assert rel(R.ema_recursion(snaps, p0, d)[0], want) <= 1e-12


# ------------------------------------------------------------------------------------------------ the bound holds for the kernel's order
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("d", [0.9, 0.999])
def test_fp32_transcription_stays_inside_the_bound(n, d):
    """The very inputs tests/test_optim_recipe_gpu.py feeds the kernel (same seeds, same hyper-parameters): the kernel's operation
    order in fp32 stays inside the bound, so only the kernel can fail it."""
    d = R.f32(d)
    steps = 4
    p, m, v, ema, grads = R.inputs(n, seed=n, steps=steps)
    _, mask = R.block_mask(n)
    kw = dict(wd=R.WD, decay_mask=mask, ema_decay=d, grad_scale=R.GRAD_SCALE)
    ref, pb, eb = R.ref_run(p, m, v, ema, grads, R.FIRST_STEP, **R.HYPER, **kw)
    st = (p, m, v, ema)
    for j, g in enumerate(grads):
        st = R.kernel_f32_step(st, g, R.FIRST_STEP + j, **R.HYPER, **kw)
        assert all(x.dtype == np.float32 for x in st)
    perr, eerr = np.abs(st[0] - ref[0]), np.abs(st[3] - ref[3])
    print(f"n={n} d={d}: p err/bound max {float(np.max(perr / pb)):.3f}, ema err/bound max {float(np.max(eerr / eb)):.3f}")
    assert (perr <= pb).all() and (eerr <= eb).all()
    assert float(np.max(pb / np.abs(ref[0]).clip(1e-3))) < 1e-3 and float(np.max(eb / np.abs(ref[3]).clip(1e-3))) < 1e-3      # a bound that says something
    moved = np.abs(ref[0] - p.astype(np.float64))
    assert np.median(moved) > 100 * np.median(pb)                                                  # ... far below what the steps do


# ------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("case", range(len(R.LR_CASES)))
def test_lr_at_matches_hand_written_values(case):
    args, table = R.LR_CASES[case]
    cfg = OptimConfig(lr=R.LR0, **args)
    for k, ratio in table.items():
        assert lr_at(cfg, k) == pytest.approx(R.LR0 * ratio, rel=1e-14, abs=0), (args, k)
    with pytest.raises(ValueError):
        lr_at(cfg, -1)


def test_lr_at_shapes():
    cos = OptimConfig(lr=1.0, schedule="cosine", warmup_steps=3, total_steps=50, min_lr_ratio=0.05)
    lin = OptimConfig(lr=1.0, schedule="linear", warmup_steps=3, total_steps=50, min_lr_ratio=0.05)
    for cfg in (cos, lin):
        vals = [lr_at(cfg, k) for k in range(60)]
        assert vals[:3] == [1 / 3, 2 / 3, 1.0] and vals[3] == 1.0
        assert all(a >= b for a, b in zip(vals[3:], vals[4:])) and vals[50:] == [0.05] * 10
    mid = 3 + (50 - 3) / 2
    assert math.isclose(0.5 * (lr_at(cos, 26) + lr_at(cos, 27)), (1 + 0.05) / 2, rel_tol=1e-3) and 26 < mid < 27
    assert lr_at(OptimConfig(lr=0.5), 10 ** 9) == 0.5


# ------------------------------------------------------------------------------------------------ OptimConfig
def test_optim_config_round_trip_and_defaults():
    import json
    c = OptimConfig()
    assert (c.lr, c.betas, c.eps, c.weight_decay, c.no_decay, c.warmup_steps, c.schedule, c.total_steps, c.min_lr_ratio, c.ema_decay) == \
        (1e-4, (0.9, 0.999), 1e-8, 0.0, ("bias", "norm"), 0, "constant", None, 0.0, None)
    assert c.plain
    full = OptimConfig(lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.05, no_decay=("bias", "norm", "embedding"), warmup_steps=10,
                       schedule="cosine", total_steps=1000, min_lr_ratio=0.01, ema_decay=0.999)
    assert not full.plain
    d = json.loads(json.dumps(full.to_dict()))                    # plain data
    back = OptimConfig.from_dict(dict(d, unknown_key=1))
    assert back == full and isinstance(back.betas, tuple) and isinstance(back.no_decay, tuple)
    assert OptimConfig.from_dict(c.to_dict()) == c
    for part in (dict(weight_decay=0.1), dict(ema_decay=0.0), dict(warmup_steps=1), dict(schedule="linear", total_steps=5)):
        assert not OptimConfig(**part).plain


@pytest.mark.parametrize("bad", [dict(lr=-1.0), dict(lr=float("nan")), dict(betas=(0.9,)), dict(betas=(0.9, 1.0)), dict(eps=-1e-8),
                                 dict(weight_decay=-0.1), dict(weight_decay=float("inf")), dict(no_decay=("",)), dict(warmup_steps=-1),
                                 dict(warmup_steps=1.5), dict(schedule="step"), dict(schedule="cosine"), dict(schedule="linear", total_steps=0),
                                 dict(schedule="cosine", warmup_steps=5, total_steps=5), dict(min_lr_ratio=1.5), dict(min_lr_ratio=-0.1),
                                 dict(ema_decay=1.5), dict(ema_decay=-0.1), dict(ema_decay=float("nan"))])
def test_optim_config_refuses_bad_values(bad):
    with pytest.raises(ValueError):
        OptimConfig(**bad)


# ------------------------------------------------------------------------------------------------ decay-block map
def test_decay_block_map_of_a_hand_made_table():
    """Offsets as FlatParams lays them (every start a multiple of ALIGN = 64), with a hole of two blocks nobody owns."""
    assert ALIGN == 64
    offsets = {"enc.conv.weight": (0, 130),        # blocks 0, 1, 2 (the third is partial): decays
               "enc.conv.bias": (192, 5),          # block 3: a bias
               "enc.norm.weight": (256, 64),       # block 4: 2-D but named norm
               "dec.gain": (320, 64),              # block 5: 1-D
               "dec.out.weight": (512, 64),        # block 8: decays; blocks 6, 7 belong to nobody
               "dec.embedding.weight": (576, 65)}  # blocks 9, 10: decays unless named in no_decay
    ndims = {"enc.conv.weight": 4, "enc.conv.bias": 1, "enc.norm.weight": 2, "dec.gain": 1, "dec.out.weight": 2, "dec.embedding.weight": 2}
    total = 704
    assert decay_block_map(offsets, ndims, total, ("bias", "norm")) == [1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1]
    assert decay_block_map(offsets, ndims, total, ("bias", "norm", "embedding")) == [1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0]
    assert decay_block_map(offsets, ndims, total, ()) == [1, 1, 1, 0, 1, 0, 0, 0, 1, 1, 1]
    assert decays("a.weight", 2, ("bias",)) and not decays("a.weight", 1, ()) and not decays("a.bias_proj", 2, ("bias",))
    with pytest.raises(ValueError):
        decay_block_map({"w": (32, 64)}, {"w": 2}, 128, ())


# ------------------------------------------------------------------------------------------------ FusedAdam's host state
def _cpu_optimizer(optim=None):
    torch.manual_seed(0)
    mods = nn.ModuleDict(dict(encoder=nn.Linear(5, 7), decoder=nn.Linear(7, 3)))
    flat = FlatParams(list(mods.named_parameters()), torch.device("cpu"), torch.float32)
    return flat, FusedAdam(flat, optim=optim)


def test_fused_adam_configuration_and_state():
    flat, plain = _cpu_optimizer()
    assert plain.param_groups[0]["weight_decay"] == 0 and not plain._recipe and flat.ema is None
    sd = plain.state_dict()
    assert sd["calls"] == 0 and "optim" not in sd and "ema" not in sd
    _, same = _cpu_optimizer(OptimConfig())
    assert not same._recipe and same.param_groups[0]["lr"] == 1e-4
    cfg = OptimConfig(lr=2e-3, weight_decay=0.1, schedule="cosine", warmup_steps=2, total_steps=9, ema_decay=0.9)
    flat, opt = _cpu_optimizer(cfg)
    g = opt.param_groups[0]
    assert opt._recipe and g["weight_decay"] == 0.1 and g["lr"] == 2e-3
    want = [0] * (flat.total // ALIGN)
    for name, (off, cnt) in flat.offsets.items():
        if name.endswith("weight"):
            want[off // ALIGN:(off + cnt + ALIGN - 1) // ALIGN] = [1] * ((cnt + ALIGN - 1) // ALIGN)
    assert opt._decay_blocks.tolist() == want and 0 in want and 1 in want
    assert flat.ema is not flat.master and torch.equal(flat.ema, flat.master) and opt.ema_decay == 0.9
    opt.calls, opt.steps = 5, dict(encoder=4, decoder=5)
    flat.ema.add_(1.0)
    sd = copy.deepcopy(opt.state_dict())
    assert sd["calls"] == 5 and sd["optim"] == cfg.to_dict() and torch.equal(sd["ema"], flat.ema) and sd["ema_decay"] == 0.9
    flat2, fresh = _cpu_optimizer()                                # a fresh optimizer WITHOUT a config takes all of it
    fresh.load_state_dict(sd)
    assert fresh.calls == 5 and fresh.optim == cfg and fresh._recipe and torch.equal(flat2.ema, sd["ema"])
    assert fresh.param_groups[0]["lr"] == lr_at(cfg, 4) and fresh._decay_blocks.tolist() == want
    old = {k: v for k, v in sd.items() if k not in ("calls", "optim", "ema", "ema_decay")}      # a dict from before the recipe
    flat3, older = _cpu_optimizer()
    older.load_state_dict(old)
    assert older.calls == sd["step"] and older.optim is None and flat3.ema is None and not older._recipe
    with pytest.raises(ValueError):
        opt.enable_ema(1.5)
    with pytest.raises(RuntimeError):
        with plain.ema_weights():
            pass
