"""omr_adamw_ema and omr_swap_f32 on the GPU: bit for bit the ENTRIES omr_adam / omr_adam_guarded when nothing new is asked for
(they are argument adapters onto the same launch: the tests prove that every argument is passed through; that the one kernel
computes what the three kernels before it computed is tests/test_optim_bits_gpu.py's job), the skip, the decay-block map, the
EMA's exact edges, and decay and EMA values against the fp64 restatement of tests/optim_refs.py inside the bound derived there (P_OPS(k) = 14 + 2 k roundings per step on |p| + |t|, E_OPS = 3 on max(|ema|, |p|); tests/test_optim_refs_cpu.py
shows an fp32 transcription of the kernel's order inside that bound on these very inputs)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import optim_refs as R  # noqa: E402
from omr_a2s_multimodal_transformer_amd import kernels as K  # noqa: E402
from omr_a2s_multimodal_transformer_amd._lib import cur_stream, lib, ptr  # noqa: E402

DEV = "cuda:0"
GRID_CAP, THREADS = 2048, 256                          # csrc/optim.hip: AW_MAX_GRID, AW_THREADS
N_WRAP = GRID_CAP * THREADS * 4 + 4 * THREADS + 3      # the grid-stride loop wraps once (one more trip for the first workgroup), scalar tail of 3
SIZES = [1, 3, 4, 63, 64, 65, 4 * 1024 + 1, N_WRAP]
STEPS = 4
H = R.HYPER
NAN = float("nan")
OMR_ERR_ARG = -1                                       # csrc/omr_common.h


def bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8 if t.dtype == torch.uint8 else torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b, what=""):
    assert torch.equal(bits(a), bits(b)), f"{what}: bits differ"


@functools.lru_cache(maxsize=None)
def host_inputs(n):
    """tests/optim_refs.py's inputs for size n (seed n), computed once and never written to."""
    arrays = R.inputs(n, seed=n, steps=STEPS)
    for a in arrays[:4] + tuple(arrays[4]):
        a.setflags(write=False)
    return arrays


def device_state(n, lowp=True):
    p, m, v, ema, grads = host_inputs(n)
    p, m, v, ema = (torch.from_numpy(x.copy()).to(DEV) for x in (p, m, v, ema))
    return dict(p=p, m=m, v=v, ema=ema, lp=p.to(torch.bfloat16) if lowp else None), [torch.from_numpy(g.copy()).to(DEV) for g in grads]


def clone(st):
    return {k: None if t is None else t.clone() for k, t in st.items()}


def new_step(st, g, step, *, ema=False, **kw):
    K.adam_step(st["p"], g, st["m"], st["v"], step, H["lr"], (H["b1"], H["b2"]), H["eps"], R.GRAD_SCALE, p_lowp=st["lp"],
                ema=st["ema"] if ema else None, **kw)


def entry_args(st, g, step):
    """The arguments omr_adam and omr_adam_guarded share, for a call of the C entry itself."""
    return (ptr(st["p"]), ptr(g), ptr(st["m"]), ptr(st["v"]), ptr(st["lp"]), st["p"].numel(), step, H["lr"], H["b1"], H["b2"], H["eps"], R.GRAD_SCALE)


def assert_state_bits(a, b, what, keys=("p", "m", "v", "lp")):
    for k in keys:
        if a[k] is not None:
            same_bits(a[k], b[k], f"{what}: {k}")


def real_ctl(g, max_norm):
    ws = torch.empty(K.grad_norm_workspace_bytes(g.numel(), 1), dtype=torch.uint8, device=DEV)
    ctl = K.new_step_ctl(DEV)
    K.grad_norm(g, [(0, g.numel())], R.GRAD_SCALE, max_norm, ws, ctl)
    return ctl, K.read_step_ctl(ctl.cpu())


# ------------------------------------------------------------------------------------------------ nothing new asked for: omr_adam's bits
@pytest.mark.parametrize("n", SIZES)
def test_plain_is_omr_adam_bit_for_bit(n):
    """weight_decay = 0, ema = NULL, ctl = NULL; three consecutive steps, grad_scale = 0.5, with and without the bf16 copy."""
    for lowp in (True, False):
        a, grads = device_state(n, lowp)
        b = clone(a)
        start = a["p"].clone()
        for j in range(3):
            lib().call("omr_adam", *entry_args(a, grads[j], R.FIRST_STEP + j), cur_stream())
            new_step(b, grads[j], R.FIRST_STEP + j)
            assert_state_bits(a, b, f"n={n} lowp={lowp} step {j}")
        assert not torch.equal(a["p"], start)
        same_bits(b["ema"], torch.from_numpy(host_inputs(n)[3].copy()), "ema is not touched without an ema pointer")


@pytest.mark.parametrize("n", SIZES)
def test_guarded_is_omr_adam_guarded_bit_for_bit(n):
    a, grads = device_state(n)
    b = clone(a)
    norm = float(np.sqrt((host_inputs(n)[4][0].astype(np.float64) ** 2).sum())) * R.GRAD_SCALE
    ctl, rec = real_ctl(grads[0], norm / 10)
    assert rec.apply == 1 and 0.09 < rec.clip < 0.11
    lib().call("omr_adam_guarded", *entry_args(a, grads[0], R.FIRST_STEP), ptr(ctl), cur_stream())
    new_step(b, grads[0], R.FIRST_STEP, ctl=ctl)
    assert_state_bits(a, b, f"n={n}")
    c = clone(device_state(n)[0])
    new_step(c, grads[0], R.FIRST_STEP)
    assert not torch.equal(c["p"], b["p"])                                                   # (the clip did act)


# ------------------------------------------------------------------------------------------------ skip
@pytest.mark.parametrize("n", SIZES)
def test_a_nonfinite_gradient_writes_nothing(n):
    _, grads = device_state(n)
    g = grads[0]
    g[n // 2] = NAN
    ctl, rec = real_ctl(g, 1.0)
    assert rec.apply == 0 and rec.nonfinite == 1
    gen = torch.Generator().manual_seed(n)
    pattern = torch.randint(-2 ** 31, 2 ** 31 - 1, (5, n), generator=gen, dtype=torch.int64).to(torch.int32)     # any bits, NaN patterns included
    st = dict(p=pattern[0].view(torch.float32).to(DEV), m=pattern[1].view(torch.float32).to(DEV), v=pattern[2].view(torch.float32).to(DEV),
              ema=pattern[3].view(torch.float32).to(DEV), lp=pattern[4].to(torch.int16).view(torch.bfloat16).to(DEV))
    before = clone(st)
    blocks = torch.from_numpy(R.block_mask(n)[0]).to(DEV)
    new_step(st, g, R.FIRST_STEP, ema=True, ema_decay=R.f32(0.9), weight_decay=R.WD, decay_blocks=blocks, ctl=ctl)
    assert_state_bits(st, before, f"n={n}", keys=("p", "m", "v", "lp", "ema"))


# ------------------------------------------------------------------------------------------------ decay
@pytest.mark.parametrize("n", [65, 4 * 1024 + 1, N_WRAP])
def test_decay_follows_the_block_map(n):
    """Alternating blocks, the last one partial: blocks marked 0 keep the weight_decay = 0 bits, blocks marked 1 follow the fp64
    restatement inside the bound and differ from the undecayed run.  One step and STEPS steps."""
    blocks_h, mask_h = R.block_mask(n)
    assert n % 64 and blocks_h[-1] in (0, 1) and blocks_h[:2].tolist() == [1, 0]
    blocks, mask = torch.from_numpy(blocks_h).to(DEV), torch.from_numpy(mask_h)
    p, m, v, ema, grads_h = host_inputs(n)
    dec, grads = device_state(n)
    und = clone(dec)
    every = clone(dec)
    for j in range(STEPS):
        new_step(dec, grads[j], R.FIRST_STEP + j, weight_decay=R.WD, decay_blocks=blocks)
        new_step(und, grads[j], R.FIRST_STEP + j)
        new_step(every, grads[j], R.FIRST_STEP + j, weight_decay=R.WD)                       # decay_blocks = NULL: every element decays
        if j == 0:
            first = clone(dec)
    for k in ("p", "lp"):
        a, b, c = dec[k].cpu(), und[k].cpu(), every[k].cpu()
        same_bits(a[~mask], b[~mask], f"n={n}: {k} of the blocks marked 0")
        same_bits(a[mask], c[mask], f"n={n}: {k} of the blocks marked 1 against the NULL map")
    assert (dec["p"].cpu()[mask] != und["p"].cpu()[mask]).all()
    for k in ("m", "v"):
        same_bits(dec[k], und[k], f"n={n}: {k} does not see the decay")
    for steps, got in ((1, first), (STEPS, dec)):
        ref, pb, _ = R.ref_run(p, m, v, None, grads_h[:steps], R.FIRST_STEP, **H, wd=R.WD, decay_mask=mask_h, grad_scale=R.GRAD_SCALE)
        err = np.abs(got["p"].cpu().numpy().astype(np.float64) - ref[0])
        print(f"n={n} steps={steps}: p err / bound max {float(np.max(err / pb)):.3f}")
        assert (err <= pb).all()
        same_bits(got["lp"], got["p"].to(torch.bfloat16), "the bf16 copy is the rounded new p")


# ------------------------------------------------------------------------------------------------ EMA
@pytest.mark.parametrize("n", SIZES)
def test_ema_edges_are_exact(n):
    st, grads = device_state(n)
    ema0 = st["ema"].clone()
    zero, one = clone(st), clone(st)
    new_step(zero, grads[0], R.FIRST_STEP, ema=True, ema_decay=0.0)
    same_bits(zero["ema"], zero["p"], f"n={n}: ema_decay = 0 leaves the new p")
    assert not torch.equal(zero["ema"], ema0)
    new_step(one, grads[0], R.FIRST_STEP, ema=True, ema_decay=1.0)
    same_bits(one["ema"], ema0, f"n={n}: ema_decay = 1 leaves ema")
    assert_state_bits(zero, one, f"n={n}: the EMA does not change the step")
    plain = clone(st)
    new_step(plain, grads[0], R.FIRST_STEP)
    assert_state_bits(zero, plain, f"n={n}: ... nor does the ema pointer")


@pytest.mark.parametrize("d", [0.9, 0.999])
@pytest.mark.parametrize("n", [63, 4 * 1024 + 1, N_WRAP])
def test_ema_values_against_fp64(n, d):
    """Four steps with decay on alternating blocks and the EMA, as tests/test_optim_refs_cpu.py runs them on the host."""
    d = R.f32(d)
    blocks_h, mask_h = R.block_mask(n)
    blocks = torch.from_numpy(blocks_h).to(DEV)
    p, m, v, ema, grads_h = host_inputs(n)
    runs = []
    for _ in range(2):
        st, grads = device_state(n)
        for j in range(STEPS):
            new_step(st, grads[j], R.FIRST_STEP + j, ema=True, ema_decay=d, weight_decay=R.WD, decay_blocks=blocks)
        runs.append(st)
    assert_state_bits(runs[0], runs[1], f"n={n} d={d}: two runs", keys=("p", "m", "v", "lp", "ema"))
    ref, pb, eb = R.ref_run(p, m, v, ema, grads_h, R.FIRST_STEP, **H, wd=R.WD, decay_mask=mask_h, ema_decay=d, grad_scale=R.GRAD_SCALE)
    perr = np.abs(runs[0]["p"].cpu().numpy().astype(np.float64) - ref[0])
    eerr = np.abs(runs[0]["ema"].cpu().numpy().astype(np.float64) - ref[3])
    print(f"n={n} d={d}: p err / bound max {float(np.max(perr / pb)):.3f}, ema err / bound max {float(np.max(eerr / eb)):.3f}")
    assert (perr <= pb).all() and (eerr <= eb).all()
    assert (np.abs(ref[3] - ema.astype(np.float64)) > eb).mean() > 0.9                         # the average moved by more than the bound


# ------------------------------------------------------------------------------------------------ arguments
def test_adamw_ema_refuses_bad_arguments():
    st, grads = device_state(65)
    wide = {k: None if t is None else torch.cat([t, t]) for k, t in st.items()}
    g2 = torch.cat([grads[0], grads[0]])
    args = (H["lr"], (H["b1"], H["b2"]), H["eps"])
    for off in ("p", "m", "v", "ema", "lp"):                         # one pointer one element off a 16-byte boundary
        t = {k: (x[1:65] if k == off else x[:64]) for k, x in wide.items()}
        with pytest.raises(RuntimeError, match="invalid argument"):
            K.adam_step(t["p"], g2[:64], t["m"], t["v"], 1, *args, p_lowp=t["lp"], ema=t["ema"], ema_decay=0.5)
    with pytest.raises(RuntimeError, match="invalid argument"):
        K.adam_step(st["p"][:64], g2[1:65], st["m"][:64], st["v"][:64], 1, *args)
    with pytest.raises(RuntimeError, match="invalid argument"):
        K.adam_step(st["p"], grads[0], st["m"], st["v"], 0, *args)                      # steps are 1-based
    for bad in (-0.1, 1.5, NAN):
        with pytest.raises(RuntimeError, match="invalid argument"):
            K.adam_step(st["p"], grads[0], st["m"], st["v"], 1, *args, ema=st["ema"], ema_decay=bad)
    before = clone(st)
    torch.cuda.synchronize()
    assert_state_bits(st, before, "a refused call launches nothing", keys=("p", "m", "v", "lp", "ema"))


def test_adam_entries_refuse_a_misaligned_gradient():
    """omr_adam and omr_adam_guarded keep omr_adamw_ema's contract: g one element off a 16-byte boundary is OMR_ERR_ARG, nothing runs."""
    st, grads = device_state(65)
    g2 = torch.cat([grads[0], grads[0]])
    ctl, rec = real_ctl(grads[0], None)
    assert rec.apply == 1
    before = clone(st)
    part = {k: t[:64] for k, t in st.items()}
    assert lib().query("omr_adam", *entry_args(part, g2[1:65], 1), cur_stream()) == OMR_ERR_ARG
    assert lib().query("omr_adam_guarded", *entry_args(part, g2[1:65], 1), ptr(ctl), cur_stream()) == OMR_ERR_ARG
    assert lib().query("omr_adam_guarded", *entry_args(part, g2[:64], 1), None, cur_stream()) == OMR_ERR_ARG      # and still no NULL record
    torch.cuda.synchronize()
    assert_state_bits(st, before, "a refused call launches nothing", keys=("p", "m", "v", "lp", "ema"))


# ------------------------------------------------------------------------------------------------ omr_swap_f32
@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_exactly(n):
    gen = torch.Generator().manual_seed(n)
    a0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32)
    b0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32)
    pad = 8
    a, b = torch.zeros(n + pad, device=DEV), torch.zeros(n + pad, device=DEV)                  # the elements behind n must stay zero
    a[:n], b[:n] = a0.to(DEV), b0.to(DEV)
    K.swap_f32(a[:n], b[:n])
    same_bits(a[:n], b0, "a holds b")
    same_bits(b[:n], a0, "b holds a")
    assert not a[n:].any() and not b[n:].any()
    K.swap_f32(a[:n], b[:n])
    same_bits(a[:n], a0, "and back")
    same_bits(b[:n], b0, "and back")


def test_swap_refuses_misaligned_and_overlapping():
    buf = torch.arange(64, dtype=torch.float32, device=DEV)
    other = torch.zeros(64, device=DEV)
    for a, b in ((buf[1:9], other[0:8]), (other[0:8], buf[1:9]),            # 4 bytes off a 16-byte boundary
                 (buf[0:8], buf[4:12]), (buf[4:12], buf[0:8]), (buf[0:8], buf[0:8])):      # aligned, but the ranges overlap
        with pytest.raises(RuntimeError, match="invalid argument"):
            K.swap_f32(a, b)
    K.swap_f32(buf[0:8], buf[8:16])                                         # neighbours do not overlap
    torch.cuda.synchronize()
    assert buf[:16].tolist() == [float(i) for i in list(range(8, 16)) + list(range(8))] and not other.any()
