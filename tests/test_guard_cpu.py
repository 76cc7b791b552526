"""CPU-only: the guarded optimizer step's argument checks (nothing is launched), the record's layout, the host bookkeeping of
the lagged apply / skip decision (params.StepLedger, scripted) and the Trainer's arguments."""
import ctypes

import pytest
import torch
import torch.nn as nn

from omr_a2s_multimodal_transformer_amd import _lib
from omr_a2s_multimodal_transformer_amd import kernels as K
from omr_a2s_multimodal_transformer_amd.params import FlatParams, FusedAdam, StepLedger

ERR_ARG = -1


def _grad_norm(n, ranges, g=True, ws=True, ctl=True):
    """omr_grad_norm on HOST memory: every call here has to be refused before the first launch (there is no GPU)."""
    nr = len(ranges)
    raw = (ctypes.c_char * (4 * max(n, 4) + 1024 + 256 + 64))()           # g | ws | ctl, each 16-byte aligned: only the case under test is wrong
    base = (ctypes.addressof(raw) + 15) // 16 * 16
    buf, work, rec = base, base + 4 * max(n, 4), base + 4 * max(n, 4) + 1024
    begins = (ctypes.c_long * max(nr, 1))(*[b for b, _ in ranges])
    ends = (ctypes.c_long * max(nr, 1))(*[e for _, e in ranges])
    return _lib.lib().fns["omr_grad_norm"](buf if g else None, n, begins, ends, nr, 1.0, 0.0, work if ws else None, rec if ctl else None, None)


@pytest.mark.parametrize("what,n,ranges", [
    ("0 ranges", 64, []),
    ("17 ranges", 17 * 8, [(8 * i, 8 * i + 4) for i in range(17)]),
    ("unsorted", 64, [(32, 48), (0, 16)]),
    ("overlapping", 64, [(0, 20), (16, 32)]),
    ("end past n", 64, [(0, 16), (32, 68)]),
    ("begin not a multiple of 4", 64, [(0, 16), (18, 32)]),
    ("empty range", 64, [(16, 16)]),
    ("negative begin", 64, [(-4, 16)]),
])
def test_grad_norm_refuses_bad_ranges_before_any_launch(what, n, ranges):
    assert _grad_norm(n, ranges) == ERR_ARG, what


def test_grad_norm_refuses_null_pointers_and_empty_buffers():
    ok = [(0, 16), (32, 64)]
    assert _grad_norm(64, ok, ctl=False) == ERR_ARG
    assert _grad_norm(64, ok, ws=False) == ERR_ARG
    assert _grad_norm(64, ok, g=False) == ERR_ARG
    assert _grad_norm(0, [(0, 4)]) == ERR_ARG


def test_workspace_size_is_monotone_and_checks_its_arguments():
    q = _lib.lib().query
    chunk = K.GRAD_NORM_CHUNK
    sizes = [q("omr_grad_norm_workspace_bytes", n, 3) for n in (1, 4, chunk - 4, chunk, chunk + 4, 3 * chunk + 20, 10 ** 7, 2 ** 31 + 8)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # room for every slot whatever the ranges are: sum over ranges of ceil(len / chunk) <= n / chunk + n_ranges, 16 bytes each
    for n, nr in ((4, 1), (chunk + 4, 1), (3 * chunk + 20, 16), (64 * 16, 16)):
        assert q("omr_grad_norm_workspace_bytes", n, nr) >= 16 * (n // chunk + nr)
    for nr in (0, 17, -1):
        assert q("omr_grad_norm_workspace_bytes", 1024, nr) == ERR_ARG
    assert q("omr_grad_norm_workspace_bytes", 0, 1) == ERR_ARG
    assert all(q("omr_grad_norm_workspace_bytes", 1024, nr) > 0 for nr in (1, 16))
    with pytest.raises(RuntimeError):
        K.grad_norm_workspace_bytes(1024, 17)


def test_step_ctl_mirror_has_the_c_layout():
    """sizeof(omr_step_ctl) = double + 2 float + 2 int + 16 double, no padding; the field offsets of the header's struct."""
    assert ctypes.sizeof(K.StepCtl) == 8 + 4 + 4 + 4 + 4 + 16 * 8 == 152
    offs = {f: getattr(K.StepCtl, f).offset for f, _ in K.StepCtl._fields_}
    assert offs == dict(sumsq=0, norm=8, clip=12, apply=16, nonfinite=20, range_sumsq=24)
    import re
    text = open(_lib.HEADER).read()
    body = re.search(r"typedef struct omr_step_ctl \{(.*?)\} omr_step_ctl;", text, flags=re.S).group(1)
    assert [" ".join(s.split()) for s in body.strip().split(";") if s.strip()] == [
        "double sumsq", "float norm, clip", "int apply, nonfinite", "double range_sumsq[16]"]
    assert K.new_step_ctl("cpu").numel() == 152


def test_constants_come_from_the_header():
    assert K.GRAD_NORM_CHUNK == 256 * K.GRAD_NORM_K and K.GRAD_NORM_K % 4 == 0 and K.GRAD_NORM_MAX_RANGES == 16
    assert K.DECAY_BLOCK == _lib.header_constant("OMR_ADAM_DECAY_BLOCK") == 64
    protos = _lib.parse_header()
    assert protos["omr_adam_guarded"][1][:12] == protos["omr_adam"][1][:12]         # omr_adam's arguments, then the record
    assert protos["omr_adam_guarded"][1][12:] == ["const omr_step_ctl* ctl", "void* stream"]
    assert _lib.lib().query("omr_abi_version") == 2


# ---------------------------------------------------------------------------------------------------------------- bookkeeping
ALL = ("encoder", "decoder")


def _run(ledger, script):
    """script: [(touched names, applied)] -> (counts the launches of each step read, counts after each record was settled).
    The order of FusedAdam.step: settle the previous step, count this one, launch; the last record is settled on demand."""
    launched, settled = [], []
    prev = None
    for names, applied in script:
        if prev is not None:
            ledger.settle(*prev)
            settled.append(dict(ledger.steps))
        k = ledger.count(names)
        launched.append({n: ledger.steps[n] for n in names})
        prev = (k, applied)
    ledger.settle(*prev)
    settled.append(dict(ledger.steps))
    return launched, settled


def test_ledger_applied_skipped_applied_applied():
    """Every sub-module touched; the second step is skipped on the device.  The counts that hold once each step's record is in
    are 1, 1, 2, 3.  At launch time the skipped step itself was (tentatively, harmlessly: it wrote nothing) launched with 2;
    every APPLIED step is launched with its exact count 1, 2, 3 -- that is what the bias corrections need."""
    led = StepLedger(ALL)
    launched, settled = _run(led, [(ALL, True), (ALL, False), (ALL, True), (ALL, True)])
    assert [s["encoder"] for s in settled] == [s["decoder"] for s in settled] == [1, 1, 2, 3]
    assert [l["decoder"] for l in launched] == [1, 2, 2, 3]
    assert [l["decoder"] for l, applied in zip(launched, (True, False, True, True)) if applied] == [1, 2, 3]
    assert led.skipped == 1 and led.issued == 4 and led.open is None


def test_ledger_takes_a_skipped_modality_drop_step_back_from_its_own_sub_modules():
    names = ("image_encoder", "audio_encoder", "cross_attn", "decoder")
    led = StepLedger(names)
    audio = ("audio_encoder", "decoder")
    image = ("image_encoder", "decoder")
    launched, settled = _run(led, [(names, True), (audio, False), (image, True), (audio, True), (names, True)])
    assert settled[1] == dict(image_encoder=1, audio_encoder=1, cross_attn=1, decoder=1)         # the skipped step: nothing counted
    assert launched[2] == dict(image_encoder=2, decoder=2)                                          # exact for the next applied step
    assert launched[3] == dict(audio_encoder=2, decoder=3)
    assert led.steps == dict(image_encoder=3, audio_encoder=3, cross_attn=2, decoder=4) and led.skipped == 1


def test_ledger_settle_is_idempotent_and_one_step_is_open_at_most():
    led = StepLedger(ALL)
    k = led.count(ALL)
    assert led.open == k == 0
    with pytest.raises(RuntimeError):
        led.count(ALL)
    led.settle(k, False)
    led.settle(k, False)
    led.settle(k, True)
    led.settle(k + 5, False)
    assert led.steps == dict(encoder=0, decoder=0) and led.skipped == 1 and led.open is None
    k = led.count(("decoder",))
    led.settle(k - 1, False)            # an older record again: the open step is not touched
    assert led.open == k and led.steps == dict(encoder=0, decoder=1)
    led.settle(k, True)
    led.settle(k, False)
    assert led.steps == dict(encoder=0, decoder=1) and led.skipped == 1


def _cpu_optimizer():
    torch.manual_seed(0)
    mods = nn.ModuleDict(dict(encoder=nn.Linear(5, 7), decoder=nn.Linear(7, 3)))
    flat = FlatParams(list(mods.named_parameters()), torch.device("cpu"), torch.float32)
    return FusedAdam(flat)


def test_state_dict_round_trips_skipped_and_accepts_the_unguarded_form():
    opt = _cpu_optimizer()
    assert "skipped" not in opt.state_dict() and opt.skipped == 0
    opt.enable_guard(max_norm=1.0)
    led = opt._ledger
    for applied in (True, False, True):
        led.settle(led.count(ALL), applied)
    sd = opt.state_dict()
    assert sd["skipped"] == 1 and sd["steps"] == dict(encoder=2, decoder=2) and sd["step"] == 2
    other = _cpu_optimizer()
    other.enable_guard(skip_nonfinite=True)
    other.load_state_dict(sd)
    assert other.skipped == 1 and other.steps == dict(encoder=2, decoder=2) and other.state_dict()["skipped"] == 1
    plain = _cpu_optimizer().state_dict()                   # the form without `skipped`
    other.load_state_dict(plain)
    assert other.skipped == 0 and other.step_count == 0
    unguarded = _cpu_optimizer()
    unguarded.load_state_dict(sd)                           # and the guarded form into an optimizer without a guard
    assert unguarded.steps == dict(encoder=2, decoder=2) and "skipped" not in unguarded.state_dict()
    opt.disable_guard()
    assert "skipped" not in opt.state_dict() and opt.steps == dict(encoder=2, decoder=2)


def test_enable_guard_checks_its_arguments():
    opt = _cpu_optimizer()
    with pytest.raises(ValueError):
        opt.enable_guard(max_norm=None, skip_nonfinite=False)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            opt.enable_guard(max_norm=bad)
    assert opt._guard is None and opt.last_grad_norm is None and opt.last_range_norms is None


def test_trainer_arguments():
    from omr_a2s_multimodal_transformer_amd.lightning_shim import Trainer
    with pytest.raises(ValueError, match="norm"):
        Trainer(gradient_clip_algorithm="value", gradient_clip_val=1.0)
    t = Trainer(gradient_clip_val=1.0)
    assert t.gradient_clip_val == 1.0 and not t.skip_nonfinite
    t = Trainer(max_epochs=2)
    assert t.gradient_clip_val is None and not t.skip_nonfinite                      # the defaults: fit() as before
    assert Trainer(gradient_clip_val=0).gradient_clip_val is None                    # Lightning: 0 means no clipping
    assert Trainer(skip_nonfinite=True, gradient_clip_algorithm="norm").skip_nonfinite
