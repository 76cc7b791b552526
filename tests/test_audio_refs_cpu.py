"""CPU-only: the audio front end's case tables (tests/audio_refs.py) with torch CPU fp32 arithmetic standing in for the kernels.

Every check tests/test_audio_branches_gpu.py makes on the device is made here on `post_standin` / `stft_standin` /
`resample_standin`.  A correct implementation meets every check; each damaged one is rejected by the case named next to it.
Also here: the fp32 basis against the fp64 periodic-Hann basis, the resampling plan against its restatement, the plan-size
refusal."""
import numpy as np
import pytest
import torch

import audio_refs as R


def _basis32():
    from omr_a2s_multimodal_transformer_amd import audio
    return audio._basis("cpu").numpy()


def _plan(case):
    from omr_a2s_multimodal_transformer_amd import audio
    up, down = R.up_down(case[0], case[1])
    if up == down:
        return None
    H, lo, g = audio._resample_plan(up, down, "cpu")
    return H.numpy(), lo, g


# ------------------------------------------------------------------------------------------------ post-processing alone
@pytest.mark.parametrize("case", R.POST_CASES, ids=lambda c: c.name)
def test_a_correct_post_meets_every_check(case):
    before = R.post_spec(case)
    after, out, _ = R.post_standin(before)
    assert R.post_check(before, after, out, who=f"cpu {case.name}") <= 1.0
    again = R.post_standin(before)
    assert np.array_equal(R.bits(out), R.bits(again[1]))


def test_the_post_table_reaches_what_it_names():
    c = R.POST["post-wrap"]
    assert c.frames * c.bins == 524550 and c.frames * c.bins - R.SWEEP == 262
    before = R.post_spec(c)
    m = R.post_mag_ref(before)
    assert int(np.argmax(m)) == m.size - 1 and m.reshape(-1)[-1] == 1000.0 and np.sort(m.reshape(-1))[-2] < 950.0
    at_floor, under_amin = R.post_floor_fractions(before)
    print(f"post-wrap: {at_floor:.3%} at the floor, {under_amin:.3%} under amin")
    assert at_floor >= 0.05 and under_amin >= 0.01
    # both sweeps hold elements of every kind: at the floor, above it, under amin -- in pass 1's order and in pass 2's
    box = R.db_box(m, m)
    for flat in (box.zero.reshape(-1), box.zero.T.reshape(-1)):
        assert flat[R.SWEEP:].any() and not flat[R.SWEEP:].all()
    t = R.POST["post-tiny"]
    assert t.frames * t.bins < 256 and t.bins != 195
    u = R.post_mag_ref(R.post_spec(R.POST["post-under-amin"]))
    assert u.min() >= 1e-7 and u.max() <= 9e-6 * (1 + 1e-6)
    assert not R.post_spec(R.POST["post-silent"]).any()


def test_dirty_workspace_second_run_is_judged_on_its_own_maximum():
    loud = R.post_spec(R.DIRTY_LOUD)
    quiet = (loud * np.float32(1e-3)).astype(np.float32)
    _, _, ws = R.post_standin(loud, ws=-1)
    after, out, _ = R.post_standin(quiet, ws=ws)
    assert R.post_check(quiet, after, out, who="cpu post-dirty-ws") <= 1.0


POST_DAMAGED = [
    # (damage, the case that rejects it)
    ("max_first_sweep", "post-wrap"),            # the unique maximum is the last element, in the second sweep
    ("db_second_sweep_dropped", "post-wrap"),
    ("amin_1e-10", "post-under-amin"),
    ("amin_1e-10", "post-quiet"),
    ("amin_1e-4", "post-quiet"),                 # post-wrap's floor (0.1) hides amin altogether: this case's floor is under it
    ("clamp_absolute", "post-wrap"),
    ("clamp_absolute", "post-tiny"),
    ("natural_log", "post-wrap"),
    ("natural_log", "post-one"),
]


@pytest.mark.parametrize("damage,name", POST_DAMAGED, ids=[f"{d}-{n}" for d, n in POST_DAMAGED])
def test_a_damaged_post_is_rejected(damage, name):
    before = R.post_spec(R.POST[name])
    after, out, _ = R.post_standin(before, damage)
    with pytest.raises(AssertionError):
        R.post_check(before, after, out, who=f"cpu {damage} {name}")


def test_the_sweep_damages_are_invisible_below_one_sweep():
    """post-one has 195 elements: no second sweep, so losing it changes nothing -- post-wrap is what reaches it."""
    before = R.post_spec(R.POST["post-one"])
    for damage in ("max_first_sweep", "db_second_sweep_dropped"):
        assert np.array_equal(R.bits(R.post_standin(before, damage)[1]), R.bits(R.post_standin(before)[1]))


def test_a_stale_maximum_is_rejected_by_the_dirty_workspace_case():
    loud = R.post_spec(R.DIRTY_LOUD)
    quiet = (loud * np.float32(1e-3)).astype(np.float32)
    _, _, ws = R.post_standin(loud, "stale_max", ws=0)
    after, out, _ = R.post_standin(quiet, "stale_max", ws=ws)
    with pytest.raises(AssertionError):
        R.post_check(quiet, after, out, who="cpu stale_max post-dirty-ws")
    after, out, _ = R.post_standin(loud, "stale_max", ws=-1)             # 0xFFFFFFFF is a NaN: without the memset nothing survives it
    with pytest.raises(AssertionError):
        R.post_check(loud, after, out, who="cpu stale_max on 0xFFFFFFFF")


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_non_finite_magnitudes(kind):
    spec, where = R.nonfinite_specs()[kind]
    R.nonfinite_check(kind, where, R.post_standin(spec)[1], who=f"cpu {kind}")
    if kind == "nan":                                                   # the parent's kernels: fmaxf drops the NaN in both passes
        with pytest.raises(AssertionError):
            R.nonfinite_check(kind, where, R.post_standin(spec, "nan_dropped")[1], who="cpu nan_dropped")
        m = np.maximum(1e-5, R.post_mag_ref(spec))                      # numpy's own semantics, the oracle's: maximum and max keep the NaN
        assert np.isnan(m.max()) and np.isnan(np.maximum(20 * np.log10(m) - 20 * np.log10(m.max()), -80.0)).all()


def test_a_nan_sample_end_to_end():
    y = R.stft_signal(R.STFT["impulses-five"])
    y[1500] = np.nan
    assert torch.isnan(R.stft_standin(y)).all()
    from oracle import ref_cpu
    assert np.isnan(ref_cpu.log_stft(y)).all()


# ------------------------------------------------------------------------------------------------ log_stft end to end
def test_the_fp32_basis_is_one_rounding_of_the_periodic_hann_basis():
    r = R.basis_check(_basis32())
    print(f"basis: largest |b32 - b64| / (u |b64|) = {r:.4f}")
    assert r <= 1.0
    sym = R.basis64(symmetric=True).astype(np.float32)
    assert R.basis_check(sym) > 100.0


@pytest.mark.parametrize("case", R.STFT_CASES, ids=lambda c: c.name)
def test_a_correct_log_stft_meets_every_check(case):
    out = R.stft_standin(R.stft_signal(case))
    assert R.stft_check(case, out, _basis32(), who=f"cpu {case.name}") <= 1.0
    if case.all_one:
        assert bool((out == 1.0).all())


def test_the_stft_table_reaches_what_it_names():
    b = _basis32()
    frames = lambda name: R.stft_frames(R.stft_signal(R.STFT[name]))
    a = frames("impulse-mid")
    assert a.shape == (7, 2048) and [int(np.flatnonzero(r)[0]) if r.any() else -1 for r in a] == [-1, 1540, 1028, 516, 4, -1, -1]
    box = R.db_box(*R.stft_mag_box(R.stft_signal(R.STFT["impulse-mid"]), b)[:2])
    assert [bool(box.zero[f].all()) for f in range(7)] == [True, False, False, False, True, True, True]      # 4 of 7 frames exactly 0.0
    a = frames("impulse-edge")
    assert [int(np.flatnonzero(r)[0]) if r.any() else -1 for r in a] == [1028, 516, 4, -1, -1, -1, -1]
    box = R.db_box(*R.stft_mag_box(R.stft_signal(R.STFT["impulse-edge"]), b)[:2])
    assert box.zero[2].all() and not box.zero[:2].any()                 # window index 4: under the floor, so the clamp is reached
    m_lo, m_hi, k_eff = R.stft_mag_box(R.stft_signal(R.STFT["impulses-five"]), b)
    assert k_eff == 3 and (m_hi[6] > 0).all()                           # the last frame carries the sample at 3171
    assert np.ptp(m_lo[1]) > 0.1                                        # interference: the magnitudes differ across bins
    for name, f in (("n0", 1), ("n1", 1), ("n511", 1), ("n512", 2), ("silent-5000", 10), ("amplitude-1e-9", 10)):
        assert 1 + R.STFT[name].n // 512 == f


STFT_DAMAGED = [
    ("symmetric_hann", "impulse-mid"),           # the impulse sits on window index 1540 / 1028 / 516: the frames' ratio is the window's
    ("no_centre_padding", "impulse-mid"),
    ("no_centre_padding", "impulse-edge"),
    ("hop_511", "impulse-mid"),
    ("hop_511", "impulses-five"),
    ("last_frame_dropped", "impulses-five"),     # only this case has a sample in the last frame
    ("not_transposed", "impulses-five"),
    ("not_transposed", "impulse-edge"),
]


@pytest.mark.parametrize("damage,name", STFT_DAMAGED, ids=[f"{d}-{n}" for d, n in STFT_DAMAGED])
def test_a_damaged_log_stft_is_rejected(damage, name):
    case = R.STFT[name]
    out = R.stft_standin(R.stft_signal(case), damage)
    with pytest.raises(AssertionError):
        R.stft_check(case, out, _basis32(), who=f"cpu {damage} {name}")


def test_a_dropped_last_frame_is_invisible_where_it_is_silent():
    y = R.stft_signal(R.STFT["impulse-mid"])
    assert torch.equal(R.stft_standin(y, "last_frame_dropped"), R.stft_standin(y))


# ------------------------------------------------------------------------------------------------ resampler
@pytest.mark.parametrize("case", R.RESAMPLE_CASES, ids=R.resample_id)
def test_the_plan_times_the_frames_meets_the_resampler_bound(case):
    plan = _plan(case)
    k_pad = plan[0].shape[1] if plan else 0
    assert R.resample_check(case, R.resample_standin(case, plan), k_pad, who="cpu") <= 1.0


def test_the_resampler_table_reaches_what_it_names():
    shape = {}
    for case in R.RESAMPLE_CASES:
        plan = _plan(case)
        if plan is None:
            continue
        (H, lo, g), (up, down) = plan, R.up_down(case[0], case[1])
        n_out = -(-case[2] * up // down)
        shape[R.resample_id(case)] = (g, H.shape[0], H.shape[1], -(-n_out // H.shape[0]), n_out)
        assert lo % 4 == 0 and (g * down) % 4 == 0 and H.shape[1] % 8 == 0
    assert shape["11025-22050-n301"] == (4, 8, 32, 76, 602)
    assert shape["11025-22050-n4"][3:] == (1, 8) and shape["11025-22050-n5"][3:] == (2, 10)
    assert shape["66150-22050-n50"][:2] == (4, 4)
    assert shape["22050-16000-n1500"] == (4, 1280, 1800, 1, 1089)
    assert shape["44100-22050-n1"][4] == 1 and shape["44100-22050-n2"][4] == 1 and shape["16000-22050-n1"][4] == 2
    for case in R.RESAMPLE_CASES:                                       # the frame stride g * down is the GEMM's lda: under K everywhere
        if R.resample_id(case) in shape:
            assert shape[R.resample_id(case)][0] * R.up_down(case[0], case[1])[1] < shape[R.resample_id(case)][2]


@pytest.mark.parametrize("case", [c for c in R.RESAMPLE_CASES if c[0] != c[1]], ids=R.resample_id)
def test_the_plan_equals_its_restatement(case):
    up, down = R.up_down(case[0], case[1])
    H, lo, g = _plan(case)
    H2, lo2, g2 = R.plan_restated(up, down)
    assert (lo, g) == (lo2, g2) and H.dtype == np.float32 and np.array_equal(H, H2.astype(np.float32))


RESAMPLE_DAMAGED = [
    ("phase_plus_one", (11025, 22050, 301)),
    ("phase_plus_one", (44100, 22050, 2)),
    ("phase_plus_one", (22050, 16000, 1500)),
    ("lo_not_rounded", (11025, 22050, 301)),
    ("lo_not_rounded", (24000, 22050, 1000)),
    ("last_row_dropped", (11025, 22050, 5)),
    ("last_row_dropped", (11025, 22050, 4)),
    ("last_row_dropped", (44100, 22050, 1)),
]


@pytest.mark.parametrize("damage,case", RESAMPLE_DAMAGED, ids=[f"{d}-{R.resample_id(c)}" for d, c in RESAMPLE_DAMAGED])
def test_a_damaged_resampler_is_rejected(damage, case):
    up, down = R.up_down(case[0], case[1])
    plan = R.plan_restated(up, down, damage if damage != "last_row_dropped" else None)
    if damage == "lo_not_rounded":
        assert plan[1] != -((len(R.ref_cpu.resample_filter(up, down)[0]) - 1 - R.ref_cpu.resample_filter(up, down)[1] * down) // up), "this ratio's first tap is aligned already"
    out = R.resample_standin(case, plan, damage)
    with pytest.raises(AssertionError):
        R.resample_check(case, out, plan[0].shape[1], who=f"cpu {damage}")


def test_an_oversized_plan_is_refused_before_it_is_built():
    import time
    from omr_a2s_multimodal_transformer_amd import audio
    t0 = time.perf_counter()
    with pytest.raises(ValueError):
        audio._resample_plan(22050, 22051, "cpu")
    assert time.perf_counter() - t0 < 5.0
    for orig, target in sorted({c[:2] for c in R.RESAMPLE_CASES if c[0] != c[1]} | {(32000, 22050)}):
        up, down = R.up_down(orig, target)
        H, _, _ = audio._resample_plan(up, down, "cpu")
        assert H.numel() <= audio.MAX_PLAN_ENTRIES
    assert tuple(audio._resample_plan(441, 640, "cpu")[0].shape) == (441, 672)
