"""Branch-level tests of the audio front end on the device: `stft_mag_max_kernel` / `stft_db_kernel` behind `omr_log_stft_post`
(csrc/elementwise.hip), `audio.log_stft` and `audio.resample_poly` (one fp32 GEMM each over strided, overlapping rows), against
the fp64 references and interval checks of tests/audio_refs.py (derivation: DESIGN.md, "Audio front end coverage").  Every test
prints its largest error / bound ratio before it asserts <= 1; exactly determined values are compared bit for bit.
tests/test_audio_refs_cpu.py runs the same tables with torch CPU arithmetic and shows which wrong kernels these checks see."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import audio_refs as R  # noqa: E402
from omr_a2s_multimodal_transformer_amd import audio  # noqa: E402
from omr_a2s_multimodal_transformer_amd._lib import cur_stream, lib, ptr  # noqa: E402

DEV = "cuda:0"
DIRTY = -1                                                               # 0xFFFFFFFF in the maximum workspace before the call


def run_post(before: np.ndarray, ws: torch.Tensor = None):
    """omr_log_stft_post on a copy of `before` with a sentinel row behind spec and behind out, the workspace holding DIRTY unless
    one is passed in.  -> (spec after, out [bins, frames]) as numpy, after checking both sentinel rows."""
    f, b = before.shape[0], before.shape[1] // 2
    spec = torch.full((f + 1, 2 * b), R.SENTINEL, dtype=torch.float32, device=DEV)
    spec[:f] = torch.from_numpy(before).to(DEV)
    out = torch.full((b + 1, f), R.SENTINEL, dtype=torch.float32, device=DEV)
    if ws is None:
        ws = torch.full((1,), DIRTY, dtype=torch.int32, device=DEV)
    lib().call("omr_log_stft_post", ptr(spec), f, b, ptr(ws), ptr(out), cur_stream())
    spec, out = spec.cpu().numpy(), out.cpu().numpy()
    assert (spec[f] == np.float32(R.SENTINEL)).all() and (out[b] == np.float32(R.SENTINEL)).all(), "written past the end of spec or out"
    return spec[:f], out[:b]


@pytest.mark.parametrize("case", R.POST_CASES, ids=lambda c: c.name)
def test_post(case):
    before = R.post_spec(case)
    after, out = run_post(before)
    assert R.post_check(before, after, out, who=f"gpu {case.name}") <= 1.0
    if case.name == "post-wrap":
        at_floor, under_amin = R.post_floor_fractions(before)
        assert at_floor >= 0.05 and under_amin >= 0.01
    after2, out2 = run_post(before)                                       # the atomic maximum is order-independent
    assert np.array_equal(R.bits(out), R.bits(out2)) and np.array_equal(R.bits(after), R.bits(after2)), "two runs differ"


def test_post_dirty_workspace():
    """A loud spec, then one 60 dB quieter on the same workspace, which starts as 0xFFFFFFFF: each is judged on its own maximum."""
    loud = R.post_spec(R.DIRTY_LOUD)
    quiet = (loud * np.float32(1e-3)).astype(np.float32)
    ws = torch.full((1,), DIRTY, dtype=torch.int32, device=DEV)
    after, out = run_post(loud, ws)
    r1 = R.post_check(loud, after, out, who="gpu post-dirty-ws loud")
    assert int(ws.cpu()) == int(np.float32(1000.0).view(np.int32)), "the workspace holds the maximum's bits"
    after, out = run_post(quiet, ws)
    r2 = R.post_check(quiet, after, out, who="gpu post-dirty-ws quiet")
    assert max(r1, r2) <= 1.0


@pytest.mark.parametrize("what", ["frames-0", "frames-neg", "bins-0", "bins-neg", "null-spec", "null-ws", "null-out"])
def test_post_refusals(what):
    f, b = 3, 7
    spec = torch.full((f, 2 * b), R.SENTINEL, dtype=torch.float32, device=DEV)
    out = torch.full((b, f), R.SENTINEL, dtype=torch.float32, device=DEV)
    ws = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    args = {"frames-0": (ptr(spec), 0, b, ptr(ws), ptr(out)), "frames-neg": (ptr(spec), -1, b, ptr(ws), ptr(out)),
            "bins-0": (ptr(spec), f, 0, ptr(ws), ptr(out)), "bins-neg": (ptr(spec), f, -2, ptr(ws), ptr(out)),
            "null-spec": (None, f, b, ptr(ws), ptr(out)), "null-ws": (ptr(spec), f, b, None, ptr(out)),
            "null-out": (ptr(spec), f, b, ptr(ws), None)}[what]
    assert lib().query("omr_log_stft_post", *args, cur_stream()) == -1
    torch.cuda.synchronize()
    assert bool((spec == R.SENTINEL).all()) and bool((out == R.SENTINEL).all()) and int(ws.cpu()) == 77, "a refused call wrote something"


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_post_non_finite(kind):
    spec, where = R.nonfinite_specs()[kind]
    _, out = run_post(spec)
    R.nonfinite_check(kind, where, out, who=f"gpu {kind}")


def test_post_nan_in_the_second_sweep():
    """The NaN in the last element of post-wrap's shape: it reaches the maximum through the grid-stride loop's second iteration."""
    spec = R.post_spec(R.POST["post-wrap"])
    spec[-1, -1] = np.nan                                                  # im of the last element
    _, out = run_post(spec)
    R.nonfinite_check("nan", None, out, who="gpu nan second sweep")


@pytest.mark.parametrize("case", R.STFT_CASES, ids=lambda c: c.name)
def test_log_stft(case):
    y = torch.from_numpy(R.stft_signal(case)).to(DEV)
    out = audio.log_stft(y)
    assert R.stft_check(case, out, audio._basis("cpu").numpy(), who=f"gpu {case.name}") <= 1.0
    assert torch.equal(out, audio.log_stft(y))


def test_log_stft_nan_sample():
    y = R.stft_signal(R.STFT["impulses-five"])
    y[1500] = np.nan
    out = audio.log_stft(torch.from_numpy(y).to(DEV))
    assert tuple(out.shape) == (1, R.BINS, 7) and bool(torch.isnan(out).all()), f"{int((~torch.isnan(out)).sum())} outputs are not NaN"


@pytest.mark.parametrize("case", R.RESAMPLE_CASES, ids=R.resample_id)
def test_resample_poly(case):
    orig, target, _ = case
    x = torch.from_numpy(R.resample_input(case)).to(DEV)
    keep = x.clone()
    y = audio.resample_poly(x, orig, target)
    up, down = R.up_down(orig, target)
    k_pad = 0 if up == down else audio._resample_plan(up, down, "cpu")[0].shape[1]
    assert R.resample_check(case, y, k_pad, who="gpu") <= 1.0
    assert y.data_ptr() != x.data_ptr() and torch.equal(x, keep)
