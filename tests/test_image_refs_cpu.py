"""CPU-only: the score-image front end's case table (tests/image_refs.py) with numpy standing in for the two kernels, the oracle's
restatement of Pillow against Pillow itself, the host tables, and the host parts of image.py.

Every check tests/test_image_branches_gpu.py makes on the device is made here on `hpass_standin` / `vpass_standin`, fed with the
library's host tables: a correct implementation meets every check, and each damaged one (`test_wrong_*`) is rejected by the case
named in its assertion.  The oracle is compared with live Pillow where it is importable (rows and columns of impulses, steps and
{0, 255} noise at every size pair of the table: the impulse responses are Pillow's own coefficients) and with Pillow's recorded
outputs in tests/golden/f11b_image.npz.  The host table code also runs under AddressSanitizer / UBSan as a program of its own."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import image_refs as R
from oracle import ref_cpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "f11b_image.npz")
TABLE_PAIRS = [(i, o) for i in range(1, 49) for o in range(1, 49)] + [(2048, 33), (3000, 1500), (699, 279), (4096, 128), (128, 4096)]
BE = R.standin_backend()


# ------------------------------------------------------------------------------------------------ the host tables
def test_host_tables_equal_the_oracles_and_leave_accumulator_headroom():
    """omr_resample_ksize / omr_resample_coeffs == pil_bicubic_tables for every pair of [1, 48]^2 and five large ones, and per pair
    255 max_row sum |coef| + 2^21 < 2^31: the kernels accumulate in int32."""
    from omr_a2s_multimodal_transformer_amd import _lib
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    worst, at = 0.0, None
    for i, o in TABLE_PAIRS:
        bounds, coefs = ref_cpu.pil_bicubic_tables(i, o)
        ks = cdll.omr_resample_ksize(i, o)
        assert ks == coefs.shape[1], (i, o)
        b = np.empty((o, 2), dtype=np.int32)
        c = np.empty((o, ks), dtype=np.int32)
        assert cdll.omr_resample_coeffs(i, o, ctypes.c_void_p(b.ctypes.data), ctypes.c_void_p(c.ctypes.data)) == ks, (i, o)
        assert np.array_equal(b, bounds) and np.array_equal(c, coefs), (i, o)
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 0] + b[:, 1] <= i).all() and (b[:, 1] <= ks).all(), (i, o)
        head = (255 * int(np.abs(c.astype(np.int64)).sum(axis=1).max()) + (1 << 21)) / 2.0 ** 31
        assert head < 1.0, (i, o, head)
        if head > worst:
            worst, at = head, (i, o)
    print(f"largest 255 sum |coef| + 2^21 = {worst:.4f} x 2^31 at {at}")
    assert at == (14, 13) and abs(worst - 0.6329) < 1e-4              # what DESIGN.md records


def test_the_table_reaches_what_it_names():
    b, k = R.ref_tables(*R.FULL_WINDOW)
    assert (b[:, 1] == k.shape[1]).any()                               # a window of all ksize taps exists
    assert R.ref_tables(2048, 33)[1].shape[1] == 251
    for i, o in R.WINDOWS:
        assert any(c.name == f"h-window-{i}-{o}" for c in R.CASES) and any(c.name == f"v-window-{i}-{o}" for c in R.CASES)
    shapes = {(c.h, c.out) if c.kernel == "h" else (c.out, c.w) for c in R.CASES if c.item == 5}
    assert shapes == set(R.THREAD_SHAPES) and 3 * 171 == 2 * 256 + 1
    assert {c.c for c in R.H_CASES if c.item == 1} == {1, 3, 4}
    up = R.ref_tables(5, 64)[0]
    assert up[0, 0] == 0 and up[-1, 0] + up[-1, 1] == 5 and up[0, 1] < 4 and up[-1, 1] < 4      # windows cut at both borders


# ------------------------------------------------------------------------------------------------ the oracle against Pillow
def _lines(n: int):
    """One-row images [1, n]: an impulse at every position (255 on 0 and 0 on 255), a step, the {0, 255} noise."""
    eye = np.eye(n, dtype=np.uint8) * 255
    yield "impulses", eye
    yield "dark impulses", 255 - eye
    step = np.zeros((1, n), dtype=np.uint8)
    step[0, n // 2:] = 255
    yield "step", step
    yield "noise", R.binary_noise(n).reshape(1, n)


@pytest.mark.parametrize("pair", R.SIZE_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_oracle_equals_live_pillow_on_rows_and_columns(pair):
    Image = pytest.importorskip("PIL.Image")
    i, o = pair
    for kind, rows in _lines(i):
        want = np.asarray(Image.fromarray(rows).resize((o, rows.shape[0])))
        assert np.array_equal(ref_cpu.pil_resize_L(rows, rows.shape[0], o), want), f"{kind} rows {i} -> {o}"
        cols = np.ascontiguousarray(rows.T)
        want = np.asarray(Image.fromarray(cols).resize((cols.shape[1], o)))
        assert np.array_equal(ref_cpu.pil_resize_L(cols, o, cols.shape[1]), want), f"{kind} columns {i} -> {o}"


def _golden():
    g = np.load(GOLD)
    for n in sorted(k[:-4] for k in g.files if k.endswith("_out")):
        oh, ow = (int(v) for v in g[n + "_size"])
        yield n, g[n + "_pixels"], oh, ow, g[n + "_out"]


def test_oracle_equals_the_edge_golden_vectors():
    n_cases = 0
    for name, px, oh, ow, out in _golden():
        assert px.size <= 2048
        assert np.array_equal(ref_cpu.pil_resize_L(px, oh, ow), out), name
        if name.startswith("sq_"):
            assert ow == int(oh * px.shape[1] / px.shape[0])
            assert np.array_equal(ref_cpu.preprocess_image(px, oh)[0], out.astype(np.float32) / np.float32(255.0)), name
        n_cases += 1
    assert n_cases == 4 * len(R.SIZE_PAIRS) + 11
    h, w, oh, ow = R.ORDER_SHAPE
    g = np.load(GOLD)
    assert np.array_equal(g[f"sq_order_{h}x{w}_{oh}_pixels"], R.order_pixels()[..., 0])
    first_h, first_v = R.order_refs()
    assert np.array_equal(g[f"sq_order_{h}x{w}_{oh}_out"], first_h) and not np.array_equal(first_h, first_v)     # Pillow: horizontal first


# ------------------------------------------------------------------------------------------------ the stand-in passes the table
@pytest.mark.parametrize("case", R.H_CASES, ids=lambda c: c.name)
def test_a_correct_hpass_meets_every_check(case):
    R.check_h(case, BE)


@pytest.mark.parametrize("case", R.V_CASES, ids=lambda c: c.name)
def test_a_correct_vpass_meets_every_check(case):
    R.check_v(case, BE)


def test_a_correct_pipeline_meets_the_order_check():
    R.check_order(lambda px, oh, ow: R.resize_through(BE, px, oh, ow))


@pytest.mark.parametrize("what", sorted(R.H_REFUSALS))
def test_the_hpass_standin_refuses(what):
    R.check_h_refusal(what, BE)


@pytest.mark.parametrize("what", sorted(R.V_REFUSALS))
def test_the_vpass_standin_refuses(what):
    R.check_v_refusal(what, BE)


# ------------------------------------------------------------------------------------------------ damaged stand-ins
def _rejected(check, name: str, h_damage=None, v_damage=None) -> bool:
    """The named case with a damaged stand-in; True when one of the check's own assertions fails."""
    try:
        check(R.CASE[name], R.standin_backend(h_damage, v_damage))
    except AssertionError as e:
        print(f"{h_damage or v_damage} / {name}: {str(e)[:160]}")
        return True
    return False


def test_wrong_luma_without_rounding():
    assert _rejected(R.check_h, "h-ch3-convert", h_damage="luma_no_round")


def test_wrong_luma_by_the_float_formula():
    assert _rejected(R.check_h, "h-all-triples", h_damage="luma_float")


def test_wrong_alpha_premultiplied():
    assert _rejected(R.check_h, "h-alpha-convert", h_damage="alpha_premultiplied")


def test_wrong_pass_without_rounding_term():
    assert _rejected(R.check_h, "h-ch1-resample", h_damage="no_round") and _rejected(R.check_v, "v-f32-resample", v_damage="no_round")


def test_wrong_pass_wraps_instead_of_clipping():
    assert _rejected(R.check_h, "h-clip-64-23", h_damage="wrap") and _rejected(R.check_v, "v-clip-64-23", v_damage="wrap")


def test_wrong_clip_at_the_upper_side_only():
    assert _rejected(R.check_h, "h-clip-5-64", h_damage="clip_upper_only") and _rejected(R.check_v, "v-clip-5-64", v_damage="clip_upper_only")


def test_wrong_vertical_pass_first():
    with pytest.raises(AssertionError, match="horizontal pass first"):
        R.check_order(lambda px, oh, ow: R.resize_vertical_first(BE, px, oh, ow))


def test_wrong_xmin_off_by_one():
    assert _rejected(R.check_h, "h-window-14-13", h_damage="xmin_plus_one")


def test_wrong_window_truncated_to_ksize_minus_one_taps():
    """A loop capped at ksize - 1 taps is no defect: a window reaches ksize taps only where its outermost tap lies at the edge of the
    cubic's support, and that tap's weight rounds to 0 -- asserted for every table of the list, so the capped stand-in passes
    h-window-13-23, which has such windows.  What can be seen is a window one tap short of its own count: rejected by h-window-14-13."""
    n_full = 0
    for i, o in TABLE_PAIRS:
        b, k = R.ref_tables(i, o)
        full = b[:, 1] == k.shape[1]
        n_full += int(full.sum())
        assert (k[full, -1] == 0).all(), (i, o)
    assert n_full >= 8 and not _rejected(R.check_h, "h-window-13-23", h_damage="taps_capped")
    assert _rejected(R.check_h, "h-window-14-13", h_damage="taps_minus_one")


def test_wrong_row_stride_ignored():
    assert _rejected(R.check_h, "h-pitch-plus5-resample", h_damage="stride_ignored")


def test_wrong_pixel_pitch_4_for_rgb():
    assert _rejected(R.check_h, "h-pitch-4w-convert", h_damage="pixel_pitch_4")


def test_wrong_destination_row_pitch_ignored():
    assert _rejected(R.check_v, "v-f32-resample-pitch3", v_damage="dst_pitch_ignored")


def test_wrong_output_past_h_x_w_written():
    assert _rejected(R.check_v, "v-bf16-convert-slot", v_damage="writes_past")


def test_wrong_reciprocal_instead_of_division():
    assert _rejected(R.check_v, "v-all-bytes-f32", v_damage="reciprocal")
    v = np.arange(256, dtype=np.float32)
    assert int((v * (np.float32(1.0) / np.float32(255.0)) != v / np.float32(255.0)).sum()) == 126


def test_wrong_bf16_by_truncation():
    assert _rejected(R.check_v, "v-all-bytes-bf16", v_damage="bf16_truncated")


def test_wrong_last_partial_block_lost():
    assert _rejected(R.check_h, "h-threads-3x171", h_damage="last_block_lost") and _rejected(R.check_v, "v-threads-3x171", v_damage="last_block_lost")


def test_the_float_luma_differs_on_a_small_share_of_triples():
    """Why the 2^24 case exists: random bytes meet the 0.056 % of triples where the float 601 formula differs only by chance."""
    px = R.case_pixels(R.CASE["h-all-triples"]).reshape(-1, 3).astype(np.float64)
    f = np.floor(0.299 * px[:, 0] + 0.587 * px[:, 1] + 0.114 * px[:, 2] + 0.5).astype(np.uint8)
    share = float((f != R.luma_all_triples(R.case_pixels(R.CASE["h-all-triples"])).reshape(-1)).mean())
    print(f"float 601 luma differs on {share:.4%} of all RGB triples")
    assert 0.0 < share < 0.002


# ------------------------------------------------------------------------------------------------ image.py, host side
class _Img:
    """What as_hwc_uint8 looks at in a PIL image: `.mode`, and the array interface."""

    def __init__(self, mode, arr):
        self.mode, self._arr = mode, arr

    def __array__(self, dtype=None, copy=None):
        return self._arr if dtype is None else self._arr.astype(dtype)


def test_as_hwc_uint8_accepts_and_refuses():
    from omr_a2s_multimodal_transformer_amd import image as I
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(6, 9, 4), dtype=np.uint8)
    for bad in (a.astype(np.float32), a[:, :, :2], a[None], a.astype(np.float64)[..., 0], torch.from_numpy(a).float(), a[:, :, :2][..., 0][None, None]):
        with pytest.raises(ValueError):
            I.as_hwc_uint8(bad)
    for mode in ("P", "LA", "I;16", None):
        with pytest.raises(ValueError):
            I.as_hwc_uint8(_Img(mode, a[..., 0]))
    for mode, arr in (("L", a[..., 0]), ("RGB", a[..., :3]), ("RGBA", a)):
        t = I.as_hwc_uint8(_Img(mode, arr))
        assert t.is_contiguous() and t.dtype == torch.uint8 and np.array_equal(t.numpy().reshape(arr.shape), arr)
    for view in (a[:, :, :3], a[::2, 1:8:3], a.transpose(1, 0, 2), a[..., 1], a[::-1]):
        assert not view.flags["C_CONTIGUOUS"]
        t = I.as_hwc_uint8(view)
        assert t.is_contiguous() and t.dim() == 3 and np.array_equal(t.numpy().reshape(view.shape), view)
    tv = torch.from_numpy(a)[:, 2:7, :3]
    assert np.array_equal(I.as_hwc_uint8(tv).numpy(), a[:, 2:7, :3]) and I.as_hwc_uint8(tv).is_contiguous()


def test_resized_width_is_pythons_float_arithmetic():
    from omr_a2s_multimodal_transformer_amd import image as I
    for h in (1, 2, 3, 7, 64, 111, 317, 4097, 16777217):
        for w in (1, 2, 5, 699, 4096, 16777217, 50000001):
            assert I.resized_width(h, w, None) == (h, w)
            for H in (1, 16, 64, 128, 4097):                           # H * w passes 2^24 (fp32 would round it) and, at the end, 2^32
                assert I.resized_width(h, w, H) == (H, int(H * w / h)), (h, w, H)
    assert I.resized_width(3, 1, 2) == (2, 0) and I.resized_width(7, 3, 7) == (7, 3)
    assert int(64 * 16777217 / 64) == 16777217 and 64 * 16777217 > 2 ** 24


def test_a_resulting_width_of_zero_is_refused():
    """3 x 1 at height 2 is 2 x 0: refused on the host, before anything is allocated on or sent to the device."""
    from omr_a2s_multimodal_transformer_amd import image as I
    thin = np.zeros((3, 1), dtype=np.uint8)
    assert I.resized_width(3, 1, 2) == (2, 0)
    with pytest.raises(ValueError, match="2x0"):
        I.preprocess_image(thin, 2, device="cuda:0")
    with pytest.raises(ValueError, match="2x0"):
        I.image_batch([np.zeros((4, 8, 3), dtype=np.uint8), thin], 2, device="cuda:0")


# ------------------------------------------------------------------------------------------------ host tables under sanitizers
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _sanitizer_link_flags(cxx: str, tmp_path):
    """How a sanitized program links and starts with this compiler, decided on a one-line program before the real sources are
    compiled: the runtimes as archives inside the program if the compiler has them, else the shared ones.  None: no usable runtime."""
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        exe = str(tmp_path / ("probe_static" if extra else "probe_shared"))
        if subprocess.run([cxx, *SANITIZE, str(src), "-o", exe, *extra], capture_output=True).returncode == 0 \
                and subprocess.run([exe], capture_output=True).returncode == 0:
            return extra
    return None


def test_host_table_code_under_address_and_undefined_sanitizers(tmp_path):
    """tests/host/resample_tables_main.cpp + csrc/resample_host.cpp, the Makefile's flags for that file plus the sanitizers, as a child
    process of its own: nothing is loaded into this interpreter and nothing is preloaded.  Skips only without a compiler or without a
    sanitizer runtime that an empty program links and starts with; after that, a failed build or run of the real sources fails."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    link = _sanitizer_link_flags(cxx, tmp_path)
    if link is None:
        pytest.skip("no usable sanitizer runtime for the host compiler")
    exe = str(tmp_path / "resample_tables_main")
    built = subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-g", *SANITIZE, "-I" + os.path.join(REPO, "include"),
                            os.path.join(HERE, "host", "resample_tables_main.cpp"),
                            os.path.join(REPO, "omr_a2s_multimodal_transformer_amd", "csrc", "resample_host.cpp"), "-o", exe, *link],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout and "0.6329" in run.stdout
