"""Branch-level tests of the score-image front end on the device: `gray_hpass_kernel<1 / 3 / 4>` and `vpass_to_float_kernel<float / bf16>`
(csrc/image.hip) through their entries `omr_image_gray_hpass` / `omr_image_vpass_to_float` called directly, then image.py through
its public functions.  Cases, references and checks are those of tests/image_refs.py ("Image front end coverage");
tests/test_image_refs_cpu.py runs the same table with numpy in the kernels' place and shows which wrong kernels these checks see.
Integer work and one correctly rounded division: every comparison is bit equality."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import image_refs as R  # noqa: E402
from oracle import ref_cpu  # noqa: E402
from oracle.kernel_refs import SENTINEL, assert_bit_equal  # noqa: E402
from omr_a2s_multimodal_transformer_amd import image as I  # noqa: E402
from omr_a2s_multimodal_transformer_amd._lib import cur_stream, lib, ptr  # noqa: E402

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f11b_image.npz")


def _positive(*v) -> bool:
    return all(x > 0 for x in v)


def run_h(src, off, h, w, c, row_stride, bounds, coefs, ksize, out_w, dst):
    """omr_image_gray_hpass on device copies of the host buffers -> (return code, dst afterwards)."""
    if src is not None and dst is not None and _positive(h, w, c, out_w, row_stride):   # what the launch may touch lies inside the buffers
        assert off + (h - 1) * row_stride + w * (c if c in (1, 3, 4) else max(c, 4)) <= src.size and h * out_w <= dst.size
    s = None if src is None else torch.from_numpy(src).to(DEV)
    d = None if dst is None else torch.from_numpy(dst.copy()).to(DEV)
    rc = lib().query("omr_image_gray_hpass", None if s is None else s.data_ptr() + off, h, w, c, row_stride, ptr(bounds), ptr(coefs), ksize, out_w, ptr(d),
                     cur_stream())
    torch.cuda.synchronize()
    return rc, None if d is None else d.cpu().numpy()


def run_v(src, h, w, bounds, coefs, ksize, out_h, out_dtype, dst, off, dst_row_stride):
    """omr_image_vpass_to_float into a view `off` elements into a device copy of dst -> (return code, dst afterwards)."""
    if src is not None and dst is not None and _positive(h, w, out_h, dst_row_stride):
        assert h * w <= src.size and off + (out_h - 1) * dst_row_stride + w <= dst.numel()
    s = None if src is None else torch.from_numpy(src).to(DEV)
    d = None if dst is None else dst.to(DEV)
    rc = lib().query("omr_image_vpass_to_float", ptr(s), h, w, ptr(bounds), ptr(coefs), ksize, out_h, out_dtype,
                     None if d is None else d.data_ptr() + off * d.element_size(), dst_row_stride, cur_stream())
    torch.cuda.synchronize()
    return rc, None if d is None else d.cpu()


BE = R.Backend(run_h, run_v, lambda i, o: I._tables(i, o, 0))


# ------------------------------------------------------------------------------------------------ the entries themselves
@pytest.mark.parametrize("case", R.H_CASES, ids=lambda c: c.name)
def test_hpass(case):
    R.check_h(case, BE)


@pytest.mark.parametrize("case", R.V_CASES, ids=lambda c: c.name)
def test_vpass(case):
    R.check_v(case, BE)


def test_pass_order():
    R.check_order(lambda px, oh, ow: R.resize_through(BE, px, oh, ow))
    h, w, oh, ow = R.ORDER_SHAPE
    assert_bit_equal(I.preprocess_image(R.order_pixels(), oh, device=DEV)[0].cpu(), R.to_float_ref(R.order_refs()[0], "f32"), "preprocess_image on the order case")


@pytest.mark.parametrize("what", sorted(R.H_REFUSALS))
def test_hpass_refusals(what):
    R.check_h_refusal(what, BE)


@pytest.mark.parametrize("what", sorted(R.V_REFUSALS))
def test_vpass_refusals(what):
    R.check_v_refusal(what, BE)


# ------------------------------------------------------------------------------------------------ image.py: views
def _view_cases():
    """name -> (device view [h, w, c], the same pixels as a contiguous host array)."""
    rng = np.random.default_rng(77)
    rgba = torch.from_numpy(rng.integers(0, 256, size=(20, 50, 4), dtype=np.uint8)).to(DEV)
    rgb = torch.from_numpy(rng.integers(0, 256, size=(20, 60, 3), dtype=np.uint8)).to(DEV)
    whc = torch.from_numpy(rng.integers(0, 256, size=(50, 20, 3), dtype=np.uint8)).to(DEV)
    gray = torch.from_numpy(rng.integers(0, 256, size=(20, 64), dtype=np.uint8)).to(DEV)
    views = {
        "rgb-of-rgba": rgba[:, :, :3],                                 # stride(1) = 4 != c
        "width-slice": rgb[:, 10:50],                                  # stride(0) > w * c: passed through
        "permuted": whc.permute(1, 0, 2),                              # stride(0) = 3 < w * c, stride(1) = 60
        "gray-pitch": gray[:, :50].unsqueeze(-1),                      # c == 1, rows 64 bytes apart
        "rows-stepped": rgb[::2],                                      # stride(0) = 2 w c: passed through
        "rgba-width-slice": rgba[:, 3:47],
        "one-channel-of-rgb": rgb[:, :, 1:2],                          # c == 1 with stride(1) = 3
        "expanded-row": rgb[:1].expand(20, 60, 3),                     # stride(0) = 0
    }
    return {k: (v, v.cpu().contiguous().numpy()) for k, v in views.items()}


VIEW_NAMES = ["rgb-of-rgba", "width-slice", "permuted", "gray-pitch", "rows-stepped", "rgba-width-slice", "one-channel-of-rgb", "expanded-row"]


@pytest.mark.parametrize("img_height", [None, 16], ids=["same-size", "height-16"])
@pytest.mark.parametrize("name", VIEW_NAMES)
def test_preprocess_image_into_takes_views(name, img_height):
    view, px = _view_cases()[name]
    assert not view.is_contiguous() and tuple(view.shape) == px.shape
    ref = torch.from_numpy(ref_cpu.preprocess_image(px[..., 0] if px.shape[2] == 1 else px, img_height))[0]
    H, W = ref.shape
    for dtype in (torch.float32, torch.bfloat16):
        want = torch.full((H + 2, W + 3), SENTINEL, dtype=dtype)
        want[:H, :W] = ref.to(dtype)
        out = torch.full((H + 2, W + 3), SENTINEL, dtype=dtype, device=DEV)
        before = view.clone()
        assert I.preprocess_image_into(view, img_height, out) == (H, W)
        assert_bit_equal(out.cpu(), want, f"{name} at height {img_height}, {dtype}")
        assert torch.equal(view, before), "the source view changed"


def test_a_width_of_zero_is_refused_on_the_device_too():
    px = torch.zeros((3, 1, 1), dtype=torch.uint8, device=DEV)
    out = torch.full((4, 4), SENTINEL, device=DEV)
    with pytest.raises(ValueError, match="2x0"):
        I.preprocess_image_into(px, 2, out)
    with pytest.raises(ValueError):
        I.preprocess_image_into(px.float(), None, out)
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ image.py: no second pass, batches
@pytest.mark.parametrize("c", [1, 3])
def test_img_height_equal_to_the_height(c):
    """No table at all: c == 1 runs the vertical kernel's conversion alone, c == 3 the luma conversion and then that."""
    px = np.random.default_rng(5 + c).integers(0, 256, size=(33, 71, c), dtype=np.uint8)
    ref = torch.from_numpy(ref_cpu.preprocess_image(px[..., 0] if c == 1 else px, None))
    for H in (33, None):
        assert_bit_equal(I.preprocess_image(px, H, device=DEV).cpu(), ref, f"c = {c}, height {H}, fp32")
        assert_bit_equal(I.preprocess_image(px, H, dtype=torch.bfloat16, device=DEV).cpu(), ref.to(torch.bfloat16), f"c = {c}, height {H}, bf16")


@pytest.mark.parametrize("pad", [1.0, 0.0, float("nan")], ids=["pad-1", "pad-0", "pad-nan"])
def test_image_batch_bf16(pad):
    rng = np.random.default_rng(13)
    raws = [rng.integers(0, 256, size=s, dtype=np.uint8) for s in [(40, 90, 3), (32, 50), (71, 33, 4), (9, 64, 1), (20, 200, 3)]]
    refs = [torch.from_numpy(ref_cpu.preprocess_image(p[..., 0] if p.ndim == 3 and p.shape[2] == 1 else p, 32))[0] for p in raws]
    Wm = max(r.shape[1] for r in refs)
    assert len({r.shape[1] for r in refs}) == len(refs)
    for dtype in (torch.bfloat16, torch.float32):
        x, xl = I.image_batch(raws, 32, pad_value=pad, dtype=dtype, device=DEV)
        assert tuple(x.shape) == (5, 1, 32, Wm) and x.dtype == dtype and xl.tolist() == [r.shape[1] for r in refs]
        want = torch.full((5, 1, 32, Wm), pad, dtype=dtype, device=DEV).cpu()        # the fill is torch's: its bits, NaN included
        assert bool(torch.isnan(want).all()) == (pad != pad)
        for i, r in enumerate(refs):
            want[i, 0, :, : r.shape[1]] = r.to(dtype)                  # the bf16 rounding of the fp32 reference
        assert_bit_equal(x.cpu(), want, f"image_batch {dtype} pad {pad}")
        for i in (0, 3):
            one, w1 = I.image_batch([raws[i]], 32, pad_value=pad, dtype=dtype, device=DEV)
            assert_bit_equal(one[0].cpu(), I.preprocess_image(raws[i], 32, dtype=dtype, device=DEV).cpu(), "a batch of one")
            assert w1.tolist() == [refs[i].shape[1]]


def test_preprocess_image_equals_pillows_edge_golden_vectors():
    g = np.load(GOLD)
    names = sorted(k[:-4] for k in g.files if k.startswith("sq_") and k.endswith("_out"))
    assert len(names) == 11
    for n in names:
        px, out = g[n + "_pixels"], g[n + "_out"]
        got = I.preprocess_image(px, int(g[n + "_size"][0]), device=DEV)
        assert_bit_equal(got[0].cpu(), torch.from_numpy(out.astype(np.float32) / np.float32(255.0)), n)
