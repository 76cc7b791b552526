"""Score-image front end (omr_image_gray_hpass, omr_image_vpass_to_float, image.py): the case table, inputs, references, checks and
the numpy stand-ins of tests/test_image_branches_gpu.py and tests/test_image_refs_cpu.py.  DESIGN.md, "Image front end coverage".

Everything here is integer work or one correctly rounded fp32 division: every comparison is bit equality, there is no tolerance.
A check takes a `Backend`: the two entries as functions of host buffers (the GPU file uploads, calls the entry and downloads; the
CPU file passes `hpass_standin` / `vpass_standin`) and the source of the coefficient tables (image._tables on the device,
image._tables_host for the stand-ins).  The references are the oracle's (oracle.ref_cpu.pil_*), which is pinned against Pillow.

Test infrastructure only: nothing here is imported by the package."""
from __future__ import annotations

import functools
from collections import namedtuple
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from oracle import ref_cpu
from oracle.kernel_refs import SENTINEL, assert_bit_equal

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
F32, BF16 = 0, 1
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}
DTYPE_CODE = {"f32": F32, "bf16": BF16}
SRC_FILL = 0xA5                              # every source byte that is not a pixel
TMP_FILL = 0x5A                              # behind the uint8 image the horizontal pass writes
TAIL = 64                                    # bytes / elements kept behind every buffer

# run_h(src, off, h, w, channels, row_stride, bounds, coefs, ksize, out_w, dst) -> (rc, dst after): src / dst flat uint8 host buffers
#   (or None: a null pointer), the image starts `off` bytes into src.
# run_v(src, h, w, bounds, coefs, ksize, out_h, out_dtype, dst, off, dst_row_stride) -> (rc, dst after): src flat uint8 [h * w], dst a
#   flat torch CPU tensor of the output type, the view starts `off` elements into it.
# tables(in_size, out_size) -> (bounds, coefs, ksize) in whatever form run_h / run_v take them.
Backend = namedtuple("Backend", "run_h run_v tables")


# ------------------------------------------------------------------------------------------------ references
@functools.lru_cache(maxsize=None)
def ref_tables(in_size: int, out_size: int):
    return ref_cpu.pil_bicubic_tables(in_size, out_size)


def pass_unclipped(img: np.ndarray, bounds: np.ndarray, coefs: np.ndarray) -> np.ndarray:
    """uint8 [h, w] -> int64 [h, out_w]: (sum + 2^21) >> 22 of one horizontal pass, before the clip to [0, 255]."""
    src = img.astype(np.int64)
    out = np.empty((img.shape[0], bounds.shape[0]), dtype=np.int64)
    for xx, (xmin, n) in enumerate(bounds):
        out[:, xx] = ((src[:, xmin:xmin + n] * coefs[xx, :n].astype(np.int64)).sum(axis=1) + (1 << 21)) >> 22
    return out


def clip_counts(img: np.ndarray, in_size: int, out_size: int):
    """(pixels under 0, pixels over 255) of the unclipped horizontal pass; it must clip to the oracle's pass."""
    b, c = ref_tables(in_size, out_size)
    u = pass_unclipped(img, b, c)
    assert np.array_equal(np.clip(u, 0, 255).astype(np.uint8), ref_cpu._pil_pass(img, b, c))
    return int((u < 0).sum()), int((u > 255).sum())


def hpass_ref(gray: np.ndarray, out_w: int) -> np.ndarray:
    return gray.copy() if out_w == gray.shape[1] else ref_cpu._pil_pass(gray, *ref_tables(gray.shape[1], out_w))


def vpass_ref(gray: np.ndarray, out_h: int) -> np.ndarray:
    if out_h == gray.shape[0]:
        return gray.copy()
    return np.ascontiguousarray(ref_cpu._pil_pass(np.ascontiguousarray(gray.T), *ref_tables(gray.shape[0], out_h)).T)


def to_float_ref(gray: np.ndarray, dtype: str) -> torch.Tensor:
    """ToTensor: float32(v) / float32(255), one correctly rounded division; bf16 is the round-to-nearest-even of that."""
    f = torch.from_numpy(gray.astype(np.float32) / np.float32(255.0))
    return f if dtype == "f32" else f.to(torch.bfloat16)


def luma_all_triples(px: np.ndarray) -> np.ndarray:
    r, g, b = (px[..., i].astype(np.uint32) for i in range(3))
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    name: str
    kernel: str                  # "h": omr_image_gray_hpass, "v": omr_image_vpass_to_float
    h: int
    w: int
    out: int                     # out_w ("h") / out_h ("v"); equal to w / h: coefs == NULL
    c: int = 1
    content: str = "random"      # random | binary ({0, 255} noise of rng(0)) | alpha | ramp (bytes 0..255) | triples (all 2^24)
    pitch: int = 0               # "h": row_stride in bytes; "v": dst_row_stride in elements; 0: packed
    offset: int = 0              # of the view into its buffer: bytes ("h") / elements ("v")
    dtype: str = "f32"
    clips: bool = False          # asserts about itself: pixels under 0 and over 255 before the clip
    item: int = 0                # the row of DESIGN.md's branch table


WINDOWS = [(1, 7), (2, 1), (5, 64), (2048, 33), (14, 13)]            # (14, 13): the largest sum |coef| of all sizes up to 48
FULL_WINDOW = (13, 23)                                                # tap count == ksize at some output pixel (asserted)
CLIP_PAIRS = [(5, 64), (37, 96), (317, 137), (64, 23)]
SIZE_PAIRS = list(dict.fromkeys(WINDOWS + [FULL_WINDOW] + CLIP_PAIRS))   # every (in, out) of items 6 and 7 once
CLIP_COUNTS = {(5, 64): (12, 12), (37, 96): (11, 16), (317, 137): (8, 9), (64, 23): (2, 3)}   # under 0 / over 255, asserted
THREAD_SHAPES = [(1, 1), (1, 257), (3, 171), (2, 256), (300, 1), (1, 700)]   # output h x w; 3 x 171 = 513: one thread alone in block 2
SLOT = dict(pitch=40, offset=1 * 24 * 40)                              # slot 1 of a [3, 1, 24, 40] batch


def _cases():
    cs = []
    for c in (1, 3, 4):                                               # 1. every instantiation, with and without tables
        cs.append(Case(f"h-ch{c}-resample", "h", 7, 45, 19, c=c, item=1))
        cs.append(Case(f"h-ch{c}-convert", "h", 7, 45, 45, c=c, item=1))
    for tag, pitch in (("plus5", 31 * 3 + 5), ("4w", 4 * 31)):        # 2. row_stride > w * channels, image 1 byte into its buffer
        cs.append(Case(f"h-pitch-{tag}-resample", "h", 9, 31, 12, c=3, pitch=pitch, offset=1, item=2))
        cs.append(Case(f"h-pitch-{tag}-convert", "h", 9, 31, 31, c=3, pitch=pitch, offset=1, item=2))
    cs.append(Case("h-pitch-ch1-plus5", "h", 9, 31, 31, c=1, pitch=36, offset=1, item=2))
    cs.append(Case("h-pitch-ch4-plus5", "h", 9, 31, 12, c=4, pitch=31 * 4 + 5, offset=1, item=2))
    cs.append(Case("h-alpha-resample", "h", 7, 45, 19, c=4, content="alpha", item=3))     # 3. alpha is ignored
    cs.append(Case("h-alpha-convert", "h", 7, 45, 45, c=4, content="alpha", item=3))
    for dt in ("f32", "bf16"):                                        # 4. both output types, with and without tables, three pitches
        for tag, out in (("resample", 19), ("convert", 45)):
            cs.append(Case(f"v-{dt}-{tag}", "v", 45, 7, out, dtype=dt, item=4))
            cs.append(Case(f"v-{dt}-{tag}-pitch3", "v", 45, 7, out, dtype=dt, pitch=10, offset=5, item=4))
        cs.append(Case(f"v-{dt}-resample-slot", "v", 45, 23, 19, dtype=dt, item=4, **SLOT))
        cs.append(Case(f"v-{dt}-convert-slot", "v", 24, 23, 24, dtype=dt, item=4, **SLOT))      # the slot's full height: the next slot follows
    for oh, ow in THREAD_SHAPES:                                      # 5. thread-count edges of both kernels
        cs.append(Case(f"h-threads-{oh}x{ow}", "h", oh, {1: 3, 257: 300, 171: 200, 256: 300, 700: 650}[ow], ow, c=3 if oh < 300 else 1, item=5))
        cs.append(Case(f"v-threads-{oh}x{ow}", "v", {1: 2, 3: 5, 2: 3, 300: 350}[oh] if (oh, ow) != (1, 1) else 3, ow, oh, item=5))
    for i, o in WINDOWS + [FULL_WINDOW]:                              # 6. window extremes, both kernels
        cs.append(Case(f"h-window-{i}-{o}", "h", 3, i, o, c=3 if i <= 14 else 1, item=6))
        cs.append(Case(f"v-window-{i}-{o}", "v", i, 5, o, dtype="bf16" if i == 5 else "f32", item=6))
    for i, o in CLIP_PAIRS:                                           # 7. clipping on both sides: a row and a column of {0, 255} noise
        cs.append(Case(f"h-clip-{i}-{o}", "h", 1, i, o, content="binary", clips=True, item=7))
        cs.append(Case(f"v-clip-{i}-{o}", "v", i, 1, o, content="binary", clips=True, item=7))
    cs.append(Case("h-all-triples", "h", 4096, 4096, 4096, c=3, content="triples", item=8))     # 8. every RGB triple once
    cs.append(Case("v-all-bytes-f32", "v", 16, 16, 16, content="ramp", item=9))              # 9. every byte through / 255
    cs.append(Case("v-all-bytes-bf16", "v", 16, 16, 16, content="ramp", dtype="bf16", item=9))
    return cs


CASES = _cases()
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
H_CASES = [c for c in CASES if c.kernel == "h"]
V_CASES = [c for c in CASES if c.kernel == "v"]


def binary_noise(n: int) -> np.ndarray:
    """n bytes of {0, 255} from rng(0): the sequence the clip counts of CLIP_COUNTS were computed with."""
    return (np.random.default_rng(0).integers(0, 2, n) * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _pixels_cached(name: str) -> np.ndarray:
    case = CASE[name]
    h, w, c = case.h, case.w, case.c
    rng = np.random.default_rng(2000 + sum(map(ord, name)))
    if case.content == "binary":
        px = binary_noise(h * w).reshape(h, w, 1)
    elif case.content == "ramp":
        px = np.arange(256, dtype=np.uint8).reshape(h, w, 1)
    elif case.content == "triples":
        v = np.arange(1 << 24, dtype=np.uint32).reshape(h, w)
        px = np.stack([(v >> 16).astype(np.uint8), (v >> 8).astype(np.uint8), v.astype(np.uint8)], axis=-1)
    else:
        px = rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
    px.setflags(write=False)
    return px


def case_pixels(case: Case) -> np.ndarray:
    """uint8 [h, w, c], read-only and cached: callers copy what they change."""
    return _pixels_cached(case.name)


def embed(px: np.ndarray, pitch: int, offset: int) -> np.ndarray:
    """The image as an interior view of a flat buffer full of SRC_FILL: rows `pitch` bytes apart, the first `offset` bytes in."""
    h, w, c = px.shape
    pitch = pitch or w * c
    buf = np.full(offset + h * pitch + TAIL, SRC_FILL, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(buf[offset:], shape=(h, w * c), strides=(pitch, 1))[:] = px.reshape(h, w * c)
    return buf


def _tables_or_none(be: Backend, in_size: int, out_size: int):
    return (None, None, 0) if in_size == out_size else be.tables(in_size, out_size)


def run_hpass(be: Backend, px: np.ndarray, out_w: int, pitch: int = 0, offset: int = 0) -> np.ndarray:
    """The horizontal entry on px [h, w, c] laid out at `pitch` / `offset` -> uint8 [h, out_w]; nothing behind h * out_w is written."""
    h, w, c = px.shape
    b, k, ks = _tables_or_none(be, w, out_w)
    dst = np.full(h * out_w + TAIL, TMP_FILL, dtype=np.uint8)
    rc, after = be.run_h(embed(px, pitch, offset), offset, h, w, c, pitch or w * c, b, k, ks, out_w, dst)
    assert rc == OK, f"omr_image_gray_hpass returned {rc}"
    assert (after[h * out_w:] == TMP_FILL).all(), "the horizontal pass wrote behind its h x out_w image"
    return after[:h * out_w].reshape(h, out_w)


def v_buffer(case_or_dtype, rows: int, pitch: int, offset: int) -> torch.Tensor:
    dtype = TORCH_DTYPE[case_or_dtype]
    return torch.full((offset + (rows + 2) * pitch + TAIL,), SENTINEL, dtype=dtype)


def v_view(buf: torch.Tensor, rows: int, cols: int, pitch: int, offset: int) -> torch.Tensor:
    return buf.as_strided((rows, cols), (pitch, 1), offset)


def run_vpass(be: Backend, gray: np.ndarray, out_h: int, dtype: str, pitch: int = 0, offset: int = 0) -> torch.Tensor:
    """The vertical entry on gray [h, w] into a view of a SENTINEL-filled buffer -> the whole buffer afterwards."""
    h, w = gray.shape
    b, k, ks = _tables_or_none(be, h, out_h)
    pitch = pitch or w
    rc, after = be.run_v(np.array(gray, dtype=np.uint8).reshape(-1), h, w, b, k, ks, out_h, DTYPE_CODE[dtype], v_buffer(dtype, out_h, pitch, offset), offset, pitch)
    assert rc == OK, f"omr_image_vpass_to_float returned {rc}"
    return after


# ------------------------------------------------------------------------------------------------ checks
def check_h(case: Case, be: Backend) -> None:
    px = case_pixels(case)
    who = case.name
    if case.content == "triples":
        ref = luma_all_triples(px)
        flat = px.reshape(-1, 3).astype(np.uint32)
        assert np.array_equal((flat[:, 0] << 16) | (flat[:, 1] << 8) | flat[:, 2], np.arange(1 << 24, dtype=np.uint32)), "not every triple once"
    else:
        ref = hpass_ref(ref_cpu.pil_gray(px), case.out)
    if case.clips:
        lo, hi = clip_counts(ref_cpu.pil_gray(px), case.w, case.out)
        print(f"{who}: {lo} pixels under 0, {hi} over 255 before the clip")
        assert (lo, hi) == CLIP_COUNTS[(case.w, case.out)] and lo >= 1 and hi >= 1, f"{who}: the case does not clip on both sides: {lo} / {hi}"
    if case.name == f"h-window-{FULL_WINDOW[0]}-{FULL_WINDOW[1]}":
        b, k = ref_tables(*FULL_WINDOW)
        full = b[:, 1] == k.shape[1]
        assert full.any(), f"{who}: no output pixel has a window of all ksize taps"
    got = run_hpass(be, px, case.out, case.pitch, case.offset)
    assert got.shape == ref.shape and np.array_equal(got, ref), f"{who}: {int((got != ref).sum())} of {ref.size} bytes differ from the reference"
    if case.pitch or case.offset:
        packed = run_hpass(be, px, case.out)
        assert np.array_equal(got, packed), f"{who}: row_stride {case.pitch} gives other bytes than the packed copy"
    if case.content == "alpha":
        assert len(np.unique(px[..., 3])) > 16
        zero = px.copy()
        zero[..., 3] = 0
        assert np.array_equal(run_hpass(be, zero, case.out), got), f"{who}: the alpha plane changes the result"


def check_v(case: Case, be: Backend) -> None:
    gray = case_pixels(case)[..., 0]
    who = case.name
    if case.content == "ramp":
        assert np.array_equal(np.sort(gray.reshape(-1)), np.arange(256))
    if case.clips:
        lo, hi = clip_counts(np.ascontiguousarray(gray.T), case.h, case.out)
        print(f"{who}: {lo} pixels under 0, {hi} over 255 before the clip")
        assert (lo, hi) == CLIP_COUNTS[(case.h, case.out)] and lo >= 1 and hi >= 1, f"{who}: the case does not clip on both sides: {lo} / {hi}"
    pitch = case.pitch or case.w
    assert pitch >= case.w
    want = v_buffer(case.dtype, case.out, pitch, case.offset)
    v_view(want, case.out, case.w, pitch, case.offset)[:] = to_float_ref(vpass_ref(gray, case.out), case.dtype)
    got = run_vpass(be, gray, case.out, case.dtype, case.pitch, case.offset)
    assert_bit_equal(got, want, f"{who}: the buffer around and inside the {case.out} x {case.w} view")


def resize_through(be: Backend, px: np.ndarray, out_h: int, out_w: int, dtype: str = "f32") -> torch.Tensor:
    """image.preprocess_image_into's two launches on the entries themselves: horizontal, then vertical -> [out_h, out_w]."""
    tmp = run_hpass(be, px, out_w)
    return v_view(run_vpass(be, tmp, out_h, dtype), out_h, out_w, out_w, 0).clone()


ORDER_SHAPE = (24, 40, 13, 21)                                        # h, w -> out_h, out_w


def order_pixels() -> np.ndarray:
    h, w = ORDER_SHAPE[:2]
    return binary_noise(h * w).reshape(h, w, 1)


def order_refs():
    """(horizontal first, vertical first) of the order case, uint8 [out_h, out_w] each."""
    h, w, oh, ow = ORDER_SHAPE
    g = order_pixels()[..., 0]
    return vpass_ref(hpass_ref(g, ow), oh), hpass_ref(vpass_ref(g, oh), ow)


def check_order(resize) -> None:
    """resize(px [h, w, 1], out_h, out_w) -> fp32 [out_h, out_w].  The two orders differ on this content (the intermediate image is
    clipped and rounded to bytes); the kernels must give the horizontal-first one, Pillow's."""
    h, w, oh, ow = ORDER_SHAPE
    first_h, first_v = order_refs()
    n = int((first_h != first_v).sum())
    print(f"order case: the two orders differ in {n} of {first_h.size} bytes")
    assert n >= 1, "the order case cannot tell the orders apart"
    assert_bit_equal(resize(order_pixels(), oh, ow), to_float_ref(first_h, "f32"), "order case (horizontal pass first)")


# ------------------------------------------------------------------------------------------------ refusals
REF_H, REF_W, REF_C, REF_OUT = 4, 6, 3, 5                             # the valid call every refusal damages in one argument
H_REFUSALS = {
    "null-src": dict(src=None), "null-dst": dict(dst=None), "h-0": dict(h=0), "h-neg": dict(h=-1), "w-0": dict(w=0), "w-neg": dict(w=-3),
    "out_w-0": dict(out_w=0), "out_w-neg": dict(out_w=-2), "channels-0": dict(c=0), "channels-2": dict(c=2), "channels-5": dict(c=5),
    "bounds-only": dict(coefs=None), "coefs-only": dict(bounds=None), "no-tables-other-width": dict(bounds=None, coefs=None),
    "ksize-0": dict(ksize=0), "ksize-neg": dict(ksize=-5), "row_stride-short": dict(row_stride=REF_W * REF_C - 1), "row_stride-0": dict(row_stride=0),
}
V_REFUSALS = {
    "null-src": dict(src=None), "null-dst": dict(dst=None), "h-0": dict(h=0), "h-neg": dict(h=-1), "w-0": dict(w=0), "w-neg": dict(w=-3),
    "out_h-0": dict(out_h=0), "out_h-neg": dict(out_h=-2), "bounds-only": dict(coefs=None), "coefs-only": dict(bounds=None),
    "no-tables-other-height": dict(bounds=None, coefs=None), "ksize-0": dict(ksize=0), "ksize-neg": dict(ksize=-5),
    "dst_row_stride-short": dict(dst_row_stride=REF_W - 1), "dtype-2": dict(out_dtype=2), "dtype-neg": dict(out_dtype=-1),
}
REFUSAL_BUFFER = 4096                                                 # large enough for every reading of the damaged arguments


def check_h_refusal(what: str, be: Backend) -> None:
    b, k, ks = be.tables(REF_W, REF_OUT)
    a = dict(src=np.full(REFUSAL_BUFFER, SRC_FILL, dtype=np.uint8), off=0, h=REF_H, w=REF_W, c=REF_C, row_stride=REF_W * REF_C, bounds=b, coefs=k,
             ksize=ks, out_w=REF_OUT, dst=np.full(REFUSAL_BUFFER, TMP_FILL, dtype=np.uint8))
    assert be.run_h(**a)[0] == OK, "the undamaged call is refused"
    a["dst"] = np.full(REFUSAL_BUFFER, TMP_FILL, dtype=np.uint8)
    a.update(H_REFUSALS[what])
    rc, after = be.run_h(**a)
    assert rc == ERR_ARG, f"omr_image_gray_hpass {what}: returned {rc}"
    assert after is None or (after == TMP_FILL).all(), f"omr_image_gray_hpass {what}: a refused call wrote to dst"


def check_v_refusal(what: str, be: Backend) -> None:
    b, k, ks = be.tables(REF_H, REF_OUT)
    for dtype in ("f32", "bf16"):
        fill = torch.full((REFUSAL_BUFFER,), SENTINEL, dtype=TORCH_DTYPE[dtype])
        a = dict(src=np.full(REFUSAL_BUFFER, SRC_FILL, dtype=np.uint8), h=REF_H, w=REF_W, bounds=b, coefs=k, ksize=ks, out_h=REF_OUT,
                 out_dtype=DTYPE_CODE[dtype], dst=fill.clone(), off=0, dst_row_stride=REF_W)
        assert be.run_v(**a)[0] == OK, "the undamaged call is refused"
        a["dst"] = fill.clone()
        a.update(V_REFUSALS[what])
        rc, after = be.run_v(**a)
        assert rc == (ERR_UNSUPPORTED if what.startswith("dtype") else ERR_ARG), f"omr_image_vpass_to_float {what}: returned {rc}"
        if after is not None:
            assert_bit_equal(after, fill, f"omr_image_vpass_to_float {what} ({dtype}): dst after a refused call")


# ------------------------------------------------------------------------------------------------ numpy in the kernels' place
H_DAMAGES = ("luma_no_round", "luma_float", "alpha_premultiplied", "no_round", "wrap", "clip_upper_only", "xmin_plus_one", "taps_capped", "taps_minus_one",
             "stride_ignored", "pixel_pitch_4", "last_block_lost")
V_DAMAGES = ("no_round", "wrap", "clip_upper_only", "dst_pitch_ignored", "writes_past", "reciprocal", "bf16_truncated", "last_block_lost")


def _fixed_pass(img: np.ndarray, bounds: np.ndarray, coefs: np.ndarray, ksize: int, damage: Optional[str]) -> np.ndarray:
    """int64 [h, w] -> uint8 [h, out] as a kernel's thread computes it: taps [xmin, xmin + n) of row `coefs[x * ksize :]`."""
    bounds = np.asarray(bounds).reshape(-1, 2)
    coefs = np.asarray(coefs).reshape(-1)
    out = np.empty((img.shape[0], bounds.shape[0]), dtype=np.int64)
    padded = np.concatenate([img, img[:, :2]], axis=1)                # a damaged window may run past the row: whatever lies there
    for x, (xmin, n) in enumerate(bounds):
        xmin, n = int(xmin), int(n)
        if damage == "xmin_plus_one":
            xmin += 1
        if damage == "taps_capped":
            n = min(n, ksize - 1)
        if damage == "taps_minus_one":
            n -= 1
        k = coefs[x * ksize:x * ksize + n].astype(np.int64)
        ss = (padded[:, xmin:xmin + n] * k).sum(axis=1) + (0 if damage == "no_round" else 1 << 21)
        out[:, x] = ss >> 22
    if damage == "wrap":
        return (out & 0xFF).astype(np.uint8)
    if damage == "clip_upper_only":
        return (np.minimum(out, 255) & 0xFF).astype(np.uint8)
    return np.clip(out, 0, 255).astype(np.uint8)


def _keep_full_blocks(n: int, damage: Optional[str]) -> int:
    return n // 256 * 256 if damage == "last_block_lost" else n


def hpass_standin(src, off, h, w, c, row_stride, bounds, coefs, ksize, out_w, dst, damage: Optional[str] = None):
    """omr_image_gray_hpass on host buffers: its refusals, then one value per output pixel i = y * out_w + x."""
    assert damage is None or damage in H_DAMAGES
    if src is None or dst is None or h <= 0 or w <= 0 or out_w <= 0 or c not in (1, 3, 4):
        return ERR_ARG, dst
    if (coefs is None) != (bounds is None) or (coefs is None and out_w != w) or (coefs is not None and ksize <= 0):
        return ERR_ARG, dst
    if row_stride < w * c:
        return ERR_ARG, dst
    rs = w * c if damage == "stride_ignored" else row_stride
    pp = 4 if (damage == "pixel_pitch_4" and c == 3) else c
    need = off + (h - 1) * rs + (w - 1) * pp + c
    assert damage is not None or need <= src.size, "the stand-in would read outside the source buffer"
    if need > src.size:
        src = np.resize(src, need)
    p = np.lib.stride_tricks.as_strided(src[off:], shape=(h, w, c), strides=(rs, pp, 1))
    if c == 1:
        luma = p[..., 0].astype(np.int64)
    else:
        r, g, b = (p[..., i].astype(np.uint32) for i in range(3))
        if damage == "alpha_premultiplied" and c == 4:
            a = p[..., 3].astype(np.uint32)
            r, g, b = r * a // 255, g * a // 255, b * a // 255
        if damage == "luma_float":
            luma = np.floor(0.299 * r + 0.587 * g + 0.114 * b + 0.5).astype(np.int64)
        else:
            luma = ((r * 19595 + g * 38470 + b * 7471 + (0 if damage == "luma_no_round" else 0x8000)) >> 16).astype(np.int64)
    out = luma.astype(np.uint8) if coefs is None else _fixed_pass(luma, bounds, coefs, ksize, damage)
    n = _keep_full_blocks(h * out_w, damage)
    dst = dst.copy()
    dst[:n] = out.reshape(-1)[:n]
    return OK, dst


def vpass_standin(src, h, w, bounds, coefs, ksize, out_h, out_dtype, dst, off, dst_row_stride, damage: Optional[str] = None):
    """omr_image_vpass_to_float on host buffers: its refusals, then one value per output pixel i = y * w + x."""
    assert damage is None or damage in V_DAMAGES
    if src is None or dst is None or h <= 0 or w <= 0 or out_h <= 0 or dst_row_stride < w:
        return ERR_ARG, dst
    if (coefs is None) != (bounds is None) or (coefs is None and out_h != h) or (coefs is not None and ksize <= 0):
        return ERR_ARG, dst
    if out_dtype not in (F32, BF16):
        return ERR_UNSUPPORTED, dst
    img = src[:h * w].reshape(h, w).astype(np.int64)
    v = img if coefs is None else _fixed_pass(np.ascontiguousarray(img.T), bounds, coefs, ksize, damage).T.astype(np.int64)
    f = v.astype(np.float32)
    f = f * (np.float32(1.0) / np.float32(255.0)) if damage == "reciprocal" else f / np.float32(255.0)
    t = torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32))
    if out_dtype == BF16:
        t = (t.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16) if damage == "bf16_truncated" else t.to(torch.bfloat16)
    assert t.dtype == dst.dtype
    dst = dst.clone()
    pitch = w if damage == "dst_pitch_ignored" else dst_row_stride
    n = _keep_full_blocks(out_h * w, damage)
    idx = (off + torch.arange(out_h)[:, None] * pitch + torch.arange(w)[None, :]).reshape(-1)[:n]
    dst[idx] = t.reshape(-1)[:n]
    if damage == "writes_past":                                        # one element behind the last row's w columns
        dst[off + (out_h - 1) * pitch + w] = 0.0
    return OK, dst


def host_tables(in_size: int, out_size: int):
    """The library's host tables (image._tables_host: no GPU involved) in the stand-ins' form."""
    from omr_a2s_multimodal_transformer_amd import image
    return image._tables_host(in_size, out_size)


def standin_backend(h_damage: Optional[str] = None, v_damage: Optional[str] = None) -> Backend:
    return Backend(functools.partial(hpass_standin, damage=h_damage), functools.partial(vpass_standin, damage=v_damage), host_tables)


def resize_vertical_first(be: Backend, px: np.ndarray, out_h: int, out_w: int) -> torch.Tensor:
    """The damaged order: the vertical tables first (through the horizontal entry on the transposed image), then horizontal."""
    g = px[..., 0]
    tall = run_hpass(be, np.ascontiguousarray(g.T)[..., None], out_h).T
    wide = run_hpass(be, np.ascontiguousarray(tall)[..., None], out_w)
    return v_view(run_vpass(be, wide, out_h, "f32"), out_h, out_w, out_w, 0).clone()
