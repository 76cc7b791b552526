"""omr_gather_augmented_batch (csrc/batch_augment.hip) through the C ABI against tests/augment_refs.py: BIT equality, for every record.
The packing is that of tests/test_resident_gather_gpu.py -- samples at odd element offsets, a sentinel byte (uint8) or NaN (fp32) in
front of, between and behind them, the output inside a larger buffer of 7.0 -- so a read outside a sample or a write outside the
output shows.  Planes: 5 x 16 (16-byte stores in both output types), 5 x 13 (one element per access) and 5 x 16 one element past a
16-byte boundary; index 0 occurs twice.  Every case also checks: the margins are intact, no gap element reaches the output (fp32
store: no NaN; uint8 store: the same samples packed with another gap byte give the same bits), two runs agree to the bit."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_refs as AR  # noqa: E402
from omr_a2s_multimodal_transformer_amd import augment as A  # noqa: E402
from oracle.kernel_refs import assert_bit_equal  # noqa: E402
from test_resident_gather_gpu import DEV, DST_DTYPES, GRID_THREADS, IDX, SIZES, SRC_DTYPES, guarded_out, margins_intact, pack  # noqa: E402

LAYOUTS = {"vec16": (16, 0), "elem13": (13, 0), "misaligned16": (16, 1)}          # name: (W, output shift in elements)
OTHER_GAP = 7                                                                        # a second gap byte for the uint8 store
H = 5


def K():
    from omr_a2s_multimodal_transformer_amd import kernels
    return kernels


def packed(sizes, src_dtype, seed):
    """pack() plus a -0.0 inside an fp32 sample, and for uint8 a second store with another byte in the gaps."""
    store, offsets, samples = pack(sizes, src_dtype, seed)
    inside = torch.zeros(store.shape, dtype=torch.bool)
    for s, o in zip(samples, offsets):
        inside[o:o + s.numel()] = True
    if src_dtype == torch.float32:
        samples[2][1, 3] = -0.0
        store[offsets[2] + 1 * samples[2].shape[1] + 3] = -0.0
        return store, None, offsets, samples
    other = store.clone()
    other[~inside] = OTHER_GAP
    return store, other, offsets, samples


def launch(store, offsets, sizes, idx, records, H_, W, dtype, pad, shift=0):
    buf, out = guarded_out((len(idx), 1, H_, W), dtype, shift)
    raw = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(len(idx), A.AUG_DTYPE.itemsize).copy()).to(DEV)
    got = K().gather_augmented_batch(store.to(DEV), torch.tensor(offsets, dtype=torch.int64, device=DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV),
                                     torch.tensor(idx, dtype=torch.int32, device=DEV), raw, H_, W, dtype, pad, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert margins_intact(buf, shift, out.numel()), "the 7.0 around the output"
    return got.cpu()


def affine(h, w, deg, scale, shear, W, **fields):
    t = math.radians(deg)
    rot = np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
    return A.affine_record(h, w, rot @ np.array([[1.0, 0.0], [shear, 1.0]]) @ np.diag([scale, scale]), (H, W), **fields)


NAN = float("nan")
# name -> record of batch row b for a sample of h x w in a plane of H x W; `u8`: the store's type (units of gain / bias / noise / fill)
CASES = {
    "identity": lambda b, h, w, W, u8: A.identity(h, w),
    "integer_shift": lambda b, h, w, W, u8: A.record(m=(1, 0, 1, 0, 1, -2), fill=255.0 if u8 else -3.5, out_h=H, out_w=W),
    "half_pixel_shift": lambda b, h, w, W, u8: A.record(m=(1, 0, 0.5, 0, 1, 0.5) if b % 2 else (1, 0, 0, 0, 1, 0.5), fill=255.0 if u8 else 0.0, out_h=h,
                                                        out_w=w),
    "rotate_2_scale_0.9": lambda b, h, w, W, u8: affine(h, w, 2.0, 0.9, 0.0, W, fill=255.0 if u8 else 0.0),
    "rotate_-1.5_scale_1.15_shear": lambda b, h, w, W, u8: affine(h, w, -1.5, 1.15, 0.2, W, fill=255.0 if u8 else 0.0),
    "wholly_outside": lambda b, h, w, W, u8: A.record(m=(1, 0, 100, 0, 1, -100) if b % 2 else (1, 0, 1000, 0, 1, 1000), fill=129.0 if u8 else 0.75,
                                                      out_h=H, out_w=W),
    "nan_in_m": lambda b, h, w, W, u8: A.record(m=[(NAN, 0, 0, 0, 1, 0), (1, 0, 0, 0, 1, NAN), (1, NAN, 0, 0, NAN, 0)][b % 3], fill=77.0 if u8 else 0.25,
                                                out_h=H, out_w=W),
    "gain_bias_clamp": lambda b, h, w, W, u8: A.record(m=(1, 0, 0, 0, 1, 0.25), gain=3.0, bias=-200.0 if u8 else -2.0, fill=255.0 if u8 else 0.0,
                                                       out_h=h, out_w=w),
    "noise": lambda b, h, w, W, u8: affine(h, w, 1.0, 1.0, 0.0, W, noise=40.0 if u8 else 0.5, gain=0.9, bias=10.0 if u8 else 0.1,
                                           fill=255.0 if u8 else 0.0, seed=(0x9ABCDEF0 << 32) | (0x12345678 + b)),
    "bands": lambda b, h, w, W, u8: A.record(m=(1, 0, 0.5, 0, 1, 0), fill=255.0 if u8 else 0.0, out_h=h, out_w=w, rows=[(1, 2), (2, 100)][:1 + b % 2],
                                             cols=[(3, 0), (-2, 4)] if b % 2 else [(5, 3), (6, 4)]),
    "extent_larger_than_the_plane": lambda b, h, w, W, u8: A.record(fill=255.0 if u8 else 0.5, out_h=1000 + b, out_w=(1 << 30) if b % 2 else W + 1),
}
MIXED = ["identity", "noise", "bands", "rotate_2_scale_0.9", "gain_bias_clamp", "half_pixel_shift"]     # row b of "mixed" takes case MIXED[b]


def records_of(case, sizes, W, u8):
    names = MIXED if case == "mixed" else [case] * len(IDX)
    return A.stack([CASES[names[b]](b, *sizes[n], W, u8) for b, n in enumerate(IDX)])


@pytest.mark.parametrize("case", list(CASES) + ["mixed"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dst", DST_DTYPES)
@pytest.mark.parametrize("src", SRC_DTYPES)
def test_augmented_gather_equals_the_numpy_restatement_bit_for_bit(src, dst, layout, case):
    W, shift = LAYOUTS[layout]
    sizes = SIZES[W]
    u8 = src == torch.uint8
    store, other, offsets, samples = packed(sizes, src, 10 + W)
    records = records_of(case, sizes, W, u8)
    pad = 1.0 if case != "identity" else 0.0
    got = launch(store, offsets, sizes, IDX, records, H, W, dst, pad, shift)
    want = AR.gather_augmented_ref(samples, IDX, records, H, W, pad, dst)
    assert_bit_equal(got, want, f"{case}: {src} -> {dst}, {layout}")
    again = launch(store, offsets, sizes, IDX, records, H, W, dst, pad, shift)
    assert_bit_equal(again, got, "two runs")
    if u8:
        assert_bit_equal(launch(other, offsets, sizes, IDX, records, H, W, dst, pad, shift), got, "another byte in the gaps of the store")
    else:
        assert not bool(torch.isnan(got).any()), "a NaN from the gaps of the store"
    if case == "identity":
        buf, out = guarded_out((len(IDX), 1, H, W), dst, shift)
        plain = K().gather_ragged_batch(store.to(DEV), torch.tensor(offsets, dtype=torch.int64, device=DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV),
                                        torch.tensor(IDX, dtype=torch.int32, device=DEV), H, W, dst, pad, out=out)
        assert_bit_equal(got, plain.cpu(), "the plain gather")
        assert_bit_equal(got[0], got[3], "the same index twice, the same record")
        if not u8 and dst == torch.float32:
            assert int(got[2].view(torch.int32)[0, 1, 3]) == -2 ** 31, "-0.0 keeps its sign"
    if case == "mixed":
        assert not torch.equal(got[0].float(), got[3].float()), "the same index twice, different records"
    if case in ("wholly_outside", "nan_in_m"):
        fill = torch.tensor(float(records[0]["fill"] / np.float32(255.0 if u8 else 1.0)), dtype=torch.float32).to(dst)      # the fp32 quotient
        assert bool((got == fill).all()), "nothing but fill"


def test_gain_and_bias_clamp_at_both_ends_of_a_u8_store():
    """The case of the matrix really reaches both ends: grays 0 .. 250 under 3 g - 200 leave [0, 255] on either side."""
    sizes = SIZES[16]
    store, _, offsets, samples = packed(sizes, torch.uint8, 26)
    records = records_of("gain_bias_clamp", sizes, 16, True)
    got = launch(store, offsets, sizes, IDX, records, H, 16, torch.float32, 0.5)
    inside = got[0, 0, :5, :16]
    assert float(inside.min()) == 0.0 and float(inside.max()) == 1.0 and bool(((inside > 0) & (inside < 1)).any())


@pytest.mark.parametrize("pad", [0.0, NAN])
def test_pad_outside_the_extent_is_the_plain_gathers(pad):
    """A NaN pad stays where the plain gather puts it: outside the extents, in both output types."""
    sizes = SIZES[16]
    store, _, offsets, samples = packed(sizes, torch.uint8, 12)
    records = records_of("rotate_2_scale_0.9", sizes, 16, True)
    for dst in DST_DTYPES:
        got = launch(store, offsets, sizes, IDX, records, H, 16, dst, pad)
        assert_bit_equal(got, AR.gather_augmented_ref(samples, IDX, records, H, 16, pad, dst), f"pad {pad} -> {dst}")
        outside = torch.ones(got.shape, dtype=torch.bool)
        for b in range(len(IDX)):
            outside[b, 0, :int(records[b]["out_h"]), :int(records[b]["out_w"])] = False
        assert outside.any() and bool(torch.isnan(got[outside]).all() if pad != pad else (got[outside] == 0).all())
        assert not bool(torch.isnan(got[~outside]).any())


def test_more_than_one_trip_through_the_grid_stride_loop():
    """fp32 -> fp32, one plane of 300 x 1024: 76 800 fragments of 16 bytes for the 65 536 threads a sample gets."""
    Hb, Wb = 300, 1024
    assert Hb * Wb // 4 > GRID_THREADS
    sizes = [(Hb, Wb), (Hb - 3, Wb - 5)]
    store, offsets, samples = pack(sizes, torch.float32, 50)
    t = math.radians(2.0)
    rot = np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
    records = A.stack([A.affine_record(Hb - 3, Wb - 5, rot * 0.9, (Hb, Wb), noise=0.25, gain=1.1, bias=-0.05, seed=99, rows=[(100, 7)], cols=[(1000, 50)]),
                       A.record(m=(1, 0, 0.5, 0, 1, 0.5), out_h=Hb, out_w=Wb)])
    got = launch(store, offsets, sizes, [1, 0], records, Hb, Wb, torch.float32, 0.0)
    assert_bit_equal(got, AR.gather_augmented_ref(samples, [1, 0], records, Hb, Wb, 0.0, torch.float32), f"{Hb} x {Wb}")
    assert not bool(torch.isnan(got).any())


def test_arguments_are_checked():
    """What omr_gather_ragged_batch refuses, and a null `aug`: OMR_ERR_ARG (-1); a dtype code the entry does not take: -3."""
    from omr_a2s_multimodal_transformer_amd._lib import header_constant, lib
    sizes = SIZES[16]
    store, _, offsets, _ = packed(sizes, torch.uint8, 3)
    s = store.to(DEV)
    off = torch.tensor(offsets, dtype=torch.int64, device=DEV)
    sz = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    idx = torch.tensor(IDX, dtype=torch.int32, device=DEV)
    records = records_of("identity", sizes, 16, True)
    aug = torch.from_numpy(records.view(np.uint8).reshape(len(IDX), 88).copy()).to(DEV)
    out = torch.zeros((len(IDX), 1, 5, 16), device=DEV)
    p = lambda t: t.data_ptr()  # noqa: E731
    q = lib().query
    U8, N, B = header_constant("OMR_DTYPE_U8"), len(sizes), len(IDX)
    name = "omr_gather_augmented_batch"
    assert q(name, U8, p(s), p(off), p(sz), N, p(idx), p(aug), 0, p(out), B, 5, 16, 0.0, None) == 0
    assert q(name, U8, p(s), p(off), p(sz), N, p(idx), None, 0, p(out), B, 5, 16, 0.0, None) == -1
    assert q(name, U8, p(s), p(off), p(sz), N, p(idx), p(aug), 0, p(out), 0, 5, 16, 0.0, None) == -1
    assert q(name, U8, p(s), p(off), p(sz), N, p(idx), p(aug), 0, p(out), 65536, 5, 16, 0.0, None) == -1
    assert q(name, U8, p(s), p(off), p(sz), N, p(idx), p(aug), 0, p(out), B, 1 << 15, 1 << 16, 0.0, None) == -1   # H * W = 2^31
    assert q(name, U8, p(s), p(off), p(sz), 0, p(idx), p(aug), 0, p(out), B, 5, 16, 0.0, None) == -1
    assert q(name, U8, p(s), p(off), p(sz), N, p(idx), p(aug), 0, p(out), B, 0, 16, 0.0, None) == -1
    for hole in range(6):
        ptrs = [p(s), p(off), p(sz), p(idx), p(aug), p(out)]
        ptrs[hole] = None
        assert q(name, U8, ptrs[0], ptrs[1], ptrs[2], N, ptrs[3], ptrs[4], 0, ptrs[5], B, 5, 16, 0.0, None) == -1, hole
    assert q(name, 1, p(s), p(off), p(sz), N, p(idx), p(aug), 0, p(out), B, 5, 16, 0.0, None) == -3
    assert q(name, 7, p(s), p(off), p(sz), N, p(idx), p(aug), 0, p(out), B, 5, 16, 0.0, None) == -3
    assert q(name, U8, p(s), p(off), p(sz), N, p(idx), p(aug), U8, p(out), B, 5, 16, 0.0, None) == -3
    assert q(name, U8, p(s), p(off), p(sz), N, p(idx), p(aug), 7, p(out), B, 5, 16, 0.0, None) == -3
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="invalid argument"):
        K().gather_augmented_batch(s, off, sz, idx[:0], aug[:0], 5, 16, torch.float32)
    with pytest.raises(AssertionError):
        K().gather_augmented_batch(s, off, sz, idx, aug[:, :80].contiguous(), 5, 16, torch.float32)
