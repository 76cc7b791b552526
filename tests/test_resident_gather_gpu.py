"""omr_gather_ragged_batch (csrc/batch_gather.hip) through the C ABI: a padded batch [B, 1, H, W] from a packed store of uint8 or fp32
samples.  The reference is torch on the host: full(pad) in fp32, out[b, 0, :h, :w] = src / 255 by fp32 division (uint8) or the fp32
source, then .to(dtype); the kernel's result has to equal it BIT for bit.  The store holds a sentinel (uint8: 251, a byte no sample
has) or NaN (fp32) in front of, between and behind the samples, and every sample starts at an odd element offset; the output lies
inside a larger buffer of 7.0 that has to stay intact.  Planes: 5 x 16 (16-byte stores in both output types) and 5 x 13 (one element per
access); sample 0 fills the plane, sample 1 is 1 x 1, index 0 occurs twice."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.kernel_refs import assert_bit_equal  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
SENTINEL = 251                       # uint8 samples are drawn from 0 .. 250
GUARD = 8                            # elements of 7.0 in front of and behind the output (32 / 16 bytes: the base stays 16-byte aligned)
SRC_DTYPES = [torch.uint8, torch.float32]
DST_DTYPES = [torch.float32, torch.bfloat16]
SIZES = {16: [(5, 16), (1, 1), (3, 7), (2, 9), (4, 16)], 13: [(5, 13), (1, 1), (3, 7), (2, 9), (4, 12)]}
IDX = [0, 1, 2, 0, 3, 4]
GRID_THREADS = 256 * 256             # the launcher's cap per sample: 256 workgroups (blockIdx.x) of 256 threads


def K():
    from omr_a2s_multimodal_transformer_amd import kernels
    return kernels


def pack(sizes, src_dtype, seed):
    """(store 1-D on the host, offsets, samples): the samples at odd element offsets, the sentinel / NaN everywhere else."""
    g = torch.Generator().manual_seed(seed)
    samples, offsets, pos = [], [], 3
    for h, w in sizes:
        if src_dtype == torch.uint8:
            s = torch.randint(0, SENTINEL, (h, w), generator=g).to(torch.uint8)
            s[0, 0], s[-1, -1] = 0, 250
        else:
            s = torch.rand((h, w), generator=g) * 4 - 2
        samples.append(s)
        offsets.append(pos)
        pos += h * w
        pos += 2 if pos % 2 else 1                      # a gap of one or two elements that makes the next offset odd
    assert all(o % 2 == 1 for o in offsets)
    store = torch.full((pos + 5,), SENTINEL if src_dtype == torch.uint8 else NAN, dtype=src_dtype)
    for s, o in zip(samples, offsets):
        store[o:o + s.numel()] = s.reshape(-1)
    return store, offsets, samples


def reference(samples, idx, H, W, pad, dtype):
    out = torch.full((len(idx), 1, H, W), pad, dtype=torch.float32)
    for b, n in enumerate(idx):
        s = samples[n]
        out[b, 0, :s.shape[0], :s.shape[1]] = s.float() / 255 if s.dtype == torch.uint8 else s
    return out.to(dtype)


def guarded_out(shape, dtype, shift):
    """A contiguous view of `shape` inside a buffer of 7.0, GUARD + shift elements in: shift 0 keeps the 16-byte alignment, 1 breaks it."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((GUARD + shift + n + GUARD,), 7.0, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[GUARD + shift:GUARD + shift + n].view(shape)
    assert (out.data_ptr() % 16 == 0) == (shift == 0)
    return buf, out


def margins_intact(buf, shift, n):
    return bool((buf[:GUARD + shift] == 7.0).all()) and bool((buf[GUARD + shift + n:] == 7.0).all())


def run(store, offsets, sizes, idx, H, W, dtype, pad, shift=0):
    buf, out = guarded_out((len(idx), 1, H, W), dtype, shift)
    got = K().gather_ragged_batch(store.to(DEV), torch.tensor(offsets, dtype=torch.int64, device=DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV),
                                  torch.tensor(idx, dtype=torch.int32, device=DEV), H, W, dtype, pad, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert margins_intact(buf, shift, out.numel()), "the 7.0 around the output"
    return got


@pytest.mark.parametrize("pad", [0.0, 1.0, NAN])
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("W", [16, 13])
@pytest.mark.parametrize("dst", DST_DTYPES)
@pytest.mark.parametrize("src", SRC_DTYPES)
def test_gather_equals_the_host_collate_bit_for_bit(src, dst, W, shift, pad):
    """shift 1: the output's base pointer is one element past a 16-byte boundary, so W = 16 takes the element path too."""
    sizes = SIZES[W]
    store, offsets, samples = pack(sizes, src, 10 + W)
    got = run(store, offsets, sizes, IDX, 5, W, dst, pad, shift)
    want = reference(samples, IDX, 5, W, pad, dst)
    assert_bit_equal(got.cpu(), want, f"{src} -> {dst}, W {W}, shift {shift}, pad {pad}")
    if pad != pad:
        assert int(torch.isnan(got).sum()) == int(torch.isnan(want).sum()) > 0, "a NaN pad comes out as NaN, and only there"
    elif src == torch.uint8:
        assert not bool((got.float() == torch.tensor(SENTINEL / 255, dtype=torch.float32).to(dst).float()).any()), "a sentinel byte of the store"
    else:
        assert not bool(torch.isnan(got).any()), "a NaN of the store"
    assert_bit_equal(got[0].cpu(), got[3].cpu(), "the same index twice")


@pytest.mark.parametrize("dst", DST_DTYPES)
@pytest.mark.parametrize("src", SRC_DTYPES)
def test_b_1_and_a_plane_larger_than_every_sample(src, dst):
    sizes = SIZES[13]
    store, offsets, samples = pack(sizes, src, 31)
    for n in range(len(sizes)):                                          # B = 1, the sample's own size: nothing is padded
        h, w = sizes[n]
        got = run(store, offsets, sizes, [n], h, w, dst, NAN)
        assert_bit_equal(got.cpu(), reference(samples, [n], h, w, NAN, dst), f"B = 1, sample {n}")
        assert not bool(torch.isnan(got).any())
    got = run(store, offsets, sizes, [2, 3], 8, 24, dst, 1.0)            # an 8 x 24 plane for 3 x 7 and 2 x 9
    assert_bit_equal(got.cpu(), reference(samples, [2, 3], 8, 24, 1.0, dst), "plane larger than the samples")


def test_uint8_values_are_those_of_the_image_front_end():
    """All 256 bytes: v / 255 by a correctly rounded division, what omr_image_vpass_to_float (image.preprocess_image) writes."""
    store = torch.arange(256, dtype=torch.uint8)
    got = run(store, [0], [(16, 16)], [0], 16, 16, torch.float32, 0.0)
    want = (torch.arange(256, dtype=torch.float64) / 255).to(torch.float32).view(1, 1, 16, 16)
    assert_bit_equal(got.cpu(), want, "v / 255")
    recip = (torch.arange(256, dtype=torch.float32) * torch.tensor(1 / 255, dtype=torch.float32)).view(1, 1, 16, 16)
    assert not torch.equal(recip, want), "a multiplication by the reciprocal would differ (the reason for the division)"


@pytest.mark.parametrize("src,dst,H,W", [(torch.uint8, torch.bfloat16, 260, 2048), (torch.float32, torch.float32, 130, 2048),
                                         (torch.uint8, torch.float32, 70, 941)])
def test_more_than_one_trip_through_the_grid_stride_loop(src, dst, H, W):
    """One plane with more fragments than the 256 * 256 = 65 536 threads a sample gets: 260 * 2048 / 8 = 130 * 2048 / 4 = 66 560 fragments
    of 16 bytes, and 70 * 941 = 65 870 single elements (W odd)."""
    vec = 1 if W % 8 else (8 if dst == torch.bfloat16 else 4)
    assert H * W // vec > GRID_THREADS
    sizes = [(H, W), (H - 3, W - 5)]
    store, offsets, samples = pack(sizes, src, 50)
    got = run(store, offsets, sizes, [1, 0], H, W, dst, 0.0)
    assert_bit_equal(got.cpu(), reference(samples, [1, 0], H, W, 0.0, dst), f"{H} x {W}")


@pytest.mark.parametrize("src", SRC_DTYPES)
def test_bf16_output_is_the_cast_of_the_fp32_output(src):
    sizes = SIZES[16]
    store, offsets, _ = pack(sizes, src, 26)
    f32 = run(store, offsets, sizes, IDX, 5, 16, torch.float32, 1.0)
    b16 = run(store, offsets, sizes, IDX, 5, 16, torch.bfloat16, 1.0)
    assert_bit_equal(b16.cpu(), K().cast(f32.contiguous(), torch.bfloat16).cpu(), "bf16 vs cast(fp32)")


def test_arguments_are_checked():
    """B = 0 and B = 65 536 -> OMR_ERR_ARG (-1), as are H * W = 2^31 and a null pointer; a dtype code the entry does not take ->
    OMR_ERR_UNSUPPORTED (-3), for the source (bf16 is no store type) and for the output (uint8 is no compute type)."""
    from omr_a2s_multimodal_transformer_amd._lib import header_constant, lib
    sizes = SIZES[16]
    store, offsets, _ = pack(sizes, torch.uint8, 3)
    s = store.to(DEV)
    off = torch.tensor(offsets, dtype=torch.int64, device=DEV)
    sz = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    idx = torch.tensor(IDX, dtype=torch.int32, device=DEV)
    out = torch.zeros((len(IDX), 1, 5, 16), device=DEV)
    p = lambda t: t.data_ptr()  # noqa: E731
    q = lib().query
    U8, N, B = header_constant("OMR_DTYPE_U8"), len(sizes), len(IDX)
    assert U8 == 2
    assert q("omr_gather_ragged_batch", U8, p(s), p(off), p(sz), N, p(idx), 0, p(out), B, 5, 16, 0.0, None) == 0
    assert q("omr_gather_ragged_batch", U8, p(s), p(off), p(sz), N, p(idx), 0, p(out), 0, 5, 16, 0.0, None) == -1
    assert q("omr_gather_ragged_batch", U8, p(s), p(off), p(sz), N, p(idx), 0, p(out), 65536, 5, 16, 0.0, None) == -1
    assert q("omr_gather_ragged_batch", U8, p(s), p(off), p(sz), N, p(idx), 0, p(out), B, 1 << 15, 1 << 16, 0.0, None) == -1   # H * W = 2^31
    assert q("omr_gather_ragged_batch", U8, p(s), p(off), p(sz), 0, p(idx), 0, p(out), B, 5, 16, 0.0, None) == -1
    for hole in range(5):
        ptrs = [p(s), p(off), p(sz), p(idx), p(out)]
        ptrs[hole] = None
        assert q("omr_gather_ragged_batch", U8, ptrs[0], ptrs[1], ptrs[2], N, ptrs[3], 0, ptrs[4], B, 5, 16, 0.0, None) == -1, hole
    assert q("omr_gather_ragged_batch", 1, p(s), p(off), p(sz), N, p(idx), 0, p(out), B, 5, 16, 0.0, None) == -3
    assert q("omr_gather_ragged_batch", 7, p(s), p(off), p(sz), N, p(idx), 0, p(out), B, 5, 16, 0.0, None) == -3
    assert q("omr_gather_ragged_batch", U8, p(s), p(off), p(sz), N, p(idx), U8, p(out), B, 5, 16, 0.0, None) == -3
    assert q("omr_gather_ragged_batch", U8, p(s), p(off), p(sz), N, p(idx), 7, p(out), B, 5, 16, 0.0, None) == -3
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="invalid argument"):
        K().gather_ragged_batch(s, off, sz, idx[:0], 5, 16, torch.float32)
