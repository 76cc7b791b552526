"""CPU-only: the numpy restatement of omr_gather_augmented_batch (tests/augment_refs.py) against things that need no kernel -- the host
collate, slices, means, the oracle's hash -- and the host logic of omr_a2s_multimodal_transformer_amd.augment and of the loader: the
struct mirror, pure draws, extents under a limit, plans on augmented sizes, shards, mask lengths."""
import ctypes
import re

import numpy as np
import pytest
import torch

import augment_refs as AR
from omr_a2s_multimodal_transformer_amd import _lib, augment as A, resident
from oracle.attention_refs import _hash32
from oracle.kernel_refs import assert_bit_equal
from test_resident_gather_gpu import IDX, SIZES, pack, reference

F = np.float32


def rec_stack(*records):
    return A.stack(records)


# ------------------------------------------------------------------------------------------------ the reference

@pytest.mark.parametrize("dst", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("src", [torch.uint8, torch.float32])
@pytest.mark.parametrize("W", [16, 13])
def test_identity_record_is_the_host_collate(src, dst, W):
    sizes = SIZES[W]
    _, _, samples = pack(sizes, src, 10 + W)
    if src == torch.float32:
        samples[2][1, 3] = -0.0
    records = rec_stack(*[A.identity(*sizes[n]) for n in IDX])
    for pad in (0.0, 1.0):
        got = AR.gather_augmented_ref(samples, IDX, records, 5, W, pad, dst)
        assert_bit_equal(got, reference(samples, IDX, 5, W, pad, dst), f"{src} -> {dst}, W {W}, pad {pad}")


@pytest.mark.parametrize("src", [torch.uint8, torch.float32])
def test_integer_translation_is_a_shifted_slice_with_fill(src):
    """dst (i, j) reads src (i + 1, j - 2): rows move up by one, columns right by two; what comes from outside the plane is `fill`."""
    _, _, samples = pack([(5, 13)], src, 4)
    s = samples[0].numpy().astype(F)
    fill = 200.0 if src == torch.uint8 else -3.5
    r = A.record(m=(1, 0, 1, 0, 1, -2), fill=fill, out_h=5, out_w=13)
    got = AR.augment_plane(samples[0].numpy(), r, 5, 13, 9.0)
    want = np.full((5, 13), fill, dtype=F)
    want[:4, 2:] = s[1:, :11]
    if src == torch.uint8:
        want = (want / F(255)).astype(F)
    assert got.tobytes() == want.tobytes()


def test_half_pixel_shift_is_the_mean_of_neighbours():
    g = np.random.default_rng(3)
    s = g.integers(0, 64, (4, 9)).astype(F)                         # small integers: the mean of two is exact in fp32
    r = A.record(m=(1, 0, 0, 0, 1, 0.5), fill=10.0, out_h=4, out_w=9)
    got = AR.augment_plane(s, r, 4, 9, 0.0)
    want = np.empty((4, 9), dtype=F)
    want[:, :8] = (s[:, :8] + s[:, 1:]) / 2
    want[:, 8] = (s[:, 8] + 10.0) / 2
    assert got.tobytes() == want.tobytes()
    r = A.record(m=(1, 0, 0.5, 0, 1, 0.5), fill=10.0, out_h=3, out_w=8)      # both axes: the mean of four
    got = AR.augment_plane(s, r, 3, 8, 0.0)
    want = (s[:3, :8] + s[:3, 1:] + s[1:, :8] + s[1:, 1:]) / 4
    assert got.tobytes() == want.astype(F).tobytes()


def test_outside_extent_is_pad_and_bands_are_fill():
    s = np.arange(20, dtype=np.uint8).reshape(4, 5)
    r = A.record(fill=255.0, out_h=3, out_w=9, rows=[(1, 1), (7, 0)], cols=[(4, 100), (-3, 4)])
    got = AR.augment_plane(s, r, 4, 6, 0.5)                          # out_w 9 is clamped to the plane's 6
    want = np.full((4, 6), 0.5, dtype=F)
    body = np.full((3, 6), 255.0, dtype=F)
    body[:, :5] = s[:3]
    body[1, :] = 255.0
    body[:, 4:] = 255.0
    body[:, :1] = 255.0
    want[:3] = (body / F(255)).astype(F)
    assert got.tobytes() == want.tobytes()


def test_hash_is_the_oracles_hash32():
    idx = np.concatenate([np.arange(1000, dtype=np.uint32), np.array([2**31, 2**32 - 1, 123456789], dtype=np.uint32)])
    for lo, hi in ((0, 0), (0xDEADBEEF, 0x12345678), (0xFFFFFFFF, 0xFFFFFFFF)):
        with np.errstate(over="ignore"):
            want = _hash32(np.uint32(lo), np.uint32(hi), idx.copy())
        assert np.array_equal(AR.hash32(lo, hi, idx), want)
    r = ((AR.hash32(5, 6, idx) >> np.uint32(8)).astype(F) * AR.TWO_M23 - F(1))
    assert r.min() >= -1 and r.max() < 1


# ------------------------------------------------------------------------------------------------ the struct mirror

def test_aug_dtype_has_the_layout_of_the_c_struct():
    text = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+OmrAugment\s*\{(.*?)\}\s*OmrAugment\s*;", text, flags=re.S).group(1)
    ctype = {"float": ctypes.c_float, "int": ctypes.c_int, "unsigned": ctypes.c_uint}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base, names = decl.split(None, 1)
        for name in (n.strip() for n in names.split(",")):
            dims = [int(d) for d in re.findall(r"\[(\d+)\]", name)]
            t = ctype[base]
            for d in reversed(dims):
                t = t * d
            fields.append((name.split("[")[0], t))

    class C(ctypes.Structure):
        _fields_ = fields

    assert [n for n, _ in fields] == list(A.AUG_DTYPE.names)
    assert ctypes.sizeof(C) == A.AUG_DTYPE.itemsize == 88
    from omr_a2s_multimodal_transformer_amd.kernels import AUGMENT_RECORD_BYTES
    assert AUGMENT_RECORD_BYTES == 88
    for name, t in fields:
        sub, offset = A.AUG_DTYPE.fields[name][:2]
        assert getattr(C, name).offset == offset and ctypes.sizeof(t) == sub.itemsize, name
    r = A.record(m=(1, 2, 3, 4, 5, 6), gain=7, bias=8, noise=9, fill=10, out_h=11, out_w=12, seed=(14 << 32) | 13, rows=[(15, 16), (17, 18)],
                 cols=[(19, 20), (21, 22)])
    c = C.from_buffer_copy(r.tobytes())
    flat = list(c.m) + [c.gain, c.bias, c.noise, c.fill, c.out_h, c.out_w, c.seed_lo, c.seed_hi] + [v for b in c.rows for v in b] + [v for b in c.cols for v in b]
    assert flat == list(range(1, 23))
    ident = A.identity(7, 9)
    assert ident["m"].tolist() == [1, 0, 0, 0, 1, 0] and (ident["out_h"], ident["out_w"]) == (7, 9) and ident["gain"] == 1 and ident["noise"] == 0
    with pytest.raises(ValueError):
        A.record(rows=[(0, 1)] * 3)


# ------------------------------------------------------------------------------------------------ draws

IMG = dict(scale=(0.8, 1.25), aspect=(0.9, 1.1), rotate_deg=3.0, shear=0.1, gain=(0.8, 1.2), bias=(-20.0, 20.0), noise=6.0, limit=(64, 96))
SPEC = dict(time_masks=2, max_time=12, freq_masks=2, max_freq=5, time_stretch=(0.8, 1.25), gain=(0.9, 1.1), limit=(35, 40))


@pytest.mark.parametrize("make", [lambda: A.ImageAugment(**IMG), lambda: A.SpecAugment(**SPEC)])
def test_draw_is_a_pure_function_of_its_five_arguments(make):
    a, b = make(), make()
    base = a.draw(7, 2, 5, 30, 40)
    for _ in range(3):
        b.draw(1, 1, 1, 9, 9)                                        # other draws in between leave no trace
    assert base.tobytes() == b.draw(7, 2, 5, 30, 40).tobytes() == a.draw(7, 2, 5, 30, 40).tobytes()
    for other in ((8, 2, 5, 30, 40), (7, 3, 5, 30, 40), (7, 2, 6, 30, 40), (7, 2, 5, 31, 40), (7, 2, 5, 30, 41)):
        assert a.draw(*other).tobytes() != base.tobytes(), other
    sizes = [(30, 40), (12, 33), (35, 40)]
    table = A.draw_all(a, 7, 2, sizes)
    assert table.dtype == A.AUG_DTYPE and table.shape == (3,)
    assert all(table[n].tobytes() == a.draw(7, 2, n, *sizes[n]).tobytes() for n in range(3))
    assert np.array_equal(A.augmented_sizes(a, 7, 2, sizes), A.extents(table)) and A.extents(table).dtype == np.int64


def forward_corners(r, h, w):
    """Where the four corners of the source rectangle [0, h] x [0, w] land in the destination (points; pixel i covers [i, i + 1))."""
    m = r["m"].astype(np.float64)
    M, t = np.array([[m[0], m[1]], [m[3], m[4]]]), np.array([m[2], m[5]])
    corners = np.array([[0.0, 0.0], [h, 0.0], [0.0, w], [h, w]])
    return (np.linalg.solve(M, (corners - 0.5 - t).T)).T + 0.5


def test_extents_never_exceed_the_limit_and_the_corners_stay_inside():
    """The plane of the largest sample IS the limit: any growth has to be taken back, and the whole rectangle still lies in the extent
    (to 1e-3 px: m is stored in fp32)."""
    aug = A.ImageAugment(**IMG)
    hit = 0
    for n, (h, w) in enumerate([(64, 96), (64, 96), (60, 96), (64, 20), (10, 96), (37, 50), (17, 9)] * 6):
        r = aug.draw(3, n // 7, n, h, w)
        oh, ow = int(r["out_h"]), int(r["out_w"])
        assert 1 <= oh <= 64 and 1 <= ow <= 96, (h, w, oh, ow)
        p = forward_corners(r, h, w)
        assert p.min() >= -1e-3 and p[:, 0].max() <= oh + 1e-3 and p[:, 1].max() <= ow + 1e-3, (h, w, oh, ow, p)
        hit += oh == 64 or ow == 96
    assert hit >= 6                                                  # the limit was reached, not just approached
    spec = A.SpecAugment(**SPEC)
    for n in range(30):
        r = spec.draw(3, 0, n, 35, 40 - n % 3)
        assert int(r["out_h"]) == 35 and 1 <= int(r["out_w"]) <= 40 and r["m"][:3].tolist() == [1, 0, 0] and r["m"][3] == 0
    free = A.ImageAugment(scale=(2.0, 2.0))                          # no limit: twice the size
    assert A.extents(free.draw(0, 0, 0, 10, 15)).tolist() == [[20, 30]]
    unit = A.ImageAugment().draw(0, 0, 0, 10, 15)                    # nothing asked for: the identity map
    assert np.array_equal(unit["m"], np.array([1, 0, 0, 0, 1, 0], dtype=F)) and A.extents(unit).tolist() == [[10, 15]] and unit["gain"] == 1


def test_masks_never_exceed_their_maxima_and_lie_inside_the_extent():
    spec = A.SpecAugment(**SPEC)
    longest_t = longest_f = 0
    for n in range(200):
        r = spec.draw(11, n % 4, n, 35, 40)
        for start, length in r["cols"].tolist():
            assert 0 <= length <= 12 and 0 <= start and start + length <= int(r["out_w"])
            longest_t = max(longest_t, length)
        for start, length in r["rows"].tolist():
            assert 0 <= length <= 5 and 0 <= start and start + length <= int(r["out_h"])
            longest_f = max(longest_f, length)
    assert (longest_t, longest_f) == (12, 5)                         # the maxima are reached
    one = A.SpecAugment(time_masks=1, max_time=3).draw(0, 0, 0, 35, 40)
    assert one["cols"][1].tolist() == [0, 0] and one["rows"].tolist() == [[0, 0], [0, 0]]
    with pytest.raises(ValueError):
        A.SpecAugment(time_masks=3, max_time=3)


# ------------------------------------------------------------------------------------------------ the loader (host side only)

class FakeStore:
    def __init__(self, sizes):
        self.sizes = torch.tensor(sizes, dtype=torch.int64)


class FakeDataset:
    """What ResidentLoader touches of a ResidentDataset, without a device: stores[k].sizes, target_lens(), batch()."""

    def __init__(self, *tables):
        self.stores = [FakeStore(t) for t in tables]
        self.calls = []

    def target_lens(self):
        return [3 + n % 5 for n in range(len(self.stores[0].sizes))]

    def batch(self, indices, dtype, records=None):
        self.calls.append((list(indices), records))
        return len(self.calls) - 1


def size_table(n, seed, hmax, wmax):
    g = torch.Generator().manual_seed(seed)
    return [(int(torch.randint(8, hmax + 1, (1,), generator=g)), int(torch.randint(8, wmax + 1, (1,), generator=g))) for _ in range(n)]


def test_a_plan_with_augmentation_covers_every_sample_once_and_budgets_the_augmented_sizes():
    table = size_table(41, 5, 64, 96)
    ds = FakeDataset(table)
    aug = A.ImageAugment(**IMG)
    budget = 3 * 64 * 96
    loader = resident.ResidentLoader(ds, 4, torch.float32, augment=aug, max_padded_pixels=budget, chunk_batches=3, seed=9, rank=0, world=1)
    plain = resident.ResidentLoader(ds, 4, torch.float32, max_padded_pixels=budget, chunk_batches=3, seed=9, rank=0, world=1)
    for epoch in (0, 1):
        loader.set_epoch(epoch)
        plain.set_epoch(epoch)
        plan = loader.plan()
        assert sorted(n for b in plan for n in b) == list(range(41))
        ext = A.augmented_sizes(aug, 9, epoch, table)
        assert plan == resident.plan_batches(ext, 4, target_lens=ds.target_lens(), max_padded_pixels=budget, chunk_batches=3, seed=9, epoch=epoch)
        for b in plan:
            assert len(b) == 1 or len(b) * ext[b, 0].max() * ext[b, 1].max() <= budget
        assert plain.plan() == resident.plan_batches(table, 4, target_lens=ds.target_lens(), max_padded_pixels=budget, chunk_batches=3, seed=9, epoch=epoch)
    ds.calls.clear()
    got = list(loader)
    assert got == list(range(len(loader.plan())))
    for (indices, records), want in zip(ds.calls, loader.plan()):
        assert indices == want and len(records) == 1 and records[0].dtype == A.AUG_DTYPE
        assert all(records[0][k].tobytes() == aug.draw(9, 1, n, *table[n]).tobytes() for k, n in enumerate(indices))
    ds.calls.clear()
    list(plain)
    assert all(records is None for _, records in ds.calls)           # no augmentation: batch() is called as it always was


def test_world_2_shards_use_the_records_of_world_1():
    ti, ta = size_table(23, 6, 64, 96), size_table(23, 7, 35, 40)
    img, spec = A.ImageAugment(**IMG), A.SpecAugment(**SPEC)
    kw = dict(augment=img, augment2=spec, max_padded_pixels=4 * (64 * 96 + 35 * 40), chunk_batches=2, seed=4)
    whole = FakeDataset(ti, ta)
    one = resident.ResidentLoader(whole, 3, torch.float32, rank=0, world=1, **kw)
    one.set_epoch(2)
    list(one)
    by_sample = {}
    for indices, (ri, ra) in whole.calls:
        for k, n in enumerate(indices):
            by_sample[n] = (ri[k].tobytes(), ra[k].tobytes())
    assert sorted(by_sample) == list(range(23))
    seen = []
    for rank in (0, 1):
        ds = FakeDataset(ti, ta)
        shard = resident.ResidentLoader(ds, 3, torch.float32, rank=rank, world=2, **kw)
        shard.set_epoch(2)
        assert shard.plan() == resident.shard_batches(one.plan(), rank, 2)
        list(shard)
        for indices, (ri, ra) in ds.calls:
            seen.extend(indices)
            assert all((ri[k].tobytes(), ra[k].tobytes()) == by_sample[n] for k, n in enumerate(indices))
    assert set(seen) == set(range(23))
    only2 = resident.ResidentLoader(FakeDataset(ti, ta), 3, torch.float32, rank=0, world=1, augment2=spec, seed=4)
    list(only2)
    assert all(r[0] is None and r[1].dtype == A.AUG_DTYPE for _, r in only2.dataset.calls)
    with pytest.raises(ValueError):
        resident.ResidentLoader(FakeDataset(ti), 3, torch.float32, rank=0, world=1, augment2=spec)
