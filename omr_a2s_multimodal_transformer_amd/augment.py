"""Per-sample augmentation for a device-resident training set: the host side of `omr_gather_augmented_batch` (csrc/batch_augment.hip).

The reference augments with a second, pre-rendered copy of every score (`image_distorted`, src/data/ar_dataset.py:258-265,377,
`use_distorted_images` of train.py:25): the same distortion every epoch, nothing for spectrograms.  Here a batch row carries one
`OmrAugment` record and the gather kernel applies it while it builds the padded plane: an affine map with a bilinear blend, gain,
bias, hashed noise and up to two row and two column bands of a fill value (include/omr_hip.h states every pixel's value).

  AUG_DTYPE / record / identity   the numpy mirror of the C struct and its constructors
  ImageAugment                    rotate . shear . diag(sy, sx) about the centre, gain / bias / noise: a fresh distortion of a score
  SpecAugment                     time stretch, time and frequency masks, gain: SpecAugment-style masking of a spectrogram
  draw_all / augmented_sizes      the records / extents of a whole size table for one (seed, epoch)

A record is a pure function of (seed, epoch, n, h, w) -- never of the batch a sample falls into, of the rank or of the world size --
so every rank and every re-plan of an epoch see the same augmented sample n.  Host arithmetic only (numpy; no torch.cuda)."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np

AUG_DTYPE = np.dtype([("m", "<f4", (6,)), ("gain", "<f4"), ("bias", "<f4"), ("noise", "<f4"), ("fill", "<f4"), ("out_h", "<i4"), ("out_w", "<i4"),
                      ("seed_lo", "<u4"), ("seed_hi", "<u4"), ("rows", "<i4", (2, 2)), ("cols", "<i4", (2, 2))])
IDENTITY_M = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
_STREAM = 0x6F6D7261                 # first word of every draw's seed sequence: keeps these streams apart from other users of the seed

Range = Tuple[float, float]


def record(m: Sequence[float] = IDENTITY_M, gain: float = 1.0, bias: float = 0.0, noise: float = 0.0, fill: float = 0.0, out_h: int = 0,
           out_w: int = 0, seed: int = 0, rows: Sequence[Sequence[int]] = (), cols: Sequence[Sequence[int]] = ()) -> np.ndarray:
    """One OmrAugment as a 0-d array of AUG_DTYPE.  m: source (y, x) of destination pixel (i, j), y = m0*i + m1*j + m2,
    x = m3*i + m4*j + m5 (rounded to fp32 here); seed: the 64-bit noise stream; rows / cols: up to two (start, length) bands each."""
    if len(rows) > 2 or len(cols) > 2:
        raise ValueError("a record holds at most two row bands and two column bands")
    r = np.zeros((), dtype=AUG_DTYPE)
    r["m"] = np.asarray(m, dtype=np.float64).reshape(6).astype(np.float32)
    r["gain"], r["bias"], r["noise"], r["fill"] = gain, bias, noise, fill
    r["out_h"], r["out_w"] = out_h, out_w
    r["seed_lo"], r["seed_hi"] = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for k, band in enumerate(rows):
        r["rows"][k] = (int(band[0]), int(band[1]))
    for k, band in enumerate(cols):
        r["cols"][k] = (int(band[0]), int(band[1]))
    return r


def identity(h: int, w: int) -> np.ndarray:
    """The record under which the augmented gather writes the plain gather's bits."""
    return record(out_h=h, out_w=w)


def stack(records: Sequence[np.ndarray]) -> np.ndarray:
    """Records -> one contiguous array [B] of AUG_DTYPE."""
    return np.array([np.asarray(r, dtype=AUG_DTYPE).reshape(()) for r in records], dtype=AUG_DTYPE).reshape(-1)


def extents(records: np.ndarray) -> np.ndarray:
    """int64 [B, 2] = (out_h, out_w) of each record."""
    records = np.asarray(records, dtype=AUG_DTYPE).reshape(-1)
    return np.stack([records["out_h"], records["out_w"]], axis=1).astype(np.int64)


def _rng(seed: int, epoch: int, n: int, h: int, w: int) -> np.random.Generator:
    words = [_STREAM] + [int(v) & 0xFFFFFFFFFFFFFFFF for v in (seed, epoch, n, h, w)]
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence(words)))


def _uniform(rng: np.random.Generator, lo_hi: Range) -> float:
    """One draw is always consumed, so a degenerate range does not shift the draws after it."""
    lo, hi = float(lo_hi[0]), float(lo_hi[1])
    u = float(rng.random())
    return lo + (hi - lo) * u


def _pair(v, name: str) -> Range:
    lo, hi = (v, v) if isinstance(v, (int, float)) else v
    if not float(lo) <= float(hi):
        raise ValueError(f"{name}: expected lo <= hi, got {v!r}")
    return float(lo), float(hi)


def affine_record(h: int, w: int, A: np.ndarray, limit: Optional[Tuple[int, int]], fit: str = "both", **fields) -> np.ndarray:
    """The record of the forward map p -> A (p - c) about the centre c = (h / 2, w / 2) of the source rectangle [0, h] x [0, w] (pixel
    i covers [i, i + 1), its value sits at i + 0.5), shifted so that the bounding box of the transformed rectangle starts at 0.
    out_h, out_w = the ceiling of that box.  A box larger than `limit` = (Hmax, Wmax) shrinks A by min(Hmax / box_h, Wmax / box_w)
    (fit "both") or by Wmax / box_w along x alone (fit "x": a stretch that has no say over the height): the whole sample still fits,
    nothing is cropped.  m is the inverse map between pixel indices, computed in float64 and stored as fp32."""
    A = np.asarray(A, dtype=np.float64).reshape(2, 2)
    c = np.array([h / 2.0, w / 2.0])
    corners = np.array([[0.0, 0.0], [h, 0.0], [0.0, w], [h, w]]) - c

    def box(A):
        q = corners @ A.T
        return q.min(axis=0), q.max(axis=0) - q.min(axis=0)

    lo, size = box(A)
    if limit is not None:
        if fit == "x":
            A = A @ np.diag([1.0, min(1.0, limit[1] / size[1])])
        else:
            A = A * min(1.0, limit[0] / size[0], limit[1] / size[1])
        lo, size = box(A)
    out_h, out_w = (max(1, int(math.ceil(s - 1e-6))) for s in size)      # 1e-6 px: a box of limit + rounding is not limit + 1
    if limit is not None:
        out_h, out_w = (min(out_h, limit[0]), min(out_w, limit[1])) if fit == "both" else (out_h, min(out_w, limit[1]))
    Ainv = np.linalg.inv(A)
    t = Ainv @ (0.5 + lo) + c - 0.5                      # index i -> point i + 0.5 -> source point -> source index
    return record(m=(Ainv[0, 0], Ainv[0, 1], t[0], Ainv[1, 0], Ainv[1, 1], t[1]), out_h=out_h, out_w=out_w, **fields)


class ImageAugment:
    """A fresh geometric and photometric distortion of a score image per (sample, epoch).  Forward map: rotate . shear . diag(sy, sx)
    about the sample's centre with sy = s / sqrt(a), sx = s * sqrt(a) for a scale s and an aspect a drawn from their ranges, the
    angle uniform in [-rotate_deg, rotate_deg], the shear (x += k y) uniform in [-shear, shear].  gain / bias / noise in the
    store's units (grays 0 .. 255 for a "u8" store): g <- gain g + bias + noise r, r uniform in [-1, 1) per pixel.  fill: what lies
    outside the page (255 = paper).  limit = (Hmax, Wmax), the model's max_input_height / max_input_width: a sample that would
    outgrow it is drawn smaller instead (the positional encoding ends there; the target still lists every symbol, so no cropping)."""

    def __init__(self, scale: Range = (1.0, 1.0), aspect: Range = (1.0, 1.0), rotate_deg: float = 0.0, shear: float = 0.0, gain: Range = (1.0, 1.0),
                 bias: Range = (0.0, 0.0), noise: float = 0.0, fill: float = 255.0, limit: Optional[Tuple[int, int]] = None):
        self.scale, self.aspect = _pair(scale, "scale"), _pair(aspect, "aspect")
        self.gain, self.bias = _pair(gain, "gain"), _pair(bias, "bias")
        if self.scale[0] <= 0 or self.aspect[0] <= 0:
            raise ValueError("scale and aspect must be positive")
        self.rotate_deg, self.shear, self.noise, self.fill = abs(float(rotate_deg)), abs(float(shear)), float(noise), float(fill)
        self.limit = None if limit is None else (int(limit[0]), int(limit[1]))

    def draw(self, seed: int, epoch: int, n: int, h: int, w: int) -> np.ndarray:
        rng = _rng(seed, epoch, n, h, w)
        s, a = _uniform(rng, self.scale), _uniform(rng, self.aspect)
        theta = math.radians(_uniform(rng, (-self.rotate_deg, self.rotate_deg)))
        k = _uniform(rng, (-self.shear, self.shear))
        gain, bias = _uniform(rng, self.gain), _uniform(rng, self.bias)
        noise_seed = int(rng.integers(0, 1 << 63))
        sy, sx = s / math.sqrt(a), s * math.sqrt(a)
        rot = np.array([[math.cos(theta), -math.sin(theta)], [math.sin(theta), math.cos(theta)]])        # on (y, x)
        A = rot @ np.array([[1.0, 0.0], [k, 1.0]]) @ np.diag([sy, sx])
        return affine_record(h, w, A, self.limit, gain=gain, bias=bias, noise=self.noise, fill=self.fill, seed=noise_seed)


class SpecAugment:
    """SpecAugment-style masking of a spectrogram [frequency, time] per (sample, epoch): `time_masks` column bands of 0 .. max_time
    frames and `freq_masks` row bands of 0 .. max_freq bins (at most two each: what a record holds), each placed uniformly inside
    the augmented extent and filled with `fill` (0 = silence); a time stretch (the affine map along x only) and a gain.  limit: as
    for ImageAugment; a stretch that would outgrow the width is drawn smaller."""

    def __init__(self, time_masks: int = 0, max_time: int = 0, freq_masks: int = 0, max_freq: int = 0, time_stretch: Range = (1.0, 1.0),
                 gain: Range = (1.0, 1.0), fill: float = 0.0, limit: Optional[Tuple[int, int]] = None):
        if not (0 <= time_masks <= 2 and 0 <= freq_masks <= 2):
            raise ValueError("a record holds at most two time masks and two frequency masks")
        if max_time < 0 or max_freq < 0:
            raise ValueError("max_time and max_freq must not be negative")
        self.time_masks, self.max_time, self.freq_masks, self.max_freq = int(time_masks), int(max_time), int(freq_masks), int(max_freq)
        self.time_stretch, self.gain, self.fill = _pair(time_stretch, "time_stretch"), _pair(gain, "gain"), float(fill)
        if self.time_stretch[0] <= 0:
            raise ValueError("time_stretch must be positive")
        self.limit = None if limit is None else (int(limit[0]), int(limit[1]))

    @staticmethod
    def _bands(rng: np.random.Generator, count: int, longest: int, extent: int):
        out = []
        for _ in range(count):
            length = min(int(rng.integers(0, longest + 1)), extent)
            out.append((int(rng.integers(0, extent - length + 1)), length))
        return out

    def draw(self, seed: int, epoch: int, n: int, h: int, w: int) -> np.ndarray:
        rng = _rng(seed, epoch, n, h, w)
        sx, gain = _uniform(rng, self.time_stretch), _uniform(rng, self.gain)
        r = affine_record(h, w, np.diag([1.0, sx]), self.limit, fit="x", gain=gain, fill=self.fill)
        cols = self._bands(rng, self.time_masks, self.max_time, int(r["out_w"]))
        rows = self._bands(rng, self.freq_masks, self.max_freq, int(r["out_h"]))
        for k, band in enumerate(rows):
            r["rows"][k] = band
        for k, band in enumerate(cols):
            r["cols"][k] = band
        return r


def draw_all(aug, seed: int, epoch: int, sizes) -> np.ndarray:
    """The records [N] of a whole size table (int [N, 2] = (h, w)) for one (seed, epoch): record n = aug.draw(seed, epoch, n, h_n, w_n)."""
    hw = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    return stack([aug.draw(seed, epoch, n, int(h), int(w)) for n, (h, w) in enumerate(hw)])


def augmented_sizes(aug, seed: int, epoch: int, sizes) -> np.ndarray:
    """int64 [N, 2]: the extents the samples of `sizes` have after their augmentation of (seed, epoch) -- what a batch plan has to budget."""
    return extents(draw_all(aug, seed, epoch, sizes))
