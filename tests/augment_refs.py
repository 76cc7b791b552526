"""omr_gather_augmented_batch (csrc/batch_augment.hip) restated in numpy float32, operation by operation in the order include/omr_hip.h
gives: every product and every sum below is ONE rounded fp32 operation (numpy float32 arithmetic never fuses), the hash runs in uint32.
Shared by tests/test_augment_refs_cpu.py (which pins it against slices, means and the host collate) and the GPU tests, which demand
bit equality with it."""
from __future__ import annotations

import numpy as np
import torch

F = np.float32
TWO_M23 = F(2.0 ** -23)


def hash32(lo, hi, idx):
    """omr_common.h hash32 on uint32 arrays (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        lo, hi = np.uint32(lo), np.uint32(hi)
        h = (np.asarray(idx, dtype=np.uint32) * np.uint32(0x9E3779B1) + lo).astype(np.uint32)
        h = h ^ (h >> np.uint32(16))
        h = (h * np.uint32(0x85EBCA6B)).astype(np.uint32)
        h = h ^ (h >> np.uint32(13))
        h = ((h + hi).astype(np.uint32) * np.uint32(0xC2B2AE35)).astype(np.uint32)
        h = h ^ (h >> np.uint32(16))
    return h


def _conv(v, is_u8: bool):
    return (np.asarray(v, dtype=F) / F(255.0)).astype(F) if is_u8 else np.asarray(v, dtype=F)


def _in_band(pos, band):
    start, length = int(band[0]), int(band[1])
    return (pos >= start) & (pos < start + length) if length > 0 else np.zeros(pos.shape, dtype=bool)


def _taps(src, y, x, fill, wanted):
    """src [h, w] float32 in source units; integer coordinates y, x; `fill` outside the plane.  Where `wanted` is False the tap is
    not looked at (the kernel does not read it) and the value returned there is never used."""
    h, w = src.shape
    inside = (y >= 0) & (y < h) & (x >= 0) & (x < w) & wanted
    out = np.full(y.shape, fill, dtype=F)
    out[inside] = src[y[inside], x[inside]]
    return out


def _lerp(v0, v1, f):
    """f == 0 ? v0 : v0 * (1 - f) + v1 * f, each operation rounded to fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        blend = ((v0 * (F(1.0) - f)).astype(F) + (v1 * f).astype(F)).astype(F)
    return np.where(f == 0, v0, blend).astype(F)


def augment_plane(sample: np.ndarray, rec, H: int, W: int, pad: float) -> np.ndarray:
    """One batch row [H, W] in float32 (before the output type's rounding).  sample: uint8 or float32 [h, w]; rec: one AUG_DTYPE record."""
    is_u8 = sample.dtype == np.uint8
    src = sample.astype(F)
    h, w = src.shape
    oh, ow = min(max(int(rec["out_h"]), 0), H), min(max(int(rec["out_w"]), 0), W)
    m = np.asarray(rec["m"], dtype=F)
    fill = F(rec["fill"])
    out = np.full((H, W), pad, dtype=F)
    if oh == 0 or ow == 0:
        return out
    ii, jj = np.meshgrid(np.arange(oh, dtype=np.int64), np.arange(ow, dtype=np.int64), indexing="ij")
    fi, fj = ii.astype(F), jj.astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (((m[0] * fi).astype(F) + (m[1] * fj).astype(F)).astype(F) + m[2]).astype(F)
        x = (((m[3] * fi).astype(F) + (m[4] * fj).astype(F)).astype(F) + m[5]).astype(F)
        y = np.fmin(np.fmax(y, F(-1.0)), F(h)).astype(F)            # fmax / fmin return the other operand for a NaN: NaN -> -1
        x = np.fmin(np.fmax(x, F(-1.0)), F(w)).astype(F)
    y0, x0 = np.floor(y), np.floor(x)
    fy, fx = (y - y0).astype(F), (x - x0).astype(F)
    iy, ix = y0.astype(np.int64), x0.astype(np.int64)
    everywhere = np.ones(iy.shape, dtype=bool)
    top = _lerp(_taps(src, iy, ix, fill, everywhere), _taps(src, iy, ix + 1, fill, fx != 0), fx)
    bottom = _lerp(_taps(src, iy + 1, ix, fill, fy != 0), _taps(src, iy + 1, ix + 1, fill, (fy != 0) & (fx != 0)), fx)
    g = _lerp(top, bottom, fy)
    gain, bias, noise = F(rec["gain"]), F(rec["bias"]), F(rec["noise"])
    with np.errstate(invalid="ignore", over="ignore"):
        if not (gain == 1 and bias == 0):
            g = ((gain * g).astype(F) + bias).astype(F)
        if noise != 0:
            with np.errstate(over="ignore"):
                index = (ii.astype(np.uint32) * np.uint32(ow) + jj.astype(np.uint32)).astype(np.uint32)
            r = (((hash32(rec["seed_lo"], rec["seed_hi"], index) >> np.uint32(8)).astype(F) * TWO_M23).astype(F) - F(1.0)).astype(F)
            g = (g + (noise * r).astype(F)).astype(F)
        if is_u8:
            g = np.fmin(np.fmax(g, F(0.0)), F(255.0)).astype(F)
        g = _conv(g, is_u8)
    banded = np.zeros((oh, ow), dtype=bool)
    for k in range(2):
        banded |= _in_band(ii, rec["rows"][k]) | _in_band(jj, rec["cols"][k])
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.where(banded, _conv(fill, is_u8), g).astype(F)
    out[:oh, :ow] = g
    return out


def gather_augmented_ref(samples, idx, records, H: int, W: int, pad: float, dtype: torch.dtype) -> torch.Tensor:
    """samples: list of uint8 / float32 [h, w] (torch or numpy); idx: B sample indices; records: AUG_DTYPE [B] -> [B, 1, H, W] in `dtype`
    (bf16: torch's round-to-nearest-even of the fp32 plane, the rounding of omr_cast)."""
    rows = []
    for b, n in enumerate(idx):
        s = samples[n]
        s = s.numpy() if isinstance(s, torch.Tensor) else np.asarray(s)
        rows.append(augment_plane(s, records[b], H, W, pad))
    return torch.from_numpy(np.stack(rows)[:, None]).to(dtype)
