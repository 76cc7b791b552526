"""Time of omr_gather_augmented_batch beside omr_gather_ragged_batch on the same C2-sized plane (32 x 256 x 4064, uint8 store -> bf16
batch) and the same drawn sizes as tools/gather_bandwidth.py (DESIGN.md "Augmentation in the gather").  Three launches per size draw:
the plain gather, the augmented gather with the identity record (the same pixels through the general path: the price of the record
and the four-tap code when nothing is blended), and the augmented gather with a typical `augment.ImageAugment` draw per sample
(rotation, shear, scale, gain, bias, noise; extents limited to the plane).  Medians of `--reps` launches timed with events after a
warm-up, all from one visit; one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.gather_bandwidth import timed  # noqa: E402


def upload(records, dev):
    return torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(len(records), -1).copy()).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    from omr_a2s_multimodal_transformer_amd import augment, kernels
    dev = torch.device("cuda", 0)
    B, H, W = 32, 256, 4064
    g = torch.Generator().manual_seed(99)
    heights = torch.randint(128, 257, (B,), generator=g).tolist()
    widths = torch.randint(568, 4065, (B,), generator=g).tolist()
    heights[0], widths[0] = H, W
    out = torch.empty((B, 1, H, W), dtype=torch.bfloat16, device=dev)
    idx = torch.arange(B, dtype=torch.int32, device=dev)
    typical = augment.ImageAugment(scale=(0.9, 1.1), aspect=(0.95, 1.05), rotate_deg=2.0, shear=0.03, gain=(0.85, 1.15), bias=(-15.0, 15.0), noise=6.0,
                                   fill=255.0, limit=(H, W))
    res = {"plane": f"{B}x{H}x{W}", "bytes_written": out.numel() * 2}
    for name, hw in (("full", [(H, W)] * B), ("drawn", list(zip(heights, widths)))):
        counts = [h * w for h, w in hw]
        offsets = torch.tensor([sum(counts[:n]) for n in range(B)], dtype=torch.int64, device=dev)
        sizes = torch.tensor(hw, dtype=torch.int32, device=dev)
        store = torch.randint(0, 256, (sum(counts),), dtype=torch.uint8, device=dev)
        ident = upload(augment.stack([augment.identity(h, w) for h, w in hw]), dev)
        drawn = augment.draw_all(typical, 1, 0, hw)
        drawn_dev = upload(drawn, dev)
        plain = timed(lambda: kernels.gather_ragged_batch(store, offsets, sizes, idx, H, W, torch.bfloat16, out=out), args.reps)
        t_ident = timed(lambda: kernels.gather_augmented_batch(store, offsets, sizes, idx, ident, H, W, torch.bfloat16, out=out), args.reps)
        t_drawn = timed(lambda: kernels.gather_augmented_batch(store, offsets, sizes, idx, drawn_dev, H, W, torch.bfloat16, out=out), args.reps)
        ext = augment.extents(drawn)
        res[name] = {"real_over_padded": round(sum(counts) / (B * H * W), 3), "augmented_over_padded": round(float((ext[:, 0] * ext[:, 1]).sum()) / (B * H * W), 3),
                     "plain_ms": round(plain, 4), "identity_ms": round(t_ident, 4), "typical_ms": round(t_drawn, 4),
                     "identity_over_plain": round(t_ident / plain, 2), "typical_over_plain": round(t_drawn / plain, 2)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
