"""Time of omr_gather_ragged_batch at the C2-sized plane (32 x 256 x 4064, uint8 store -> bf16 batch) beside a torch device-to-device copy
of as many bytes as the kernel writes (DESIGN.md "Resident dataset and bucketed batches").  Two batches: every sample fills the plane
(the kernel reads 1 byte and writes 2 per pixel), and the size draw of tools/ragged_train_throughput.py (about 0.44 of the plane is
real, the rest is padding that is only written).  Medians of `--reps` launches timed with events after a warm-up; one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    from omr_a2s_multimodal_transformer_amd import kernels
    dev = torch.device("cuda", 0)
    B, H, W = 32, 256, 4064
    g = torch.Generator().manual_seed(99)
    heights = torch.randint(128, 257, (B,), generator=g).tolist()
    widths = torch.randint(568, 4065, (B,), generator=g).tolist()
    heights[0], widths[0] = H, W
    out = torch.empty((B, 1, H, W), dtype=torch.bfloat16, device=dev)
    a, b = torch.empty_like(out), torch.empty_like(out)
    idx = torch.arange(B, dtype=torch.int32, device=dev)
    res = {"plane": f"{B}x{H}x{W}", "bytes_written": out.numel() * 2, "copy_ms": round(timed(lambda: b.copy_(a), args.reps), 4)}
    for name, hw in (("full", [(H, W)] * B), ("drawn", list(zip(heights, widths)))):
        counts = [h * w for h, w in hw]
        offsets = torch.tensor([sum(counts[:n]) for n in range(B)], dtype=torch.int64, device=dev)
        sizes = torch.tensor(hw, dtype=torch.int32, device=dev)
        store = torch.randint(0, 256, (sum(counts),), dtype=torch.uint8, device=dev)
        ms = timed(lambda: kernels.gather_ragged_batch(store, offsets, sizes, idx, H, W, torch.bfloat16, out=out), args.reps)
        res[name] = {"real_over_padded": round(sum(counts) / (B * H * W), 3), "gather_ms": round(ms, 4),
                     "written_gb_per_s": round(out.numel() * 2 / ms / 1e6, 1), "moved_gb_per_s": round((out.numel() * 2 + sum(counts)) / ms / 1e6, 1)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
