"""ConvBlocks in batch windows: does a conv chain run faster when its hand-off tensors fit the 256 MiB Infinity Cache?

    python tools/window_chain.py [--reps 7] [--warm 2] [--blocks 0,1,2,3,012] [--windows 2,4,8] [--plug 16]
    python tools/window_chain.py --blocks 1 --only-window 4 --reps 1 --warm 0 --plug 0     (one variant alone: a rocprofv3 pass)
    python tools/window_chain.py --pmc-sum DIR           (sum of a rocprofv3 --pmc pass over this tool's own kernels)

At the C2 shapes (B = 32, 256 x 2048, bf16) each of ConvBlocks 0-3, and ConvBlocks 0-2 as one chain ("012"), runs two ways through
the calls the training step makes (ConvBlock.nhwc -> functional.Conv3x3Fn -> kernels.py): over the whole batch, layer by layer, as
today; and in windows of w images, every window through the whole chain before the next one starts, the outputs joined with
torch.cat.  Backward is torch.autograd.backward over the windows' outputs, which runs the windows' chains one after the other,
last window first (autograd takes the highest sequence number first), in the launch order of the step.

Timing: HIP events around the whole chain, forward and backward apart, median / min / max over --reps runs after --warm warm-up
runs.  In front of each timed region the stream gets a plug of --plug device copies of 1 GiB, so that the host has issued (most
of) the chain before the GPU starts it: the step itself is not launch-bound (tools/host_overhead.py), a bare chain of 20 us
kernels would be.  The plug also leaves the cache cold, as the decoder of the previous step does.  `host` is the time the host
took to issue the region.  The Python `random` draws (dropout position and kind) are those of seed 100 + run for every variant and
every window, so all variants launch the same kernel instantiations.  Weight gradients stay on the main stream (--no-side-stream's
setting): the events then cover them.
"""
import argparse
import csv
import glob
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, H, W = 32, 256, 2048


def block_input_shape(i):
    """Input of ConvBlock i at the C2 shape: (height, width, channels)."""
    return [(H, W, 1), (H, W, 16), (H // 2, W // 2, 32), (H // 4, W // 4, 64)][i]


def pmc_sum(d):
    tot, launches = {}, 0
    for f in glob.glob(d + "/**/*_counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Kernel_Name"].startswith("void at::"):      # torch's own kernels: set-up, plug, cat
                continue
            tot[r["Counter_Name"]] = tot.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
            launches += 1
    for k, v in sorted(tot.items()):
        print(f"{k}: sum over {launches} launches of the library's kernels = {v:.6g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--blocks", default="0,1,2,3,012")
    ap.add_argument("--windows", default="2,4,8")
    ap.add_argument("--plug", type=int, default=16)
    ap.add_argument("--only-window", type=int, default=0, help="run this window alone, without the whole-batch row (a --pmc pass)")
    ap.add_argument("--pmc-sum", default="")
    args = ap.parse_args()
    if args.pmc_sum:
        return pmc_sum(args.pmc_sum)

    from omr_a2s_multimodal_transformer_amd.encoder import Encoder
    from omr_a2s_multimodal_transformer_amd.params import FlatParams
    from omr_a2s_multimodal_transformer_amd.runtime import WgradStream, seed_dropout

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    enc = Encoder(1).train()
    enc._flat = FlatParams(list(enc.named_parameters()), dev, torch.bfloat16)
    WgradStream.enabled = False
    seed_dropout(1)
    plug_src = torch.empty(1 << 29, dtype=torch.bfloat16, device=dev)
    plug_dst = torch.empty_like(plug_src)

    def plug():
        for _ in range(args.plug):
            plug_dst.copy_(plug_src)

    def chain(blocks, xw, first_mask):
        mask, scale = first_mask, 1.0
        for blk in blocks:
            xw, scale = blk.nhwc(xw, mask, scale, defer_out=True)
            mask = True
        return xw

    def measure(ids, w):
        blocks = [enc.conv_blocks[i] for i in ids]
        h, wd, c = block_input_shape(ids[0])
        x = (torch.rand((B, h, wd, c), device=dev) - 0.4).clamp_min_(0).to(torch.bfloat16)
        wins = [x[b0:b0 + w].detach().requires_grad_(c > 1) for b0 in range(0, B, w)]
        g = None
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        fwd, bwd, hf, hb = [], [], [], []
        for r in range(args.warm + args.reps):
            random.seed(100 + r)
            st = random.getstate()
            for xw in wins:
                xw.grad = None
            torch.cuda.synchronize()
            plug()
            ev[0].record()
            t0 = time.perf_counter()
            outs = []
            for xw in wins:
                random.setstate(st)
                outs.append(chain(blocks, xw, c > 1))
            y = torch.cat(outs) if len(outs) > 1 else outs[0]
            t1 = time.perf_counter()
            ev[1].record()
            if g is None:
                g = torch.randn(y.shape, device=dev).to(torch.bfloat16)
            gs = [g[b0:b0 + w] for b0 in range(0, B, w)]
            torch.cuda.synchronize()
            plug()
            ev[2].record()
            t2 = time.perf_counter()
            torch.autograd.backward(outs, gs)
            t3 = time.perf_counter()
            ev[3].record()
            torch.cuda.synchronize()
            if r >= args.warm:
                fwd.append(ev[0].elapsed_time(ev[1]))
                bwd.append(ev[2].elapsed_time(ev[3]))
                hf.append((t1 - t0) * 1e3)
                hb.append((t3 - t2) * 1e3)
            del outs, y
        return fwd, bwd, statistics.median(hf), statistics.median(hb)

    def row(v):
        return f"{statistics.median(v):7.3f} [{min(v):7.3f} {max(v):7.3f}]"

    print(f"B={B} {H}x{W} bf16, {args.reps} runs after {args.warm} warm-up, plug {args.plug} GiB copies; ms: median [min max]; "
          f"ratio = median / whole-batch median, spread = (max - min) / median of the whole-batch runs")
    print(f"{'blocks':6} {'window':>6} | {'forward':25} {'ratio':>6} {'host':>6} | {'backward':25} {'ratio':>6} {'host':>6} | largest hand-off MB")
    for name in args.blocks.split(","):
        ids = [int(ch) for ch in name]
        base = None
        for w in [args.only_window] if args.only_window else [B] + [int(v) for v in args.windows.split(",") if v]:
            fwd, bwd, hf, hb = measure(ids, w)
            if base is None:
                base = (statistics.median(fwd), statistics.median(bwd))
                spread = ((max(fwd) - min(fwd)) / base[0], (max(bwd) - min(bwd)) / base[1])
            hand = 0
            for i in ids:
                h, wd, _ = block_input_shape(i)
                hand = max(hand, w * h * wd * enc.conv_blocks[i].conv1.out_channels * 2)
            print(f"{name:6} {w:6d} | {row(fwd)} {statistics.median(fwd) / base[0]:6.3f} {hf:6.2f} | {row(bwd)} {statistics.median(bwd) / base[1]:6.3f} {hb:6.2f} | {hand / 1e6:7.1f}",
                  flush=True)
        print(f"{name:6} whole-batch spread: forward {spread[0]:.3f}, backward {spread[1]:.3f}", flush=True)


if __name__ == "__main__":
    main()
