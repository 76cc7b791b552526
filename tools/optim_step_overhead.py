"""What the optimizer recipe costs at the benchmark size: one step over the C2 model's flat buffers (bench.py CONFIGS["c2"]: image
encoder + 6-layer d_model=256 decoder, bf16 compute copy) through kernels.adam_step (omr_adamw_ema, the one step kernel): plain and
guarded (what a step without a recipe launches; before the three kernels became one these two rows were omr_adam's and
omr_adam_guarded's scalar kernels), and decay only, EMA only, decay + EMA -- each unguarded and behind the guard's record.

All variants run inside ONE process, interleaved: every round times each variant once, in a fixed order, over `--steps`
back-to-back launches between two events; the table gives the median over the rounds and the spread.  The plain step moves five fp32
streams and one bf16 stream per element (g, p, m, v in; p, m, v, bf16 out -> 30 bytes), the full recipe seven and one (+ ema in and
out -> 38 bytes, plus one byte of the decay map per 64 elements); the yardstick beside each time is that traffic at the
device-copy rate DESIGN.md section 3 quotes (5.25 TB/s).  The guarded variants read a record filled once (clip < 1, apply = 1);
omr_grad_norm itself is tools/guard_overhead.py's subject.

    python tools/optim_step_overhead.py [--rounds 7] [--steps 50] [--step-ms 23.3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 5.25e12        # bytes/s, DESIGN.md section 3


def piece(fn, steps):
    """Device us per call of fn over `steps` back-to-back calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--step-ms", type=float, default=23.3, help="a C2 training step, for the share (DESIGN.md: bench.py c2)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from guard_overhead import build_c2_optimizer
    from omr_a2s_multimodal_transformer_amd import kernels as K
    from omr_a2s_multimodal_transformer_amd.config import OptimConfig
    model, _ = build_c2_optimizer(dev)
    opt = model.make_optimizer(optim=OptimConfig(weight_decay=0.1, ema_decay=0.999))
    f, g = opt.flat, opt.param_groups[0]
    n = f.total
    f.grad.copy_(torch.randn(n, generator=torch.Generator().manual_seed(1)).to(dev) * 1e-3)
    ws = torch.empty(K.grad_norm_workspace_bytes(n, 1), dtype=torch.uint8, device=dev)
    ctl = K.new_step_ctl(dev)
    K.grad_norm(f.grad, [(0, n)], 1.0, 1.0, ws, ctl)
    rec = K.read_step_ctl(ctl.cpu())
    assert rec.apply == 1
    base = (f.master, f.grad, f.exp_avg, f.exp_avg_sq, 10, g["lr"], g["betas"], g["eps"], 1.0)
    blocks = opt._decay_blocks
    decay = dict(weight_decay=0.1, decay_blocks=blocks)
    ema = dict(ema=f.ema, ema_decay=0.999)
    variants = {
        "plain": (lambda: K.adam_step(*base, p_lowp=f.lowp), 30),
        "guarded": (lambda: K.adam_step(*base, p_lowp=f.lowp, ctl=ctl), 30),
        "decay": (lambda: K.adam_step(*base, p_lowp=f.lowp, **decay), 30),
        "ema": (lambda: K.adam_step(*base, p_lowp=f.lowp, **ema), 38),
        "decay+ema": (lambda: K.adam_step(*base, p_lowp=f.lowp, **decay, **ema), 38),
        "decay guarded": (lambda: K.adam_step(*base, p_lowp=f.lowp, ctl=ctl, **decay), 30),
        "ema guarded": (lambda: K.adam_step(*base, p_lowp=f.lowp, ctl=ctl, **ema), 38),
        "decay+ema guarded": (lambda: K.adam_step(*base, p_lowp=f.lowp, ctl=ctl, **decay, **ema), 38),
        "swap_f32": (lambda: K.swap_f32(f.master, f.ema), 16),
    }
    times = {k: [] for k in variants}
    for r in range(args.rounds):
        for name, (fn, _) in variants.items():
            times[name].append(piece(fn, args.steps))
        print(f"round {r}: " + ", ".join(f"{k} {v[-1]:.1f}" for k, v in times.items()))
    assert torch.isfinite(f.master).all() and torch.isfinite(f.ema).all()
    med = lambda xs: sorted(xs)[len(xs) // 2]
    print(f"parameters {n} ({n * 4 / 1e6:.1f} MB per fp32 stream), clip {rec.clip:.4f}; device us per launch, median of {args.rounds} rounds x {args.steps} launches")
    print(f"{'variant':32s} {'median':>8s} {'min':>8s} {'max':>8s} {'traffic at 5.25 TB/s':>22s} {'share of a step':>16s}")
    table = {}
    for name, (_, bytes_per) in variants.items():
        t = times[name]
        yard = n * bytes_per / COPY_RATE * 1e6
        table[name] = dict(median_us=round(med(t), 2), min_us=round(min(t), 2), max_us=round(max(t), 2), yardstick_us=round(yard, 2))
        print(f"{name:32s} {med(t):8.1f} {min(t):8.1f} {max(t):8.1f} {yard:22.1f} {med(t) / (args.step_ms * 1e3) * 100:15.3f}%")
    print(json.dumps(dict(tool="optim_step_overhead", params=n, rounds=args.rounds, steps=args.steps, step_ms=args.step_ms, clip=rec.clip, variants=table)))


if __name__ == "__main__":
    main()
