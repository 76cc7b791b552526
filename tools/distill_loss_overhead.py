"""What the fused distillation loss costs at the benchmark's own shape: M = 16 384 rows, V = 6 997, pitch 7 000, student and teachers of one dtype.
The forward + backward pair through omr_ce_distill_fwd / omr_ce_distill_bwd is timed, with one and with two teachers, against
  plain    the hard-label loss alone on the same student logits (omr_ce_fwd + omr_ce_bwd),
  torch    the same loss composed from torch ops (cross_entropy + kl_div of log_softmax / softmax) with autograd's backward,
  copy     a device copy that moves the bytes the kernels must move: every tensor read once forward, read once more and dlogits written
           backward -- (n + 1) reads forward, (n + 1) reads and one write backward for n teachers.  A copy of b bytes reads b and writes b,
           so the copy timed is of half that total.
All alternated inside ONE process so that they see the same machine and clocks; the medians over the rounds and the spread of each are printed.

    python tools/distill_loss_overhead.py [--rounds 5] [--steps 50] [--dtype bf16] [--tau 2] [--lam 0.5] [--alpha 0.5]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M, V, LD, PAD = 16384, 6997, 7000, 0


def timed(fn, steps):
    """Device us per call of fn over `steps` back-to-back calls (events around the window, which ends in a synchronise)."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--torch-steps", type=int, default=5)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--tau", type=float, default=2.0)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--alpha", type=float, default=0.5)
    args = ap.parse_args()
    from omr_a2s_multimodal_transformer_amd import kernels as K
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator().manual_seed(0)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    make = lambda: (torch.randn((M, LD), generator=g) * 3.0).to(dtype).to(dev)[:, :V]  # noqa: E731
    x, a, b = make(), make(), make()
    tgt = torch.randint(0, V, (M,), generator=g).to(dev)            # about one row in V is the pad index
    one = torch.ones(1, device=dev)
    tau, lam = args.tau, args.lam
    live = (tgt != PAD)
    count = float(live.sum())

    def plain():
        _, lse, acc2 = K.ce_fwd(x, tgt, V, PAD)
        return K.ce_bwd(x, tgt, lse, acc2, V, PAD, grad_out=one)

    def fused(n):
        tb, alpha = (b, args.alpha) if n == 2 else (None, 1.0)

        def run():
            _, lse4, _, acc4 = K.ce_distill_fwd(x, tgt, a, tb, V, PAD, alpha, tau, lam)
            return K.ce_distill_bwd(x, tgt, a, tb, lse4, acc4, V, PAD, alpha, tau, lam, grad_out=one)
        return run

    def composed(n):
        def run():
            xs = x.detach().requires_grad_(True)
            q = F.softmax(a.float() / tau, 1)
            if n == 2:
                q = args.alpha * q + (1 - args.alpha) * F.softmax(b.float() / tau, 1)
            kd = (F.kl_div(F.log_softmax(xs.float() / tau, 1), q, reduction="none").sum(1) * live).sum() * (tau * tau / count)
            loss = (1 - lam) * F.cross_entropy(xs.float(), tgt, ignore_index=PAD) + lam * kd
            loss.backward()
            return xs.grad
        return run

    def copy(n):
        nbytes = (2 * (n + 1) + 1) * M * LD * x.element_size()
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        return (lambda: dst.copy_(src)), nbytes

    # the kernels and the composition agree on what they compute, at this size, before anything is timed
    for n in (1, 2):
        want = composed(n)().float()
        got = fused(n)().float()
        err = float((got - want).abs().max()) / float(want.abs().max())
        print(f"{n} teacher(s): fused gradient vs torch composition, max abs error / max abs value = {err:.3e}")
        del want, got

    variants = {"plain": (plain, args.steps)}
    moved = {}
    for n in (1, 2):
        variants[f"fused{n}"] = (fused(n), args.steps)
        variants[f"torch{n}"] = (composed(n), args.torch_steps)
        fn, moved[n] = copy(n)
        variants[f"copy{n}"] = (fn, args.steps)
    times = {k: [] for k in variants}
    for r in range(args.rounds):
        for k, (fn, steps) in variants.items():
            times[k].append(timed(fn, steps))
        print(f"round {r}: " + " | ".join(f"{k} {v[-1]:9.1f} us" for k, v in times.items()))
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    spread = lambda xs: (max(xs) - min(xs)) / med(xs)  # noqa: E731
    m = {k: med(v) for k, v in times.items()}
    for n in (1, 2):
        print(f"{args.dtype}, {n} teacher(s), forward + backward, median of {args.rounds} rounds: fused {m[f'fused{n}']:.1f} us = "
              f"{m[f'fused{n}'] / m['plain']:.2f} x plain ({m['plain']:.1f} us), {m[f'torch{n}'] / m[f'fused{n}']:.2f} x faster than torch "
              f"({m[f'torch{n}']:.1f} us), {m[f'fused{n}'] / m[f'copy{n}']:.2f} x the copy of {moved[n] / 1e6:.0f} MB ({m[f'copy{n}']:.1f} us)")
    print(json.dumps(dict(tool="distill_loss_overhead", M=M, V=V, ld=LD, dtype=args.dtype, tau=tau, lam=lam, alpha=args.alpha, rounds=args.rounds,
                          steps=args.steps, torch_steps=args.torch_steps, us={k: round(v, 2) for k, v in m.items()},
                          spread={k: round(spread(v), 4) for k, v in times.items()}, bytes_moved=moved)))


if __name__ == "__main__":
    main()
