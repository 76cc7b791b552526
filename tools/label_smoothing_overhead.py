"""What label smoothing costs in the cross-entropy kernels at the benchmark's own shape: M = 16 384 rows, V = 6 997, ldv = 7 000, bf16.
The forward + backward pair (row kernel, finalize, gradient) is timed through the eps = 0 entries (omr_ce_fwd / omr_ce_bwd) and through
omr_ce_smooth_fwd / omr_ce_smooth_bwd at eps = 0.1, alternated inside ONE process so that both see the same box and clocks.  Both
variants read the logits twice and write dlogits once (3 * M * ldv * 2 bytes), so the expectation is a ratio near 1; the spread of the
eps = 0 pair between rounds is printed beside it, and a ratio inside that spread is no difference.

--dtype fp32 times the parity mode instead, whose smoothed gradient kernel works in fp64 (ce_smooth_bwd_f32_kernel) and is expected to cost more.

    python tools/label_smoothing_overhead.py [--rounds 7] [--steps 200] [--eps 0.1] [--dtype bf16]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M, V, LDV, PAD = 16384, 6997, 7000, 0


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    args = ap.parse_args()
    from omr_a2s_multimodal_transformer_amd import kernels as K
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator().manual_seed(0)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    buf = (torch.randn((M, LDV), generator=g) * 3.0).to(dtype).to(dev)
    logits = buf[:, :V]
    tgt = torch.randint(0, V, (M,), generator=g).to(dev)            # about one row in V is the pad index
    one = torch.ones(1, device=dev)

    def plain():
        _, lse, acc2 = K.ce_fwd(logits, tgt, V, PAD)
        return K.ce_bwd(logits, tgt, lse, acc2, V, PAD, grad_out=one)

    def smooth():
        _, _, lse, _, acc3 = K.ce_smooth_fwd(logits, tgt, V, PAD, args.eps)
        return K.ce_smooth_bwd(logits, tgt, lse, acc3, V, PAD, args.eps, grad_out=one)

    off, on = [], []
    for r in range(args.rounds):
        off.append(timed(plain, args.steps))
        on.append(timed(smooth, args.steps))
        print(f"round {r}: eps = 0 {off[-1]:8.1f} us | eps = {args.eps} {on[-1]:8.1f} us | ratio {on[-1] / off[-1]:.4f}")
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    spread = lambda xs: (max(xs) - min(xs)) / med(xs)  # noqa: E731
    bytes_moved = 3 * M * LDV * buf.element_size()
    print(f"forward + backward, device time, median of {args.rounds} rounds x {args.steps} pairs: eps = 0 {med(off):.1f} us "
          f"(spread {100 * spread(off):.2f} %), eps = {args.eps} {med(on):.1f} us (spread {100 * spread(on):.2f} %), ratio {med(on) / med(off):.4f}; "
          f"{bytes_moved / 1e6:.0f} MB per pair = {bytes_moved / med(off) / 1e6:.2f} / {bytes_moved / med(on) / 1e6:.2f} TB/s")
    print(json.dumps(dict(tool="label_smoothing_overhead", M=M, V=V, ldv=LDV, dtype=args.dtype, eps=args.eps, rounds=args.rounds, steps=args.steps,
                          us_plain=round(med(off), 2), us_smooth=round(med(on), 2), ratio=round(med(on) / med(off), 4),
                          spread_plain=round(spread(off), 4), spread_smooth=round(spread(on), 4),
                          us_plain_rounds=[round(v, 2) for v in off], us_smooth_rounds=[round(v, 2) for v in on])))


if __name__ == "__main__":
    main()
