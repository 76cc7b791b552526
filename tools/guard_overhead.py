"""What the guarded optimizer step costs at the benchmark size: opt.step() of the C2 model's flat buffers (bench.py CONFIGS["c2"]:
image encoder + 6-layer d_model=256 decoder, bf16 compute copy) with the guard off and on, alternated inside ONE process so that
both see the same box and clocks.

The yardstick for the guarded step is the unguarded step plus one streaming read of the gradient (total * 4 bytes) and two
launches (omr_grad_norm's slot pass and its one-workgroup finish); the read is priced at the device-copy rate DESIGN.md section
3 quotes for tensors beyond the Infinity Cache (5.25 TB/s) -- the gradient itself is smaller than the cache, so this is the
conservative price.  The device time is taken with events around `--steps` back-to-back steps; the host time per call is printed
beside it (in this loop nothing runs between two steps, so with the guard on the host waits for the previous step's record --
in training that record is a whole forward and backward old).

    python tools/guard_overhead.py [--rounds 5] [--steps 50]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 5.25e12        # bytes/s, DESIGN.md section 3 (tools/stream_ceiling.py: 1.07 GB in + 1.07 GB out)


def build_c2_optimizer(dev):
    from bench import CONFIGS
    from omr_a2s_multimodal_transformer_amd import synthetic as syn
    from omr_a2s_multimodal_transformer_amd.config import ModelConfig
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    c = CONFIGS["c2"]
    V = syn.GRANDSTAFF_VOCAB
    cfg = ModelConfig(d_model=c["d"], nhead=4, ff_dim=c["d"], num_layers=c["layers"], compute_dtype=c["dtype"])
    w2i = {("<PAD>" if i == 0 else "<eos>" if i == syn.GRANDSTAFF_EOS else "<sos>" if i == syn.GRANDSTAFF_SOS else f"t{i}"): i for i in range(V)}
    torch.manual_seed(0)
    model = Transformer(c["img"][0], c["img"][1], c["seq"], w2i, {v: k for k, v in w2i.items()}, attn_window=-1, config=cfg)
    model.flatten_parameters(device=dev)
    return model, model.configure_optimizers()


def timed(opt, steps):
    """-> (device us per step, host us per call) over `steps` back-to-back opt.step() calls."""
    for _ in range(3):
        opt.step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.step()
    t1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps, (t1 - t0) * 1e6 / steps


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


def pieces(opt, steps):
    """The guarded step's parts, each alone: where the difference goes."""
    from omr_a2s_multimodal_transformer_amd import kernels as K
    f, g = opt.flat, opt.param_groups[0]
    ws = torch.empty(K.grad_norm_workspace_bytes(f.total, 1), dtype=torch.uint8, device=f.device)
    ctl = K.new_step_ctl(f.device)
    host = torch.zeros(ctl.numel(), dtype=torch.uint8).pin_memory()
    args = (f.master, f.grad, f.exp_avg, f.exp_avg_sq, 10, g["lr"], g["betas"], g["eps"], 1.0)
    K.grad_norm(f.grad, [(0, f.total)], 1.0, 1.0, ws, ctl)
    return dict(grad_norm=piece(lambda: K.grad_norm(f.grad, [(0, f.total)], 1.0, 1.0, ws, ctl), steps),
                adam=piece(lambda: K.adam_step(*args, p_lowp=f.lowp), steps),
                adam_guarded=piece(lambda: K.adam_step(*args, p_lowp=f.lowp, ctl=ctl), steps),
                record_copy=piece(lambda: host.copy_(ctl, non_blocking=True), steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model, opt = build_c2_optimizer(dev)
    flat = opt.flat
    flat.grad.copy_(torch.randn(flat.total, generator=torch.Generator().manual_seed(1)).to(dev) * 1e-3)
    grad_bytes = flat.total * 4
    off, on = [], []
    for r in range(args.rounds):
        opt.disable_guard()
        off.append(timed(opt, args.steps))
        opt.enable_guard(max_norm=1.0)
        on.append(timed(opt, args.steps))
        print(f"round {r}: off {off[-1][0]:8.1f} us device {off[-1][1]:8.1f} us host | on {on[-1][0]:8.1f} us device {on[-1][1]:8.1f} us host")
    assert opt.skipped == 0 and opt.last_grad_norm > 0
    med = lambda xs: sorted(xs)[len(xs) // 2]
    d_off, d_on = med([d for d, _ in off]), med([d for d, _ in on])
    h_off, h_on = med([h for _, h in off]), med([h for _, h in on])
    read_us = grad_bytes / COPY_RATE * 1e6
    print(f"parameters {flat.total} ({grad_bytes / 1e6:.1f} MB of fp32 gradient); one read at {COPY_RATE / 1e12:.2f} TB/s = {read_us:.1f} us")
    print(f"opt.step() device time, median of {args.rounds} rounds x {args.steps} steps: guard off {d_off:.1f} us, on {d_on:.1f} us, "
          f"difference {d_on - d_off:.1f} us (yardstick: {read_us:.1f} us + two launches)")
    print(f"opt.step() host time per call: guard off {h_off:.1f} us, on {h_on:.1f} us (back to back: the guarded call waits for the previous record)")
    parts = {k: round(v, 2) for k, v in pieces(opt, args.steps).items()}
    print("alone, device us per call: " + ", ".join(f"{k} {v:.1f}" for k, v in parts.items()))
    print(json.dumps(dict(tool="guard_overhead", parts=parts, params=flat.total, grad_bytes=grad_bytes, copy_rate_TBps=COPY_RATE / 1e12, read_us=round(read_us, 2),
                          device_us_off=round(d_off, 2), device_us_on=round(d_on, 2), host_us_off=round(h_off, 2), host_us_on=round(h_on, 2),
                          rounds=args.rounds, steps=args.steps, grad_norm=opt.last_grad_norm)))


if __name__ == "__main__":
    main()
