"""Per-shape timing of the GEMMs one C2 training step issues (forward NT, data-gradient NN, weight-gradient TT) and of the grouped
weight-gradient launch over the problems of one C2 decoder backward.
Usage (GPU box): python tools/gemm_shapes.py [--checkout ROOT] [--json OUT] [--no-lib]  -> table on stdout.
--checkout: import the package from the built checkout at ROOT instead of this tree (to time another commit with the same script);
--json: also write {"name/fwd|dgrad|wgrad": us, "grouped/decoder-bwd": us}; --no-lib: skip the vendor-library yardstick columns.
Development aid, not part of the product path."""
import argparse
import json
import os
import sys

import torch

R, RM = 32 * 512, 32 * 4096
LINEARS = [  # name, rows, in, out, count per step
    ("self.qkv", R, 256, 768, 6), ("self.out", R, 256, 256, 6), ("cross.q", R, 256, 256, 6), ("cross.kv", RM, 256, 512, 0), ("kv.fused", RM, 256, 3072, 1),
    ("cross.out", R, 256, 256, 6), ("ff1", R, 256, 1024, 6), ("ff2", R, 1024, 256, 6), ("head", R, 256, 6997, 1),
    ("pc.128", RM, 128, 128, 9), ("pc.128-256", RM, 128, 256, 1), ("pc.256", RM, 256, 256, 2),
]
DECODER_LAYERS, D_MODEL = 6, 256


def timeit(fn, n=20):
    fn(); fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def decoder_wgrad_problems(dev, dt):
    """What one C2 decoder backward hands to kernels.linear_wgrad_grouped: the six linears of each of the six layers, the head, and the
    all-layer K|V projection of the memory through its row-group view of the packed in_proj gradients (38 problems, two argument tables)."""
    probs = []
    for name, rows, kin, nout, cnt in LINEARS:
        if rows == R:
            for _ in range(cnt):
                probs.append((torch.randn(rows, (nout + 7) // 8 * 8, device=dev, dtype=dt)[:, :nout], torch.randn(rows, kin, device=dev, dtype=dt),
                              torch.zeros(nout, kin, device=dev), torch.zeros(nout, device=dev), None))
    L, d = DECODER_LAYERS, D_MODEL
    probs.append((torch.randn(RM, L * 2 * d, device=dev, dtype=dt), torch.randn(RM, d, device=dev, dtype=dt),
                  torch.zeros(L * 3 * d, d, device=dev), torch.zeros(L * 3 * d, device=dev), (2 * d, 3 * d, d)))
    return probs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkout", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--json")
    ap.add_argument("--no-lib", action="store_true")
    args = ap.parse_args()
    root = os.path.abspath(args.checkout)
    sys.path.insert(0, root)
    import omr_a2s_multimodal_transformer_amd as pkg
    from omr_a2s_multimodal_transformer_amd import kernels as K
    from omr_a2s_multimodal_transformer_amd.functional import split_k_for
    assert os.path.abspath(pkg.__file__).startswith(root + os.sep), f"imported {pkg.__file__}, not the package under {root}"

    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    tot = {"fwd": 0.0, "dgrad": 0.0, "wgrad": 0.0}
    out = {}
    print(f"{'name':10s} {'rows':>7s} {'in':>5s} {'out':>5s} | {'fwd us':>8s} {'TF/s':>6s} | {'dgrad us':>8s} {'TF/s':>6s} | {'wgrad us':>8s} {'TF/s':>6s} sk")
    for name, rows, kin, nout, cnt in LINEARS:
        x = torch.randn(rows, kin, device=dev, dtype=dt)
        ld = (nout + 7) // 8 * 8
        w = torch.randn(nout, kin, device=dev, dtype=dt)
        gy = torch.randn(rows, ld, device=dev, dtype=dt)[:, :nout]
        bias = torch.zeros(nout, device=dev)
        gw = torch.zeros(nout, kin, device=dev)
        gb = torch.zeros(nout, device=dev)
        ybuf = torch.empty(rows, ld, device=dev, dtype=dt)
        flops = 2.0 * rows * kin * nout
        sk = split_k_for(rows, nout, kin)
        t_f = timeit(lambda: K.gemm(x, w, bias=bias, out=ybuf[:, :nout]))
        t_d = timeit(lambda: K.gemm(gy, w, trans_b=True))
        t_w = timeit(lambda: K.gemm(gy, x, trans_a=True, trans_b=True, out=gw, accumulate=True, split_k=sk, colsum_a=gb))
        tot["fwd"] += t_f * cnt; tot["dgrad"] += t_d * cnt; tot["wgrad"] += t_w * cnt
        out[f"{name}/fwd"], out[f"{name}/dgrad"], out[f"{name}/wgrad"] = t_f, t_d, t_w
        line = f"{name:10s} {rows:7d} {kin:5d} {nout:5d} | {t_f:8.1f} {flops / t_f / 1e6:6.0f} | {t_d:8.1f} {flops / t_d / 1e6:6.0f} | {t_w:8.1f} {flops / t_w / 1e6:6.0f} {sk}"
        if not args.no_lib:
            # yardstick only (never on the product path): what the vendor library does with the same forward / data-gradient shape
            bb = bias.to(dt)
            t_lf = timeit(lambda: torch.nn.functional.linear(x, w, bb))
            gyc = gy.contiguous()
            t_ld = timeit(lambda: torch.matmul(gyc, w))
            tot.setdefault("lib fwd", 0.0); tot.setdefault("lib dgrad", 0.0)
            tot["lib fwd"] += t_lf * cnt; tot["lib dgrad"] += t_ld * cnt
            line += f" | lib fwd {t_lf:7.1f} dgrad {t_ld:7.1f}"
        print(line)
        del x, w, gy, ybuf
    probs = decoder_wgrad_problems(dev, dt)
    out["grouped/decoder-bwd"] = t_g = timeit(lambda: K.linear_wgrad_grouped(probs))
    print(f"grouped weight gradient, {len(probs)} problems of one decoder backward: {t_g:8.1f} us")
    print("per-step totals (ms):", {k: round(v / 1e3, 3) for k, v in tot.items()})
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
