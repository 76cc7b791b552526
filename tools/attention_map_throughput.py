"""Time of omr_attn_weights beside omr_attn_fwd_ws at the C2 cross-attention shape (B 32, H 4, T 512, hd 64, bf16) for S = 4096
(DESIGN.md "Attention maps").  The two are alternated, `--rounds` rounds each after a warm-up; a round enqueues `--reps` calls back
to back between one pair of events (other work shares the host: the spread over the rounds is printed beside the medians).
The map's floor is its output traffic, B T S 4 bytes; the forward never writes anything of that size.  Asserts nothing; one
JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    """ms per call: `reps` calls enqueued back to back between ONE pair of events, so the queue never runs dry and the gaps of a
    single launch on an idle queue (host issue, allocation in the Python wrapper) are not in the figure -- kernel time as long as
    the host issues a call faster than the device runs it, which the printed host_issue_ms shows."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def host_issue_ms(fn, reps):
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return 1000.0 * dt / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--keys", type=int, default=4096)
    args = ap.parse_args()
    from omr_a2s_multimodal_transformer_amd import kernels as K
    dev = torch.device("cuda", 0)
    B, H, T, S, hd = 32, 4, 512, args.keys, 64
    d = H * hd
    g = torch.Generator().manual_seed(7)
    q = (torch.rand((B, T, d), generator=g) * 2 - 1).to(dev, torch.bfloat16)
    kv = (torch.rand((B, S, 2 * d), generator=g) * 2 - 1).to(dev, torch.bfloat16)
    k, v = kv[..., :d], kv[..., d:]
    _, lse = K.attn_fwd(q, k, v, H)
    w = torch.empty((B, T, S), dtype=torch.float32, device=dev)

    def fwd():
        K.attn_fwd(q, k, v, H)

    def weights():
        K.attn_weights(q, k, lse, H, out=w)

    for _ in range(5):
        fwd()
        weights()
    torch.cuda.synchronize()
    rounds = {"attn_fwd_ms": [], "attn_weights_ms": []}
    for _ in range(args.rounds):
        rounds["attn_fwd_ms"].append(timed(fwd, args.reps))
        rounds["attn_weights_ms"].append(timed(weights, args.reps))
    out_bytes = B * T * S * 4
    res = {"shape": f"B{B} H{H} T{T} S{S} hd{hd} bf16", "map_bytes": out_bytes}
    for name, ms in rounds.items():
        res[name] = {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
    res["host_issue_ms"] = {"attn_fwd": round(host_issue_ms(fwd, args.reps), 4), "attn_weights": round(host_issue_ms(weights, args.reps), 4)}
    res["map_written_gb_per_s"] = round(out_bytes / statistics.median(rounds["attn_weights_ms"]) / 1e6, 1)
    res["rows_sum_to_one_max_err"] = float((w.sum(dim=-1) - 1.0).abs().max())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
