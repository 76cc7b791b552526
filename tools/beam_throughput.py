"""Beam-search throughput over inputs of different sizes: the loop of `beam_search` (one input per call, the selection on the
host) against `beam_search_batch` (N inputs per state, selection and cache reorder on the device) and `predict(beam=)`.
Benchmark config C2 (6-layer d_model 256 bf16 kern decoder, T = 512) with random-init weights, 64 seeded images of height 256
and widths spread over 512-4096 (memories of 1024-8192 tokens), beam 4; the head bias of <eos> is raised (the search of
tools/eval_throughput.py) so that the sequences end at different lengths.  After one warm-up pass of both routes over every
input, loop and batched route alternate `--reps` times.  Prints one JSON line:
  loop_s / batched_s                  [min, max] seconds of the repetitions: beam_search x n / beam_search_batch, --group inputs a state
  loop_tokens_per_s / batched_tokens_per_s   tokens of the returned sequences per second, at the slowest / fastest repetition resp.
  batched_slowest_vs_loop_fastest     loop_s[min] / batched_s[max]: above 1, every batched repetition beat every loop repetition
  predict_beam_s, greedy_predict_s    predict(xs, beam=4, batch_size=32) and greedy predict(xs, batch_size=32), both including the
                                      batch-size-1 encoder passes (encode_s), with their tokens/s
  single_loop_s / single_batched_s    one input: beam_search(m) against beam_search_batch([m])
  all_equal                           every batched / predict result equals the loop's (words and score)
Usage: python tools/beam_throughput.py [--n 64] [--group 8] [--beam 4] [--reps 3]"""
import argparse
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402
from omr_a2s_multimodal_transformer_amd.model import Transformer  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--group", type=int, default=8, help="inputs per batched beam state (rows = group * beam)")
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    V, T, H, WMAX = syn.GRANDSTAFF_VOCAB, 512, 256, 4096
    cfg = ModelConfig(d_model=256, nhead=4, ff_dim=256, num_layers=6, compute_dtype="bf16")
    w2i = {("<PAD>" if i == 0 else "<eos>" if i == syn.GRANDSTAFF_EOS else "<sos>" if i == syn.GRANDSTAFF_SOS else f"t{i}"): i for i in range(V)}
    i2w = {v: k for k, v in w2i.items()}
    torch.manual_seed(0)
    model = Transformer(H, WMAX, T, w2i, i2w, attn_window=-1, config=cfg)
    model.flatten_parameters(device=dev)
    model.eval()
    g = torch.Generator().manual_seed(args.seed)
    widths = [512 + int(w) // 8 * 8 for w in torch.randint(0, WMAX - 512 + 1, (args.n,), generator=g)]
    xs = [torch.rand((1, 1, H, w), generator=g).to(dev) for w in widths]
    beam, rows = args.beam, args.group * args.beam
    out = {"config": "C2 bf16, T=512, random init", "samples": args.n, "beam": beam, "inputs_per_state": args.group, "rows": rows,
           "image_height": H, "widths": [min(widths), max(widths)]}

    def tokens(results):
        return sum(len(r[0]) for r in results)

    with torch.no_grad():
        mems, t_enc = timed(lambda: [model.encode(x) for x in xs])
        lens = [m.shape[1] for m in mems]
        out["memory_tokens"] = {"min": min(lens), "mean": round(sum(lens) / len(lens), 1), "max": max(lens)}
        # ---- the <eos> bias search of tools/eval_throughput.py (until the greedy sequences of a probe group end inside T) gives
        #      the upper end: without length normalisation a beam search stops at the first position at which <eos> enters a
        #      row's top `beam`, so its band of useful biases lies below the greedy one and is narrow.  Bisect it on a probe
        #      group until the mean length is between a quarter and three quarters of T
        bias = model.decoder.out_layer.bias.omr_phys
        eos = syn.GRANDSTAFF_EOS
        base = bias[eos].item()
        rng = random.Random(args.seed)
        hi = 0.0
        for add in (0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0):
            bias[eos] = base + add + rng.uniform(-0.1, 0.1)
            lengths = [len(s) for s in model.greedy_batch(mems[:32])]
            hi = bias[eos].item() - base
            if sum(lengths) / len(lengths) < 0.7 * T:
                break
        probe = mems[:args.group]
        lo, chosen, mean = 0.0, hi, 0.0
        for _ in range(16):
            chosen = 0.5 * (lo + hi)
            bias[eos] = base + chosen
            lengths = [len(r[0]) for r in model.beam_search_batch(probe, beam)]
            mean = sum(lengths) / len(lengths)
            if 0.25 * T <= mean <= 0.75 * T:
                break
            lo, hi = (chosen, hi) if mean > 0.75 * T else (lo, chosen)
        out["eos_bias_raised_by"] = round(chosen, 4)
        out["probe_mean_length"] = round(mean, 1)

        def loop():
            return [model.beam_search(m, beam) for m in mems]

        def batched():
            res = []
            for i in range(0, len(mems), args.group):
                res += model.beam_search_batch(mems[i:i + args.group], beam)
            return res

        want, _ = timed(loop)                                 # warm-up of every shape, both routes
        got, _ = timed(batched)
        equal = got == want
        t_loop, t_batched = [], []
        for _ in range(args.reps):
            r1, dt1 = timed(loop)
            r2, dt2 = timed(batched)
            equal = equal and r1 == want and r2 == want
            t_loop.append(dt1)
            t_batched.append(dt2)
        ntok = tokens(want)
        lengths = [len(r[0]) for r in want]
        out["sequence_lengths"] = {"min": min(lengths), "mean": round(ntok / len(lengths), 1), "max": max(lengths), "distinct": len(set(lengths)),
                                   "ended_by_eos": sum(r[0][-1] == "<eos>" for r in want)}
        out["loop_s"] = [round(min(t_loop), 3), round(max(t_loop), 3)]
        out["batched_s"] = [round(min(t_batched), 3), round(max(t_batched), 3)]
        out["loop_tokens_per_s"] = round(ntok / min(t_loop), 1)                   # the loop at its fastest
        out["batched_tokens_per_s"] = round(ntok / max(t_batched), 1)             # the batched route at its slowest
        out["batched_slowest_vs_loop_fastest"] = round(min(t_loop) / max(t_batched), 2)
        # ---- one input
        m0 = mems[len(mems) // 2]
        model.beam_search_batch([m0], beam)
        s1, dt1 = timed(lambda: model.beam_search(m0, beam))
        s2, dt2 = timed(lambda: model.beam_search_batch([m0], beam)[0])
        equal = equal and s1 == s2
        out["single_memory_tokens"], out["single_sequence_length"] = int(m0.shape[1]), len(s1[0])
        out["single_loop_s"], out["single_batched_s"] = round(dt1, 3), round(dt2, 3)
        del mems
        # ---- predict with and without a beam (both encode every input at batch size 1)
        out["encode_s"] = round(t_enc, 3)
        model.predict(xs[:args.group], beam=beam, batch_size=32)
        pb, dt = timed(lambda: model.predict(xs, beam=beam, batch_size=32))
        equal = equal and pb == [w for w, _ in want]
        out["predict_beam_s"], out["predict_beam_tokens_per_s"] = round(dt, 3), round(sum(len(p) for p in pb) / dt, 1)
        model.predict(xs[:args.group], batch_size=32)
        pg, dt = timed(lambda: model.predict(xs, batch_size=32))
        out["greedy_predict_s"], out["greedy_predict_tokens_per_s"] = round(dt, 3), round(sum(len(p) for p in pg) / dt, 1)
        out["predict_beam_vs_greedy_s"] = round(out["predict_beam_s"] / out["greedy_predict_s"], 2)
    out["all_equal"] = bool(equal)
    print(json.dumps(out), flush=True)
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
