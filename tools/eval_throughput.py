"""Evaluation throughput over inputs of different sizes: the batch-size-1 greedy loop of validation_step against the ragged
batched decode (Transformer.greedy_batch on a list of memories, Transformer.evaluate).  Benchmark config C2 (6-layer d_model
256 bf16 kern decoder, T = 512) with random-init weights, 64 seeded images of height 256 and widths spread over 512-4096
(memories of 1024-8192 tokens).  Prints one JSON line:
  bs1_tokens_per_s          _greedy, one memory at a time (every row runs max_seq_len tokens: random weights seldom emit <eos>)
  ragged_tokens_per_s       greedy_batch over a list of 32 memories of different lengths
  same_size_tokens_per_s    greedy_batch over 32 copies of one memory of the set's mean length (the existing batched path)
  evaluate_s / validation_loop_s
                            wall-clock of evaluate(batch_size=32) and of validation_step x 64 + on_validation_epoch_end on the
                            same 64 samples, the head bias of <eos> raised so that the sequences end at different lengths;
                            encode_s: the 64 batch-size-1 encoder passes both of them include
  --refill                  also times evaluate(batch_size, refill=True) (continuous batching) three times, alternated with the
                            grouped evaluate, and counts the positions each plan runs (grouped: every group until its longest
                            row ends; stream: the positions of the slot state)
Usage: python tools/eval_throughput.py [--n 64] [--batch 32] [--bs1-samples 8] [--refill]"""
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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--bs1-samples", type=int, default=8, help="memories timed through the batch-size-1 loop")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--refill", action="store_true", help="also measure evaluate(refill=True)")
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
    ys = [torch.cat([torch.tensor([[syn.GRANDSTAFF_SOS]]), torch.randint(3, V, (1, int(n)), generator=g), torch.tensor([[syn.GRANDSTAFF_EOS]])], 1)
          for n in torch.randint(100, 400, (args.n,), generator=g)]
    out = {"config": "C2 bf16, T=512, random init", "samples": args.n, "batch": args.batch, "image_height": H,
           "widths": [min(widths), max(widths)]}
    with torch.no_grad():
        mems = [model.encode(x) for x in xs]
        lens = [m.shape[1] for m in mems]
        out["memory_tokens"] = {"min": min(lens), "mean": round(sum(lens) / len(lens), 1), "max": max(lens)}
        # ---- decode rates, every row runs T tokens
        model._greedy(mems[0])                                                        # warm-up
        nb = min(args.bs1_samples, len(mems))
        seqs, dt = timed(lambda: [model._greedy(m)[0] for m in mems[:nb]])
        out["bs1_tokens_per_s"] = round(sum(len(s) for s in seqs) / dt, 1)
        group = mems[:args.batch]
        model.greedy_batch(group[:2])                                                 # warm-up
        seqs, dt = timed(lambda: model.greedy_batch(group))
        out["ragged_tokens_per_s"] = round(sum(len(s) for s in seqs) / dt, 1)
        out["ragged_rows"] = len(group)
        out["ragged_group_memory_tokens"] = {"min": min(m.shape[1] for m in group), "max": max(m.shape[1] for m in group)}
        mean = sum(lens) / len(lens)
        wm = int(round(mean / ((H + 15) // 16) * 8 / 8)) * 8
        xm = torch.rand((1, 1, H, wm), generator=g).to(dev)
        mm = model.encode(xm).expand(args.batch, -1, -1).contiguous()
        model.greedy_batch(mm[:2].contiguous())
        seqs, dt = timed(lambda: model.greedy_batch(mm))
        out["same_size_tokens_per_s"] = round(sum(len(s) for s in seqs) / dt, 1)
        out["same_size_memory_tokens"] = int(mm.shape[1])
        out["ragged_vs_bs1"] = round(out["ragged_tokens_per_s"] / out["bs1_tokens_per_s"], 2)
        out["ragged_vs_same_size"] = round(out["ragged_tokens_per_s"] / out["same_size_tokens_per_s"], 3)
        # ---- evaluate vs the validation loop: raise the <eos> bias until the sequences of a probe group end inside T
        bias = model.decoder.out_layer.bias.omr_phys
        eos = syn.GRANDSTAFF_EOS
        base = bias[eos].item()
        rng = random.Random(args.seed)
        probe = mems[:args.batch]
        chosen = None
        for add in (0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0):
            bias[eos] = base + add + rng.uniform(-0.1, 0.1)
            lengths = [len(s) for s in model.greedy_batch(probe)]
            chosen = bias[eos].item() - base
            if sum(lengths) / len(lengths) < 0.7 * T:
                break
        out["eos_bias_raised_by"] = round(chosen, 3)
        del mems
    batches = list(zip(xs, ys))
    with torch.no_grad():
        _, t_enc = timed(lambda: [model.encode(x) for x in xs])          # the batch-size-1 encoder passes both paths share
    out["encode_s"] = round(t_enc, 3)
    metrics_b, t_eval = timed(lambda: model.evaluate(batches, batch_size=args.batch))

    def loop():
        for i, b in enumerate(batches):
            model.validation_step(b, i)
        lengths = [len(p) for p in model.YHat]
        return model.on_validation_epoch_end(), lengths

    (metrics_1, lengths), t_loop = timed(loop)
    out["predicted_lengths"] = {"min": min(lengths), "mean": round(sum(lengths) / len(lengths), 1), "max": max(lengths),
                                "distinct": len(set(lengths))}
    out["evaluate_s"] = round(t_eval, 3)
    out["validation_loop_s"] = round(t_loop, 3)
    out["evaluate_speedup"] = round(t_loop / t_eval, 2)
    out["evaluate_equals_validation_loop"] = metrics_b == metrics_1
    out["metrics"] = metrics_b
    ok = metrics_b == metrics_1
    if args.refill:
        from omr_a2s_multimodal_transformer_amd.evaluation import plan_groups
        states = []
        model._refill_state_hook = states.append
        model.evaluate(batches[:args.batch // 2], batch_size=args.batch, refill=True)      # warm-up
        del states[:]
        grouped_s, refill_s = [], []
        for _ in range(3):
            metrics_r, t = timed(lambda: model.evaluate(batches, batch_size=args.batch, refill=True))
            ok = ok and metrics_r == metrics_1
            refill_s.append(round(t, 3))
            grouped_s.append(round(timed(lambda: model.evaluate(batches, batch_size=args.batch))[1], 3))
        with torch.no_grad():
            mem_lens = [model.encode(x).shape[1] for x in xs]
        singles, groups = plan_groups(mem_lens, args.batch)
        out["evaluate_refill_s"] = refill_s
        out["evaluate_grouped_s"] = grouped_s
        out["refill_speedup_vs_grouped"] = round(min(grouped_s) / min(refill_s), 2)
        out["refill_speedup_vs_validation_loop"] = round(t_loop / min(refill_s), 2)
        out["positions_grouped"] = sum(max(lengths[i] for i in g) for g in groups)
        out["positions_refill"] = sum(s.positions for s in states) // 3
        out["evaluate_refill_equals_validation_loop"] = ok
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
