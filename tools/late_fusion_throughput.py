"""Late-fusion evaluation throughput over pairs of different sizes: the batch-size-1 loops the reference runs over its test set
(weighted_prediction per pair, src/multimodal/weighted_multimodal/test.py:154-172; get_pred_seq_and_pred_prob_seq per sample,
src/multimodal/smith_waterman/test.py:113-134) against their batched forms (weighted_predict, Transformer.predict_with_probs).
Two unimodal models of benchmark config C2 (6-layer d_model 256 bf16 kern decoder, T = 512) with random-init weights, seeded
pairs: images of height 256 and audio inputs of height 192, widths spread over 512-4096 independently, the head bias of <eos>
raised in both models so that the sequences end at different lengths.  Prints one JSON line:
  loop_s                    wall-clock of [weighted_prediction(...) for every pair], timed twice (before and after the batched
                            run): the spread between the two is the noise margin
  batched_s                 weighted_predict(batch_size)
  sweep_loop_s / sweep_batched_s
                            the same for a sweep over 5 alphas (loop: 5 x the loop above; batched: one call with the list)
  probs_loop_s / probs_batched_s
                            get_pred_seq_and_pred_prob_seq per image against predict_with_probs
  *_tokens_per_s            predicted tokens over the wall-clock above
  equal                     every batched output equals the loop's (exit status 1 otherwise)
  batched_faster / sweep_below_5x
                            batched_s < min(loop_s); sweep_batched_s < 5 * batched_s
  --refill: also weighted_predict(refill=True) (continuous batching), three runs alternated with the grouped call
  --beam K: also beam search over the fusion (an extension: the reference decodes greedily): the weighted_beam_search loop over
            the pairs against weighted_predict(beam=K), three runs each, alternated, after a warm-up
            (beam_loop_s / beam_batched_s; beside batched_s, the greedy weighted_predict of the same pairs)
Usage: python tools/late_fusion_throughput.py [--n 64] [--batch 32] [--refill] [--beam 4]"""
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
from omr_a2s_multimodal_transformer_amd.weighted_fusion import weighted_beam_search, weighted_predict, weighted_prediction  # noqa: E402

SWEEP = [0.1, 0.3, 0.5, 0.7, 0.9]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def n_tokens(preds):
    return sum(len(p) for p in preds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--refill", action="store_true", help="also time weighted_predict(refill=True), alternated with the grouped call")
    ap.add_argument("--beam", type=int, default=1, help="also time weighted_beam_search per pair against weighted_predict(beam=K)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    V, T, HI, HA, WMAX = syn.GRANDSTAFF_VOCAB, 512, 256, 192, 4096
    cfg = ModelConfig(d_model=256, nhead=4, ff_dim=256, num_layers=6, compute_dtype="bf16")
    w2i = {("<PAD>" if i == 0 else "<eos>" if i == syn.GRANDSTAFF_EOS else "<sos>" if i == syn.GRANDSTAFF_SOS else f"t{i}"): i for i in range(V)}
    i2w = {v: k for k, v in w2i.items()}
    models = []
    for seed, h in ((0, HI), (1, HA)):
        torch.manual_seed(seed)
        m = Transformer(h, WMAX, T, w2i, i2w, attn_window=-1, config=cfg)
        m.flatten_parameters(device=dev)
        m.eval()
        models.append(m)
    img, aud = models
    g = torch.Generator().manual_seed(args.seed)

    def widths():
        return [512 + int(w) // 8 * 8 for w in torch.randint(0, WMAX - 512 + 1, (args.n,), generator=g)]

    wi, wa = widths(), widths()
    pairs = [(torch.rand((1, 1, HI, a), generator=g).to(dev), torch.rand((1, 1, HA, b), generator=g).to(dev)) for a, b in zip(wi, wa)]
    out = {"config": "2 x C2 bf16, T=512, random init", "pairs": args.n, "batch": args.batch, "alpha": args.alpha, "sweep": SWEEP,
           "image": {"height": HI, "widths": [min(wi), max(wi)]}, "audio": {"height": HA, "widths": [min(wa), max(wa)]}}
    with torch.no_grad():
        # ---- raise the <eos> bias of both models until the sequences of a probe group end inside T
        eos = syn.GRANDSTAFF_EOS
        biases = [m.decoder.out_layer.bias.omr_phys for m in models]
        base = [b[eos].item() for b in biases]
        rng = random.Random(args.seed)
        probe = pairs[:args.batch]
        weighted_prediction(pairs[0][0], pairs[0][1], img, aud, args.alpha)          # warm-up of both paths
        chosen = None
        for add in (0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0):
            for b, b0 in zip(biases, base):
                b[eos] = b0 + add + rng.uniform(-0.1, 0.1)
            lengths = [len(s) for s in weighted_predict(probe, img, aud, args.alpha, args.batch)]
            chosen = add
            if sum(lengths) / len(lengths) < 0.5 * T:
                break
        out["eos_bias_raised_by"] = chosen
        # ---- weighted fusion, one alpha: loop, batched, loop again
        loop = lambda a: [weighted_prediction(xi, xa, img, aud, a) for xi, xa in pairs]
        want, t_loop1 = timed(lambda: loop(args.alpha))
        got, t_batched = timed(lambda: weighted_predict(pairs, img, aud, args.alpha, args.batch))
        want2, t_loop2 = timed(lambda: loop(args.alpha))
        lengths = [len(p) for p in want]
        ntok = n_tokens(want)
        out["predicted_lengths"] = {"min": min(lengths), "mean": round(ntok / len(lengths), 1), "max": max(lengths), "distinct": len(set(lengths))}
        out["loop_s"] = [round(t_loop1, 3), round(t_loop2, 3)]
        out["batched_s"] = round(t_batched, 3)
        out["loop_tokens_per_s"] = [round(ntok / t_loop1, 1), round(ntok / t_loop2, 1)]
        out["batched_tokens_per_s"] = round(ntok / t_batched, 1)
        out["speedup_vs_faster_loop"] = round(min(t_loop1, t_loop2) / t_batched, 2)
        equal = {"weighted": got == want and want2 == want}
        # ---- the alpha sweep both ways
        sweep_want, t_sweep_loop = timed(lambda: {a: loop(a) for a in SWEEP})
        sweep_got, t_sweep = timed(lambda: weighted_predict(pairs, img, aud, SWEEP, args.batch))
        ntok_sweep = sum(n_tokens(p) for p in sweep_want.values())
        out["sweep_loop_s"] = round(t_sweep_loop, 3)
        out["sweep_batched_s"] = round(t_sweep, 3)
        out["sweep_loop_tokens_per_s"] = round(ntok_sweep / t_sweep_loop, 1)
        out["sweep_batched_tokens_per_s"] = round(ntok_sweep / t_sweep, 1)
        out["sweep_speedup"] = round(t_sweep_loop / t_sweep, 2)
        out["sweep_over_single_batched"] = round(t_sweep / t_batched, 2)
        equal["sweep"] = sweep_got == sweep_want
        # ---- tokens + top-1 values of one model (the inputs of the Smith-Waterman fusion)
        xs = [xi for xi, _ in pairs]
        img.get_pred_seq_and_pred_prob_seq(xs[0])
        probs_want, t_probs_loop = timed(lambda: [img.get_pred_seq_and_pred_prob_seq(x) for x in xs])
        probs_got, t_probs = timed(lambda: img.predict_with_probs(xs, args.batch))
        ntok_probs = sum(len(w) for w, _ in probs_want)
        out["probs_loop_s"] = round(t_probs_loop, 3)
        out["probs_batched_s"] = round(t_probs, 3)
        out["probs_loop_tokens_per_s"] = round(ntok_probs / t_probs_loop, 1)
        out["probs_batched_tokens_per_s"] = round(ntok_probs / t_probs, 1)
        out["probs_speedup"] = round(t_probs_loop / t_probs, 2)
        equal["predict_with_probs"] = probs_got == ([w for w, _ in probs_want], [p for _, p in probs_want])
        if args.refill:
            weighted_predict(pairs[:args.batch // 2], img, aud, args.alpha, args.batch, refill=True)      # warm-up
            grouped_s, refill_s = [], []
            for _ in range(3):
                got_r, t = timed(lambda: weighted_predict(pairs, img, aud, args.alpha, args.batch, refill=True))
                equal["weighted_refill"] = equal.get("weighted_refill", True) and got_r == want
                refill_s.append(round(t, 3))
                grouped_s.append(round(timed(lambda: weighted_predict(pairs, img, aud, args.alpha, args.batch))[1], 3))
            out["refill_s"] = refill_s
            out["grouped_s"] = grouped_s
            out["refill_speedup_vs_grouped"] = round(min(grouped_s) / min(refill_s), 2)
            out["refill_speedup_vs_faster_loop"] = round(min(t_loop1, t_loop2) / min(refill_s), 2)
        if args.beam > 1:
            beam_loop = lambda: [weighted_beam_search(xi, xa, img, aud, args.alpha, args.beam)[0] for xi, xa in pairs]
            weighted_beam_search(pairs[0][0], pairs[0][1], img, aud, args.alpha, args.beam)      # warm-up of both routes
            weighted_predict(pairs[:max(1, args.batch // args.beam)], img, aud, args.alpha, args.batch, beam=args.beam)
            beam_loop_s, beam_batched_s = [], []
            for _ in range(3):
                want_b, t = timed(beam_loop)
                beam_loop_s.append(round(t, 3))
                got_b, t = timed(lambda: weighted_predict(pairs, img, aud, args.alpha, args.batch, beam=args.beam))
                beam_batched_s.append(round(t, 3))
                equal["weighted_beam"] = equal.get("weighted_beam", True) and got_b == want_b
            ntok_b = n_tokens(want_b)
            out["beam"] = args.beam
            out["beam_pairs_per_state"] = max(1, args.batch // args.beam)
            out["beam_loop_s"] = beam_loop_s
            out["beam_batched_s"] = beam_batched_s
            out["beam_loop_tokens_per_s"] = round(ntok_b / min(beam_loop_s), 1)
            out["beam_batched_tokens_per_s"] = round(ntok_b / min(beam_batched_s), 1)
            out["beam_batched_slowest_vs_loop_fastest"] = round(min(beam_loop_s) / max(beam_batched_s), 2)
            out["beam_batched_vs_greedy_batched_s"] = round(min(beam_batched_s) / t_batched, 2)
            out["beam_differs_from_greedy"] = sum(1 for a, b in zip(want_b, want) if a != b)
    out["equal"] = equal
    out["batched_faster"] = t_batched < min(t_loop1, t_loop2)
    out["sweep_below_5x"] = t_sweep < 5 * t_batched
    print(json.dumps(out), flush=True)
    return 0 if all(equal.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
