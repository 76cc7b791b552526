"""Training throughput on a batch of different-sized score images (DESIGN.md "Ragged training"): 32 images, heights 128-256, widths
568-4064, bf16, the C2 model (6 decoder layers, d_model 256, kern vocabulary, T = 512), fwd + bwd + Adam, dropout on.

  (a) ragged   one step over the zero-padded batch with per-sample sizes (Transformer.forward with xl [B, 2])
  (b) alone    32 batch-size-1 forward + backward passes into the same gradient buffer, weighted n_b / N, and one optimizer step:
               the only way to get (a)'s semantics without the ragged route -- the baseline
  (c) dense    one step of the dense route at the padded size: other arithmetic (the padding enters the convs and the norms); the
               speed ceiling

The three are run alternately, `--rounds` times, `--steps` steps each after `--warmup`; prints one JSON line with the samples/s of
every round and their medians.  `--only a|b|c` runs one of them (for a kernel trace of its own)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--only", default="", choices=["", "a", "b", "c"])
    args = ap.parse_args()

    from omr_a2s_multimodal_transformer_amd import synthetic as syn
    from omr_a2s_multimodal_transformer_amd.config import C2_IMAGE
    from omr_a2s_multimodal_transformer_amd.image import collate_ragged
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    from omr_a2s_multimodal_transformer_amd.runtime import seed_dropout

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    V, T, B = syn.GRANDSTAFF_VOCAB, args.seq, args.batch
    sos, eos = syn.GRANDSTAFF_SOS, syn.GRANDSTAFF_EOS
    w2i = {("<PAD>" if i == 0 else "<eos>" if i == eos else "<sos>" if i == sos else f"t{i}"): i for i in range(V)}
    i2w = {v: k for k, v in w2i.items()}
    torch.manual_seed(0)
    random.seed(1234)
    g = torch.Generator().manual_seed(99)
    heights = torch.randint(128, 257, (B,), generator=g).tolist()
    widths = torch.randint(568, 4065, (B,), generator=g).tolist()
    heights[0], widths[0] = 256, 4064                     # the plane the benchmark names
    imgs = [torch.rand((1, h, w), generator=g) for h, w in zip(heights, widths)]
    x, sizes = collate_ragged(imgs)
    H, W = x.shape[2], x.shape[3]
    _, _, y_in, y_out = syn.synthetic_unimodal_batch(B, 16, 8, T, V, sos, eos, seed=1234)
    counts = (y_out != 0).sum(1).tolist()
    N = float(sum(counts))
    model = Transformer(H, W, T, w2i, i2w, attn_window=-1, teacher_forcing_prob=0.2, config=C2_IMAGE)
    model.flatten_parameters(device=dev)
    model.train()
    seed_dropout(1234, 0)
    opt = model.configure_optimizers()

    x_d, y_out_d, y_in_p = x.to(dev), y_out.to(dev), y_in.pin_memory()
    crops = [im.unsqueeze(0).to(dev) for im in imgs]
    lens = [((h + 15) // 16) * ((w + 7) // 8) for h, w in zip(heights, widths)]
    xl_alone = [torch.tensor([n], dtype=torch.int32) for n in lens]
    xl_dense = torch.tensor(lens, dtype=torch.int32)       # the dense route's memory lengths (its +1.0 key mask)
    y_in_rows = [y_in[b:b + 1].contiguous().pin_memory() for b in range(B)]
    y_out_rows = [y_out_d[b:b + 1].contiguous() for b in range(B)]

    def step_ragged(i):
        opt.zero_grad()
        loss = model.training_step((x_d, sizes, y_in_p, y_out_d), i)
        loss.backward()
        opt.step()
        return loss

    def step_alone(i):
        opt.zero_grad()
        for b in range(B):
            loss = model.training_step((crops[b], xl_alone[b], y_in_rows[b], y_out_rows[b]), i)
            (loss * (counts[b] / N)).backward()
        opt.step()
        return loss

    def step_dense(i):
        opt.zero_grad()
        loss = model.training_step((x_d, xl_dense, y_in_p, y_out_d), i)
        loss.backward()
        opt.step()
        return loss

    modes = {"a": ("ragged", step_ragged), "b": ("alone", step_alone), "c": ("dense", step_dense)}
    order = [args.only] if args.only else ["a", "b", "c"]
    rates = {modes[k][0]: [] for k in order}
    for _ in range(args.rounds):
        for k in order:
            name, fn = modes[k]
            for i in range(args.warmup):
                fn(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                loss = fn(i)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert torch.isfinite(loss), name
            rates[name].append(round(B * args.steps / dt, 2))
    out = {"metric": "training samples/sec on 32 different-sized images", "unit": "samples/s", "dtype": "bf16", "batch": B, "seq_len": T,
           "plane": f"{H}x{W}", "pixels_real_over_padded": round(sum(h * w for h, w in zip(heights, widths)) / (B * H * W), 3),
           "steps": args.steps, "warmup": args.warmup, "rounds": rates,
           "median": {k: statistics.median(v) for k, v in rates.items()}, "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2**30, 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
