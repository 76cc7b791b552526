"""Multimodal training throughput on a batch of different-sized (image, spectrogram) pairs (DESIGN.md "Ragged multimodal training"):
C4's per-GPU batch of 8 pairs, image heights 128-256 and widths 568-4064, spectrograms of 195 bins x 128-512 frames, bf16, the C4
model (two encoders, `concat` mixer, 6 decoder layers, d_model 256, kern vocabulary, T = 512), fwd + bwd + Adam, dropout on.

  (a) ragged   one step over the two zero-padded batches with per-sample sizes (MultimodalTransformer.forward with xli, xla [B, 2])
  (b) alone    8 batch-size-1 forward + backward passes (xli = xla = None) into the same gradient buffer, weighted n_b / N, and one
               optimizer step: the only way to get (a)'s semantics without the ragged route -- the baseline
  (c) dense    one step of the dense route at the padded sizes: other arithmetic (the padding enters the convs and the norms of both
               encoders); the speed ceiling

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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--mixer", default="concat", choices=["concat", "attn_img", "attn_audio", "attn_both"])
    ap.add_argument("--only", default="", choices=["", "a", "b", "c"])
    args = ap.parse_args()

    from omr_a2s_multimodal_transformer_amd import synthetic as syn
    from omr_a2s_multimodal_transformer_amd.config import C2_IMAGE
    from omr_a2s_multimodal_transformer_amd.image import collate_ragged_pairs
    from omr_a2s_multimodal_transformer_amd.model import MultimodalTransformer
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
    frames = torch.randint(128, 513, (B,), generator=g).tolist()
    heights[0], widths[0] = 256, 4064                     # the planes are fixed; the widest image does not have the longest audio
    frames[-1] = 512
    imgs = [torch.rand((1, h, w), generator=g) for h, w in zip(heights, widths)]
    auds = [torch.rand((1, 195, f), generator=g) for f in frames]
    xi, si, xa, sa = collate_ragged_pairs(imgs, auds)
    (Hi, Wi), (Ha, Wa) = xi.shape[2:], xa.shape[2:]
    _, _, y_in, y_out = syn.synthetic_unimodal_batch(B, 16, 8, T, V, sos, eos, seed=1234)
    counts = (y_out != 0).sum(1).tolist()
    N = float(sum(counts))
    model = MultimodalTransformer(Hi, Wi, Ha, Wa, T, w2i, i2w, mixer_type=args.mixer, attn_window=-1, teacher_forcing_prob=0.2,
                                  teacher_forcing_modality_prob=0.2, config=C2_IMAGE)           # bench.py's C4 model
    model.flatten_parameters(device=dev)
    model.train()
    seed_dropout(1234, 0)
    opt = model.configure_optimizers()

    xi_d, xa_d, y_out_d, y_in_p = xi.to(dev), xa.to(dev), y_out.to(dev), y_in.pin_memory()
    crops_i = [im.unsqueeze(0).to(dev) for im in imgs]
    crops_a = [au.unsqueeze(0).to(dev) for au in auds]
    len_i = [((h + 15) // 16) * ((w + 7) // 8) for h, w in zip(heights, widths)]
    len_a = [((195 + 15) // 16) * ((f + 7) // 8) for f in frames]
    xli_dense = torch.tensor(len_i, dtype=torch.int32)     # the dense route's memory lengths
    xla_dense = torch.tensor(len_a, dtype=torch.int32)
    y_in_rows = [y_in[b:b + 1].contiguous().pin_memory() for b in range(B)]
    y_out_rows = [y_out_d[b:b + 1].contiguous() for b in range(B)]

    def step_ragged(i):
        opt.zero_grad()
        loss = model.training_step((xi_d, si, xa_d, sa, y_in_p, y_out_d), i)
        loss.backward()
        opt.step()
        return loss

    def step_alone(i):
        opt.zero_grad()
        for b in range(B):
            loss = model.training_step((crops_i[b], None, crops_a[b], None, y_in_rows[b], y_out_rows[b]), i)
            (loss * (counts[b] / N)).backward()
        model._touched = None                              # each pair drew its own modality: every sub-module may hold a gradient
        opt.step()
        return loss

    def step_dense(i):
        opt.zero_grad()
        loss = model.training_step((xi_d, xli_dense, xa_d, xla_dense, y_in_p, y_out_d), i)
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
    out = {"metric": f"training samples/sec on {B} different-sized (image, audio) pairs", "unit": "samples/s", "dtype": "bf16", "batch": B,
           "seq_len": T, "mixer": args.mixer, "image_plane": f"{Hi}x{Wi}", "audio_plane": f"{Ha}x{Wa}",
           "image_pixels_real_over_padded": round(sum(h * w for h, w in zip(heights, widths)) / (B * Hi * Wi), 3),
           "audio_pixels_real_over_padded": round(sum(195 * f for f in frames) / (B * Ha * Wa), 3),
           "memory_rows": {"image": len_i, "audio": len_a},
           "steps": args.steps, "warmup": args.warmup, "rounds": rates,
           "median": {k: statistics.median(v) for k, v in rates.items()}, "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2**30, 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
