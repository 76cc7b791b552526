"""Training throughput through three input paths (DESIGN.md "Resident dataset and bucketed batches"): the C2 model (6 decoder layers,
d_model 256, kern vocabulary) in bf16, T = 512, 1 024 synthetic score images with the size draw of tools/ragged_train_throughput.py
(heights 128-256, widths 568-4064, values k / 255), targets as long as the image is wide; one epoch of fwd + bwd + Adam over the
ragged route, batch size 32.

  (i)   host      ddp.ShardedLoader + image.collate_ragged from host tensors, random batches: the only way before the resident set
  (ii)  bucketed  the batches of resident.plan_batches, built by the same host collate
  (iii) resident  the same plan through resident.ResidentLoader: one gather kernel per batch, no host pixel work

The paths alternate, `--rounds` times.  Every (round, path) is a process of its own under its own time limit, started by a parent
that never touches the GPU; a child that fails or runs out of time ends the run.  Per path: samples/s of the epoch, real / padded
pixels of its batches, the host time per step between the return of one optimizer step and the call of the next training_step
(fetching and uploading the batch), and torch.cuda.max_memory_reserved (the plane's shape changes with every step).  Prints one
JSON line."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PATHS = {"i": "host", "ii": "bucketed", "iii": "resident"}


def child(args):
    import torch

    from omr_a2s_multimodal_transformer_amd import synthetic as syn
    from omr_a2s_multimodal_transformer_amd.config import C2_IMAGE
    from omr_a2s_multimodal_transformer_amd.ddp import ShardedLoader
    from omr_a2s_multimodal_transformer_amd.image import collate_ragged
    from omr_a2s_multimodal_transformer_amd.lightning_shim import _to_device
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    from omr_a2s_multimodal_transformer_amd.resident import ResidentDataset, ResidentLoader, ResidentStore, padded_ratio, plan_batches
    from omr_a2s_multimodal_transformer_amd.runtime import seed_dropout

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    V, T, B, N = syn.GRANDSTAFF_VOCAB, args.seq, args.batch, args.samples
    sos, eos = syn.GRANDSTAFF_SOS, syn.GRANDSTAFF_EOS
    w2i = {("<PAD>" if i == 0 else "<eos>" if i == eos else "<sos>" if i == sos else f"t{i}"): i for i in range(V)}
    i2w = {v: k for k, v in w2i.items()}
    torch.manual_seed(0)
    random.seed(1234)
    g = torch.Generator().manual_seed(99)
    heights = torch.randint(128, 257, (N,), generator=g).tolist()
    widths = torch.randint(568, 4065, (N,), generator=g).tolist()
    sizes = torch.tensor(list(zip(heights, widths)))
    images = [torch.randint(0, 256, (1, h, w), generator=g, dtype=torch.uint8).float() / 255 for h, w in zip(heights, widths)]
    targets = []
    for w in widths:                                       # 8 .. T - 2 tokens, proportional to the width
        n = max(8, min(T - 2, w * (T - 2) // 4064))
        toks = torch.randint(1, V, (n,), generator=g)
        toks[(toks == sos) | (toks == eos)] = 1
        targets.append(torch.cat([torch.tensor([sos]), toks, torch.tensor([eos])]))

    def collate(items):
        x, xl = collate_ragged([im for im, _ in items])
        t = max(y.numel() for _, y in items) - 1
        y_in = torch.zeros((len(items), t), dtype=torch.int64)
        y_out = torch.zeros((len(items), t), dtype=torch.int64)
        for b, (_, y) in enumerate(items):
            y_in[b, :y.numel() - 1], y_out[b, :y.numel() - 1] = y[:-1], y[1:]
        return x, xl, y_in, y_out

    host_set = list(zip(images, targets))
    plan_kw = dict(chunk_batches=args.chunk_batches, seed=0)

    def epoch_batches(epoch):
        """(iterator over the epoch's batches, real / padded pixels of its plan)."""
        if args.path == "i":
            loader = ShardedLoader(host_set, B, collate, rank=0, world=1, seed=0)
            loader.set_epoch(epoch)
            idx = loader.indices()
            return iter(loader), padded_ratio([idx[i:i + B] for i in range(0, N, B)], sizes)
        plan = plan_batches(sizes, B, epoch=epoch, **plan_kw)
        if args.path == "ii":
            return (collate([host_set[n] for n in b]) for b in plan), padded_ratio(plan, sizes)
        resident.set_epoch(epoch)
        assert resident.plan() == plan
        return iter(resident), padded_ratio(plan, sizes)

    if args.path == "iii":
        store = ResidentStore("u8", dev)
        store.reserve(sum(h * w for h, w in zip(heights, widths)))
        for im in images:
            store.append(im)
        resident = ResidentLoader(ResidentDataset(images=store, targets=targets), B, torch.bfloat16, rank=0, world=1, **plan_kw)

    model = Transformer(256, 4064, T, w2i, i2w, attn_window=-1, teacher_forcing_prob=0.2, config=C2_IMAGE)
    model.flatten_parameters(device=dev)
    model.train()
    seed_dropout(1234, 0)
    opt = model.configure_optimizers()

    def run(batches, limit=None):
        steps = samples = 0
        wait = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while limit is None or steps < limit:
            tw = time.perf_counter()
            batch = next(batches, None)
            if batch is None:
                break
            batch = _to_device(batch, dev)
            wait += time.perf_counter() - tw
            opt.zero_grad()
            loss = model.training_step(batch, steps)
            loss.backward()
            opt.step()
            steps += 1
            samples += batch[0].shape[0]
        torch.cuda.synchronize()
        assert torch.isfinite(loss), args.path
        return samples, steps, wait, time.perf_counter() - t0

    run(epoch_batches(100)[0], limit=args.warmup)
    batches, ratio = epoch_batches(args.round)
    samples, steps, wait, dt = run(batches)
    assert samples == N, (samples, N)
    print(json.dumps({"path": PATHS[args.path], "round": args.round, "samples_per_s": round(samples / dt, 1), "steps": steps,
                      "real_over_padded": round(ratio, 3), "input_ms_per_step": round(1e3 * wait / steps, 2),
                      "max_memory_reserved_gb": round(torch.cuda.max_memory_reserved() / 2**30, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--chunk-batches", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds one (round, path) process may take")
    ap.add_argument("--path", default="", choices=[""] + list(PATHS))
    ap.add_argument("--round", type=int, default=0)
    args = ap.parse_args()
    if args.path:
        return child(args)
    rows = []
    for r in range(args.rounds):
        for p in PATHS:
            cmd = [sys.executable, os.path.abspath(__file__), "--path", p, "--round", str(r)] + [
                f"--{k}={getattr(args, k.replace('-', '_'))}" for k in ("batch", "samples", "seq", "chunk-batches", "warmup")]
            out = subprocess.run(cmd, timeout=args.step_timeout, check=True, capture_output=True, text=True).stdout
            rows.append(json.loads(out.strip().splitlines()[-1]))
            print(rows[-1], file=sys.stderr, flush=True)
    summary = {}
    for name in PATHS.values():
        mine = [x for x in rows if x["path"] == name]
        summary[name] = {"samples_per_s": [x["samples_per_s"] for x in mine], "median_samples_per_s": statistics.median(x["samples_per_s"] for x in mine),
                         "real_over_padded": [x["real_over_padded"] for x in mine],
                         "input_ms_per_step": [x["input_ms_per_step"] for x in mine],
                         "max_memory_reserved_gb": max(x["max_memory_reserved_gb"] for x in mine)}
    print(json.dumps({"metric": "training samples/sec over one epoch per input path", "unit": "samples/s", "dtype": "bf16", "batch": args.batch,
                      "samples": args.samples, "seq_len": args.seq, "chunk_batches": args.chunk_batches, "paths": summary}), flush=True)


if __name__ == "__main__":
    main()
