"""Speculative greedy decoding against the parent commit's `predict` on the same inputs, in the same visit, in alternating fresh
processes.

Target: 6 layers, d = 256, ff = 1024; draft: 2 layers, same widths and vocabulary; bf16; <eos> suppressed, so every input runs
max_seq_len = 256 positions; inputs 64 x 1024 (512 memory keys); batch 1, 4 and 32.  Per batch, in this order and each in its own
process: `predict` of the checkout given with --parent (a BUILT checkout of the commit before the feature: the yardstick; the package
is imported from there and from nowhere else), plain `predict` of this tree (the route without a draft, which this feature does not
touch: it should match the parent's), then for k in {2, 4, 8} `predict` with an unrelated random 2-layer draft (nothing accepted:
every cycle yields one token, so elapsed / cycles is the time of one cycle), then k = 4 with a copy of the target as the draft
(everything accepted; its cycle is dearer: the draft is the 6-layer model), then the plain and the parent's `predict` again.

A cycle's launches do not depend on what is accepted, so for acceptance rate a (accepted / drafted) a cycle yields 1 + a * k tokens
in the time measured with the random draft: tokens/s(a) = B * (1 + a * k) / t_cycle, and the break-even rate is the a at which that
equals the yardstick's tokens/s (the parent's `predict` when --parent is given, else this tree's plain `predict`).  No pass mark: the
numbers go to DESIGN.md "Speculative decoding".  Acceptance on trained models is not measured here (there are no trained checkpoints
in this repository).

    git worktree add ../parent <parent commit> && make -C ../parent/omr_a2s_multimodal_transformer_amd/csrc
    python tools/spec_decode_throughput.py --parent ../parent      # the whole table, one JSON line per measurement and a summary
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAX_SEQ, H, W = 256, 64, 1024


def child(mode: str, k: int, batch: int, repeats: int, root: str) -> None:
    sys.path.insert(0, root)
    import torch
    import omr_a2s_multimodal_transformer_amd as pkg
    assert os.path.dirname(os.path.dirname(os.path.abspath(pkg.__file__))) == os.path.abspath(root), pkg.__file__
    from omr_a2s_multimodal_transformer_amd import synthetic as syn
    from omr_a2s_multimodal_transformer_amd.config import ModelConfig
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    V = syn.GRANDSTAFF_VOCAB
    w2i, i2w = syn.make_vocab(V)

    def model(layers: int, seed: int):
        cfg = ModelConfig(d_model=256, nhead=4, ff_dim=1024, num_layers=layers, compute_dtype="bf16", dropout=0.0, encoder_dropout=0.0)
        m = Transformer(H, W, MAX_SEQ, w2i, i2w, config=cfg)
        m.load_state_dict(syn.seeded_state_dict(syn.transformer_shapes(V, 256, 1024, layers), seed), strict=False)
        m.flatten_parameters()
        m.eval()
        m.decoder.out_layer.bias.omr_phys[w2i["<eos>"]] = -1e4
        return m

    target = model(6, 11)
    draft = None if mode in ("plain", "parent") else model(6, 11) if mode == "copy" else model(2, 23)
    g = torch.Generator().manual_seed(3)
    xs = [torch.rand((1, 1, H, W), generator=g).to("cuda") for _ in range(batch)]
    kw = {} if draft is None else dict(draft=draft, draft_len=k)
    with torch.no_grad():
        out = target.predict(xs, batch_size=batch, **kw)          # warm-up
        times = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = target.predict(xs, batch_size=batch, **kw)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
    tokens = sum(len(s) for s in out)
    best = min(times)
    rec = dict(mode=mode, k=k, batch=batch, seconds=best, tokens=tokens, tokens_per_s=tokens / best)
    if draft is not None:
        s = target.last_spec_stats
        rec.update(cycles=s["cycles"], drafted=s["drafted"], accepted=s["accepted"], ms_per_cycle=1e3 * best / max(s["cycles"], 1))
    print(json.dumps(rec), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 4, 32])
    ap.add_argument("--parent", default=None, help="root of a built checkout of the parent commit: the yardstick")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.k, args.batch, args.repeats, args.root)
        return
    rows = []
    yard = "parent" if args.parent else "plain"
    order = [("plain", 0), ("random", 2), ("random", 4), ("random", 8), ("copy", 4), ("plain", 0)]
    if args.parent:
        order = [("parent", 0)] + order + [("parent", 0)]
    for batch in args.batches:
        for mode, k in order:
            root = os.path.abspath(args.parent) if mode == "parent" else ROOT
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--k", str(k), "--batch", str(batch), "--repeats", str(args.repeats),
                   "--root", root]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if res.returncode != 0:
                print(res.stderr[-2000:], file=sys.stderr)
                raise SystemExit(f"measurement {mode} k={k} batch={batch} failed with {res.returncode}")
            rec = json.loads(res.stdout.strip().splitlines()[-1])
            rows.append(rec)
            print(json.dumps(rec), flush=True)
    for batch in args.batches:
        plain = max(r["tokens_per_s"] for r in rows if r["batch"] == batch and r["mode"] == yard)
        for r in rows:
            if r["batch"] == batch and r["mode"] == "random":
                t_cycle = r["seconds"] / r["cycles"]
                break_even = (plain * t_cycle / batch - 1.0) / r["k"]
                full = batch * (1 + r["k"]) / t_cycle
                print(f"batch {batch:2d} k {r['k']}: {yard} {plain:8.0f} tok/s; cycle {1e3 * t_cycle:6.3f} ms; all accepted {full:8.0f} tok/s "
                      f"({full / plain:4.2f}x); break-even acceptance {break_even:5.2f}")


if __name__ == "__main__":
    main()
