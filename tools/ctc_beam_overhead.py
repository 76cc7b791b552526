"""What the joint CTC / attention beam search costs, and that the default did not move.  The model and inputs are those of
tools/beam_throughput.py (C2 bf16, T = 512, random init, seeded images of height 256 and widths 512-4096, beam 4) with a CTC head of
ctc_pool = 16 (one frame per grid column: 64-508 frames) and the <eos> bias raised by the amount recorded in profiles/beam_throughput.json.

  python tools/ctc_beam_overhead.py [--n 64] [--pairs 3] [--parent DIR]

1. predict(beam=4, batch_size=32) of a built checkout of the parent commit (--parent DIR) and of this tree without the keyword, and this
   tree's predict(beam=4, ctc_decode=0.3), alternated as fresh child processes --pairs times (this process has not touched the GPU then):
   medians, their ratios and the pair-to-pair spread (max / min - 1 of each series).
2. In this process: device time per position of a 32-row state (8 inputs x beam 4) over memories of 4096 tokens (256 frames) without and
   with the CTC score (BeamDecodeState.run over positions 4..35, <eos> suppressed so that nobody stops), and device time of the score and
   the advance kernel alone at Fmax = 1024 and 4096 (8 inputs x beam 4, V = the model's; device events around 50 launches each).
Prints one JSON line.  --child plain|joint --root DIR is what the child processes run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS_BIAS = 1.6726           # profiles/beam_throughput.json, eos_bias_raised_by
LAM = 0.3


def build(root):
    sys.path.insert(0, root)
    import torch
    from omr_a2s_multimodal_transformer_amd import synthetic as syn
    from omr_a2s_multimodal_transformer_amd.config import ModelConfig
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    V, T, H, WMAX = syn.GRANDSTAFF_VOCAB, 512, 256, 4096
    cfg = ModelConfig(d_model=256, nhead=4, ff_dim=256, num_layers=6, compute_dtype="bf16", ctc_weight=0.3, ctc_pool=16)
    w2i = {("<PAD>" if i == 0 else "<eos>" if i == syn.GRANDSTAFF_EOS else "<sos>" if i == syn.GRANDSTAFF_SOS else f"t{i}"): i for i in range(V)}
    torch.manual_seed(0)
    model = Transformer(H, WMAX, T, w2i, {v: k for k, v in w2i.items()}, attn_window=-1, config=cfg)
    model.flatten_parameters(device=dev)
    model.eval()
    model.decoder.out_layer.bias.omr_phys[syn.GRANDSTAFF_EOS] += EOS_BIAS
    return torch, syn, model, dev, (H, WMAX)


def images(torch, dev, n, H, WMAX, seed=7):
    g = torch.Generator().manual_seed(seed)
    widths = [512 + int(w) // 8 * 8 for w in torch.randint(0, WMAX - 512 + 1, (n,), generator=g)]
    return [torch.rand((1, 1, H, w), generator=g).to(dev) for w in widths]


def child(mode, root, n):
    torch, syn, model, dev, (H, WMAX) = build(root)
    xs = images(torch, dev, n, H, WMAX)
    kw = dict(ctc_decode=LAM) if mode == "joint" else {}
    with torch.no_grad():
        model.predict(xs[:8], beam=4, batch_size=32, **kw)             # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        preds = model.predict(xs, beam=4, batch_size=32, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    lengths = [len(p) for p in preds]
    print(json.dumps(dict(mode=mode, seconds=dt, tokens=sum(lengths), ended_by_eos=sum(p[-1] == "<eos>" for p in preds), min_len=min(lengths),
                          max_len=max(lengths), digest=hash(tuple(tuple(p) for p in preds)) & 0xffffffff)), flush=True)


def run_child(mode, root, n):
    env = dict(os.environ, PYTHONHASHSEED="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root, "--n", str(n)], capture_output=True, text=True,
                       env=env, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"child {mode} in {root} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def spread(v):
    return max(v) / min(v) - 1.0


def device_us(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def device_us_once(torch, fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0


def in_process(out):
    torch, syn, model, dev, _ = build(HERE)
    from omr_a2s_multimodal_transformer_amd import kernels as K
    V, beam, N = len(model.w2i), 4, 8
    sos, eos, blank = syn.GRANDSTAFF_SOS, syn.GRANDSTAFF_EOS, 0
    with torch.no_grad():
        # ---- the kernels alone
        for fmax in (1024, 4096):
            g = torch.Generator().manual_seed(fmax)
            logits = (torch.randn((N, fmax, K.round_up(V, 8)), generator=g) * 2.0).to(dev, torch.bfloat16)[:, :, :V]
            flen = torch.full((N,), fmax, dtype=torch.int32, device=dev)
            blk = K.CtcPrefixBlock(logits, flen, V, beam, blank, sos, eos, LAM)
            cand = torch.randint(3, eos, (N * beam, beam), generator=g).to(dev)
            parents = torch.arange(beam, dtype=torch.int32).repeat(N).to(dev)
            tokens = cand[:, 0].contiguous()
            delta = torch.empty((N * beam, beam), dtype=torch.float32, device=dev)
            blk.advance(0, parents, tokens)                              # parity 1 holds one-token hypotheses: the general recursion
            out[f"score_us_F{fmax}"] = round(device_us(torch, lambda: blk.scores(1, cand, out=delta), 50), 1)
            out[f"advance_us_F{fmax}"] = round(device_us(torch, lambda: blk.advance(1, parents, tokens), 50), 1)
            out[f"init_us_F{fmax}"] = round(device_us(torch, lambda: K.CtcPrefixBlock(logits, flen, V, beam, blank, sos, eos, LAM), 5), 1)
        # ---- a 32-row position without and with the score: 8 memories of 4096 tokens (grid 16 x 256: 256 frames at ctc_pool = 16)
        model.decoder.out_layer.bias.omr_phys[eos] -= 40.0               # nobody stops inside the timed positions
        xs = [torch.rand((1, 1, 256, 2048), generator=torch.Generator().manual_seed(50 + i)).to(dev) for i in range(N)]
        mems = [model.encode(x) for x in xs]
        steps = 32

        def positions(joint):                                            # device time of positions 4 .. 35 of one state, per position
            st = model.decoder.init_beam_decode(mems, beam, sos=sos, eos=eos)
            if joint:
                st.attach_ctc(*model._ctc_group(mems), LAM)
            st.run(4)
            us = device_us_once(torch, lambda: st.run(steps)) / steps
            assert not any(st.done())
            return us
        positions(False), positions(True)                                # warm-up
        plain, joint = [], []
        for _ in range(3):
            plain.append(positions(False))
            joint.append(positions(True))
        out["position_us_plain"] = round(statistics.median(plain), 1)
        out["position_us_joint_F256"] = round(statistics.median(joint), 1)
        out["position_us_spread"] = [round(spread(plain), 4), round(spread(joint), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--parent", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--root", default=HERE)
    args = ap.parse_args()
    if args.child:
        child(args.child, os.path.abspath(args.root), args.n)
        return 0
    out = {"config": "C2 bf16, T=512, random init, ctc_pool=16", "samples": args.n, "beam": 4, "lambda": LAM, "eos_bias_raised_by": EOS_BIAS}
    series = {"tree_plain": [], "tree_joint": []}
    if args.parent:
        series["parent_plain"] = []
    digests = {}
    for p in range(args.pairs):                                      # child processes first: this process has not touched the GPU yet
        for name in series:
            mode, root = ("joint" if name == "tree_joint" else "plain"), (os.path.abspath(args.parent) if name == "parent_plain" else HERE)
            r = run_child(mode, root, args.n)
            series[name].append(r["seconds"])
            digests.setdefault(name, set()).add(r["digest"])
            out[name + "_last"] = {k: r[k] for k in ("tokens", "ended_by_eos", "min_len", "max_len")}
        print(f"pair {p}: " + " | ".join(f"{k} {v[-1]:.3f} s" for k, v in series.items()), flush=True)
    for name, v in series.items():
        out[name + "_s"] = dict(median=round(statistics.median(v), 4), all=[round(x, 4) for x in v], spread=round(spread(v), 4))
    if args.parent:
        out["tree_plain_vs_parent"] = round(statistics.median(series["tree_plain"]) / statistics.median(series["parent_plain"]), 4)
        out["tree_joint_vs_parent"] = round(statistics.median(series["tree_joint"]) / statistics.median(series["parent_plain"]), 4)
        out["plain_predictions_equal_parent"] = digests["tree_plain"] == digests["parent_plain"] and len(digests["tree_plain"]) == 1
    out["tree_joint_vs_tree_plain"] = round(statistics.median(series["tree_joint"]) / statistics.median(series["tree_plain"]), 4)
    in_process(out)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
