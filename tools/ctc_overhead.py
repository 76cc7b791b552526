"""What the CTC auxiliary head costs on the C2 training step (bench.py's own workload: 32 images of 256 x 2048, 4 096 memory rows each,
T = 512, V = 6 997, bf16): the step (forward + backward + Adam) with ctc_weight 0, with 0.3 at ctc_pool 1, and with 0.3 at ctc_pool 4,
alternated inside ONE process so that all three see the same box and clocks; then the head's own pieces at the same shapes, each timed
alone: the head GEMM (forward), omr_ctc_fwd, the row pass of the same rows through omr_ce_fwd (what is left of omr_ctc_fwd is the prep, the
sweep launch and the finalize), and omr_ctc_bwd.

--parent DIR: a built checkout of the parent commit.  bench.py of DIR and of this tree are then run alternately as fresh child processes
(--pairs times): the acceptance figure is that ctc_weight = 0 -- this tree's bench.py -- costs what the parent costs, within the spread of the
pairs of the visit.

    python tools/ctc_overhead.py [--rounds 3] [--steps 10] [--parent DIR --pairs 3 --bench-steps 20]
"""
import argparse
import json
import os
import random
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W, T, LAYERS, D = 32, 256, 2048, 512, 6, 256


def build(weight, pool, dev):
    from omr_a2s_multimodal_transformer_amd import synthetic as syn
    from omr_a2s_multimodal_transformer_amd.config import ModelConfig
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    V = syn.GRANDSTAFF_VOCAB
    w2i = {("<PAD>" if i == 0 else "<eos>" if i == syn.GRANDSTAFF_EOS else "<sos>" if i == syn.GRANDSTAFF_SOS else f"t{i}"): i for i in range(V)}
    cfg = ModelConfig(d_model=D, nhead=4, ff_dim=D, num_layers=LAYERS, compute_dtype="bf16", ctc_weight=weight, ctc_pool=pool)
    torch.manual_seed(0)
    m = Transformer(H, W, T, w2i, {v: k for k, v in w2i.items()}, attn_window=-1, teacher_forcing_prob=0.2, config=cfg)
    x, xl, y_in, y_out = syn.synthetic_unimodal_batch(B, H, W, T, V, syn.GRANDSTAFF_SOS, syn.GRANDSTAFF_EOS, seed=1234)
    m.flatten_parameters(device=dev)
    m.train()
    opt = m.configure_optimizers()
    batch = (x.to(dev), xl.to(dev), y_in.pin_memory(), y_out.to(dev))

    def step(i):
        opt.zero_grad()
        loss = m.training_step(batch, i)
        loss.backward()
        opt.step()
        return loss

    return m, step, batch


def wall_ms(step, steps):
    for i in range(2):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def device_us(fn, steps=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def pieces(m, batch, pool, dev):
    """The head's kernels alone, at the shapes the step gives them."""
    from omr_a2s_multimodal_transformer_amd import kernels as K
    V = len(m.w2i)
    gh, gw = (H + 15) // 16, (W + 7) // 8
    F = K.ctc_frame_count(gh, gw, pool)
    g = torch.Generator().manual_seed(0)
    frames = torch.randn((B * F, D), generator=g).to(torch.bfloat16).to(dev)
    w = m.ctc_head.weight.omr_lowp
    buf = torch.empty((B * F, K.round_up(V, 8)), dtype=torch.bfloat16, device=dev)
    head = lambda: K.gemm(frames, w, bias=m.ctc_head.bias.omr_phys, out=buf[:, :V])  # noqa: E731
    head()
    logits = buf.view(B, F, -1)[:, :, :V]
    flen = torch.full((B,), F, dtype=torch.int32, device=dev)
    y = batch[3]
    state = {}

    def fwd():
        state["out"] = K.ctc_fwd(logits, flen, y, V, 0, m.w2i["<eos>"])

    fwd()
    rows_t = torch.randint(1, V, (B * F,), generator=g).to(dev)
    out = dict(frames=F, head_gemm_fwd_us=device_us(head), ctc_fwd_us=device_us(fwd),
               row_pass_us=device_us(lambda: K.ce_fwd(buf[:, :V], rows_t, V, 0)),
               ctc_bwd_us=device_us(lambda: K.ctc_bwd(logits, flen, y, state["out"][4], V, 0)),
               workspace_mb=round(K.ctc_workspace_bytes(B, F, y.shape[1], V) / 1e6, 1), infeasible=int(state["out"][2].cpu()))
    out["prep_sweep_finalize_us"] = out["ctc_fwd_us"] - out["row_pass_us"]
    return {k: (round(v, 1) if isinstance(v, float) else v) for k, v in out.items()}


def bench_ms(root, steps):
    root = os.path.abspath(root)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "3"], cwd=root,
                       capture_output=True, text=True, check=True)
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--parent", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    args = ap.parse_args()
    med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
    spread = lambda xs: (max(xs) - min(xs)) / med(xs)  # noqa: E731
    result = dict(tool="ctc_overhead")
    if args.parent:                                    # child processes first: this process has not touched the GPU yet
        mine, theirs = [], []
        for p in range(args.pairs):
            theirs.append(bench_ms(args.parent, args.bench_steps))
            mine.append(bench_ms(ROOT, args.bench_steps))
            print(f"pair {p}: parent {theirs[-1]:.3f} ms | this tree (ctc_weight = 0) {mine[-1]:.3f} ms | ratio {mine[-1] / theirs[-1]:.4f}", flush=True)
        result["bench_pairs"] = dict(parent_ms=theirs, tree_ms=mine, ratio=round(med(mine) / med(theirs), 4), spread_parent=round(spread(theirs), 4),
                                     spread_tree=round(spread(mine), 4))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    settings = [(0.0, 1), (0.3, 1), (0.3, 4)]
    ms = {s: [] for s in settings}
    built = {}
    for s in settings:
        random.seed(1234)
        built[s] = build(s[0], s[1], dev)
    for r in range(args.rounds):
        for s in settings:
            ms[s].append(wall_ms(built[s][1], args.steps))
        print(f"round {r}: " + " | ".join(f"w {s[0]} pool {s[1]}: {ms[s][-1]:.2f} ms" for s in settings), flush=True)
    result["step_ms"] = {f"w{s[0]}_pool{s[1]}": round(med(ms[s]), 3) for s in settings}
    result["step_spread"] = {f"w{s[0]}_pool{s[1]}": round(spread(ms[s]), 4) for s in settings}
    for s in settings[1:]:
        result[f"pieces_pool{s[1]}"] = pieces(built[s][0], built[s][2], s[1], dev)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
