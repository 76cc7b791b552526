"""Records the bits that tests/test_optim_bits_gpu.py pins (tests/golden/optim_bits.json): one sha256 of the raw output bytes per case
of the three optimizer entries (DESIGN.md "Optimizer step: one kernel").

    python tools/record_optim_bits.py CHECKOUT [OUT.json]

CHECKOUT is the root of a BUILT checkout of this project; the package is imported from there and from nowhere else, so the golden of
the commit before the three kernels became one is taken with a checkout of that commit (79e5dd9, "Loss kernels: ..."):

    git worktree add ../parent 79e5dd9 && make -C ../parent/omr_a2s_multimodal_transformer_amd/csrc
    python tools/record_optim_bits.py ../parent tests/golden/optim_bits.json

Run against this tree it prints the hashes the test computes.  The C entries are driven directly (lib().call with ptr / cur_stream of
_lib), never through kernels.py, whose wrappers changed with the kernels.  Inputs: tests/optim_refs.py's inputs(n, seed=n, steps=3),
HYPER, GRAD_SCALE, FIRST_STEP, WD and block_mask(n); the omr_adam cases flip the gradients' signs by those of
oracle.kernel_refs.adam_inputs()'s gradients (repeated cyclically up to n), so both signs of g pass through the moments.  Sizes:
tests/test_optim_recipe_gpu.py's SIZES and oracle.kernel_refs.ADAM_N, where the scalar grid of the removed kernels wrapped.
Per size, three consecutive steps on one state, every output hashed after every step:
  adam/lp0, adam/lp1                     omr_adam without / with the bf16 copy                       p, m, v, lp
  guarded/clip                           omr_adam_guarded, a fresh omr_grad_norm record per step,
                                         max_norm = a tenth of that gradient's scaled norm           p, m, v, lp
  adamw/{plain,decay,ema,decay+ema}/{free,guarded}
                                         omr_adamw_ema: weight_decay = WD on alternating blocks,
                                         ema_decay = f32(0.999), without / behind such a record      p, m, v, lp, ema
"inputs" holds one hash of the input arrays per size: a mismatch there means the inputs changed, not the kernels.  No atomic reaches
any output.  Needs a GPU."""
import ctypes
import hashlib
import json
import os
import struct
import sys

DEV = "cuda:0"
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3
N_WRAP = 2048 * 256 * 4 + 4 * 256 + 3                  # tests/test_optim_recipe_gpu.py: the vector loop wraps once, scalar tail of 3
ADAM_N = 2048 * 256 + 77                               # oracle/kernel_refs.py: the removed scalar kernels' grid wrapped here
SIZES = [1, 3, 4, 63, 64, 65, 4 * 1024 + 1, N_WRAP, ADAM_N]
ADAMW = {"plain": (False, False), "decay": (True, False), "ema": (False, True), "decay+ema": (True, True)}
CTL_BYTES = 152                                        # sizeof(omr_step_ctl); clip and apply at bytes 12 and 16


def case_tables():
    """(optim_refs, oracle.kernel_refs): this tree's, wherever the package under test comes from."""
    for p in (HERE, os.path.join(HERE, "tests")):
        if p not in sys.path:
            sys.path.append(p)
    import optim_refs as R
    from oracle import kernel_refs as KR
    assert KR.ADAM_N == ADAM_N
    return R, KR


def host_inputs(n: int) -> dict:
    """Everything a size's cases read, as numpy arrays."""
    import numpy as np
    R, KR = case_tables()
    p, m, v, ema, grads = R.inputs(n, seed=n, steps=STEPS)
    signs = [np.sign(np.resize(g.numpy(), n)).astype(np.float32) for g in KR.adam_inputs()["grads"][:STEPS]]
    return dict(p=p, m=m, v=v, ema=ema, grads=grads, signed=[g * s for g, s in zip(grads, signs)], blocks=R.block_mask(n)[0])


def input_digest(inp: dict) -> str:
    h = hashlib.sha256()
    for a in [inp["p"], inp["m"], inp["v"], inp["ema"], *inp["grads"], *inp["signed"], inp["blocks"]]:
        h.update(a.tobytes())
    return h.hexdigest()


def update(h, *tensors) -> None:
    """Feed the raw bytes of the tensors, in order."""
    import torch
    for t in tensors:
        t = t.detach().contiguous().cpu()
        h.update((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy().tobytes())


def compute(L) -> dict:
    """{"cases": {case: sha256}, "inputs": {size: sha256}} with L = the _lib module of the checkout under test."""
    import numpy as np
    import torch
    R, _ = case_tables()
    call, ptr, stream = L.lib().call, L.ptr, L.cur_stream
    H = R.HYPER
    hyper = (H["lr"], H["b1"], H["b2"], H["eps"])
    d = R.f32(0.999)
    cases, inputs = {}, {}

    for n in SIZES:
        inp = host_inputs(n)
        inputs[f"n={n}"] = input_digest(inp)
        dev = lambda a: torch.from_numpy(a.copy()).to(DEV)  # noqa: E731
        grads, signed, blocks = [dev(g) for g in inp["grads"]], [dev(g) for g in inp["signed"]], dev(inp["blocks"])
        ws = torch.empty(L.lib().query("omr_grad_norm_workspace_bytes", n, 1), dtype=torch.uint8, device=DEV)
        begin, end = (ctypes.c_long * 1)(0), (ctypes.c_long * 1)(n)

        def state(lowp=True):
            p = dev(inp["p"])
            return dict(p=p, m=dev(inp["m"]), v=dev(inp["v"]), ema=dev(inp["ema"]), lp=p.to(torch.bfloat16) if lowp else None)

        def record(j):
            """A fresh record for step j's gradient: clip = a tenth, from a real omr_grad_norm."""
            norm = float(np.sqrt((inp["grads"][j].astype(np.float64) ** 2).sum())) * R.GRAD_SCALE
            ctl = torch.zeros(CTL_BYTES, dtype=torch.uint8, device=DEV)
            call("omr_grad_norm", ptr(grads[j]), n, begin, end, 1, R.GRAD_SCALE, norm / 10, ptr(ws), ptr(ctl), stream())
            clip, apply = struct.unpack_from("<fi", ctl.cpu().numpy().tobytes(), 12)
            assert apply == 1 and 0.09 < clip < 0.11, (n, j, apply, clip)
            return ctl

        def run(name, step_fn, keys, lowp=True):
            st, h = state(lowp), hashlib.sha256()
            for j in range(STEPS):
                step_fn(st, j, R.FIRST_STEP + j)
                update(h, *(st[k] for k in keys if st[k] is not None))
            cases[f"{name}/n={n}"] = h.hexdigest()

        def adam(st, j, step):
            call("omr_adam", ptr(st["p"]), ptr(signed[j]), ptr(st["m"]), ptr(st["v"]), ptr(st["lp"]), n, step, *hyper, R.GRAD_SCALE, stream())

        def guarded(st, j, step):
            call("omr_adam_guarded", ptr(st["p"]), ptr(grads[j]), ptr(st["m"]), ptr(st["v"]), ptr(st["lp"]), n, step, *hyper, R.GRAD_SCALE,
                 ptr(record(j)), stream())

        def adamw(decay, ema, guard):
            def step_fn(st, j, step):
                call("omr_adamw_ema", ptr(st["p"]), ptr(grads[j]), ptr(st["m"]), ptr(st["v"]), ptr(st["lp"]), ptr(st["ema"]) if ema else None,
                     ptr(blocks) if decay else None, n, step, *hyper, R.WD if decay else 0.0, d if ema else 0.0, R.GRAD_SCALE,
                     ptr(record(j)) if guard else None, stream())
            return step_fn

        run("adam/lp0", adam, ("p", "m", "v", "lp"), lowp=False)
        run("adam/lp1", adam, ("p", "m", "v", "lp"))
        run("guarded/clip", guarded, ("p", "m", "v", "lp"))
        for name, (decay, ema) in ADAMW.items():
            for guard in (False, True):
                run(f"adamw/{name}/{'guarded' if guard else 'free'}", adamw(decay, ema, guard), ("p", "m", "v", "lp", "ema"))
    torch.cuda.synchronize()
    return dict(cases=cases, inputs=inputs)


def main() -> None:
    root = os.path.abspath(sys.argv[1])
    sys.path.insert(0, root)
    import omr_a2s_multimodal_transformer_amd as pkg
    from omr_a2s_multimodal_transformer_amd import _lib
    assert os.path.abspath(pkg.__file__).startswith(root + os.sep), f"imported {pkg.__file__}, not the package under {root}"
    out = compute(_lib)
    for kind in ("inputs", "cases"):
        for k in sorted(out[kind]):
            print(kind, k, out[kind][k], flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
