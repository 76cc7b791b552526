"""Records the bits that tests/test_instnorm_bits_gpu.py pins (tests/golden/instnorm_bits.json): one sha256 of the raw output bytes per
case of the InstanceNorm slot protocol (DESIGN.md "InstanceNorm slot protocol") -- the dense entries, the extent entries and the two
fused conv backwards that reduce into the slots.

    python tools/record_instnorm_bits.py CHECKOUT [OUT.json]

CHECKOUT is the root of a BUILT checkout of this project; the package is imported from there and from nowhere else, so the golden of
the commit before the protocol was written once is taken with a checkout of that commit (76405df, "Ragged training: ..."):

    git worktree add ../parent 76405df && make -C ../parent/omr_a2s_multimodal_transformer_amd/csrc
    python tools/record_instnorm_bits.py ../parent tests/golden/instnorm_bits.json

Run against this tree it prints the hashes the test computes.  Every case is deterministic (no atomics reach the hashed outputs: the
weight / bias gradients of the fused backwards are sums of atomics and are left out); inputs are real-valued, from seeded CPU
generators, so the order of every summation matters.  Needs a GPU."""
import hashlib
import json
import os
import sys

DEV = "cuda:0"
DENSE_SHAPE = (3, 37, 50)                        # B, H, W: odd, the last block of stage 1 has a partial slab
DENSE_WIDTHS = (16, 128, 256)                    # 256: two rounds in the slot reduction
PLANE, SIZES = (64, 96), ((64, 96), (37, 50), (17, 9))      # tests/test_extent_kernels_gpu.py's ragged batch
EXTENT_WIDTHS = (1, 3, 24, 128)                  # the scalar path, idle threads, the vector path
FUSED_SHAPE = (2, 20, 72)                        # tiles overhang both ways; fewer blocks per image than slots


def digest(*tensors) -> str:
    """sha256 over the raw bytes of the tensors, in order."""
    import torch
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().contiguous().cpu()
        if t.dtype == torch.bfloat16:
            t = t.view(torch.int16)
        h.update(t.numpy().tobytes())
    return h.hexdigest()


def compute(K) -> dict:
    """{case: sha256} with K = the kernels module of the checkout under test."""
    import torch
    out = {}

    def rnd(shape, seed, scale=1.0):
        return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale

    def slot_part(ws, B, C):
        return ws.view(-1)[: ws.numel() - B * C * 2]          # everything but the compact sums [B][C][2] at the end

    # ---- dense entries
    B, H, W = DENSE_SHAPE
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        for C in DENSE_WIDTHS:
            tag = f"dense/{name}/C{C}/"
            x = torch.relu(rnd((B, H, W, C), 100 + C) + 0.3).to(dt).to(DEV)
            g = rnd((B, H, W, C), 200 + C, 0.5).to(dt).to(DEV)
            mean, rstd = K.instnorm_stats(x)
            out[tag + "stats"] = digest(mean, rstd)
            out[tag + "bwd"] = digest(K.instnorm_bwd(g, x, mean, rstd, relu_mask=False))
            out[tag + "bwd_relu"] = digest(K.instnorm_bwd(g, x, mean, rstd, relu_mask=True, relu_scale=1.25))
            # a workspace filled by the conv epilogue (16 -> C channels): stat_mode 1 -> finalize; stat_mode 2 -> reduce_sums -> bwd_apply
            x16 = rnd((B, H, W, 16), 300 + C).to(dt).to(DEV)
            w = rnd((C, 3, 3, 16), 400 + C, 1.0 / 12).to(dt).to(DEV)
            bias = rnd((C,), 500 + C, 0.1).to(DEV)
            ws, slots = K.conv_stat_ws(B, H, W, C, DEV)
            ws.fill_(float("nan"))                            # every slot must be written, the spare ones as zeros
            y = K.conv3x3(x16, w, bias, relu=True, stat_mode=1, stat_ws=ws, stat_slots=slots)
            ymean, yrstd = K.instnorm_finalize(ws, slots, B, C, H * W)
            out[tag + "conv_stats"] = digest(slot_part(ws, B, C), ymean, yrstd)
            ws2, slots2 = K.conv_stat_ws(B, H, W, C, DEV)
            ws2.fill_(float("nan"))
            dxh = K.conv3x3(x16, w, None, stat_mode=2, stat_ws=ws2, stat_slots=slots2, stat_x=y, stat_stats=(ymean, yrstd))
            K.instnorm_reduce_sums(ws2, slots2, B, C)
            sums = digest(ws2)                                # slots and compact sums
            dx = K.instnorm_bwd_apply(dxh, y, ymean, yrstd, ws2, slots2, relu_mask=True, relu_scale=2.0)
            out[tag + "conv_bwd_sums"] = sums
            out[tag + "conv_bwd_apply"] = digest(dx)

    # ---- extent entries: NaN outside the extents
    B, (H, W) = len(SIZES), PLANE
    ext = torch.tensor(SIZES, dtype=torch.int32, device=DEV)
    inside = torch.zeros((B, H, W, 1), dtype=torch.bool)
    for b, (h, w_) in enumerate(SIZES):
        inside[b, :h, :w_] = True
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        for C in EXTENT_WIDTHS:
            tag = f"extent/{name}/C{C}/"
            nan = torch.full((B, H, W, C), float("nan"))
            x = torch.where(inside, torch.relu(rnd((B, H, W, C), 600 + C) + 0.3), nan).to(dt).to(DEV)
            g = torch.where(inside, rnd((B, H, W, C), 700 + C, 0.5), nan).to(dt).to(DEV)
            y, mean, rstd = K.instnorm_extent_fwd(x, ext)
            out[tag + "fwd"] = digest(y, mean, rstd)
            out[tag + "bwd"] = digest(K.instnorm_extent_bwd(g, x, mean, rstd, ext))
            out[tag + "bwd_relu"] = digest(K.instnorm_extent_bwd(g, x, mean, rstd, ext, relu_mask=True, relu_scale=1.25))

    # ---- fused conv backwards (bf16) that normalised their input on load: dx and the WHOLE workspace (pre-filled: the kernels write
    #      the slots only), spare slots included
    B, H, W = FUSED_SHAPE
    bf = torch.bfloat16
    for tag, c, strided in (("fused/xn16", 16, False), ("fused/s2", 32, True)):
        x = torch.relu(rnd((B, H, W, c), 800 + c)).to(bf).to(DEV)
        gshape = (B, (H + 1) // 2, (W + 1) // 2, c) if strided else (B, H, W, c)
        g = rnd(gshape, 810 + c, 0.5).to(bf).to(DEV)
        wf = K.conv3x3_weight_flip(rnd((c, 3, 3, c), 820 + c, 0.2).to(bf).to(DEV))
        mean, rstd = K.instnorm_stats(x)
        ws, slots = K.conv_stat_ws(B, H, W, c, DEV)
        ws.fill_(77.0)
        dw = torch.zeros((c, 3, 3, c), device=DEV)
        db = torch.zeros(c, device=DEV)
        if strided:
            dx = K.conv3x3_bwd_fused_s2(g, x, wf, dw, db, mean, rstd, ws, slots)
        else:
            dx = K.conv3x3_bwd_fused(g, x, wf, dw, db, False, 1.0, xnorm=(mean, rstd, ws, slots))
        out[tag] = digest(dx, ws)
    torch.cuda.synchronize()
    return out


def main() -> None:
    root = os.path.abspath(sys.argv[1])
    sys.path.insert(0, root)
    import omr_a2s_multimodal_transformer_amd as pkg
    from omr_a2s_multimodal_transformer_amd import kernels as K
    assert os.path.abspath(pkg.__file__).startswith(root + os.sep), f"imported {pkg.__file__}, not the package under {root}"
    out = compute(K)
    for k in sorted(out):
        print(k, out[k], flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
