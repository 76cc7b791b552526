"""Bit parity of the attention kernels between two builds of libomr_hip.so (one library per process, chosen by OMR_HIP_LIB):
  python tools/attn_parity.py dump OUT.pt        o, lse, dq, dk, dv, the decode partials and decode_linear(part=...) of a fixed
                                                 seeded case list, with the library the process loaded
  python tools/attn_parity.py compare A.pt B.pt  every tensor of the two dumps bit for bit; prints one JSON line, exit 1 on a difference
The kernels have no atomics and sum in fixed order, so two builds that compute the same arithmetic give the same bits.
Cases: every ATTN_CASES row of tests/test_kernels_gpu.py in both dtypes (cross_key_split: forward and dQ split the keys), the
rows of test_attention_fwd_bwd_with_dropout_vs_torch_fp32 (read from the test's parametrize mark; the last one splits the keys
under dropout) in fp32 and bf16, one hd-32 dropout case, the decode rows T = 1, S = 700 / 1100 with and without kv_len, and the benchmark's
cross-attention shape (B 32, 4 heads, T 512, S 4096, bf16, dropout 0.1 + key bias)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"


def rnd(shape, seed, dtype):
    return ((torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1)).to(DEV, dtype)


def fwd_bwd(K, out, name, B, T, S, d, H, dtype, **kw):
    q, k, v, g = rnd((B, T, d), 1, dtype), rnd((B, S, d), 2, dtype), rnd((B, S, d), 3, dtype), rnd((B, T, d), 4, dtype)
    o, lse = K.attn_fwd(q, k, v, H, **kw)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    K.attn_bwd(q, k, v, o, g, lse, dq, dk, dv, H, **kw)
    for n, t in (("o", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
        out[f"{name}/{n}"] = t.cpu()


def key_bias(B, S, kind):
    kb = torch.zeros(B, S)
    for i, l in enumerate((S, (2 * S) // 3, S // 3)[:B]):
        kb[i, l:] = 1.0 if kind == "plus1" else float("-inf")
    return kb.to(DEV)


def dump(path):
    from omr_a2s_multimodal_transformer_amd import kernels as K
    from omr_a2s_multimodal_transformer_amd._lib import LIB_PATH, lib, ptr, cur_stream, dtype_code
    import test_kernels_gpu as tk
    import test_attention_r3_gpu as tr
    r3_rows = next(m.args[1] for m in tr.test_attention_fwd_bwd_with_dropout_vs_torch_fp32.pytestmark if m.args[0] == "T,S,causal,p")
    out = {}
    for dtype in (torch.float32, torch.bfloat16):
        dn = "f32" if dtype == torch.float32 else "bf16"
        for name, T, S, d, H, causal, window, kb, blk in tk.ATTN_CASES:
            B = 3
            kw = dict(causal=causal, window=window, key_bias=None if kb is None else key_bias(B, S, kb))
            if blk:
                kw["blk_lq"] = torch.tensor([T, T // 2, T // 4], dtype=torch.int32, device=DEV)
                kw["blk_lkv"] = torch.tensor([S, S // 2, S // 5], dtype=torch.int32, device=DEV)
            fwd_bwd(K, out, f"{name}/{dn}", B, T, S, d, H, dtype, **kw)
        for T, S, causal, p in r3_rows:
            kb = torch.zeros(2, S)
            kb[0, S - 40:] = 1.0
            kb[1, S - 25:] = float("-inf")
            fwd_bwd(K, out, f"r3_T{T}_S{S}/{dn}", 2, T, S, 128, 2, dtype, causal=causal, key_bias=kb.to(DEV), dropout_p=p, seed=99)
        fwd_bwd(K, out, f"hd32_drop/{dn}", 2, 70, 150, 128, 4, dtype, key_bias=key_bias(2, 150, "plus1"), dropout_p=0.25, seed=5)
        # decode rows: merged output, the partials, decode_linear's merge prologue; with and without per-row key counts
        for S in (700, 1100):
            B, H, d = 3, 4, 256
            hd = d // H
            q, k, v = rnd((B, 1, d), 5, dtype), rnd((B, S, d), 6, dtype), rnd((B, S, d), 7, dtype)
            part, ns = K.attn_fwd_split_partials(q, k, v, H)
            out[f"decode_S{S}/{dn}/partials"] = part.cpu().clone()
            if ns > 1:
                w, bias = rnd((d, d), 8, dtype), rnd((d,), 9, torch.float32)
                out[f"decode_S{S}/{dn}/decode_linear"] = K.decode_linear(w, bias, part=part, heads=H)[0].cpu()
            n = lib().query("omr_attn_split_workspace_floats", B, H, 1, S, hd)
            for tag, kv_len in (("full", None), ("kv_len", torch.tensor([S, (2 * S) // 3, 5], dtype=torch.int32, device=DEV))):
                o = torch.empty_like(q)
                lse = torch.empty((B, H, 1), dtype=torch.float32, device=DEV)
                ws = torch.empty(max(n, 1), dtype=torch.float32, device=DEV)
                lib().call("omr_attn_fwd_split_varlen", dtype_code(dtype), ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), d, d, d, d, d, S * d, S * d, d,
                           B, H, 1, S, hd, None, ptr(kv_len), ptr(ws), n, cur_stream())
                out[f"decode_S{S}/{dn}/{tag}/o"] = o.cpu()
                out[f"decode_S{S}/{dn}/{tag}/lse"] = lse.cpu()
    fwd_bwd(K, out, "bench_cross/bf16", 32, 512, 4096, 256, 4, torch.bfloat16, key_bias=key_bias(32, 4096, "plus1")[:32], dropout_p=0.1, seed=7)
    torch.cuda.synchronize()
    torch.save(out, path)
    print(json.dumps({"library": LIB_PATH, "tensors": len(out), "file": path}))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    bits = lambda t: t.contiguous().view(torch.uint8)
    differ = [n for n in sorted(set(a) | set(b)) if n not in a or n not in b or a[n].shape != b[n].shape or not torch.equal(bits(a[n]), bits(b[n]))]
    print(json.dumps({"tensors": len(a), "bit_identical": not differ, "differ": differ}))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
