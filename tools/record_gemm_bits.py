"""Records the bits that tests/test_gemm_bits_gpu.py pins (tests/golden/gemm_bits.json): one sha256 of the raw output bytes per case of
the GEMM family (DESIGN.md "GEMM family: shared steps").

    python tools/record_gemm_bits.py CHECKOUT [OUT.json]

CHECKOUT is the root of a BUILT checkout of this project; the package is imported from there and from nowhere else, so the golden of
the commit before the family's shared steps were written once is taken with a checkout of that commit (d747dd0, "Panel, tall and
grouped GEMMs: ..."):

    git worktree add ../parent d747dd0 && make -C ../parent/omr_a2s_multimodal_transformer_amd/csrc
    python tools/record_gemm_bits.py ../parent tests/golden/gemm_bits.json

Run against this tree it prints the hashes the test computes.  The case tables are this tree's (oracle/kernel_refs.py,
oracle/gemm_refs.py, oracle/decode_refs.py); the calls go through the checkout's kernels.gemm / gemm_row_groups / quantize_rows_fp8 /
gemm_fp8, whose signatures both sides share.  Hashed: everything a call writes -- the WHOLE C buffer with its padding, sentinel rows
and guard rows, and for fp8 also the codes and the scales.  Only outputs that no atomic reaches:
  tile/<name>        KR.GEMM_PRODUCT_CASES, GEMM_EPILOGUE_CASES                 M = 130, N = 70, K = 45 (FULLK) / 301 (pipelined)
  tile/<name>        KR.GEMM_DROPOUT_CASES, with the fused dropout
  tile/<name>        the split1 cases of KR.GEMM_COLSUM_CASES: C only (one split stores C; the column sums go through LDS and global
                     float atomics and are left out)
  group/<name>       G1, G2 of gemm_refs.TILE_GROUP_CASES (G3 is split-K 3)
  panel/P4, tall/T4  the real-valued cases of gemm_refs at the smallest M their routes accept
  fp8/<tag>-m<M>-k<K>  test_fp8_gemm_ragged's calls: codes and scales of both operands, then the whole C buffer
"inputs" holds one hash of the input arrays per case: a mismatch there means the inputs changed, not the kernels.  Needs a GPU."""
import hashlib
import json
import os
import sys

DEV = "cuda:0"
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case_tables():
    """(oracle.kernel_refs, oracle.gemm_refs, oracle.decode_refs): this tree's, wherever the package under test comes from."""
    if HERE not in sys.path:
        sys.path.append(HERE)
    from oracle import decode_refs as DR
    from oracle import gemm_refs as GR
    from oracle import kernel_refs as KR
    return KR, GR, DR


def tile_cases():
    """(case, with the fused dropout) of the generic kernel's table."""
    KR, _, _ = case_tables()
    plain = KR.GEMM_PRODUCT_CASES + KR.GEMM_EPILOGUE_CASES + tuple(c for c in KR.GEMM_COLSUM_CASES if c.split_k == 1)
    assert all(c.split_k == 1 for c in plain + KR.GEMM_DROPOUT_CASES)
    return [(c, False) for c in plain] + [(c, True) for c in KR.GEMM_DROPOUT_CASES]


def ref_cases():
    """(key, case) of oracle/gemm_refs.py: the non-split row-group cases of the tile kernel, P4 and T4."""
    _, GR, _ = case_tables()
    out = [(f"group/{c.name}", c) for c in GR.TILE_GROUP_CASES if c.split_k == 1]
    assert sorted(k[6:8] for k, _ in out) == ["G1", "G1", "G2", "G2", "G2", "G2"]
    out += [("panel/" + GR.case("P4").name, GR.case("P4")), ("tall/" + GR.case("T4").name, GR.case("T4"))]
    assert all(not c.exact for _, c in out[-2:]) and all(c.splits == 1 and not c.colsum for _, c in out)
    return out


def update(h, *tensors) -> None:
    """Feed the raw bytes of the tensors' whole storage views, in order (None: a marker byte)."""
    import torch
    for t in tensors:
        if t is None:
            h.update(b"\0")
            continue
        t = t.detach().contiguous().cpu()
        h.update((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy().tobytes())


def digest(*tensors) -> str:
    h = hashlib.sha256()
    update(h, *tensors)
    return h.hexdigest()


def whole(view):
    """The whole buffer behind an operand view (guard rows, padding)."""
    return view._base if view._base is not None else view


def compute(K) -> dict:
    """{"cases": {case: sha256}, "inputs": {case: sha256}} with K = the kernels module of the checkout under test."""
    import torch
    KR, GR, DR = case_tables()
    cases, inputs = {}, {}

    for c, fused in tile_cases():
        inp = KR.gemm_inputs(c)
        key = f"tile/{c.name}"
        inputs[key] = digest(inp["a_buf"], inp["b_buf"], inp["bias"], inp["c_buf"], inp.get("colsum0"))
        a_buf, b_buf, c_buf = inp["a_buf"].to(DEV), inp["b_buf"].to(DEV), inp["c_buf"].to(DEV)
        cs = inp["colsum0"].to(DEV) if c.colsum else None
        K.gemm(KR.view2d(a_buf, *inp["a_shape"]), KR.view2d(b_buf, *inp["b_shape"]), trans_a=c.ta, trans_b=c.tb,
               bias=None if inp["bias"] is None else inp["bias"].to(DEV), relu=c.relu, out=KR.view2d(c_buf, c.M, c.N),
               accumulate=c.accumulate, split_k=c.split_k, colsum_a=cs, drop=c.drop if fused else None)
        cases[key] = digest(c_buf)

    for key, c in ref_cases():
        inp = GR.inputs(c)
        inputs[key] = digest(whole(inp["a"]), whole(inp["b"]), inp["bias"], inp["c_buf"])
        a, b, c_buf = GR.on_device(inp["a"], DEV), GR.on_device(inp["b"], DEV), inp["c_buf"].to(DEV)
        bias = None if inp["bias"] is None else inp["bias"].to(DEV)
        assert GR.gemm_route(c, all(t.data_ptr() % 16 == 0 for t in (a, b, c_buf))) == c.route
        if c.group is None:
            K.gemm(a, b, trans_a=c.ta, trans_b=c.tb, bias=bias, relu=c.relu, out=c_buf[:c.M, :c.N])
        else:
            K.gemm_row_groups(a, b, c_buf, c.M, c.N, c.K, trans_a=c.ta, trans_b=c.tb, bias=bias, group=c.group)
        cases[key] = digest(c_buf)
        del a, b, c_buf

    for dtype in KR.DTYPES:
        for M, Kd in DR.FP8_CASES:
            inp = DR.fp8_inputs(M, Kd, dtype)
            key = f"fp8/{KR.TAG[dtype]}-m{M}-k{Kd}"
            inputs[key] = digest(inp["x_buf"], inp["w"], inp["bias"])
            a8, sa = K.quantize_rows_fp8(inp["x_buf"].to(DEV)[:M, :Kd])
            w8, sw = K.quantize_rows_fp8(inp["w"].to(DEV))
            c_buf = torch.full((M + 2, DR.FP8_N + 8), KR.SENTINEL, dtype=dtype, device=DEV)
            K.gemm_fp8(a8, sa, w8, sw, bias=inp["bias"].to(DEV), out=c_buf[:M, :DR.FP8_N])
            cases[key] = digest(a8, sa, w8, sw, c_buf)
    torch.cuda.synchronize()
    return dict(cases=cases, inputs=inputs)


def main() -> None:
    root = os.path.abspath(sys.argv[1])
    sys.path.insert(0, root)
    import omr_a2s_multimodal_transformer_amd as pkg
    from omr_a2s_multimodal_transformer_amd import kernels
    assert os.path.abspath(pkg.__file__).startswith(root + os.sep), f"imported {pkg.__file__}, not the package under {root}"
    out = compute(kernels)
    for kind in ("inputs", "cases"):
        for k in sorted(out[kind]):
            print(kind, k, out[kind][k], flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
