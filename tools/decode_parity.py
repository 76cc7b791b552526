"""Bit parity of the native decode executor between two builds of libomr_hip.so (one library per process, chosen by OMR_HIP_LIB):
  python tools/decode_parity.py dump OUT.pt        tokens, top-1 values, final fp32 logits and (beam entries) the search block of a
                                                   fixed seeded case list, with the library the process loaded
  python tools/decode_parity.py compare A.pt B.pt  every tensor of the two dumps bit for bit; prints one JSON line, exit 1 on a difference
The kernels have no atomics and sum in fixed order, so two builds that issue the same launches give the same bits.
Cases (2-layer decoders over seeded synthetic memories, d = 128): lock-step B = 1 and B = 3 in fp32 and bf16 with window -1 and 4;
ragged memories of 70, 300 and 700 tokens; three slots at positions (0, 5, 11); a weighted pair in lock-step and over slots; beam 3
over two inputs; weighted beam 3; fp8 weights; and the generic-width path (ff = 2304, which the row kernel refuses; d = 64 cannot
stand in for it: omr_add_layernorm_fwd takes widths 128 / 256 / 512 only), with and without fp8 weights."""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
V, D, STEPS = 60, 128, 12


def rnd(shape, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(DEV)


def model(seed, dtype="fp32", window=-1, ff=128, fp8=False, max_len=40):
    from omr_a2s_multimodal_transformer_amd import synthetic as syn
    from omr_a2s_multimodal_transformer_amd.config import ModelConfig
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    w2i, i2w = syn.make_vocab(V)
    cfg = ModelConfig(d_model=D, nhead=4, ff_dim=ff, num_layers=2, compute_dtype=dtype, fp8_decode=fp8)
    m = Transformer(32, 96, max_len, w2i, i2w, attn_window=window, config=cfg).eval()
    m.load_state_dict(syn.seeded_state_dict(syn.transformer_shapes(V, d=D, ff=ff, layers=2), seed, mode="torch_default"), strict=False)
    m.flatten_parameters()
    return m


def greedy(out, name, m, mem, B):
    """STEPS positions from one call, then one position's logits."""
    st = m.decoder.init_decode(mem)
    tok = torch.full((B, 1), m.w2i["<sos>"], dtype=torch.int64, device=DEV)
    toks, top1 = m.decoder.decode_tokens(tok, st, STEPS)
    logits = st.step_logits(toks[-1].view(B, 1)).clone()
    out[f"{name}/tokens"], out[f"{name}/top1"], out[f"{name}/logits"] = toks.cpu(), top1.cpu(), logits.cpu()


def staggered(states, mems_of):
    """Three slots of every state brought to positions (0, 5, 11): all admitted, then slot 1 and slot 0 handed on.  Yields
    (positions to run next, the slot that was just handed on)."""
    for st, mems in zip(states, mems_of):
        for slot in range(3):
            st.admit(slot, mems[slot])
    yield 6, None
    for handed_on, n in ((1, 5), (0, 4)):
        for st, mems in zip(states, mems_of):
            st.admit(handed_on, mems[handed_on])
        yield n, handed_on


def dump(path):
    from omr_a2s_multimodal_transformer_amd._lib import LIB_PATH, cur_stream, lib, ptr
    from omr_a2s_multimodal_transformer_amd.decoder import WeightedBeamState
    out = {}
    with torch.no_grad():
        for dtype in ("fp32", "bf16"):
            for window in (-1, 4):
                m = model(11, dtype, window)
                for B in (1, 3):
                    greedy(out, f"lockstep/{dtype}/w{window}/B{B}", m, rnd((B, 100, D), 20 + B), B)
        m = model(12, "bf16")
        sos, eos = m.w2i["<sos>"], m.w2i["<eos>"]
        mems = [rnd((n, D), 30 + n) for n in (70, 300, 700)]
        greedy(out, "ragged", m, mems, 3)
        greedy(out, "fp8", model(12, "bf16", fp8=True), rnd((3, 100, D), 41), 3)
        greedy(out, "generic_width", model(13, "fp32", ff=2304), rnd((2, 100, D), 42), 2)
        greedy(out, "generic_width_fp8", model(13, "fp32", ff=2304, fp8=True), rnd((2, 100, D), 42), 2)
        greedy(out, "generic_width_ragged", model(13, "bf16", ff=2304), mems, 3)

        # slots at positions (0, 5, 11)
        lowp = m.decoder.memory_list(mems)
        st = m.decoder.init_slot_decode(3, 700, DEV, sos)
        for i, (n, _) in enumerate(staggered([st], [lowp])):
            toks, top1 = st.run_rows(n)
            out[f"slots/{i}/tokens"], out[f"slots/{i}/top1"] = toks.cpu(), top1.cpu()

        # a weighted pair of models: lock-step over ragged states, then over slots
        ma, mb = model(14, "bf16"), model(15, "fp32", window=4)
        mems_b = [rnd((n, D), 50 + n) for n in (90, 260, 400)]
        sa, sb = ma.decoder.init_decode(mems), mb.decoder.init_decode(mems_b)
        tok = torch.full((3,), sos, dtype=torch.int64, device=DEV)
        toks = torch.empty((STEPS, 3), dtype=torch.int64, device=DEV)
        prob = torch.empty((STEPS, 3), dtype=torch.float32, device=DEV)
        lib().call("omr_weighted_decode_steps_varlen", ctypes.byref(sa.desc), ptr(sa.mem_len), ctypes.byref(sb.desc), ptr(sb.mem_len), 0.4, ptr(tok), 0,
                   STEPS, ptr(toks), ptr(prob), ptr(sa.logits), ptr(sb.logits), cur_stream())
        for n, t in (("tokens", toks), ("prob", prob), ("tok", tok), ("logits_a", sa.logits[:, :V]), ("logits_b", sb.logits[:, :V])):
            out[f"weighted/{n}"] = t.cpu().clone()
        sa, sb = ma.decoder.init_slot_decode(3, 700, DEV, sos), mb.decoder.init_slot_decode(3, 400, DEV, sos)
        tok.fill_(sos)
        for i, (n, handed_on) in enumerate(staggered([sa, sb], [ma.decoder.memory_list(mems), mb.decoder.memory_list(mems_b)])):
            if handed_on is not None:
                tok[handed_on:handed_on + 1].fill_(sos)
            t_max = sa.begin(n)
            sb.begin(n)
            toks = torch.empty((n, 3), dtype=torch.int64, device=DEV)
            prob = torch.empty((n, 3), dtype=torch.float32, device=DEV)
            lib().call("omr_weighted_decode_steps_rows", ctypes.byref(sa.desc), ptr(sa.mem_len), ctypes.byref(sb.desc), ptr(sb.mem_len), ptr(sa.pos),
                       t_max, 0.4, ptr(tok), n, ptr(toks), ptr(prob), ptr(sa.logits), ptr(sb.logits), cur_stream())
            sa.advance(n)
            sb.advance(n)
            out[f"weighted_rows/{i}/tokens"], out[f"weighted_rows/{i}/prob"] = toks.cpu(), prob.cpu()
        out["weighted_rows/logits_a"], out["weighted_rows/logits_b"] = sa.logits[:, :V].cpu().clone(), sb.logits[:, :V].cpu().clone()

        # beam 3 over two inputs, one model and the weighted pair
        bs = ma.decoder.init_beam_decode(mems[1:], 3, sos, eos)
        bs.run(STEPS)
        live = torch.tensor([not d for d in bs.done()]).repeat_interleave(3)       # a finished input's rows run on stale caches: not compared
        out["beam/last_logits"] = torch.where(live[:, None], bs.logits[:, :V].cpu(), torch.zeros(()))
        for k, v in bs.snapshot().items():
            out[f"beam/{k}"] = torch.from_numpy(v.copy())
        wb = WeightedBeamState(ma.decoder, mems[1:], mb.decoder, mems_b[1:], 3, sos, eos, alpha=0.4)
        wb.run(STEPS)
        for k, v in wb.search.snapshot().items():
            out[f"weighted_beam/{k}"] = torch.from_numpy(v.copy())
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
