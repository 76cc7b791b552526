"""Reference code for ragged multimodal training (MultimodalTransformer.forward with xli and xla [B, 2], csrc/extent.hip
omr_concat_memory_*): plain torch on the CPU.  Shared by tests/test_multimodal_ragged_refs_cpu.py (which pins it in fp64 against
oracle.ref_cpu.multimodal_forward of every pair alone) and the GPU tests of the kernel pair and of the model.

"Alone" = the pair at batch size 1 with xli = xla = None (validation_step's form): nothing is padded, so nothing is masked."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

import extent_refs as E
from oracle import ref_cpu as R

# the shapes of the issue: images are extent_refs.SIZES in its 64 x 96 plane (memories of 48 / 21 / 4 rows); the audio plane is 35 x 40
# (memories of 9 / 15 / 4 rows).  The longest image is not the longest audio: Smax = 57 is not 48 + 15.
IMG_PLANE, IMG_SIZES = E.PLANE, E.SIZES
AUD_PLANE = (35, 40)
AUD_SIZES = ((35, 24), (35, 40), (20, 9))
IMG_LENS, AUD_LENS = (48, 21, 4), (9, 15, 4)
V, T, D, LAYERS = 30, 12, 128, 2
TARGET_LENS = (11, 7, 4)
MIXERS = ("concat", "attn_img", "attn_audio", "attn_both")


def memory_lengths(sizes) -> List[int]:
    return [h * w for h, w in E.extent_levels([tuple(int(v) for v in s) for s in sizes])[-1]]


# ------------------------------------------------------------------------------------------------ the kernel pair

def concat_rows(a: torch.Tensor, la: Sequence[int], b: Optional[torch.Tensor], lb: Optional[Sequence[int]], smax: int, shift: int = 0) -> torch.Tensor:
    """a [B, La, C], b [B, Lb, C] (or None: lb is not used) -> [B, smax, C] by slicing: rows [0, la) of a, then rows [0, lb) of b, then
    zeros; rows the concatenation has beyond smax are dropped.  Lengths are clamped to the tensors.  Rows of a / b at or past their
    lengths are not touched (NaN there stays out).  shift: b starts at row la + shift (the CPU test breaks the offset on purpose)."""
    B, La, C = a.shape
    out = torch.zeros((B, smax, C), dtype=a.dtype)
    for i in range(B):
        n = min(max(int(la[i]), 0), La)
        out[i, :min(n, smax)] = a[i, :min(n, smax)]
        if b is not None:
            m = min(max(int(lb[i]), 0), b.shape[1])
            start = n + shift
            m = max(0, min(m, smax - start))
            out[i, start:start + m] = b[i, :m]
    return out


def concat_rows_adjoint(g: torch.Tensor, la: Sequence[int], La: int, lb: Optional[Sequence[int]], Lb: int) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """g [B, smax, C] -> (da [B, La, C], db [B, Lb, C] or None for Lb = 0): the transpose of concat_rows; rows of g at or past la + lb
    are not touched."""
    B, smax, C = g.shape
    da = torch.zeros((B, La, C), dtype=g.dtype)
    db = torch.zeros((B, Lb, C), dtype=g.dtype) if Lb else None
    for i in range(B):
        n = min(max(int(la[i]), 0), La)
        da[i, :min(n, smax)] = g[i, :min(n, smax)]
        if Lb:
            m = max(0, min(min(max(int(lb[i]), 0), Lb), smax - n))
            db[i, :m] = g[i, n:n + m]
    return da, db


def concat_row_map_brute(la: int, lb: int, smax: int) -> dict:
    """{output row: ("a" | "b", source row)} of one sample, row by row: the order of torch.cat([xi, xa], dim=1) of the sample alone."""
    rows, r = {}, 0
    for which, n in (("a", la), ("b", lb)):
        for k in range(n):
            if r < smax:
                rows[r] = (which, k)
            r += 1
    return rows


# ------------------------------------------------------------------------------------------------ the model (fp64 on the CPU)

def packed_memory(sd, prefix: str, x: torch.Tensor, sizes, plane: Tuple[int, int], d_model: int) -> Tuple[torch.Tensor, List[int]]:
    """extent_refs.masked_encoder -> + 2-D PE on the padded grid -> extent_refs.pack_rows: ([B, Smax, d], [S_b])."""
    pe = R.pe2d_table(d_model, math.ceil(plane[0] / R.HEIGHT_REDUCTION), math.ceil(plane[1] / R.WIDTH_REDUCTION))
    f = E.masked_encoder(sd, prefix, x, sizes)
    f = (f + pe[:, :, :f.shape[2], :f.shape[3]].to(f.dtype)).permute(0, 2, 3, 1)
    grid = E.extent_levels([tuple(int(v) for v in s) for s in sizes])[-1]
    lens = [h * w for h, w in grid]
    return E.pack_rows(f, grid, max(lens)), lens


def _attend(sd, query: torch.Tensor, lq: List[int], kv: torch.Tensor, lkv: List[int], nhead: int, key_mask: str) -> torch.Tensor:
    """The shared cross_attn module.  key_mask "exact": -inf on the keys at and past each sample's own key length; "none": no mask;
    "block": the reference's quirk-2 block mask (oracle.ref_cpu.cross_attention with both lengths)."""
    if key_mask == "block":
        return R.cross_attention(sd, "cross_attn.", query, torch.tensor(lq), kv, torch.tensor(lkv), nhead)
    bias = None
    if key_mask == "exact":
        bias = torch.zeros((kv.shape[0], 1, 1, kv.shape[1]), dtype=query.dtype)
        bias.masked_fill_(R._len_mask(kv.shape[1], torch.tensor(lkv)).view(kv.shape[0], 1, 1, -1), float("-inf"))
    else:
        assert key_mask == "none", key_mask
    a = "cross_attn.attention."
    return R.mha(query, kv, sd[a + "in_proj_weight"], sd[a + "in_proj_bias"], sd[a + "out_proj.weight"], sd[a + "out_proj.bias"], nhead, bias)


def mix_packed(sd, kind: str, mi: torch.Tensor, li: List[int], ma: torch.Tensor, la: List[int], nhead: int, key_mask: str = "exact",
               concat_shift: int = 0) -> Tuple[torch.Tensor, List[int]]:
    """The four mixers over packed memories -> (memory [B, Smax, d] zero at and past each sample's length, the lengths)."""
    both = [a + b for a, b in zip(li, la)]
    if kind == "concat":
        return concat_rows(mi, li, ma, la, max(both), concat_shift), both
    if kind == "attn_img":          # q = audio, kv = image
        x = _attend(sd, ma, la, mi, li, nhead, key_mask)
        return concat_rows(x, la, None, None, x.shape[1]), la
    if kind == "attn_audio":        # q = image, kv = audio
        x = _attend(sd, mi, li, ma, la, nhead, key_mask)
        return concat_rows(x, li, None, None, x.shape[1]), li
    if kind == "attn_both":         # the second attention's keys are the ATTENDED audio (quirk 3), masked by the audio lengths
        xa2 = _attend(sd, ma, la, mi, li, nhead, key_mask)
        xi2 = _attend(sd, mi, li, xa2, la, nhead, key_mask)
        return concat_rows(xi2, li, xa2, la, max(both), concat_shift), both
    raise ValueError(kind)


def ragged_multimodal_ref(sd, xi: torch.Tensor, sizes_i, xa: torch.Tensor, sizes_a, y_in: torch.Tensor, cfg: "R.OracleCfg", mixer_type: str,
                          img_plane: Tuple[int, int], aud_plane: Tuple[int, int], modality: str = "both", key_mask: str = "exact",
                          concat_shift: int = 0) -> torch.Tensor:
    """The ragged route written out: masked encoder per modality -> PE -> pack_rows -> mixer with exact key masks -> the oracle
    decoder with the bool mask over the mixed lengths.  -> logits [B, V, T].  key_mask / concat_shift: the negative controls."""
    mi, li = packed_memory(sd, "image_encoder.", xi, sizes_i, img_plane, cfg.d_model)
    ma, la = packed_memory(sd, "audio_encoder.", xa, sizes_a, aud_plane, cfg.d_model)
    if modality == "image":
        mem, lens = mi, li
    elif modality == "audio":
        mem, lens = ma, la
    else:
        mem, lens = mix_packed(sd, mixer_type, mi, li, ma, la, cfg.nhead, key_mask, concat_shift)
    return R.decoder(sd, "decoder.", y_in, mem, R._len_mask(mem.shape[1], torch.tensor(lens)), cfg)


# ------------------------------------------------------------------------------------------------ the batch of the issue

def rnd(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=dtype)


def make_targets(w2i, target_lens=TARGET_LENS, vocab: int = V, t: int = T):
    """(y_in, y_out [B, T] 0-padded, tokens counted by the loss per sample)."""
    sos, eos = w2i["<sos>"], w2i["<eos>"]
    B = len(target_lens)
    y_in = torch.zeros((B, t), dtype=torch.int64)
    y_out = torch.zeros((B, t), dtype=torch.int64)
    g = torch.Generator().manual_seed(77)
    for b, n in enumerate(target_lens):
        toks = torch.randint(1, vocab, (n,), generator=g)
        toks[(toks == sos) | (toks == eos)] = 1
        y = torch.cat([torch.tensor([sos]), toks, torch.tensor([eos])])
        y_in[b, :n + 1], y_out[b, :n + 1] = y[:-1], y[1:]
    return y_in, y_out, [n + 1 for n in target_lens]


def make_pairs(img_sizes=IMG_SIZES, aud_sizes=AUD_SIZES, dtype=torch.float32, pad: float = 0.0):
    """(image crops [1, 1, h, w], audio crops, xi [B, 1, H, W] padded with `pad`, sizes_i int64 [B, 2], xa, sizes_a)."""
    ci = [rnd((1, 1, h, w), 500 + b, dtype) for b, (h, w) in enumerate(img_sizes)]
    ca = [rnd((1, 1, h, w), 600 + b, dtype) for b, (h, w) in enumerate(aud_sizes)]

    def collate(crops):
        H, W = max(c.shape[2] for c in crops), max(c.shape[3] for c in crops)
        x = torch.full((len(crops), 1, H, W), pad, dtype=dtype)
        for b, c in enumerate(crops):
            x[b, :, :c.shape[2], :c.shape[3]] = c[0]
        return x, torch.tensor([[c.shape[2], c.shape[3]] for c in crops], dtype=torch.int64)

    xi, si = collate(ci)
    xa, sa = collate(ca)
    return ci, ca, xi, si, xa, sa
