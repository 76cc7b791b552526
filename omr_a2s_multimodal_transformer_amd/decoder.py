"""Transformer decoder on HIP kernels -- same class names, constructor signature, attribute and state-dict
names as the reference's src/transformer/decoder.py (which wraps nn.TransformerDecoder, post-norm, ReLU).
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from . import functional as Fn
from . import kernels as K
from ._lib import cur_stream, dtype_code, lib, ptr, require_cuda
from .runtime import next_seed


def sinusoid_1d(max_len: int, emb_dim: int) -> torch.Tensor:
    """decoder.py:21-27 -> [1, max_len, emb_dim]."""
    pos = torch.arange(max_len).unsqueeze(1)
    den = torch.pow(10000, torch.arange(0, emb_dim, 2) / emb_dim)
    pe = torch.zeros(1, max_len, emb_dim)
    pe[0, :, 0::2] = torch.sin(pos / den)
    pe[0, :, 1::2] = torch.cos(pos / den)
    return pe


def _to_dev(t: torch.Tensor, device) -> torch.Tensor:
    """Host -> device without blocking the host (pinned staging + non-blocking copy); device tensors pass through.  A blocking
    copy would wait for the whole previous step (it drains the stream) and stop the host from issuing the next step's
    launches while the GPU is still busy."""
    if t.device == device:
        return t
    if not t.is_cuda and not t.is_pinned() and torch.cuda.is_available():
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


def _dropout(x: torch.Tensor, p: float, training: bool) -> torch.Tensor:
    if not training or p <= 0.0:
        return x
    return Fn.DropoutFn.apply(x, p, next_seed("rows", p), False, False)


class PositionalEncoding1D(nn.Module):
    """decoder.py:7-32."""

    def __init__(self, max_len: int, emb_dim: int, dropout_p: float = 0.1):
        super().__init__()
        self.dropout_p = dropout_p
        self.register_buffer("pe", sinusoid_1d(max_len, emb_dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, T, d = x.shape
        y = K.add_pe2d(x.contiguous().view(B, 1, T, d), self.pe[0].view(1, -1, d)).view(B, T, d)
        return _dropout(y, self.dropout_p, self.training)


class Embedding(nn.Module):
    """nn.Embedding parameter holder: N(0,1) init with the padding row zeroed (decoder.py:73-77)."""

    def __init__(self, num_embeddings: int, embedding_dim: int, padding_idx: Optional[int] = None):
        super().__init__()
        self.num_embeddings, self.embedding_dim, self.padding_idx = num_embeddings, embedding_dim, padding_idx
        w = torch.randn(num_embeddings, embedding_dim)
        if padding_idx is not None:
            w[padding_idx].zero_()
        self.weight = nn.Parameter(w)


class Linear(nn.Module):
    def __init__(self, in_features: int, out_features: int):
        super().__init__()
        bound = 1.0 / math.sqrt(in_features)
        self.weight = nn.Parameter(torch.empty(out_features, in_features).uniform_(-bound, bound))
        self.bias = nn.Parameter(torch.empty(out_features).uniform_(-bound, bound))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return Fn.linear(x, self.weight, self.bias)


class LayerNorm(nn.Module):
    def __init__(self, d: int, eps: float = 1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(d))
        self.bias = nn.Parameter(torch.zeros(d))


class MultiheadAttention(nn.Module):
    """nn.MultiheadAttention parameter layout (packed in_proj rows [Wq; Wk; Wv], out_proj) and default init
    (Xavier-uniform in_proj_weight, zero in_proj_bias / out_proj.bias)."""

    def __init__(self, embed_dim: int, num_heads: int, dropout: float = 0.0):
        super().__init__()
        self.embed_dim, self.num_heads, self.dropout = embed_dim, num_heads, dropout
        bound = math.sqrt(6.0 / (4 * embed_dim))
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim).uniform_(-bound, bound))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = Linear(embed_dim, embed_dim)
        with torch.no_grad():
            self.out_proj.bias.zero_()

    def self_attention(self, x, causal: bool, window: int, key_bias, training: bool):
        qkv = Fn.linear(x, self.in_proj_weight, self.in_proj_bias)
        p = self.dropout if training else 0.0
        o = Fn.AttentionFn.apply(qkv, None, self.num_heads, causal, window, key_bias, None, None, p, next_seed("attn", p) if p > 0 else 0)
        return Fn.linear(o, self.out_proj.weight, self.out_proj.bias)

    def project_kv(self, memory):
        d = self.embed_dim
        return Fn.linear(memory, self.in_proj_weight, self.in_proj_bias, rows=(d, 3 * d))

    def cross_attention(self, x, kv, key_bias, training: bool, blk_lq=None, blk_lkv=None, weights=None):
        """weights (None, or a dict of kernels.attn_weights keywords: out / out_scale / accumulate): also write the head-averaged
        attention map of this call -- post-dropout in training, from the words the forward read -- and leave it in weights["out"].
        The attention itself is launched exactly as without it."""
        d = self.embed_dim
        q = Fn.linear(x, self.in_proj_weight, self.in_proj_bias, rows=(0, d))
        p = self.dropout if training else 0.0
        seed = next_seed("attn", p) if p > 0 else 0
        if weights is None:
            o = Fn.AttentionFn.apply(q, kv, self.num_heads, False, -1, key_bias, blk_lq, blk_lkv, p, seed)
        else:
            tap = []
            o = Fn.AttentionFn.apply(q, kv, self.num_heads, False, -1, key_bias, blk_lq, blk_lkv, p, seed, tap)
            qt, kt, lse, words = tap[0]
            weights["out"] = K.attn_weights(qt.detach(), kt.detach(), lse, self.num_heads, key_bias=key_bias, blk_lq=blk_lq, blk_lkv=blk_lkv,
                                            dropout_p=p, drop_words=words, out=weights.get("out"), out_scale=weights.get("out_scale"),
                                            accumulate=bool(weights.get("accumulate", False)))
        return Fn.linear(o, self.out_proj.weight, self.out_proj.bias)


class TransformerDecoderLayer(nn.Module):
    """Post-norm nn.TransformerDecoderLayer(relu, batch_first) math, torch nn/modules/transformer.py:1129-1199."""

    def __init__(self, d_model: int, nhead: int, dim_feedforward: int, dropout: float):
        super().__init__()
        self.self_attn = MultiheadAttention(d_model, nhead, dropout)
        self.multihead_attn = MultiheadAttention(d_model, nhead, dropout)
        self.linear1 = Linear(d_model, dim_feedforward)
        self.linear2 = Linear(dim_feedforward, d_model)
        self.norm1, self.norm2, self.norm3 = LayerNorm(d_model), LayerNorm(d_model), LayerNorm(d_model)
        self.dropout_p = dropout

    fused_node = True       # one autograd node per layer (functional.DecoderLayerFn) instead of one per operation: same kernels, same bits

    def forward(self, x, memory, window: int, self_key_bias, mem_key_bias, kv=None, per_op: bool = False, weights=None):
        """kv: this layer's cross-attention K|V of `memory` when the decoder projected all layers at once.  per_op: take the
        per-operation path whatever `fused_node` says; weights: see MultiheadAttention.cross_attention (per-operation path only)."""
        tr, p = self.training, self.dropout_p
        assert weights is None or per_op
        if self.fused_node and kv is not None and x.is_contiguous() and not per_op:
            pp = p if tr else 0.0
            # the seeds of the layer's six dropout sites, drawn in the order the per-operation path draws them
            seeds = tuple(next_seed(kind, pp) for kind in ("attn", "rows", "attn", "rows", "rows", "rows")) if pp > 0.0 else (0,) * 6
            return Fn.DecoderLayerFn.apply(x, kv, self, window, self_key_bias, mem_key_bias, pp, seeds)
        drop = (lambda: (p, next_seed("rows", p))) if (tr and p > 0.0) else (lambda: None)      # dropout1/2/3 ride inside the add+LayerNorm kernels
        sa = self.self_attn.self_attention(x, True, window, self_key_bias, tr)
        x = Fn.AddLayerNormFn.apply(sa, x, self.norm1.weight, self.norm1.bias, drop())
        if kv is None:
            kv = self.multihead_attn.project_kv(memory)
        ca = self.multihead_attn.cross_attention(x, kv, mem_key_bias, tr, weights=weights)
        x = Fn.AddLayerNormFn.apply(ca, x, self.norm2.weight, self.norm2.bias, drop())
        h = Fn.linear(x, self.linear1.weight, self.linear1.bias, relu=True, mask_own=True, drop=drop())     # FFN dropout in the GEMM epilogue
        ff = Fn.linear(h, self.linear2.weight, self.linear2.bias)
        return Fn.AddLayerNormFn.apply(ff, x, self.norm3.weight, self.norm3.bias, drop())


class TransformerDecoder(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward, dropout, num_layers):
        super().__init__()
        # nn.TransformerDecoder deep-copies ONE layer, so all layers start identical
        first = TransformerDecoderLayer(d_model, nhead, dim_feedforward, dropout)
        layers = [first]
        for _ in range(num_layers - 1):
            l = TransformerDecoderLayer(d_model, nhead, dim_feedforward, dropout)
            l.load_state_dict(first.state_dict())
            layers.append(l)
        self.layers = nn.ModuleList(layers)


class Conv1d(nn.Module):
    """nn.Conv1d(k=1) parameter holder: weight [out, in, 1] (decoder.py:98-102)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        bound = 1.0 / math.sqrt(in_channels)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 1).uniform_(-bound, bound))
        self.bias = nn.Parameter(torch.empty(out_channels).uniform_(-bound, bound))


class Decoder(nn.Module):
    """decoder.py:35-148.  forward(tgt [B,T] int64, memory [B,S,d], memory_len) -> logits [B, V, T]
    (a stride permutation of the row-major [B*T, V] buffer the head GEMM writes)."""

    def __init__(self, output_size: int, max_seq_len: int, num_embeddings: int, embedding_dim: int = 256, padding_idx: int = 0,
                 ff_dim: int = 256, dropout_p: float = 0.1, nhead: int = 4, num_transformer_layers: int = 8, attn_window: int = -1):
        super().__init__()
        if (embedding_dim // nhead) not in (32, 64) or embedding_dim % nhead:
            raise NotImplementedError("HIP attention kernels cover head_dim 32 and 64 (reference: 256/4 = 64)")
        self.embedding = Embedding(num_embeddings, embedding_dim, padding_idx)
        self.pos_1d = PositionalEncoding1D(max_seq_len, embedding_dim, dropout_p)
        self.attn_window = attn_window
        self.transformer_decoder = TransformerDecoder(embedding_dim, nhead, ff_dim, dropout_p, num_transformer_layers)
        self.out_layer = Conv1d(embedding_dim, output_size)
        self.padding_idx = padding_idx
        self.output_size = output_size

    # ---- mask builders (host logic; vectorised restatement of decoder.py:150-254) ---------------------------
    def get_memory_key_padding_mask(self, memory: torch.Tensor, memory_len: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """None -> None; bool [B,S] -> cloned bool mask (-inf semantics); integer lengths -> FLOAT32 0/1 mask
        that is ADDED to the scores (+1.0 on padded keys: reference quirk 1, decoder.py:186-188)."""
        if memory_len is None:
            return None
        if memory_len.dtype == torch.bool:
            assert memory_len.shape[0] == memory.shape[0], f"Different batch sizes for memory and memory_len: {memory.shape[0]} != {memory_len.shape[0]}"
            assert memory_len.shape[1] == memory.shape[1], f"Different sequence lengths for memory and memory_len: {memory.shape[1]} != {memory_len.shape[1]}"
            return memory_len.clone()
        pos = torch.arange(memory.shape[1], device=memory.device).unsqueeze(0)
        return (pos >= memory_len.to(memory.device).long().unsqueeze(1)).to(torch.float32)

    @staticmethod
    def create_variable_window_mask(size: int, window_size: int, dtype=torch.float32, device=torch.device("cpu")) -> torch.Tensor:
        """decoder.py:191-217 (materialised form, for API parity; the kernels take `window` as a parameter)."""
        i = torch.arange(size, device=device).unsqueeze(1)
        j = torch.arange(size, device=device).unsqueeze(0)
        vis = j <= i
        if window_size < size:
            vis = vis & (j >= i - window_size)
        return torch.full((size, size), float("-inf"), dtype=dtype, device=device).masked_fill(vis, 0.0)

    def get_tgt_masks(self, tgt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        T = tgt.shape[1]
        if self.attn_window > 0:
            tgt_mask = self.create_variable_window_mask(T, self.attn_window, device=tgt.device)
        else:
            tgt_mask = self.create_variable_window_mask(T, T, device=tgt.device)
        return tgt_mask, (tgt == 0).to(torch.float32)

    @staticmethod
    def _as_key_bias(mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        if mask is None:
            return None
        if mask.dtype == torch.bool:
            return torch.zeros(mask.shape, dtype=torch.float32, device=mask.device).masked_fill(mask, float("-inf"))
        return mask.contiguous()

    def _cross_kv_pack(self, dt):
        """Row-group views over the packed cross-attention in_proj parameters of all layers, valid when the flat buffer holds
        them back to back (params._placement_order; checked here on every call, so any other layout just takes the per-layer path)."""
        layers = self.transformer_decoder.layers
        ws = [l.multihead_attn.in_proj_weight for l in layers]
        bs = [l.multihead_attn.in_proj_bias for l in layers]
        if len(layers) < 2 or getattr(ws[0], "omr_phys", None) is None:
            return None
        d = ws[0].shape[1]
        if (2 * d) % 128:
            return None
        L = len(layers)

        def block(tensors, rows):
            t0 = tensors[0]
            step = t0.numel() * t0.element_size()
            if any(t.data_ptr() != t0.data_ptr() + i * step or not t.is_contiguous() for i, t in enumerate(tensors)):
                return None
            return torch.as_strided(t0, (L * rows,) + tuple(t0.shape[1:]), t0.stride())

        w = block([Fn.wt(p, dt) for p in ws], 3 * d)
        gw = block([p.omr_grad for p in ws], 3 * d)
        b = block([p.omr_phys for p in bs], 3 * d)
        gb = block([p.omr_grad for p in bs], 3 * d)
        if w is None or gw is None or b is None or gb is None:
            return None
        return dict(L=L, d=d, w=w, gw=gw, b=b, gb=gb)

    def _compute_dtype(self) -> torch.dtype:
        """bf16 when the flat parameter buffer keeps a low-precision copy of the matrices, else fp32."""
        return torch.bfloat16 if getattr(self.embedding.weight, "omr_lowp", None) is not None else torch.float32

    def _in_compute_dtype(self, memory: torch.Tensor) -> torch.Tensor:
        dt = self._compute_dtype()
        return K.cast(memory.contiguous(), dt) if memory.dtype != dt else memory.contiguous()

    def memory_list(self, memories, refuse_long: bool = True) -> List[torch.Tensor]:
        """Memories [1, S_b, d] or [S_b, d] -> the list of [S_b, d] in the compute dtype, checked (check_ragged_memories)
        before anything is launched."""
        mems = [m[0] if m.dim() == 3 else m for m in memories]
        check_ragged_memories([m.shape for m in mems], self.embedding.weight.shape[1], refuse_long)
        return [self._in_compute_dtype(m) for m in mems]

    # ---- KV-cached greedy decoding (SURVEY.md section 8b `decode_step`, section 8f rank 1).  The reference re-runs the whole
    #      prefix every step (model.py:184-193, O(T^3)) and reads the argmax back per token.  Here the native executor
    #      omr_decode_steps (csrc/decode.hip) runs whole tokens from ONE host call each: it projects the new token, appends
    #      its self-attention K|V to the cache, reads the cross-attention K|V projected once, and chains the chosen token to
    #      the next position through device memory.  Same kernels, same per-row arithmetic order as the training forward.
    @torch.no_grad()
    def init_decode(self, memory) -> "DecodeState":
        """memory [B, S, d] -> the decode state of B same-sized inputs.  A LIST of memories ([1, S_b, d] or [S_b, d] each) gives
        one ragged state: padded to S = max S_b, row b's cross-attention sees its own S_b keys (omr_decode_steps_varlen)."""
        if isinstance(memory, (list, tuple)):
            return DecodeState(self, self.memory_list(memory), self._compute_dtype())
        return DecodeState(self, self._in_compute_dtype(memory), self._compute_dtype())

    def takes_slot_state(self, capacity: int = 0) -> bool:
        """Whether this decoder's widths take a decode state with slots (omr_decode_steps_rows: the row kernel of
        csrc/decode.hip) for memories of up to `capacity` tokens (0: the longest a ragged state takes); the library is asked, with a
        descriptor that carries the widths only."""
        layer = self.transformer_decoder.layers[0]
        ds = _DecodeDesc()
        ds.dtype, ds.d, ds.nhead, ds.ff = dtype_code(self._compute_dtype()), self.embedding.weight.shape[1], layer.self_attn.num_heads, layer.linear1.weight.shape[0]
        ds.fp8, ds.max_len, ds.S = int(bool(getattr(self, "fp8_weights", False))), self.pos_1d.pe.shape[1], capacity or MAX_RAGGED_MEMORY
        return lib().query("omr_decode_steps_rows", ctypes.byref(ds), None, None, 0, None, 0, None, None, None, None) != -3

    @torch.no_grad()
    def init_slot_decode(self, rows: int, capacity: int, device, sos: int = 2) -> "SlotDecodeState":
        """A decode state of `rows` slots for memories of up to `capacity` tokens each (continuous batching)."""
        if not self.takes_slot_state(capacity):
            raise RuntimeError("init_slot_decode: this decoder's widths do not take omr_decode_steps_rows")
        return SlotDecodeState(self, rows, capacity, self._compute_dtype(), device, sos)

    def width_text(self) -> str:
        """The widths `takes_slot_state` goes by, for error messages."""
        layer = self.transformer_decoder.layers[0]
        return f"d = {self.embedding.weight.shape[1]}, ff = {layer.linear1.weight.shape[0]}, {layer.self_attn.num_heads} heads"

    @torch.no_grad()
    def init_spec_decode(self, draft: "Decoder", memory, draft_memory, k: int = 4, sos: int = 2, eos: int = 1,
                         max_out: Optional[int] = None) -> "SpecDecodeState":
        """The state of a speculative greedy decode (omr_spec_decode_cycles; an extension of the reference's greedy loop): this
        decoder is the target, `draft` a cheaper decoder with the same vocabulary that proposes k tokens per cycle.  memory /
        draft_memory: lists of [S_b, d] / [1, S_b, d] memories, one pair per input, each model's own encoding of it; the limits
        of a ragged state apply to both (check_ragged_memories).  max_out: tokens per input at most (default: the shorter
        positional table).  Caches of both models, the grouped workspace and the output runs are allocated here."""
        as_list = lambda m: list(m) if isinstance(m, (list, tuple)) else [m]         # noqa: E731
        return SpecDecodeState(self, as_list(memory), draft, as_list(draft_memory), k, sos, eos, max_out)

    @torch.no_grad()
    def init_beam_decode(self, memory, beam: int, sos: int = 2, eos: int = 1) -> "BeamDecodeState":
        """The state of a beam search over N inputs at once, `beam` hypotheses each (omr_beam_decode_steps).  memory: [1, S, d],
        or a list of memories [S_b, d] / [1, S_b, d] of different lengths; each is projected by the GEMM a batch-size-1 state
        of it runs, and its hypotheses share that K|V.  sos / eos: the token ids (defaults: the id layout of the reference's
        vocabularies with 3 special tokens, synthetic.make_vocab).  The limits of a ragged state apply (check_ragged_memories)."""
        if not 1 <= beam <= MAX_BEAM:
            raise ValueError(f"beam must be in 1..{MAX_BEAM}, got {beam}")
        if beam > self.output_size or not (0 <= sos < self.output_size and 0 <= eos < self.output_size):
            raise ValueError(f"beam decode: beam {beam}, sos {sos}, eos {eos} do not fit a vocabulary of {self.output_size}")
        mems = self.memory_list(memory if isinstance(memory, (list, tuple)) else [memory])
        return BeamDecodeState(self, mems, self._compute_dtype(), beam, sos, eos)

    @torch.no_grad()
    def decode_step(self, token: torch.Tensor, st: "DecodeState") -> torch.Tensor:
        """token int64 [B,1] -> fp32 logits of the next position ([V] for B = 1, else [B,V]); advances the cache.  Every
        sample of the batch is at the same position t; rows are computed independently (same per-row arithmetic as bs = 1)."""
        logits = st.step_logits(token)
        return logits[0] if logits.shape[0] == 1 else logits

    @torch.no_grad()
    def decode_tokens(self, token: torch.Tensor, st: "DecodeState", n_steps: int):
        """Greedy-decode n_steps positions starting from `token` (int64 [B,1]) without a host round trip in between:
        -> (tokens int64 [n_steps, B], their fp32 top-1 logits [n_steps, B]), both on the device (model.py:187,253)."""
        return st.run(token, n_steps)

    def forward(self, tgt: torch.Tensor, memory: torch.Tensor, memory_len: Optional[torch.Tensor]) -> torch.Tensor:
        return self._run(tgt, memory, memory_len)

    @torch.no_grad()
    def cross_attention_maps(self, tgt: torch.Tensor, memory: torch.Tensor, memory_len: Optional[torch.Tensor],
                             layers=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """`forward` in eval mode plus where it looked: -> (logits [B, V, T], maps fp32 [B, T, S]).  maps[b, t] is the cross-attention
        distribution over the S memory rows of the position that predicts token t, averaged over the heads (what
        nn.MultiheadAttention returns with need_weights=True) and over the decoder layers `layers` (an iterable of layer indices;
        default: all).  The layers run on the per-operation path -- the kernels of the fused node, so the logits are `forward`'s bit
        for bit -- and each selected layer adds its map into one buffer (omr_attn_weights, out_scale 1 / (H * len(layers))).  Keys a
        memory mask hides get exactly 0.  Training mode raises: the decoder's dropout draws are not replayed."""
        return self._cross_attention_maps(tgt, memory, memory_len, layers, True)

    def _cross_attention_maps(self, tgt, memory, memory_len, layers, tgt_padding_bias: bool):
        """cross_attention_maps; tgt_padding_bias=False (model._align only) leaves out the +1.0 `forward` adds on target keys equal
        to 0 when there is a memory mask (reference quirk 1), as in a decode without a memory mask: a row of a padded batch then
        equals its batch-size-1 pass also when its words contain token 0.  The logits are then not `forward`'s."""
        if self.training:
            raise ValueError("cross_attention_maps runs in eval mode: the decoder's dropout draws are not replayed")
        L = len(self.transformer_decoder.layers)
        sel = sorted(set(range(L) if layers is None else (int(i) for i in layers)))
        if not sel or sel[0] < 0 or sel[-1] >= L:
            raise ValueError(f"layers must name at least one of the decoder's {L} layers, got {layers}")
        H = self.transformer_decoder.layers[0].multihead_attn.num_heads
        maps = dict(layers=sel, out=None, out_scale=1.0 / (H * len(sel)), accumulate=False)
        logits = self._run(tgt, memory, memory_len, maps=maps, tgt_padding_bias=tgt_padding_bias)
        return logits, maps["out"]

    def _run(self, tgt: torch.Tensor, memory: torch.Tensor, memory_len: Optional[torch.Tensor], maps=None, tgt_padding_bias: bool = True) -> torch.Tensor:
        emb_w, dt = self.embedding.weight, self._compute_dtype()
        memory = self._in_compute_dtype(memory)
        B, T = tgt.shape
        # Host copies of the token ids / integer lengths (the Trainer keeps integer tensors on the host) tell, without a device
        # round trip, when a mask is all zeros: adding 0.0 to every score is the identity, so such a mask is not built and the
        # attention kernels take their bias-free path.  Device-resident inputs keep the general path.
        mem_full = memory_len is not None and not memory_len.is_cuda and memory_len.dtype != torch.bool and bool((memory_len >= memory.shape[1]).all())
        tgt_no_pad = not tgt.is_cuda and not bool((tgt == 0).any())
        tgt = _to_dev(tgt, memory.device)
        x = Fn.EmbedPEFn.apply(tgt.contiguous(), emb_w, self.pos_1d.pe[0], self.padding_idx, dt)
        x = _dropout(x, self.pos_1d.dropout_p, self.training)
        mem_mask = None if mem_full else self.get_memory_key_padding_mask(memory, None if memory_len is None else _to_dev(memory_len, memory.device))
        mem_bias = self._as_key_bias(mem_mask)
        # tgt_key_padding_mask = (tgt == 0).float() is ADDED (+1.0); dropped when there is no memory mask (decoder.py:131-132)
        self_bias = None if (memory_len is None or tgt_no_pad or not tgt_padding_bias) else (tgt == 0).to(torch.float32).contiguous()
        window = self.attn_window if self.attn_window > 0 else -1
        layers = self.transformer_decoder.layers
        pack = self._cross_kv_pack(dt)
        kvs = [None] * len(layers)
        if pack is not None:
            sink = Fn.KVGradSink()
            kvs = Fn.FusedCrossKVFn.apply(memory, pack, sink, layers[0].multihead_attn.in_proj_weight)
            for li, kv in enumerate(kvs):
                kv.omr_grad_sink = (sink, li)
        for li, (layer, kv) in enumerate(zip(layers, kvs)):
            if maps is None:
                x = layer(x, memory, window, self_bias, mem_bias, kv)
                continue
            weights = None
            if li in maps["layers"]:
                weights = dict(out=maps["out"], out_scale=maps["out_scale"], accumulate=maps["out"] is not None)
            x = layer(x, memory, window, self_bias, mem_bias, kv, per_op=True, weights=weights)
            if weights is not None:
                maps["out"] = weights["out"]
        V = self.output_size
        logits = Fn.linear(x, self.out_layer.weight, self.out_layer.bias, out_ld=K.round_up(V, 8))  # [B,T,V], row pitch round_up(V,8)
        return logits.permute(0, 2, 1)  # [B, V, T] (decoder.py:145-146)


# A ragged decode state (memories of different lengths in one batch) keeps every row bit-equal to its batch-size-1 decode
# only in the key-split cross-attention kernel with 256-key splits: at most 64 splits (decode.hip MAXSPLIT), and more than
# 64 keys per row (a shorter memory alone takes the query-per-wave kernel).  Python routes the short rows to batch size 1.
MAX_RAGGED_MEMORY = 64 * 256
MIN_RAGGED_MEMORY = 64
MAX_BEAM = 8                 # OMR_MAX_BEAM: beam * beam candidates of an input are one wavefront of the selection kernel


def takes_ragged_state(length: int) -> bool:
    """Whether a memory of `length` tokens may be a row of a ragged decode state; any other is decoded alone, at batch size 1.
    THE routing rule of evaluation.plan_pair_groups, _Base.greedy_batch and _Base.beam_search_batch."""
    return MIN_RAGGED_MEMORY < length <= MAX_RAGGED_MEMORY


def check_ragged_memories(shapes, d: int, refuse_long: bool = True) -> None:
    """Refuse, before anything is launched, memories a ragged decode state cannot take.  refuse_long = False lets a memory of
    more than MAX_RAGGED_MEMORY rows pass: the caller decodes it alone (_Base.beam_search_batch)."""
    if not shapes:
        raise ValueError("ragged decode: no memories given")
    for i, shp in enumerate(shapes):
        if len(shp) != 2 or shp[1] != d:
            raise ValueError(f"ragged decode: memory {i} has shape {tuple(shp)}, expected [S, {d}] or [1, S, {d}]")
        if shp[0] < 1:
            raise ValueError(f"ragged decode: memory {i} is empty (0 rows)")
        if refuse_long and shp[0] > MAX_RAGGED_MEMORY:
            raise ValueError(f"ragged decode: memory {i} has {shp[0]} rows, more than the {MAX_RAGGED_MEMORY} a ragged batch takes "
                             "(64 key splits of 256); decode it alone")


class _DecodeDesc(ctypes.Structure):
    """omr_decode_desc of include/omr_hip.h."""
    _fields_ = [(n, ctypes.c_int) for n in ("dtype", "B", "L", "d", "nhead", "ff", "V", "ldv", "max_len", "S", "window", "fp8")] + [
        ("emb", ctypes.c_void_p), ("pe", ctypes.c_void_p), ("layer_w", ctypes.c_void_p), ("head_w", ctypes.c_void_p), ("head_b", ctypes.c_void_p),
        ("self_kv", ctypes.c_void_p), ("cross_kv", ctypes.c_void_p), ("cross_ld", ctypes.c_long), ("cross_bs", ctypes.c_long),
        ("ws", ctypes.c_void_p), ("ws_bytes", ctypes.c_long),
        ("layer_w8", ctypes.c_void_p), ("layer_s8", ctypes.c_void_p), ("head_w8", ctypes.c_void_p), ("head_s8", ctypes.c_void_p)]


class DecodeState:
    """Device state of one KV-cached decode: the cross-attention K|V of every layer projected ONCE into one [memories, S, L*2d]
    buffer, the self-attention K|V cache [L, B, max_len, 2d], the position t, and the descriptor omr_decode_steps reads.
    Rows are independent: B same-sized inputs decode in lock-step (batched greedy), or B hypotheses share one memory (beam).
    rows_per_memory > 1 (BeamDecodeState): B = memories * rows_per_memory rows, those of a memory reading its one K|V slot."""

    gstate = None          # grammar.GrammarState: the automaton the picks of this state are constrained by (None: unconstrained)

    LAYER_PARAMS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                    "norm1.weight", "norm1.bias", "multihead_attn.in_proj_weight", "multihead_attn.in_proj_bias",
                    "multihead_attn.out_proj.weight", "multihead_attn.out_proj.bias", "norm2.weight", "norm2.bias",
                    "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm3.weight", "norm3.bias")
    FP8_PARAMS = ("self_attn.in_proj_weight", "self_attn.out_proj.weight", "multihead_attn.in_proj_weight",
                  "multihead_attn.out_proj.weight", "linear1.weight", "linear2.weight")          # OMR_DECODE_LAYER_FP8 order

    def __init__(self, dec: "Decoder", memory, dt: torch.dtype, rows_per_memory: int = 1):
        layers = dec.transformer_decoder.layers
        self.dec, self.dtype, self.t = dec, dt, 0
        self.L, self.d = len(layers), dec.embedding.weight.shape[1]
        ragged = isinstance(memory, list)              # [S_b, d] memories of different lengths (Decoder.init_decode)
        mems = memory if ragged else [memory.reshape(-1, self.d)]
        n_mem = len(memory) if ragged else memory.shape[0]
        self.B = n_mem * rows_per_memory
        self.S = max(m.shape[0] for m in memory) if ragged else memory.shape[1]
        self.max_len = dec.pos_1d.pe.shape[1]
        self.V, self.ldv = dec.output_size, K.round_up(dec.output_size, 8)
        L, d, dev = self.L, self.d, mems[0].device
        # cross-attention K|V rows [d, 3d) of every layer's packed in_proj over the memory: one GEMM where the flat buffer
        # holds the layers back to back (Decoder._cross_kv_pack), else one GEMM per layer into its column block.  Ragged: one
        # GEMM per memory into the first S_b rows of its slot -- the very GEMM a batch-size-1 state of that memory runs
        self.cross_kv = torch.empty((n_mem, self.S, L * 2 * d), dtype=dt, device=dev)
        for b, mem2 in enumerate(mems):
            self._project(mem2, self.cross_kv[b, :mem2.shape[0]] if ragged else self.cross_kv.view(-1, L * 2 * d))
        self.cross_bs = self.S * L * 2 * d
        # memory b's length (device int32), or None: every row sees all S rows
        self.mem_len = torch.tensor([m.shape[0] for m in mems], dtype=torch.int32).to(dev) if ragged else None
        self.self_kv = torch.empty((L, self.B, self.max_len, 2 * d), dtype=dt, device=dev)
        self._weights()
        self.desc = _DecodeDesc()
        self._bind()

    def _project(self, mem2: torch.Tensor, kv2: torch.Tensor) -> None:
        """The cross-attention K|V of every layer of memory rows mem2 [n, d] into kv2 [n, L*2d]."""
        dec, dt, L, d = self.dec, self.dtype, self.L, self.d
        pack = dec._cross_kv_pack(dt)
        if pack is not None:
            K.gemm_row_groups(mem2, pack["w"], kv2, mem2.shape[0], L * 2 * d, d, bias=pack["b"], group=(2 * d, 3 * d, d, 1))
        else:
            for li, layer in enumerate(dec.transformer_decoder.layers):
                mha = layer.multihead_attn
                w = Fn.wt(mha.in_proj_weight, dt)
                K.gemm(mem2, w[d:], bias=mha.in_proj_bias.omr_phys[d:], out=kv2[:, li * 2 * d:(li + 1) * 2 * d])

    def _weights(self) -> None:
        """The host arrays of device pointers the descriptor carries (and the fp8 copies of the matrices)."""
        dec, dt = self.dec, self.dtype
        layers = dec.transformer_decoder.layers

        def pointer(p):            # matrices in the compute dtype, vectors (biases, LayerNorm) fp32
            return (Fn.wt(p, dt) if p.dim() >= 2 else p.omr_phys).data_ptr()

        ptrs = []
        for layer in layers:
            named = dict(layer.named_parameters())
            ptrs += [pointer(named[n]) for n in self.LAYER_PARAMS]
        self._layer_w = (ctypes.c_void_p * len(ptrs))(*ptrs)
        self.pe = dec.pos_1d.pe[0].contiguous()
        # fp8 mode (BASELINE config 5, an extension): every matrix of the step quantised ONCE to OCP e4m3 with a scale per
        # output row; the executor quantises the activations per token and runs the fp8 MFMA GEMM (omr_gemm_fp8)
        self.fp8 = bool(getattr(dec, "fp8_weights", False))
        self._fp8 = []
        if self.fp8:
            def quantised(p):
                w = Fn.wt(p, dt)
                q, s = K.quantize_rows_fp8(w.view(w.shape[0], -1))
                self._fp8.append((q, s))
                return q.data_ptr(), s.data_ptr()

            pairs = [quantised(dict(layer.named_parameters())[n]) for layer in layers for n in self.FP8_PARAMS]
            self._layer_w8 = (ctypes.c_void_p * len(pairs))(*[a for a, _ in pairs])
            self._layer_s8 = (ctypes.c_void_p * len(pairs))(*[b for _, b in pairs])
            self._head8 = quantised(dec.out_layer.weight)

    def _bind(self) -> None:
        """(Re)fill the descriptor after B / the buffers changed."""
        dec, ds = self.dec, self.desc
        ds.dtype, ds.B, ds.L, ds.d, ds.nhead = dtype_code(self.dtype), self.B, self.L, self.d, dec.transformer_decoder.layers[0].self_attn.num_heads
        ds.ff, ds.V, ds.ldv, ds.max_len, ds.S = dec.transformer_decoder.layers[0].linear1.weight.shape[0], self.V, self.ldv, self.max_len, self.S
        ds.window, ds.fp8 = (dec.attn_window if dec.attn_window > 0 else -1), int(self.fp8)
        if self.fp8:
            ds.layer_w8, ds.layer_s8 = ctypes.cast(self._layer_w8, ctypes.c_void_p), ctypes.cast(self._layer_s8, ctypes.c_void_p)
            ds.head_w8, ds.head_s8 = self._head8
        ds.emb, ds.pe = Fn.wt(dec.embedding.weight, self.dtype).data_ptr(), self.pe.data_ptr()
        ds.layer_w = ctypes.cast(self._layer_w, ctypes.c_void_p)
        ds.head_w, ds.head_b = Fn.wt(dec.out_layer.weight, self.dtype).data_ptr(), dec.out_layer.bias.omr_phys.data_ptr()
        ds.self_kv, ds.cross_kv, ds.cross_ld, ds.cross_bs = self.self_kv.data_ptr(), self.cross_kv.data_ptr(), self.L * 2 * self.d, self.cross_bs
        ds.ws, ds.ws_bytes = 0, 0
        nbytes = lib().query("omr_decode_workspace_bytes", ctypes.byref(ds))
        if nbytes <= 0:
            raise RuntimeError("libomr_hip: omr_decode_workspace_bytes rejected the decode descriptor")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.self_kv.device)
        ds.ws, ds.ws_bytes = self.ws.data_ptr(), nbytes
        self.logits = torch.empty((self.B, self.ldv), dtype=torch.float32, device=self.self_kv.device)
        self.tok = torch.empty(self.B, dtype=torch.int64, device=self.self_kv.device)

    def share_memory_between(self, rows: int) -> None:
        """Beam search: `rows` hypotheses over the ONE memory this state was initialised with (cross K|V batch stride 0)."""
        if self.mem_len is not None:
            raise RuntimeError("share_memory_between: beam search does not take a ragged decode state")
        assert self.B == 1 and self.t == 0
        self.B, self.cross_bs = rows, 0
        self.self_kv = torch.empty((self.L, rows, self.max_len, 2 * self.d), dtype=self.dtype, device=self.self_kv.device)
        self._bind()

    def reorder_rows(self, parents: torch.Tensor) -> None:
        """Beam search: row i continues hypothesis parents[i] (re-gathers the self-attention cache rows)."""
        if self.mem_len is not None:
            raise RuntimeError("reorder_rows: beam search does not take a ragged decode state")
        self.self_kv = self.self_kv.index_select(1, parents)
        self.desc.self_kv = self.self_kv.data_ptr()

    def rewind(self) -> None:
        """Decode again from <sos> over the same memories (an alpha sweep of the weighted fusion): the cross-attention K|V
        stay as projected; the self-attention cache is overwritten from position 0 and never read beyond t."""
        self.t = 0

    def _check(self, token: torch.Tensor, n: int) -> None:
        require_cuda(token)
        if token.numel() != self.B or token.dtype != torch.int64:
            raise RuntimeError(f"decode: expected {self.B} int64 tokens, got {tuple(token.shape)} {token.dtype}")
        if self.t + n > self.max_len:
            raise RuntimeError("decode_step beyond max_seq_len (positional-encoding table exhausted)")

    def constrain(self, grammar):
        """Decode under `grammar` (grammar.Grammar; None: unconstrained) from here on: one automaton state per row of this
        decode state, at the start state.  -> the GrammarState, or None."""
        self.gstate = None if grammar is None else grammar.bind(self.B, self.tok.device)
        return self.gstate

    def _steps(self, t0: int, n_steps: int, toks, top1, logits) -> None:
        if self.gstate is not None:
            if toks is None:
                raise RuntimeError("a constrained decode state picks its tokens itself: use run()")
            if self.mem_len is None:
                lib().call("omr_decode_steps_grammar", ctypes.byref(self.desc), self.gstate.byref(), ptr(self.tok), t0, n_steps, ptr(toks), ptr(top1),
                           ptr(logits), cur_stream())
            else:
                lib().call("omr_decode_steps_varlen_grammar", ctypes.byref(self.desc), ptr(self.mem_len), self.gstate.byref(), ptr(self.tok), t0, n_steps,
                           ptr(toks), ptr(top1), ptr(logits), cur_stream())
        elif self.mem_len is None:
            lib().call("omr_decode_steps", ctypes.byref(self.desc), ptr(self.tok), t0, n_steps, ptr(toks), ptr(top1), ptr(logits), cur_stream())
        else:
            lib().call("omr_decode_steps_varlen", ctypes.byref(self.desc), ptr(self.mem_len), ptr(self.tok), t0, n_steps, ptr(toks), ptr(top1),
                       ptr(logits), cur_stream())

    def step_logits(self, token: torch.Tensor) -> torch.Tensor:
        """One position, no token pick: fp32 logits [B, V] (a view of this state's buffer, valid until the next call)."""
        self._check(token, 1)
        self.tok.copy_(token.reshape(-1))
        self._steps(self.t, 1, None, None, self.logits)
        self.t += 1
        return self.logits[:, :self.V]

    def run(self, token: torch.Tensor, n_steps: int):
        self._check(token, n_steps)
        self.tok.copy_(token.reshape(-1))
        toks = torch.empty((n_steps, self.B), dtype=torch.int64, device=self.tok.device)
        top1 = torch.empty((n_steps, self.B), dtype=torch.float32, device=self.tok.device)
        self._steps(self.t, n_steps, toks, top1, None)
        self.t += n_steps
        return toks, top1


class SlotDecodeState(DecodeState):
    """A decode state of `rows` SLOTS whose rows each sit at their own position (omr_decode_steps_rows): the state behind
    continuous batching of greedy evaluation (evaluation.decode_stream).  A slot takes one input at a time: admit() projects that
    memory's cross-attention K|V into the slot with the GEMM a batch-size-1 state of it runs and puts the row back to position
    0 and <sos>; what the slot's previous occupant left in the caches is never read (a row sees its own positions and its own
    memory length only).  capacity: the longest memory a slot will hold.  pos / mem_len live on the device and are uploaded
    once per run_rows call, from the host lists this state keeps."""

    def __init__(self, dec: "Decoder", rows: int, capacity: int, dt: torch.dtype, device, sos: int):
        if rows < 1 or capacity < 1:
            raise ValueError(f"slot decode state: rows {rows} and capacity {capacity} must be >= 1")
        self.dec, self.dtype, self.t, self.sos = dec, dt, 0, sos
        self.L, self.d = len(dec.transformer_decoder.layers), dec.embedding.weight.shape[1]
        self.B, self.S = rows, capacity
        self.max_len = dec.pos_1d.pe.shape[1]
        self.V, self.ldv = dec.output_size, K.round_up(dec.output_size, 8)
        L, d = self.L, self.d
        self.cross_kv = torch.empty((rows, capacity, L * 2 * d), dtype=dt, device=device)
        self.cross_bs = capacity * L * 2 * d
        self.self_kv = torch.empty((L, rows, self.max_len, 2 * d), dtype=dt, device=device)
        self._mem_len_h, self._pos_h, self._live = [1] * rows, [0] * rows, [False] * rows
        self.mem_len = torch.ones(rows, dtype=torch.int32, device=device)
        self.pos = torch.zeros(rows, dtype=torch.int32, device=device)
        self.admitted = 0                      # inputs admitted so far (more than `rows`: slots were refilled)
        self.positions = 0                     # positions run so far (each for all slots)
        self._weights()
        self.desc = _DecodeDesc()
        self._bind()
        self.tok.fill_(sos)

    def admit(self, slot: int, memory: Optional[torch.Tensor]) -> None:
        """Give `slot` to the input with this memory ([S_b, d] in the compute dtype), or to nobody (None): an idle slot runs
        from position 0 at every call and its output is dropped."""
        self._pos_h[slot] = 0
        self._live[slot] = memory is not None
        if memory is None:
            return
        n = memory.shape[0]
        if memory.dim() != 2 or memory.shape[1] != self.d or not 1 <= n <= self.S or memory.dtype != self.dtype:
            raise ValueError(f"slot decode state: a memory of shape {tuple(memory.shape)} {memory.dtype} does not fit a slot of [{self.S}, {self.d}] {self.dtype}")
        self._project(memory, self.cross_kv[slot, :n])
        self._mem_len_h[slot] = n
        self.tok[slot:slot + 1].fill_(self.sos)
        self.admitted += 1

    def furthest(self) -> int:
        """The largest position of a slot that holds an input (idle slots start over at every call)."""
        return max((p for p, live in zip(self._pos_h, self._live) if live), default=0)

    def begin(self, n_steps: int) -> int:
        """Upload the rows' positions and memory lengths for a call of n_steps positions -> the largest position."""
        for b in range(self.B):
            if not self._live[b]:
                self._pos_h[b] = 0
        t_max = self.furthest()
        if n_steps < 1 or t_max + n_steps > self.max_len:
            raise RuntimeError("decode_step beyond max_seq_len (positional-encoding table exhausted)")
        self.pos.copy_(torch.tensor(self._pos_h, dtype=torch.int32))
        self.mem_len.copy_(torch.tensor(self._mem_len_h, dtype=torch.int32))
        return t_max

    def advance(self, n_steps: int) -> None:
        self.positions += n_steps
        self._pos_h = [p + n_steps for p in self._pos_h]

    def run_rows(self, n_steps: int):
        """n_steps further positions of every slot -> (tokens int64 [n_steps, rows], their fp32 top-1 logits [n_steps, rows]),
        on the device; the chosen tokens reach the next position there."""
        t_max = self.begin(n_steps)
        toks = torch.empty((n_steps, self.B), dtype=torch.int64, device=self.tok.device)
        top1 = torch.empty((n_steps, self.B), dtype=torch.float32, device=self.tok.device)
        if self.gstate is not None:
            lib().call("omr_decode_steps_rows_grammar", ctypes.byref(self.desc), ptr(self.mem_len), ptr(self.pos), t_max, self.gstate.byref(),
                       ptr(self.tok), n_steps, ptr(toks), ptr(top1), None, cur_stream())
        else:
            lib().call("omr_decode_steps_rows", ctypes.byref(self.desc), ptr(self.mem_len), ptr(self.pos), t_max, ptr(self.tok), n_steps, ptr(toks),
                       ptr(top1), None, cur_stream())
        self.advance(n_steps)
        return toks, top1

    def _no_lockstep(self, *_a, **_k):
        raise RuntimeError("a slot decode state has no common position: use admit / run_rows")

    run = step_logits = rewind = share_memory_between = reorder_rows = _no_lockstep


MAX_DRAFT_LEN = 31           # OMR_MAX_VERIFY_ROWS - 1: a cycle's proposals plus the token before them are the rows of one grouped position


def check_draft_len(k) -> None:
    """THE check of the proposals per cycle (evaluation.check_draft, SpecDecodeState)."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_DRAFT_LEN:
        raise ValueError(f"draft_len must be an integer in 1..{MAX_DRAFT_LEN}, got {k}")


def check_row_widths(name: str, dec: "Decoder") -> None:
    """THE check that a model of a speculative decode (`name`: "target" / "draft") takes the row kernel; the message names the widths."""
    if not dec.takes_slot_state():
        raise ValueError(f"speculative decode: the {name}'s decoder widths ({dec.width_text()}) are outside the row kernel")


class _SpecDesc(ctypes.Structure):
    """omr_spec_desc of include/omr_hip.h."""
    STATE_FIELDS = ("pos", "out_len", "done", "accepted", "totals", "first", "prev", "tokens", "picks", "top1", "dpicks", "out_tokens", "out_top1")
    _fields_ = [(n, ctypes.c_int) for n in ("B", "k", "eos", "max_out", "t_max", "pad_")] + [("state", ctypes.c_void_p), ("state_bytes", ctypes.c_long)] + [
        (n, ctypes.c_void_p) for n in STATE_FIELDS] + [("ws_t", ctypes.c_void_p), ("ws_t_bytes", ctypes.c_long)]


class SpecDecodeState:
    """Device state of a speculative greedy decode of B inputs (csrc/decode_spec.hip, omr_spec_decode_cycles): a ragged decode
    state of the TARGET over its memories and one of the DRAFT over its own (both models encode the input themselves), the
    target's scratch for a grouped position of k + 1 rows per slot, and the cycle state (positions, proposals, picks, output
    runs, totals) in ONE device block that snapshot() brings to the host with one copy.  start() runs position 0 of both models
    with the plain step; run_cycles(n, t_max) enqueues n cycles; plain(n, pos) runs n plain positions of the target from per-row
    positions (the tail before max_len, where a cycle no longer fits)."""

    def __init__(self, dec: "Decoder", mems, draft: "Decoder", draft_mems, k: int, sos: int, eos: int, max_out: Optional[int] = None):
        import numpy as np
        check_draft_len(k)
        if len(mems) != len(draft_mems) or not mems:
            raise ValueError(f"speculative decode: {len(mems)} memories for the target, {len(draft_mems)} for the draft")
        if draft.output_size != dec.output_size or not (0 <= sos < dec.output_size and 0 <= eos < dec.output_size):
            raise ValueError(f"speculative decode: vocabularies {dec.output_size} / {draft.output_size}, sos {sos}, eos {eos} do not fit")
        check_row_widths("target", dec)
        check_row_widths("draft", draft)
        self.target = DecodeState(dec, dec.memory_list(mems), dec._compute_dtype())
        self.draft = DecodeState(draft, draft.memory_list(draft_mems), draft._compute_dtype())
        self.B, self.k, self.R, self.sos, self.eos = self.target.B, k, k + 1, sos, eos
        self.max_len = min(self.target.max_len, self.draft.max_len)
        self.max_out = self.max_len if max_out is None else min(int(max_out), self.max_len)
        dev = self.target.self_kv.device
        sd = self.sdesc = _SpecDesc()
        sd.B, sd.k, sd.eos, sd.max_out, sd.t_max = self.B, k, eos, self.max_out, 1
        sd.state = None
        nbytes = lib().query("omr_spec_workspace_bytes", ctypes.byref(sd))
        if nbytes <= 0:
            raise RuntimeError("libomr_hip: omr_spec_workspace_bytes rejected the speculative descriptor")
        self._off = {n: int(getattr(sd, n) or 0) for n in _SpecDesc.STATE_FIELDS}      # state == NULL: the fields are offsets
        self._np = np
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        sd.state, sd.state_bytes = self.state.data_ptr(), nbytes
        if lib().query("omr_spec_workspace_bytes", ctypes.byref(sd)) != nbytes:
            raise RuntimeError("libomr_hip: omr_spec_workspace_bytes changed its answer")
        ws_bytes = lib().query("omr_decode_group_workspace_bytes", ctypes.byref(self.target.desc), self.R)
        if ws_bytes <= 0:
            raise RuntimeError("libomr_hip: omr_decode_group_workspace_bytes rejected the target's descriptor")
        self.ws_t = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        sd.ws_t, sd.ws_t_bytes = self.ws_t.data_ptr(), ws_bytes
        self.tail_pos = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.cycles = 0

    def _dev(self, name: str, dtype: torch.dtype, count: int) -> torch.Tensor:
        off = self._off[name]
        return self.state[off:off + count * torch.empty((), dtype=dtype).element_size()].view(dtype)

    def start(self):
        """Position 0 of both models with the plain step (omr_decode_steps_varlen from <sos>), and the cycle state after it: every
        slot at position 1 with one token in its run -> (tokens [B], top-1 values [B]) on the device."""
        B = self.B
        sos = torch.full((B, 1), self.sos, dtype=torch.int64, device=self.state.device)
        toks, top1 = self.target.run(sos, 1)
        self.draft.run(sos, 1)
        self.state.zero_()
        self._dev("pos", torch.int32, B).fill_(1)
        self._dev("out_len", torch.int32, B).fill_(1)
        done = toks[0] == self.eos
        self._dev("done", torch.int32, B).copy_(torch.ones_like(done) if self.max_out <= 1 else done)
        self._dev("first", torch.int64, B).copy_(toks[0])
        self._dev("prev", torch.int64, B).fill_(self.sos)
        self._dev("out_tokens", torch.int64, B * self.max_out).view(B, self.max_out)[:, 0].copy_(toks[0])
        self._dev("out_top1", torch.float32, B * self.max_out).view(B, self.max_out)[:, 0].copy_(top1[0])
        self.cycles = 0
        return toks[0], top1[0]

    def run_cycles(self, n_cycles: int, t_max: int) -> None:
        """n_cycles cycles of draft k, verify k + 1, accept, from one host call.  t_max: an upper bound of every live slot's position."""
        if n_cycles < 1 or t_max < 1 or t_max + n_cycles * self.R > self.max_len:
            raise RuntimeError("speculative decode beyond max_seq_len (positional-encoding table exhausted)")
        self.sdesc.t_max = t_max
        lib().call("omr_spec_decode_cycles", ctypes.byref(self.target.desc), ctypes.byref(self.draft.desc), ptr(self.target.mem_len),
                   ptr(self.draft.mem_len), ctypes.byref(self.sdesc), self.k, n_cycles, cur_stream())
        self.cycles += n_cycles

    def snapshot(self) -> dict:
        """One device-to-host copy of the whole block -> {field: numpy array}."""
        np = self._np
        host = self.state.cpu().numpy()
        B, R = self.B, self.R

        def view(name, dtype, count):
            off = self._off[name]
            return host[off:off + count * np.dtype(dtype).itemsize].view(dtype)

        out = {n: view(n, np.int32, B) for n in ("pos", "out_len", "done", "accepted")}
        out["totals"] = view("totals", np.int64, 2)
        out["first"], out["prev"] = view("first", np.int64, B), view("prev", np.int64, B)
        out["tokens"], out["picks"] = view("tokens", np.int64, B * R).reshape(B, R), view("picks", np.int64, B * R).reshape(B, R)
        out["top1"] = view("top1", np.float32, B * R).reshape(B, R)
        out["out_tokens"] = view("out_tokens", np.int64, B * self.max_out).reshape(B, self.max_out)
        out["out_top1"] = view("out_top1", np.float32, B * self.max_out).reshape(B, self.max_out)
        return out

    def plain(self, n_steps: int, pos: List[int]):
        """n_steps plain positions of the target (omr_decode_steps_rows), row b from pos[b], feeding the last token of its run ->
        (tokens int64 [n_steps, B], top-1 fp32 [n_steps, B]) on the device."""
        t_max = max(pos)
        if n_steps < 1 or min(pos) < 0 or t_max + n_steps > self.target.max_len:
            raise RuntimeError("decode_step beyond max_seq_len (positional-encoding table exhausted)")
        dev = self.state.device
        self.tail_pos.copy_(torch.tensor(pos, dtype=torch.int32))
        toks = torch.empty((n_steps, self.B), dtype=torch.int64, device=dev)
        top1 = torch.empty((n_steps, self.B), dtype=torch.float32, device=dev)
        lib().call("omr_decode_steps_rows", ctypes.byref(self.target.desc), ptr(self.target.mem_len), ptr(self.tail_pos), t_max,
                   ptr(self._dev("first", torch.int64, self.B)), n_steps, ptr(toks), ptr(top1), None, cur_stream())
        return toks, top1


class _BeamDesc(ctypes.Structure):
    """omr_beam_desc of include/omr_hip.h."""
    STATE_FIELDS = ("scores", "best_score", "tokens", "best_row", "best_pos", "done", "exhausted", "parents", "hist_parent", "hist_token")
    _fields_ = [(n, ctypes.c_int) for n in ("beam", "N", "eos", "max_len")] + [("state", ctypes.c_void_p), ("state_bytes", ctypes.c_long)] + [
        (n, ctypes.c_void_p) for n in STATE_FIELDS + ("self_kv2", "last_logits")]


class BeamSearchBlock:
    """The search state of a batched beam search (include/omr_hip.h, omr_beam_desc) over N inputs of `beam` rows each: one
    device block, its descriptor, the host image it started from, and the reads of it.  max_len: the positions the history
    tables hold.  One block serves a BeamDecodeState, or the two models of a WeightedBeamState."""

    def __init__(self, N: int, beam: int, sos: int, eos: int, max_len: int, device):
        import numpy as np
        self.N, self.beam, self.rows, self.max_len = N, beam, N * beam, max_len
        bd = self.bdesc = _BeamDesc()
        bd.beam, bd.N, bd.eos, bd.max_len = beam, N, eos, max_len
        bd.state = None
        nbytes = lib().query("omr_beam_workspace_bytes", ctypes.byref(bd))
        if nbytes <= 0:
            raise RuntimeError("libomr_hip: omr_beam_workspace_bytes rejected the beam descriptor")
        self._off = {n: int(getattr(bd, n) or 0) for n in _BeamDesc.STATE_FIELDS}      # state == NULL: the fields are offsets
        host = np.zeros(nbytes, dtype=np.uint8)
        self._view(host, "scores", np.float64, self.rows)[:] = ([0.0] + [float("-inf")] * (beam - 1)) * N
        self._view(host, "best_score", np.float64, N)[:] = float("-inf")
        self._view(host, "tokens", np.int64, self.rows)[:] = sos
        self._view(host, "exhausted", np.int32, N)[:] = 1
        self._initial = torch.from_numpy(host)
        self.state = self._initial.to(device)
        bd.state, bd.state_bytes = self.state.data_ptr(), nbytes
        if lib().query("omr_beam_workspace_bytes", ctypes.byref(bd)) != nbytes:
            raise RuntimeError("libomr_hip: omr_beam_workspace_bytes changed its answer")

    def rewind(self) -> None:
        """Upload the block as it was before position 0 (another search over the same inputs)."""
        self.state.copy_(self._initial)

    def _view(self, host, name: str, dtype, count: int):
        import numpy as np
        off = self._off[name]
        return host[off:off + count * np.dtype(dtype).itemsize].view(dtype)

    def _device_ints(self, name: str, count: int) -> torch.Tensor:
        off = self._off[name]
        return self.state[off:off + 4 * count].view(torch.int32)

    def done(self) -> List[bool]:
        """The `done` flag of every input (one small device-to-host copy)."""
        return [bool(v) for v in self._device_ints("done", self.N).cpu().tolist()]

    def parents(self) -> torch.Tensor:
        """int32 [N, beam], on the device: the LOCAL row each row of the next position continues (of the last position run)."""
        return self._device_ints("parents", self.rows).view(self.N, self.beam)

    def snapshot(self) -> dict:
        """One device-to-host copy of the whole search state -> {field: numpy array} (history tables [max_len, rows])."""
        import numpy as np
        host = self.state.cpu().numpy()
        rows, N = self.rows, self.N
        out = {"scores": self._view(host, "scores", np.float64, rows), "best_score": self._view(host, "best_score", np.float64, N),
               "tokens": self._view(host, "tokens", np.int64, rows), "parents": self._view(host, "parents", np.int32, rows)}
        for n in ("best_row", "best_pos", "done", "exhausted"):
            out[n] = self._view(host, n, np.int32, N)
        for n in ("hist_parent", "hist_token"):
            out[n] = self._view(host, n, np.int32, self.max_len * rows).reshape(self.max_len, rows)
        return out

    def results(self, positions: int, dead_end=None):
        """-> [(token ids, score)] per input after `positions` positions: what the host loop finds for that input alone
        (evaluation.beam_results; dead_end: as there)."""
        from .evaluation import beam_results
        s = self.snapshot()
        return beam_results(self.beam, positions, int(self.bdesc.eos), s["scores"], s["best_score"], s["best_row"], s["best_pos"], s["done"],
                            s["hist_parent"], s["hist_token"], dead_end)


class BeamDecodeState(DecodeState):
    """Device state of a beam search over N inputs at once (csrc/decode.hip, omr_beam_decode_steps): a ragged decode state of
    N memories whose B = N * beam rows are the hypotheses (row n * beam + k: hypothesis k of input n; the rows of an input read
    its one cross-attention K|V slot), two self-attention caches that alternate per position, and the search state
    (BeamSearchBlock) in one device block.  run(n) issues n positions from one host call; results() reads the block back
    once and walks the history tables on the host (evaluation.beam_results)."""

    def __init__(self, dec: "Decoder", mems, dt: torch.dtype, beam: int, sos: int, eos: int):
        super().__init__(dec, mems, dt, rows_per_memory=beam)
        self.beam, self.sos, self.eos, self.N = beam, sos, eos, len(mems)
        self.self_kv2 = torch.empty_like(self.self_kv)
        self.search = BeamSearchBlock(self.N, beam, sos, eos, self.max_len, self.self_kv.device)
        self.bdesc, self.state = self.search.bdesc, self.search.state
        self.bdesc.self_kv2, self.bdesc.last_logits = self.self_kv2.data_ptr(), self.logits.data_ptr()

    def share_memory_between(self, rows: int) -> None:
        raise RuntimeError("share_memory_between: a beam decode state already shares each memory between its hypotheses")

    ctc = None             # kernels.CtcPrefixBlock: the CTC prefix scores the selection mixes in (None: attention scores alone)

    def attach_ctc(self, logits: torch.Tensor, frame_len: torch.Tensor, weight: float):
        """The analogue of `constrain` for the joint CTC / attention search, called once before position 0: logits [N, Fmax, >= V] of the CTC
        head (input n's frames in rows [0, frame_len[n])), frame_len int32 [N], weight the CTC share of every candidate's value.  Allocates the
        prefix-score block and runs the frames' lse pass (omr_ctc_prefix_init); run() then issues omr_beam_decode_steps_ctc."""
        from .kernels import CtcPrefixBlock
        if self.t != 0:
            raise RuntimeError("attach_ctc: the search has started")
        if self.gstate is not None:
            raise ValueError("the CTC prefix score does not combine with a grammar")
        if logits.dim() != 3 or logits.shape[0] != self.N:
            raise ValueError(f"attach_ctc: logits of {tuple(logits.shape)} for {self.N} inputs")
        self.ctc = CtcPrefixBlock(logits, frame_len, self.V, self.beam, blank=self.dec.padding_idx, sos=self.sos, eos=self.eos, weight=weight)
        return self.ctc

    def run(self, n_steps: int) -> None:                   # noqa: D401 -- positions t .. t + n_steps - 1, nothing returned
        """Run n_steps positions of every input (decode step, selection, cache reorder) without a host round trip."""
        if n_steps < 1 or self.t + n_steps > self.max_len:
            raise RuntimeError("beam decode beyond max_seq_len (positional-encoding table exhausted)")
        if self.ctc is not None:
            lib().call("omr_beam_decode_steps_ctc", ctypes.byref(self.desc), ctypes.byref(self.bdesc), self.ctc.byref(), ptr(self.mem_len), self.t,
                       n_steps, cur_stream())
        elif self.gstate is not None:
            lib().call("omr_beam_decode_steps_grammar", ctypes.byref(self.desc), ctypes.byref(self.bdesc), ptr(self.mem_len), self.gstate.byref(), self.t,
                       n_steps, cur_stream())
        else:
            lib().call("omr_beam_decode_steps", ctypes.byref(self.desc), ctypes.byref(self.bdesc), ptr(self.mem_len), self.t, n_steps, cur_stream())
        self.t += n_steps

    def done(self) -> List[bool]:
        return self.search.done()

    def parents(self) -> torch.Tensor:
        return self.search.parents()

    def snapshot(self) -> dict:
        return self.search.snapshot()

    def results(self):
        """-> [(token ids, score)] per input, what _Base.beam_search finds for that input alone (evaluation.beam_results)."""
        return self.search.results(self.t, None if self.ctc is None else self.ctc.advanced().cpu().tolist())


class WeightedBeamState:
    """Device state of a beam search over the weighted late fusion of N pairs at once (csrc/decode.hip,
    omr_weighted_beam_decode_steps; an extension: the reference decodes greedily): per model a ragged decode state of
    rows_per_memory = beam over its memories with a second self-attention cache, and ONE search block (BeamSearchBlock) that
    both models read their tokens and parents from.  The history holds min(max_len) positions: no search outlives the shorter
    positional table.  run(n) issues n positions from one host call; rewind() starts another search over the same pairs (an
    alpha sweep, `alpha` being the mixing weight run() passes on): the cross-attention K|V stay as projected."""

    def __init__(self, dec_a: "Decoder", mems_a, dec_b: "Decoder", mems_b, beam: int, sos: int, eos: int, alpha: float = 0.5):
        if not 1 <= beam <= MAX_BEAM:
            raise ValueError(f"beam must be in 1..{MAX_BEAM}, got {beam}")
        if len(mems_a) != len(mems_b):
            raise ValueError(f"weighted beam state: {len(mems_a)} memories for one model, {len(mems_b)} for the other")
        V = dec_a.output_size
        if dec_b.output_size != V or beam > V or not (0 <= sos < V and 0 <= eos < V):
            raise ValueError(f"weighted beam state: vocabularies {V} / {dec_b.output_size}, beam {beam}, sos {sos}, eos {eos} do not fit")
        self.st_a = DecodeState(dec_a, dec_a.memory_list(mems_a), dec_a._compute_dtype(), rows_per_memory=beam)
        self.st_b = DecodeState(dec_b, dec_b.memory_list(mems_b), dec_b._compute_dtype(), rows_per_memory=beam)
        self.kv2_a, self.kv2_b = torch.empty_like(self.st_a.self_kv), torch.empty_like(self.st_b.self_kv)
        self.beam, self.N, self.t, self.alpha = beam, len(mems_a), 0, float(alpha)
        self.max_len = min(self.st_a.max_len, self.st_b.max_len)
        self.search = BeamSearchBlock(self.N, beam, sos, eos, self.max_len, self.st_a.self_kv.device)
        self.bdesc = self.search.bdesc
        self.bdesc.self_kv2, self.bdesc.last_logits = self.kv2_a.data_ptr(), None

    gstate = None          # grammar.GrammarState over the N * beam rows: ONE automaton state per row drives both models

    def constrain(self, grammar):
        """DecodeState.constrain for the search both models share."""
        self.gstate = None if grammar is None else grammar.bind(self.st_a.B, self.st_a.tok.device)
        return self.gstate

    def run(self, n_steps: int) -> None:
        """n_steps positions of every pair (both models' steps, the weighted selection, both cache reorders), no host round trip."""
        if n_steps < 1 or self.t + n_steps > self.max_len:
            raise RuntimeError("weighted beam decode beyond a model's max_seq_len (positional-encoding table exhausted)")
        if self.gstate is not None:
            lib().call("omr_weighted_beam_decode_steps_grammar", ctypes.byref(self.st_a.desc), ptr(self.st_a.mem_len), ctypes.byref(self.st_b.desc),
                       ptr(self.st_b.mem_len), ctypes.byref(self.bdesc), ptr(self.kv2_b), self.gstate.byref(), self.alpha, self.t, n_steps, cur_stream())
        else:
            lib().call("omr_weighted_beam_decode_steps", ctypes.byref(self.st_a.desc), ptr(self.st_a.mem_len), ctypes.byref(self.st_b.desc),
                       ptr(self.st_b.mem_len), ctypes.byref(self.bdesc), ptr(self.kv2_b), self.alpha, self.t, n_steps, cur_stream())
        self.t += n_steps

    def done(self) -> List[bool]:
        return self.search.done()

    def results(self):
        """-> [(token ids, score)] per pair, what weighted_fusion.weighted_beam_search finds for that pair alone."""
        return self.search.results(self.t)

    def rewind(self, alpha: Optional[float] = None) -> None:
        """Back to position 0 over the same pairs, with another alpha if given: the initial search block is uploaded again."""
        self.search.rewind()
        self.t = 0
        if self.gstate is not None:
            self.gstate.reset()
        if alpha is not None:
            self.alpha = float(alpha)
