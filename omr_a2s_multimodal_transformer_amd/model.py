"""Transformer / MultimodalTransformer on the HIP path -- the reference's src/transformer/model.py class surface
(constructor signatures, attributes, hooks, state-dict names) with extra keyword `config` (ModelConfig)
for the parameterised builds BASELINE.json names.  The three reference quirks are reproduced.
"""
from __future__ import annotations

import ctypes
import functools
import itertools
import math
import random
from typing import Callable, Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import functional as Fn
from . import kernels as K
from ._lib import lib
from .config import DistillConfig, ModelConfig
from .decoder import MAX_BEAM, Decoder, Linear, MultiheadAttention, _to_dev, takes_ragged_state
from .encoder import HEIGHT_REDUCTION, WIDTH_REDUCTION, Encoder
from .evaluation import (WINDOW_BATCHES, Alignment, active_ctc_decode, active_grammar, active_spec, cells_and_boxes, ctc_decode_option, decode_rows,
                         decode_spec, decode_stream, grammar_option, grid_of, plan_align_groups, plan_groups, plan_pair_groups, refill_enabled, refill_option, spec_option,
                         stream_order)
from .grammar import host_mask
from .lightning_shim import LightningModule
from .metrics import compute_metrics, compute_metrics_sharded
from .runtime import FlatModuleMixin
from .synthetic import EOS_TOKEN, SOS_TOKEN

NUM_CHANNELS = 1  # preprocessing.py:12

_DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def sinusoid_2d(num_channels: int, max_height: int, max_width: int) -> torch.Tensor:
    """model.py:33-42 -> [1, C, max_height, max_width]."""
    half = num_channels // 2
    pos_h = torch.arange(max_height).unsqueeze(1)
    pos_w = torch.arange(max_width).unsqueeze(1)
    den = torch.pow(10000, torch.arange(0, half, 2) / num_channels)
    pe = torch.zeros(1, max_height, max_width, num_channels)
    pe[0, :, :, 0:half:2] = torch.sin(pos_w / den).unsqueeze(0).repeat(max_height, 1, 1)
    pe[0, :, :, 1:half:2] = torch.cos(pos_w / den).unsqueeze(0).repeat(max_height, 1, 1)
    pe[0, :, :, half::2] = torch.sin(pos_h / den).unsqueeze(1).repeat(1, max_width, 1)
    pe[0, :, :, half + 1::2] = torch.cos(pos_h / den).unsqueeze(1).repeat(1, max_width, 1)
    return pe.permute(0, 3, 1, 2).contiguous()


class PositionalEncoding2D(nn.Module):
    """model.py:18-48.  forward takes the encoder's [B,C,h,w] output (channels_last-strided: no copy)."""

    def __init__(self, num_channels: int, max_height: int, max_width: int, dropout_p: float = 0.1) -> None:
        super().__init__()
        self.dropout_p = dropout_p
        pe = sinusoid_2d(num_channels, max_height, max_width)
        self.register_buffer("pe", pe)
        self.register_buffer("pe_hwc", pe[0].permute(1, 2, 0).contiguous(), persistent=False)  # kernel layout [maxh][maxw][C]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        xn = x.permute(0, 2, 3, 1)
        if not xn.is_contiguous():
            xn = xn.contiguous()
        y = Fn.AddPE2DFn.apply(xn, self.pe_hwc)
        if self.training and self.dropout_p > 0:
            from .runtime import next_seed
            y = Fn.DropoutFn.apply(y, self.dropout_p, next_seed("nhwc", self.dropout_p), False, False)
        return y.permute(0, 3, 1, 2)


def _flatten_memory(x: torch.Tensor) -> torch.Tensor:
    """x.flatten(2).permute(0, 2, 1).contiguous() (model.py:147): free for channels_last-strided maps."""
    return x.flatten(2).permute(0, 2, 1).contiguous()


class CrossEntropyLoss(nn.Module):
    """CrossEntropyLoss(ignore_index) on [B, V, T] logits (model.py:109,166) through the HIP CE kernels.
    label_smoothing: torch's argument of that name and range (the reference leaves it at 0).  After a forward `last_nll` holds the
    un-smoothed mean of the same rows, a detached device scalar (no sync): the figure runs with different smoothing share."""

    def __init__(self, ignore_index: int = 0, label_smoothing: float = 0.0):
        super().__init__()
        self.ignore_index = ignore_index
        self.label_smoothing = K.check_label_smoothing(label_smoothing)
        self.last_nll: Optional[torch.Tensor] = None

    def forward(self, logits_bvt: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        loss, self.last_nll = Fn.cross_entropy(logits_bvt, target, self.ignore_index, self.label_smoothing, return_nll=True)
        return loss


class DistillationLoss(nn.Module):
    """Hard-label cross-entropy plus the KL divergence to one or two teachers' logits, all [B, V, T], through the fused HIP kernels
    (functional.cross_entropy_distill; an extension).  config: DistillConfig.  After a forward `last_nll` and `last_kd` hold the two parts
    of the loss, detached device scalars (no sync)."""

    def __init__(self, ignore_index: int = 0, config: Optional[DistillConfig] = None):
        super().__init__()
        if isinstance(config, dict):
            config = DistillConfig.from_dict(config)
        self.ignore_index = ignore_index
        self.config = config if config is not None else DistillConfig()
        self.last_nll: Optional[torch.Tensor] = None
        self.last_kd: Optional[torch.Tensor] = None

    def forward(self, logits_bvt: torch.Tensor, target: torch.Tensor, teachers_bvt) -> torch.Tensor:
        teachers = (teachers_bvt,) if isinstance(teachers_bvt, torch.Tensor) else tuple(teachers_bvt)
        c = self.config
        loss, self.last_nll, self.last_kd = Fn.cross_entropy_distill(logits_bvt, target, teachers, self.ignore_index,
                                                                     alpha=c.alpha if len(teachers) == 2 else 1.0,
                                                                     temperature=c.temperature, weight=c.weight)
        return loss


def _is_pixel_sizes(xl) -> bool:
    """Whether a `forward` length argument names per-sample pixel sizes (the ragged route): a 2-D tensor [B, 2] of an integer type.
    A bool [B, S] key-padding mask (also with S == 2) and everything else is a memory_len and goes to the decoder as it always did."""
    return (isinstance(xl, torch.Tensor) and xl.dim() == 2 and xl.shape[1] == 2 and xl.dtype != torch.bool
            and not xl.is_floating_point() and not xl.is_complex())


def _pair_route(xli, xla) -> str:
    """Which route a (xli, xla) pair of `MultimodalTransformer.forward` takes: "ragged" when BOTH are per-sample pixel sizes
    (`_is_pixel_sizes`), "dense" when neither is (None, integer lengths [B], bool masks: the reference's forms); one of each is an error."""
    ri, ra = _is_pixel_sizes(xli), _is_pixel_sizes(xla)
    if ri != ra:
        raise ValueError("the ragged route takes per-sample pixel sizes [B, 2] for BOTH modalities: got "
                         f"xli {None if xli is None else tuple(xli.shape)} and xla {None if xla is None else tuple(xla.shape)}")
    return "ragged" if ri else "dense"


def _pad_mask(n: int, lens_dev: torch.Tensor) -> torch.Tensor:
    """bool [B, n], True = no key: the rows at and past each sample's length (device lengths, no sync)."""
    return torch.arange(n, device=lens_dev.device).unsqueeze(0) >= lens_dev.unsqueeze(1)


def _beam_option(fn):
    """Gives a `predict` / `evaluate` method the keyword `beam` (1 .. 8, default 1).  The method's own parameter list -- part
    of the public surface the late-fusion code and its tests build on -- stays as it is; beam = 1 calls it as before, a
    wider beam is checked here, before anything is encoded, and makes `_predict` decode every input with `beam_search` /
    `beam_search_batch` for the duration of the call."""
    @functools.wraps(fn)
    def call(self, *args, beam: int = 1, **kwargs):
        if not isinstance(beam, int) or not 1 <= beam <= MAX_BEAM:
            raise ValueError(f"beam must be an integer in 1..{MAX_BEAM}, got {beam}")
        if beam == 1:
            return fn(self, *args, **kwargs)
        before, self._decode_beam = self._decode_beam, beam
        try:
            return fn(self, *args, **kwargs)
        finally:
            self._decode_beam = before
    return call


class _Base(FlatModuleMixin, LightningModule):
    _decode_beam = 1          # beam width `_predict` decodes with (set by _beam_option for the duration of a call)
    _refill_sync_every = 8    # positions per read-back of a refilled decode (evaluation.decode_stream); results do not depend on it
    decode_grammar = None     # grammar.Grammar every decode of this model is constrained by unless a call says `grammar=` (evaluation.grammar_option)
    _refill_state_hook = None  # called with every SlotDecodeState `_greedy_stream` creates, before its first admission (tests)
    _spec_sync_every = 4      # cycles per read-back of a speculative decode (evaluation.decode_spec); results do not depend on it
    last_spec_stats = None    # {"cycles", "drafted", "accepted", "tokens"} of the last call with draft= (evaluation.spec_option)

    def _common_init(self, w2i, i2w, ytest_i2w, max_seq_len, attn_window, teacher_forcing_prob, config: Optional[ModelConfig]):
        if isinstance(config, dict):
            config = ModelConfig.from_dict(config)
        self.config = config if config is not None else ModelConfig()
        if "config" in self.hparams:
            self.hparams["config"] = self.config.to_dict()   # plain data: checkpoints load with weights_only=True
        self._default_compute_dtype = _DTYPES[self.config.compute_dtype]
        self.w2i, self.i2w = w2i, i2w
        self.ytest_i2w = ytest_i2w if ytest_i2w is not None else i2w
        self.padding_idx = w2i["<PAD>"]
        self.max_seq_len = max_seq_len
        self.teacher_forcing_prob = teacher_forcing_prob
        self.attn_window = attn_window
        self.compute_loss = CrossEntropyLoss(ignore_index=self.padding_idx, label_smoothing=self.config.label_smoothing)
        self.ctc_weight, self.ctc_pool = K.check_ctc(self.config.ctc_weight, self.config.ctc_pool)
        self.Y: List[List[str]] = []
        self.YHat: List[List[str]] = []

    def _make_decoder(self) -> Decoder:
        c = self.config
        dec = Decoder(output_size=len(self.w2i), max_seq_len=self.max_seq_len, num_embeddings=len(self.w2i), embedding_dim=c.d_model,
                      padding_idx=self.padding_idx, ff_dim=c.ff_dim, dropout_p=c.dropout, nhead=c.nhead,
                      num_transformer_layers=c.num_layers, attn_window=self.attn_window)
        dec.fp8_weights = bool(c.fp8_decode)         # KV-cached decoding on the fp8 MFMA (decoder.DecodeState)
        return dec

    # ---- data parallel (ddp.py): bucket boundaries are autograd nodes placed where a bucket's gradients are final
    _reducer = None

    def attach_reducer(self, process_group=None):
        """One bucket per top-level sub-module (encoder(s) | decoder+mixer), reduced as backward leaves it."""
        from .ddp import GradReducer
        flat = self.ensure_flat()
        enc_names = [n for n in flat.names if n.startswith(("encoder.", "image_encoder.", "audio_encoder."))]
        dec_names = [n for n in flat.names if n not in set(enc_names)]
        buckets = [flat.slice_of(enc_names), flat.slice_of(dec_names)]
        self._reducer = GradReducer(flat, process_group, buckets)
        self._reducer.broadcast_state()        # replicas start from rank 0's parameters (and Adam moments), like Lightning's DDP wrapper
        return self._reducer

    def _boundary(self, *mems: torch.Tensor):
        """Memory hand-off encoder(s) -> [mixer ->] decoder: when backward gets here every gradient of the decoder-side bucket
        is final."""
        if not torch.is_grad_enabled():
            return mems[0] if len(mems) == 1 else mems
        from .ddp import GradBoundary      # without a reducer the node only starts the decoder's collected weight gradients (runtime.WgradStream)
        return GradBoundary.apply(self._reducer, (1,), *mems)

    def _pack_encode(self, enc: Encoder, pos: "PositionalEncoding2D", x: torch.Tensor, sizes: torch.Tensor) -> Tuple[torch.Tensor, List[int], torch.Tensor]:
        """Ragged batch through one encoder: x [B, C, Hmax, Wmax] with sample b's sizes[b] = (h_b, w_b) pixels in the top-left corner ->
        (memory [B, Smax, d], [S_b], S_b int32 on the device) with S_b = ceil(h_b / 16) * ceil(w_b / 8).  encoder -> 2-D PE on the
        padded grid -> pack.  The extents of all resolutions are computed and uploaded once (Encoder.extent_table)."""
        flat = self.ensure_flat()
        if sizes.dim() != 2 or sizes.shape != (x.shape[0], 2):
            raise ValueError(f"per-sample sizes must be [B, 2] (height, width), got {tuple(sizes.shape)} for a batch of {x.shape[0]}")
        x = x.to(flat.device, non_blocking=True)
        table = enc.extent_table(sizes, flat.device)
        grid, grid_dev = table.host[-1], table.dev[-1]                            # int32 [B, 2]: each sample's feature grid
        lens = (grid[:, 0].long() * grid[:, 1].long()).tolist()
        self._memory_grid = (grid_dev, grid)                                      # what the CTC head's frame order needs (Transformer._ctc_logits)
        f = enc.forward_nhwc(x, flat.compute_dtype, extents=table).permute(0, 3, 1, 2)
        f = pos(f).permute(0, 2, 3, 1)                                            # NHWC again (a view of the PE kernel's output)
        mem = Fn.PackMemoryFn.apply(f, grid_dev, max(lens))
        return mem, lens, grid_dev[:, 0] * grid_dev[:, 1]

    def configure_optimizers(self):
        """torch.optim.Adam(lr=1e-4, amsgrad=False) over all parameters (model.py:134-139,475-483) as ONE fused kernel."""
        return self.make_optimizer(lr=1e-4)

    def _i2w(self, token: int) -> str:
        d = self.i2w
        return d[token] if token in d else d[str(token)]

    @torch.no_grad()
    def _greedy(self, memory: torch.Tensor, want_probs: bool = False, use_cache: bool = True, chunk: int = 16):
        """Autoregressive loop of validation_step / get_pred_seq_and_pred_prob_seq (model.py:182-193,247-260):
        bs=1, memory_len=None, argmax of the last-step logits, stop after <eos> or max_seq_len tokens.
        use_cache=True runs the KV-cached native executor (Decoder.decode_tokens: `chunk` tokens per host call, the chosen
        token chained to the next position on the device; the host reads a chunk back at a time and cuts the sequence after
        <eos>, so at most chunk - 1 positions are computed in vain); use_cache=False re-runs the whole prefix each step
        exactly like the reference.  Both give the same tokens (tests/test_model_gpu.py)."""
        if use_cache:
            ids, top1 = self._greedy_state(self.decoder.init_decode(memory), chunk, want_probs)
            return [self._i2w(t) for t in ids[0]], top1[0]
        if active_grammar(self) is not None:
            raise ValueError("a grammar constrains the KV-cached decode only: the pick of the full re-run is not on the device")
        y_in = torch.full((1, 1), self.w2i[SOS_TOKEN], dtype=torch.int64, device=memory.device)
        yhat: List[str] = []
        probs: List[float] = []
        for _ in range(self.max_seq_len):
            logits = self.decoder(tgt=y_in, memory=memory, memory_len=None)   # [1, V, t]
            last = logits[0, :, -1]
            last32 = K.cast(last.contiguous(), torch.float32) if last.dtype != torch.float32 else last.contiguous()
            idx, val = K.argmax(last32)
            token = int(idx.item())
            word = self._i2w(token)
            yhat.append(word)
            if want_probs:
                probs.append(float(val.item()))
            if word == EOS_TOKEN:
                break
            y_in = torch.cat([y_in, idx.view(1, 1)], dim=1)
        return yhat, probs

    @grammar_option
    @torch.no_grad()
    def greedy_batch(self, memory, sync_every: int = 8) -> List[List[str]]:
        """KV-cached greedy decode of B inputs at once (the reference loops bs = 1,
        model.py:182-193).  Rows of the batch never interact, so each sequence equals what `_greedy` returns for that sample
        alone (tests/test_model_gpu.py).  `memory` [B, S, d]: same-sized inputs.  A LIST of memories ([1, S_b, d] or [S_b, d])
        of different lengths -- padding would change the encoder features, so the reference pads nothing at inference -- is
        decoded as one ragged state (tests/test_ragged_decode_gpu.py); memories of at most 64 tokens go through `_greedy`.
        Returns one word list per memory, in input order.  The host reads the chosen tokens back every `sync_every` steps only.
        Keyword `grammar` (evaluation.grammar_option): every pick is the best token the automaton allows (`_greedy_state`)."""
        if not isinstance(memory, (list, tuple)):
            return self._words(self._greedy_state(self.decoder.init_decode(memory), sync_every)[0])
        mems = self.decoder.memory_list(memory)
        out: List[Optional[List[str]]] = [None] * len(mems)
        batched = []
        for i, m in enumerate(mems):
            if takes_ragged_state(m.shape[0]):
                batched.append(i)
            else:                                        # alone, such a memory takes another attention kernel: decode it alone
                out[i] = self._greedy(m.unsqueeze(0))[0]
        if batched:
            state = self.decoder.init_decode([mems[i] for i in batched])
            for i, seq in zip(batched, self._words(self._greedy_state(state, sync_every)[0])):
                out[i] = seq
        return out

    def _words(self, seqs: List[List[int]]) -> List[List[str]]:
        return [[self._i2w(t) for t in seq] for seq in seqs]

    def _greedy_state(self, state, sync_every: int, want_probs: bool = False):
        """Greedy decode of every row of a decode state at position 0 (evaluation.decode_rows): -> (token ids, top-1 logits)
        per row, each cut after its <eos> or max_seq_len tokens.  The logits (want_probs; else empty lists) are the floats
        get_pred_seq_and_pred_prob_seq returns for that row alone.  Under a grammar (evaluation.active_grammar) every pick is
        the largest logit among the tokens the automaton allows in the row's state, that logit is the value returned, and the
        states advance on the device (DecodeState.constrain); a row that reaches max_seq_len before an accepting state returns a
        valid prefix."""
        gstate = state.constrain(active_grammar(self))
        tok = torch.full((state.B, 1), self.w2i[SOS_TOKEN], dtype=torch.int64, device=state.tok.device)

        def step(n: int):
            nonlocal tok
            toks, top1 = self.decoder.decode_tokens(tok, state, n)   # n positions, tokens chained on the device
            tok = toks[-1].view(-1, 1)
            top1_h = top1.cpu().tolist() if want_probs else None
            return toks.cpu().tolist(), top1_h                        # one device sync for the whole chunk

        return decode_rows(step, state.B, self.w2i[EOS_TOKEN], self.max_seq_len, sync_every, want_probs, gstate)

    def _greedy_stream(self, mems: List[torch.Tensor], rows: int, want_probs: bool = False):
        """Greedy decode of memories that all take a ragged state through ONE decode state of `rows` slots, a finished row's
        slot going to the next memory (Decoder.init_slot_decode, evaluation.decode_stream): -> (token ids, top-1 logits) per
        memory, in the order given, each what `_greedy_state` of that memory alone returns."""
        mems = self.decoder.memory_list(mems)
        lens = [m.shape[0] for m in mems]
        state = self.decoder.init_slot_decode(min(rows, len(mems)), max(lens), mems[0].device, self.w2i[SOS_TOKEN])
        if self._refill_state_hook is not None:
            self._refill_state_hook(state)
        gstate = state.constrain(active_grammar(self))

        def admit(slot: int, i: Optional[int]) -> None:
            state.admit(slot, None if i is None else mems[i])

        def step(n: int):
            toks, top1 = state.run_rows(n)
            top1_h = top1.cpu().tolist() if want_probs else None
            return toks.cpu().tolist(), top1_h                        # one device sync for the whole chunk

        return decode_stream(step, admit, stream_order(lens), state.B, self.w2i[EOS_TOKEN], self.max_seq_len, self._refill_sync_every, want_probs,
                             gstate)

    def _greedy_spec(self, mems: List[torch.Tensor], draft_mems: List[torch.Tensor], spec, want_probs: bool = False):
        """Speculative greedy decode of memories that all take a ragged state (Decoder.init_spec_decode, evaluation.decode_spec):
        spec.draft's decoder proposes spec.k tokens per cycle over its own memories, this model's decoder verifies them in one
        grouped position -> (token ids, top-1 logits) per memory, each what `_greedy_state` of that memory alone returns.  Adds the
        device totals to `last_spec_stats`."""
        state = self.decoder.init_spec_decode(spec.draft.decoder, mems, draft_mems, spec.k, self.w2i[SOS_TOKEN], self.w2i[EOS_TOKEN],
                                              max_out=self.max_seq_len)
        tok0, top0 = state.start()
        first = (tok0.cpu().tolist(), top0.cpu().tolist() if want_probs else None)
        lens = [1] * state.B

        def cycles(n: int, t_max: int):
            state.run_cycles(n, t_max)
            snap = state.snapshot()                                   # one device sync for the whole chunk
            new_t, new_v = [], []
            for b in range(state.B):
                n_b = int(snap["out_len"][b])
                new_t.append(snap["out_tokens"][b, lens[b]:n_b].tolist())
                new_v.append(snap["out_top1"][b, lens[b]:n_b].tolist() if want_probs else None)
                lens[b] = n_b
            cycles.totals = snap["totals"]
            return new_t, new_v

        def plain(n: int, pos: List[int]):
            toks, top1 = state.plain(n, pos)
            return toks.cpu().tolist(), top1.cpu().tolist() if want_probs else None

        cycles.totals = (0, 0)
        out, values = decode_spec(first, cycles, plain, state.B, self.w2i[EOS_TOKEN], self.max_seq_len, state.R, self._spec_sync_every, want_probs)
        stats = self.last_spec_stats if self.last_spec_stats is not None else {"cycles": 0, "drafted": 0, "accepted": 0, "tokens": 0}
        stats["cycles"] += state.cycles
        stats["drafted"] += int(cycles.totals[0])
        stats["accepted"] += int(cycles.totals[1])
        stats["tokens"] += sum(len(seq) for seq in out)
        self.last_spec_stats = stats
        return out, values

    @torch.no_grad()
    def _predict(self, items: Iterable, encode: Callable[[object], torch.Tensor], batch_size: int, want_probs: bool = False):
        """Greedy predictions of inputs of any size, in input order, each equal to `_greedy` of that input alone.  A window
        of WINDOW_BATCHES * batch_size inputs at a time is encoded at batch size 1 (like validation_step), grouped by memory
        length (evaluation.plan_groups) and decoded group by group as ragged batches of up to batch_size rows.
        want_probs: -> (predictions, the top-1 logits of their positions) like `_greedy(..., want_probs=True)`.
        Called with a beam (`_beam_option`): the words of `beam_search` of every input instead, decoded
        batch_size // beam inputs at a time (`beam_search_batch`: a group has at most batch_size rows).
        Called with refill=True (evaluation.refill_option; greedy only): the memories of a window that take a ragged state stream through ONE decode state of
        min(batch_size, count) slots (`_greedy_stream`) instead of running group by group until each group's longest row ends;
        a decoder whose widths omr_decode_steps_rows does not take decodes in groups as without the flag.
        Called with grammar= (evaluation.grammar_option), or on a model with `decode_grammar`: every route above decodes under
        that automaton (grammar.Grammar); with None nothing is allocated or launched for it.  A prediction that reaches
        max_seq_len before an accepting state is a valid prefix.
        Called with draft= (evaluation.spec_option; greedy only): the draft encodes every input itself, and the inputs of which BOTH
        memories take a ragged state are decoded speculatively, group by group (`_greedy_spec`); the others go through `_greedy`.
        Same predictions and values."""
        if batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        beam = 1 if want_probs else self._decode_beam          # predict_with_probs takes no beam
        refill = refill_enabled()
        spec = active_spec()                                   # evaluation.check_draft has refused beam, refill and a grammar beside it
        if refill and beam > 1:
            raise ValueError("refill=True decodes greedily: the beam state (two caches, a history table) has no slots to refill")
        if beam > 1:
            rows = max(1, batch_size // beam)

            def decode_single(mem):
                return self.beam_search(mem, beam)[0], None        # with ctc_decode= (evaluation.ctc_decode_option): the joint search

            def decode_group(group):
                ctc = self._ctc_group(group) if active_ctc_decode() is not None else None
                return [(seq, None) for seq, _ in self._beam_state(group, beam, 8, ctc=ctc)]
        else:
            rows = batch_size

            def decode_single(mem):
                return self._greedy(mem, want_probs=want_probs)

            def decode_group(group):
                ids, top1 = self._greedy_state(self.decoder.init_decode(group), 8, want_probs)
                return zip(self._words(ids), top1)

        it = iter(items)
        preds: List[List[str]] = []
        probs: List[List[float]] = []
        while True:
            window = list(itertools.islice(it, WINDOW_BATCHES * batch_size))
            if not window:
                return (preds, probs) if want_probs else preds
            mems = [encode(x) for x in window]
            out: List[Optional[List[str]]] = [None] * len(mems)
            outp: List[Optional[List[float]]] = [None] * len(mems)
            if spec is not None:
                dmems = [spec.encode(x) for x in window]
                singles, groups = plan_pair_groups([m.shape[1] for m in mems], [m.shape[1] for m in dmems], rows)
                for g in groups:
                    ids, top1 = self._greedy_spec([mems[i] for i in g], [dmems[i] for i in g], spec, want_probs)
                    for i, seq, t1 in zip(g, self._words(ids), top1):
                        out[i], outp[i] = seq, t1
                groups = []
                del dmems
            else:
                singles, groups = plan_groups([m.shape[1] for m in mems], rows)
            for i in singles:
                out[i], outp[i] = decode_single(mems[i])
            if refill and groups and self.decoder.takes_slot_state(max(mems[i].shape[1] for g in groups for i in g)):
                rest = [i for g in groups for i in g]
                ids, top1 = self._greedy_stream([mems[i] for i in rest], rows, want_probs)
                for i, seq, t1 in zip(rest, self._words(ids), top1):
                    out[i], outp[i] = seq, t1
                groups = []
            for g in groups:                                   # planned: every memory of a group takes a ragged state
                for i, (seq, top1) in zip(g, decode_group([mems[i] for i in g])):
                    out[i], outp[i] = seq, top1
            preds += out
            probs += outp
            del mems

    @torch.no_grad()
    def _evaluate(self, batches: Iterable, inputs_of: Callable, batch_size: int) -> Dict[str, float]:
        """validation_step over `batches` + on_validation_epoch_end, decoded in ragged batches: the same metrics dict, without
        logging and without touching self.Y / self.YHat.  The counts go through metrics.ed_counts (compute_metrics_sharded
        combines them across ranks)."""
        truth: List[List[str]] = []

        def inputs():
            for batch in batches:
                y = batch[-1]
                assert y.size(0) == 1, "evaluate takes the batches of validation_step (batch_size = 1)"
                truth.append([self.ytest_i2w[i] for i in y[0][1:].tolist()])
                yield inputs_of(batch)

        preds = self._predict(inputs(), self._encode_input, batch_size)
        return compute_metrics(y_true=truth, y_pred=preds)

    @torch.no_grad()
    def _align(self, items: Iterable, sizes_of: Callable, words, batch_size: int, layers, return_maps: bool) -> List[Alignment]:
        """`align` of both model classes.  Every input is encoded at batch size 1 (`_encode_input`, like `_predict`); its words
        come from `_predict` (greedy) unless given; then ONE teacher-forced Decoder.cross_attention_maps pass per group of up to
        batch_size inputs (evaluation.plan_align_groups: memories padded with zeros to the group's longest behind a bool key
        mask, targets [<sos>] + ids[:-1] padded with the pad index) gives row t = the distribution of the position that predicts
        token t, and omr_argmax over the row's own S_b keys (first index on ties) the memory row it leaned on.  sizes_of(item) ->
        (sizes, split) of evaluation.cells_and_boxes."""
        was_training = self.training
        self.eval()
        try:
            items = list(items)
            mems = [self._encode_input(x) for x in items]
            if words is None:
                words = self._predict(range(len(mems)), lambda i: mems[i], batch_size)
            words = [list(w) for w in words]
            if len(words) != len(items):
                raise ValueError(f"align: {len(words)} word lists for {len(items)} inputs")
            ids = [[self.w2i[w] for w in seq] for seq in words]
            dev, sos, pad = mems[0].device if mems else None, self.w2i[SOS_TOKEN], self.padding_idx
            out: List[Optional[Alignment]] = [None] * len(items)
            for group in plan_align_groups([len(s) for s in ids], [m.shape[1] for m in mems], batch_size):
                group = [i for i in group if ids[i]]               # no tokens: nothing to align (an empty Alignment below)
                if not group:
                    continue
                tmax, smax = max(len(ids[i]) for i in group), max(mems[i].shape[1] for i in group)
                tgt = torch.full((len(group), tmax), pad, dtype=torch.int64)
                memory = torch.zeros((len(group), smax, mems[group[0]].shape[2]), dtype=mems[group[0]].dtype, device=dev)
                lens = torch.tensor([mems[i].shape[1] for i in group], dtype=torch.int64)
                for b, i in enumerate(group):
                    tgt[b, :len(ids[i])] = torch.tensor([sos] + ids[i][:-1], dtype=torch.int64)
                    memory[b, :mems[i].shape[1]] = mems[i][0]
                mask = None if bool((lens == smax).all()) else _pad_mask(smax, lens.to(dev))
                with torch.no_grad():
                    _, maps = self.decoder._cross_attention_maps(tgt.to(dev), memory, mask, layers, False)
                picks = [K.argmax(maps[b, :len(ids[i]), :mems[i].shape[1]]) for b, i in enumerate(group)]
                for b, (i, (idx, val)) in enumerate(zip(group, picks)):
                    sizes, split = sizes_of(items[i])
                    index = idx.cpu().numpy()
                    cell, box, source = cells_and_boxes(index, sizes, split)
                    own = maps[b, :len(ids[i]), :mems[i].shape[1]].contiguous() if return_maps else None
                    out[i] = Alignment(words=words[i], index=index, weight=val.cpu().numpy(), cell=cell, box=box, source=source, maps=own)
            for i, a in enumerate(out):
                if a is None:
                    cell, box, source = cells_and_boxes([], *sizes_of(items[i]))
                    out[i] = Alignment(words=words[i], index=np.zeros(0, np.int64), weight=np.zeros(0, np.float32), cell=cell, box=box,
                                       source=source, maps=None)
            return out
        finally:
            self.train(was_training)

    @ctc_decode_option(4, beam_at=1)
    @grammar_option
    @torch.no_grad()
    def beam_search(self, memory: torch.Tensor, beam: int = 4) -> Tuple[List[str], float]:
        """Beam-search decode of ONE input (BASELINE config C5; an extension -- the reference only decodes greedily).  The
        `beam` hypotheses are the batch rows of the KV-cached step; scores are sums of log-probabilities (no length
        normalisation); beam = 1 reproduces `_greedy` token for token.  Returns (words incl. <eos> if reached, score).
        Keyword `grammar` (evaluation.grammar_option): the logits of the tokens the automaton forbids in a hypothesis' state are
        -inf before the log-softmax, and a candidate the table forbids is dropped whatever its value.
        Keyword `ctc_decode` (evaluation.ctc_decode_option; Transformer with a CTC head, beam >= 2): the joint CTC / attention search.  Every
        candidate's value becomes fl32(fl32(wa * log-probability) + fl32(wc * delta)), delta its CTC prefix score against the hypothesis it
        extends (include/omr_hip.h, omr_ctc_prefix_scores; `memory` must be what `encode` returned: its grid travels with it); the candidate
        list, the order, the walk and the stop rule stay.  This loop is the yardstick of the batched route."""
        assert memory.shape[0] == 1 and beam >= 1
        ctc = None
        if active_ctc_decode() is not None:
            ctc = K.CtcPrefixBlock(*self._ctc_group([memory]), len(self.w2i), beam, blank=self.padding_idx, sos=self.w2i[SOS_TOKEN],
                                   eos=self.w2i[EOS_TOKEN], weight=active_ctc_decode())
        grammar = active_grammar(self)
        gstates = [grammar.start] * beam if grammar is not None else None
        sos, eos = self.w2i[SOS_TOKEN], self.w2i[EOS_TOKEN]
        dev = memory.device
        state = self.decoder.init_decode(memory)
        state.share_memory_between(beam)                     # every hypothesis reads the same memory K|V; own self-attention cache rows
        tok = torch.full((beam, 1), sos, dtype=torch.int64, device=dev)
        scores = [0.0] + [float("-inf")] * (beam - 1)       # only the first row is a real hypothesis before the first step
        seqs: List[List[int]] = [[] for _ in range(beam)]
        best_done: Tuple[float, Optional[List[int]]] = (float("-inf"), None)
        exhausted = True                                     # the loop ran out of positions with hypotheses still alive
        for pos in range(self.max_seq_len):
            logits = self.decoder.decode_step(tok, state)
            logits = logits if logits.dim() == 2 else logits.view(1, -1)
            if grammar is not None:
                logits = logits.masked_fill(~host_mask(grammar, gstates, logits.device), float("-inf"))
            idx, val = K.topk_logprob(logits.contiguous(), beam)
            if ctc is not None:                                       # the mix of omr_beam_select_ctc, in numpy float32: two products, one add
                wa, wc = (np.float32(w) for w in K.ctc_mix_weights(ctc.weight))
                with np.errstate(invalid="ignore"):
                    val = torch.from_numpy(wa * val.cpu().numpy() + wc * ctc.scores(pos & 1, idx).cpu().numpy())
            idx_h, val_h = idx.cpu().tolist(), val.cpu().tolist()
            cands = [(scores[b] + val_h[b][j], b, idx_h[b][j]) for b in range(beam) if scores[b] > float("-inf") for j in range(beam)]
            if grammar is not None:
                cands = [c for c in cands if grammar.walk([c[2]], gstates[c[1]])[0] >= 0]
            cands.sort(key=lambda c: (-c[0], c[1], c[2]))
            parents, new_tok, new_scores, new_seqs = [], [], [], []
            for sc, b, t in cands:
                if t == eos:
                    if sc > best_done[0]:
                        best_done = (sc, seqs[b] + [t])
                    continue
                parents.append(b); new_tok.append(t); new_scores.append(sc); new_seqs.append(seqs[b] + [t])
                if len(parents) == beam:
                    break
            if not parents or new_scores[0] <= best_done[0]:        # scores only fall: no live hypothesis can overtake the best finished one
                exhausted = False
                break
            while len(parents) < beam:                                # pad with dead rows
                parents.append(parents[0]); new_tok.append(new_tok[0]); new_scores.append(float("-inf")); new_seqs.append([])
            pidx = torch.tensor(parents, dtype=torch.int64, device=dev)
            state.reorder_rows(pidx)
            tok = torch.tensor(new_tok, dtype=torch.int64, device=dev).view(beam, 1)
            scores, seqs = new_scores, new_seqs
            if ctc is not None:                                       # the survivors' prefix states, into the other parity
                ctc.advance(pos & 1, pidx.to(torch.int32), tok.view(-1))
            if grammar is not None:
                gstates = [grammar.walk([t], gstates[b])[0] for b, t in zip(parents, new_tok)]
        if exhausted and scores[0] > best_done[0]:
            best_done = (scores[0], seqs[0])                          # ran out of length: the best unfinished hypothesis wins
        if ctc is not None and best_done[1] is None:
            best_done = (scores[0], seqs[0])                          # a dead end: no label fits the frames left and <eos> was no candidate
        return [self._i2w(t) for t in best_done[1]], best_done[0]

    @ctc_decode_option(4, beam_at=1)
    @grammar_option
    @torch.no_grad()
    def beam_search_batch(self, memories, beam: int = 4, sync_every: int = 8) -> List[Tuple[List[str], float]]:
        """`beam_search` of N inputs at once, on the device (Decoder.init_beam_decode; csrc/decode.hip omr_beam_decode_steps):
        -> [(words, score)] in input order, each exactly what `beam_search(memory, beam)` returns for that input alone
        (tests/test_beam_batch_gpu.py).  memories: a list of [1, S_b, d] / [S_b, d] of different lengths.  The selection, the
        scores and the cache reorder stay on the device; the host reads the `done` flags every `sync_every` positions only
        and the whole state once at the end.  Memories of at most 64 or more than 16 384 tokens go through `beam_search`.
        Keyword `grammar` (evaluation.grammar_option): the constrained selection (omr_beam_decode_steps_grammar).
        Keyword `ctc_decode` (evaluation.ctc_decode_option): the joint CTC / attention search of `beam_search`, on the device
        (omr_beam_decode_steps_ctc); the memories must be what `encode` returned ([1, S_b, d] each)."""
        if not 1 <= beam <= MAX_BEAM:
            raise ValueError(f"beam must be in 1..{MAX_BEAM}, got {beam}")
        if sync_every < 1:
            raise ValueError(f"sync_every must be >= 1, got {sync_every}")
        joint = active_ctc_decode() is not None
        if joint:
            memories = list(memories)                    # the CTC head reads each memory as `encode` returned it, grid attached
        mems = self.decoder.memory_list(memories, refuse_long=False)
        out: List[Optional[Tuple[List[str], float]]] = [None] * len(mems)
        batched = []
        for i, m in enumerate(mems):
            if takes_ragged_state(m.shape[0]):
                batched.append(i)
            else:                                        # alone, such a memory takes another attention kernel: search it alone
                out[i] = self.beam_search(memories[i] if joint else m.unsqueeze(0), beam)
        if batched:
            ctc = self._ctc_group([memories[i] for i in batched]) if joint else None
            for i, result in zip(batched, self._beam_state([mems[i] for i in batched], beam, sync_every, ctc=ctc)):
                out[i] = result
        return out

    def _ctc_group(self, memories):
        """For the joint CTC / attention search: the CTC head's logits of every memory of a group, each computed from that memory alone as
        `encode` returned it (batch size 1, its own dense grid), copied into ONE zeroed buffer [N, Fmax, round_up(V, 8)] -> (its
        [N, Fmax, V] view, frame counts int32 [N]): what BeamDecodeState.attach_ctc takes.  A group of one goes the same way, so the
        per-input loop and the batched state read the same bits."""
        parts = [self._ctc_logits_of(m) for m in memories]
        V, fmax = len(self.w2i), max(lg.shape[1] for lg, _ in parts)
        buf = torch.zeros((len(parts), fmax, K.round_up(V, 8)), dtype=parts[0][0].dtype, device=parts[0][0].device)
        for n, (lg, _) in enumerate(parts):
            buf[n, :lg.shape[1], :V] = lg[0]
        return buf[:, :, :V], torch.cat([fl for _, fl in parts])

    def _ctc_logits_of(self, memory: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        raise ValueError("ctc_decode= is for Transformer: this model has no CTC head")

    def _beam_state(self, mems, beam: int, sync_every: int, ctc=None) -> List[Tuple[List[str], float]]:
        """The search of `beam_search_batch` over memories that all take a ragged state: one BeamDecodeState, run to the end.
        ctc: `_ctc_group` of these memories for the joint search (None: the attention scores alone)."""
        state = self.decoder.init_beam_decode(mems, beam, sos=self.w2i[SOS_TOKEN], eos=self.w2i[EOS_TOKEN])
        state.constrain(active_grammar(self))
        if ctc is not None:
            state.attach_ctc(*ctc, active_ctc_decode())
        left = self.max_seq_len
        while left > 0:
            n = min(sync_every, left)
            state.run(n)
            left -= n
            if left > 0 and all(state.done()):                # one small device sync per chunk
                break
        return [([self._i2w(t) for t in seq], score) for seq, score in state.results()]

    @torch.no_grad()
    def test_step(self, batch, batch_idx) -> None:
        self.validation_step(batch, batch_idx)

    @torch.no_grad()
    def on_validation_epoch_end(self, name: str = "val", print_random_samples: bool = False) -> Dict[str, float]:
        # data-parallel evaluation: each rank decoded its shard; the edit-distance counts are all-reduced (metrics.py)
        metrics = compute_metrics_sharded(self.Y, self.YHat) if self._reducer is not None else compute_metrics(y_true=self.Y, y_pred=self.YHat)
        for k, v in metrics.items():
            self.log(f"{name}_{k}", v, prog_bar=True, logger=True, on_epoch=True)
        if print_random_samples:
            index = random.randint(0, len(self.Y) - 1)
            print(f"Ground truth - {self.Y[index]}")
            print(f"Prediction - {self.YHat[index]}")
        self.Y.clear()
        self.YHat.clear()
        return metrics

    @torch.no_grad()
    def on_test_epoch_end(self) -> Dict[str, float]:
        return self.on_validation_epoch_end(name="test", print_random_samples=True)


##################################################################### UNIMODAL TRANSFORMER


class Transformer(_Base):
    """model.py:54-262."""

    def __init__(self, max_input_height: int, max_input_width: int, max_seq_len: int, w2i: Dict[str, int], i2w: Dict[int, str],
                 ytest_i2w: Optional[Dict[int, str]] = None, attn_window: int = -1, teacher_forcing_prob: float = 0.5,
                 config: Optional[ModelConfig] = None) -> None:
        super().__init__()
        self.save_hyperparameters()
        self._common_init(w2i, i2w, ytest_i2w, max_seq_len, attn_window, teacher_forcing_prob, config)
        self.max_input_height, self.max_input_width = max_input_height, max_input_width
        c = self.config
        self.encoder = Encoder(in_channels=NUM_CHANNELS, dropout=c.encoder_dropout, out_channels=c.d_model)
        self.pos_2d = PositionalEncoding2D(num_channels=c.d_model, max_height=math.ceil(max_input_height / HEIGHT_REDUCTION),
                                           max_width=math.ceil(max_input_width / WIDTH_REDUCTION), dropout_p=c.dropout)
        self.decoder = self._make_decoder()
        if self.ctc_weight > 0:        # after the decoder: its parameters close the decoder-side range of the flat buffers (attach_reducer)
            self.ctc_head = Linear(c.d_model, len(w2i))

    def encode(self, x: torch.Tensor) -> torch.Tensor:
        """encoder -> 2-D PE -> flatten -> [B, S, d] (model.py:143-147,176-180)."""
        flat = self.ensure_flat()
        x = x.to(flat.device, non_blocking=True)
        f = self.encoder.forward_nhwc(x, flat.compute_dtype).permute(0, 3, 1, 2)
        self._memory_grid = (None, (f.shape[2], f.shape[3]))       # every sample's grid is the whole plane
        mem = self._boundary(_flatten_memory(self.pos_2d(f)))
        if self.ctc_weight > 0:
            mem.ctc_grid = self._memory_grid[1]                    # travels with the memory: `predict` encodes many before it decodes one (`_ctc_logits_of`)
        return mem

    def _encode_packed(self, x: torch.Tensor, sizes: torch.Tensor) -> Tuple[torch.Tensor, List[int], torch.Tensor]:
        """Ragged batch: x [B, C, Hmax, Wmax] with sample b's sizes[b] = (h_b, w_b) pixels in the top-left corner -> (memory
        [B, Smax, d], [S_b], S_b on the device) with S_b = ceil(h_b / 16) * ceil(w_b / 8): rows [0, S_b) of sample b are `encode` of b
        alone (to rounding: the InstanceNorm sums are added in another order), the rows behind them zeros.  encoder -> 2-D PE on the
        padded grid -> pack.  The extents of all resolutions are computed and uploaded once (Encoder.extent_table)."""
        mem, lens, lens_dev = self._pack_encode(self.encoder, self.pos_2d, x, sizes)
        return self._boundary(mem), lens, lens_dev

    @torch.no_grad()
    def encode_ragged(self, x: torch.Tensor, sizes: torch.Tensor) -> List[torch.Tensor]:
        """Memories [S_b, d] of a padded batch of inputs of different sizes (`image.collate_ragged`), one encoder pass for all:
        each equals `encode` of that input alone to rounding (not bit for bit: `predict` / `evaluate` keep the batch-size-1 encoder)."""
        mem, lens, _ = self._encode_packed(x, sizes)
        return [mem[b, :n] for b, n in enumerate(lens)]

    def forward(self, x: torch.Tensor, xl: torch.Tensor, y_in: torch.Tensor) -> torch.Tensor:
        """xl as the decoder's memory_len, the reference's forms (every sample fills the plane of x): None, integer lengths [B], or a bool
        key-padding mask [B, S].  An INTEGER xl of shape [B, 2] -- never a valid memory_len -- holds the (height, width) in pixels
        of each sample's content in the top-left corner of x and takes the ragged route: sample b's logits, loss share and gradients are
        those of b run alone at its own size; the memory rows past a sample's own length are masked out (-inf)."""
        return self._forward_memory(x, xl, y_in)[0]

    def _forward_memory(self, x: torch.Tensor, xl: torch.Tensor, y_in: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """`forward` -> (logits, the memory the decoder read): what `training_step` hands the CTC head."""
        if self._is_pixel_sizes(xl):
            mem, _, lens_dev = self._encode_packed(x, xl)
            return self.decoder(tgt=y_in, memory=mem, memory_len=_pad_mask(mem.shape[1], lens_dev)), mem     # bool [B, Smax]: True = no key
        mem = self.encode(x)
        return self.decoder(tgt=y_in, memory=mem, memory_len=xl), mem     # host-resident ids / lengths go as they are: the decoder reads them before the copy

    def _ctc_logits(self, mem: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The CTC head on the memory `encode` / `_encode_packed` returned last: memory -> time-ordered frames (each sample's grid column by
        column, ctc_pool grid rows averaged per frame) -> head -> (logits [B, F, V] at a row pitch of round_up(V, 8), frame counts int32 [B])."""
        if self.ctc_weight <= 0:
            raise ValueError("this model has no CTC head: build it with ModelConfig(ctc_weight > 0)")
        grid_dev, grid = self._memory_grid
        if grid_dev is None:
            gh, gw = grid
            fmax = K.ctc_frame_count(gh, gw, self.ctc_pool)
        else:
            gh = gw = 0
            fmax = max(K.ctc_frame_count(h, w, self.ctc_pool) for h, w in grid.tolist())
        frames, frame_len = Fn.CTCFramesFn.apply(mem, grid_dev, gh, gw, self.ctc_pool, fmax)
        V = len(self.w2i)
        return Fn.linear(frames, self.ctc_head.weight, self.ctc_head.bias, out_ld=K.round_up(V, 8)), frame_len

    def _ctc_logits_of(self, memory: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """`_ctc_logits` of ONE memory [1, S, d] by the grid `encode` attached to it, whatever was encoded since."""
        grid = getattr(memory, "ctc_grid", None)
        if grid is None or memory.dim() != 3 or memory.shape[0] != 1:
            raise ValueError("ctc_decode= takes memories as `encode` returned them ([1, S, d], one input each): a slice or a copy has lost its grid")
        before, self._memory_grid = getattr(self, "_memory_grid", None), (None, grid)
        try:
            return self._ctc_logits(memory.contiguous())
        finally:
            self._memory_grid = before

    _is_pixel_sizes = staticmethod(_is_pixel_sizes)

    def apply_teacher_forcing(self, y: torch.Tensor) -> torch.Tensor:
        """model.py:152-160: each non-pad token is replaced w.p. teacher_forcing_prob by randint(0, V-1) drawn
        from Python's `random` in row-major order (same draw sequence as the reference's double loop)."""
        out = y.detach().to("cpu", torch.int64).contiguous().clone()
        # The B x T double loop runs in C on the interpreter's OWN generator state (omr_teacher_forcing_noise: the calls
        # CPython's random.random / random.randint would make, in the reference's order), 1.8 ms -> 0.2 ms per C2 step.
        version, internal, gauss = random.getstate()
        state = (ctypes.c_uint * 624)(*internal[:624])
        index = ctypes.c_int(internal[624])
        lib().call("omr_teacher_forcing_noise", out.data_ptr(), out.numel(), float(self.teacher_forcing_prob), int(self.padding_idx), len(self.w2i),
                   ctypes.cast(state, ctypes.c_void_p), ctypes.byref(index))
        random.setstate((version, tuple(state) + (index.value,), gauss))
        out = out.to(y.dtype)
        return out.pin_memory() if (not y.is_cuda and torch.cuda.is_available()) else out.to(y.device)

    _distillation = None      # distill.Distillation: the teachers `training_step` distils from (set_distillation); never a sub-module

    def set_distillation(self, distillation) -> None:
        """Attaches a distill.Distillation (training_step then trains towards its teachers) or, with None, detaches it.  The teachers do not
        become sub-modules.  ValueError when a teacher's vocabulary differs or the model smooths its labels."""
        if distillation is not None:
            if self.ctc_weight > 0:
                raise ValueError("distillation and the CTC head do not combine: train with ctc_weight = 0 or without teachers")
            distillation.attach(self)
        self._distillation = distillation

    def _distillation_step(self, batch) -> torch.Tensor:
        """training_step with teachers: y_in is noised once, and the student and every teacher decode from that same y_in."""
        d = self._distillation
        (x, xl), y_in, y_out, calls = d.split(batch)
        y_in = self.apply_teacher_forcing(y_in)
        teachers = d.teacher_logits(calls, y_in)          # before the student's forward: nothing of theirs runs between it and its backward
        yhat = self.forward(x=x, xl=xl, y_in=y_in)
        loss = d.loss(yhat, _to_dev(y_out, yhat.device), teachers)
        self.log("train_loss", loss, prog_bar=True, logger=True, on_epoch=True)
        self.log("train_nll", d.loss.last_nll, prog_bar=True, logger=True, on_epoch=True)
        self.log("train_kd", d.loss.last_kd, prog_bar=True, logger=True, on_epoch=True)
        return loss

    def training_step(self, batch, batch_idx) -> torch.Tensor:
        if self._distillation is not None:
            return self._distillation_step(batch)
        x, xl, y_in, y_out = batch
        y_in = self.apply_teacher_forcing(y_in)
        if self.ctc_weight > 0:
            return self._ctc_step(x, xl, y_in, y_out)
        yhat = self.forward(x=x, xl=xl, y_in=y_in)
        loss = self.compute_loss(yhat, _to_dev(y_out, yhat.device))
        self.log("train_loss", loss, prog_bar=True, logger=True, on_epoch=True)
        if self.compute_loss.label_smoothing > 0:      # the un-smoothed mean: comparable between runs that smooth differently
            self.log("train_nll", self.compute_loss.last_nll, prog_bar=True, logger=True, on_epoch=True)
        return loss

    last_ctc = None           # (loss, rows [B], infeasible [1]) of the last `_ctc_step`: detached device tensors (no sync)

    def _ctc_step(self, x, xl, y_in, y_out) -> torch.Tensor:
        """training_step with the CTC head: loss = (1 - w) CE + w CTC, both against y_out (the CTC labels end in front of <eos>), the CTC
        part on the memory the decoder read.  Label smoothing applies to the CE part only."""
        yhat, mem = self._forward_memory(x, xl, y_in)
        y_dev = _to_dev(y_out, yhat.device)
        ce = self.compute_loss(yhat, y_dev)
        logits, frame_len = self._ctc_logits(mem)
        ctc, rows, infeasible = Fn.ctc_loss(logits, frame_len, y_dev, self.padding_idx, self.w2i[EOS_TOKEN])
        w = self.ctc_weight
        loss = (1.0 - w) * ce + w * ctc
        self.last_ctc = (ctc.detach(), rows, infeasible)
        self.log("train_loss", loss, prog_bar=True, logger=True, on_epoch=True)
        self.log("train_ce", ce.detach(), prog_bar=True, logger=True, on_epoch=True)
        self.log("train_ctc", ctc.detach(), prog_bar=True, logger=True, on_epoch=True)
        self.log("ctc_infeasible", infeasible, prog_bar=False, logger=True, on_epoch=True)
        if self.compute_loss.label_smoothing > 0:
            self.log("train_nll", self.compute_loss.last_nll, prog_bar=True, logger=True, on_epoch=True)
        return loss

    @torch.no_grad()
    def predict_ctc(self, xs: Iterable[torch.Tensor], batch_size: int = 32) -> List[List[str]]:
        """The encoder-only transcript of inputs [1, C, H_b, W_b] (or [C, H_b, W_b]) of any size, in input order: batch_size inputs at a time
        through the ragged batch encoder (`collate_ragged` + `_encode_packed`), the CTC head, and the arg-max path with repeats collapsed and
        blanks dropped (kernels.ctc_greedy) -- no decoder, no decode loop; the host reads tokens and lengths once per batch."""
        if self.ctc_weight <= 0:
            raise ValueError("this model has no CTC head: build it with ModelConfig(ctc_weight > 0)")
        if batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        from .image import collate_ragged
        was_training = self.training
        self.eval()
        out: List[List[str]] = []
        try:
            it = iter(xs)
            while True:
                group = [x[0] if x.dim() == 4 else x for x in itertools.islice(it, batch_size)]
                if not group:
                    break
                x, sizes = collate_ragged(group)
                mem, _, _ = self._encode_packed(x, sizes)
                logits, frame_len = self._ctc_logits(mem)
                tokens, lengths, _, _ = K.ctc_greedy(logits, frame_len, len(self.w2i), self.padding_idx)
                tokens, lengths = tokens.cpu(), lengths.cpu().tolist()
                out.extend(self._words([tokens[b, :n].tolist() for b, n in enumerate(lengths)]))
        finally:
            self.train(was_training)
        return out

    @torch.no_grad()
    def evaluate_ctc(self, batches: Iterable, batch_size: int = 32) -> Dict[str, float]:
        """The metrics of `evaluate` (sym-er / seq-er) with `predict_ctc`'s transcripts as predictions.  The truth of a batch ends in front
        of its <eos>: the CTC path emits none."""
        if self.ctc_weight <= 0:
            raise ValueError("this model has no CTC head: build it with ModelConfig(ctc_weight > 0)")
        truth: List[List[str]] = []

        def inputs():
            for batch in batches:
                y = batch[-1]
                assert y.size(0) == 1, "evaluate_ctc takes the batches of validation_step (batch_size = 1)"
                words = [self.ytest_i2w[i] for i in y[0][1:].tolist()]
                truth.append(words[:words.index(EOS_TOKEN)] if EOS_TOKEN in words else words)
                yield batch[0]

        preds = self.predict_ctc(inputs(), batch_size)
        return compute_metrics(y_true=truth, y_pred=preds)

    @torch.no_grad()
    def validation_step(self, batch, batch_idx) -> None:
        x, y = batch
        assert x.size(0) == y.size(0) == 1, "Inference only supports batch_size = 1"
        yhat, _ = self._greedy(self.encode(x))
        self.Y.append([self.ytest_i2w[i.item()] for i in y[0][1:]])
        self.YHat.append(yhat)

    @torch.no_grad()
    def get_pred_seq_and_pred_prob_seq(self, x: torch.Tensor) -> Tuple[List[str], List[float]]:
        """model.py:226-262 (returns the top-1 LOGIT as "probability", like the reference)."""
        assert x.size(0) == 1, "Inference only supports batch_size = 1"
        return self._greedy(self.encode(x), want_probs=True)

    def _encode_input(self, x: torch.Tensor) -> torch.Tensor:
        assert x.size(0) == 1, "predict takes inputs of batch size 1 ([1, C, H, W]); their sizes may differ"
        return self.encode(x)

    @ctc_decode_option(1)
    @spec_option
    @grammar_option
    @refill_option
    @_beam_option
    @torch.no_grad()
    def predict(self, xs: Iterable[torch.Tensor], batch_size: int = 32) -> List[List[str]]:
        """Greedy predictions of inputs [1, C, H_b, W_b] of any size, in input order: each equals validation_step's decode
        of that input, decoded batch_size memories at a time.  Keyword `beam` (2 .. 8, `_beam_option`): the words of
        `beam_search` of each input, batch_size // beam inputs at a time.  Keyword `refill` (default False, `refill_option`;
        greedy only): continuous batching, a finished row's slot goes to the next input (`_predict`); same predictions.
        Keywords `draft`, `draft_len` (evaluation.spec_option; also on `predict_with_probs` and `evaluate`): speculative decoding, a
        cheaper model with this model's vocabulary proposes `draft_len` tokens per pass of this one; same predictions and values;
        `last_spec_stats` holds the call's cycles and proposals made / accepted."""
        return self._predict(xs, self._encode_input, batch_size)

    @spec_option
    @grammar_option
    @refill_option
    @torch.no_grad()
    def predict_with_probs(self, xs: Iterable[torch.Tensor], batch_size: int = 32) -> Tuple[List[List[str]], List[List[float]]]:
        """get_pred_seq_and_pred_prob_seq (model.py:226-262) of inputs [1, C, H_b, W_b] of any size, decoded batch_size
        memories at a time: (words, top-1 logits) per input, in input order, each equal to the batch-size-1 call's.
        Keyword `refill` (default False, `refill_option`): continuous batching (`_predict`), same values.
        Keyword `grammar` (evaluation.grammar_option): the values are the top-1 ALLOWED logits."""
        return self._predict(xs, self._encode_input, batch_size, want_probs=True)

    @ctc_decode_option(1)
    @spec_option
    @grammar_option
    @refill_option
    @_beam_option
    @torch.no_grad()
    def evaluate(self, batches: Iterable, batch_size: int = 32) -> Dict[str, float]:
        """The metrics of validation_step over `batches` ((x, y) each) followed by on_validation_epoch_end, decoded in batches.
        Keyword `beam` (2 .. 8, `_beam_option`): the predictions are those of `beam_search`.  Keyword `refill` (default False,
        `refill_option`; greedy only): continuous batching (`_predict`), same metrics."""
        return self._evaluate(batches, lambda batch: batch[0], batch_size)

    modality = "image"        # what this model's one encoder reads ("audio" for an A2S model): the `source` of its alignments

    def align(self, xs: Iterable[torch.Tensor], words: Optional[List[List[str]]] = None, batch_size: int = 32, layers=None,
              return_maps: bool = False) -> List[Alignment]:
        """Where the decoder looked: one evaluation.Alignment per input [1, C, H_b, W_b], in input order -- per token of `words`
        (default: `predict`'s greedy words of that input) the memory row with the largest cross-attention weight (heads and the
        decoder layers `layers` averaged; default all), its cell of the encoder grid and its box in input pixels (`_align`)."""
        return self._align(xs, lambda x: (((self.modality, x.shape[-2], x.shape[-1]),), None), words, batch_size, layers, return_maps)


##################################################################### MULTIMODAL TRANSFORMER


class CrossAttention(nn.Module):
    """model.py:268-355.  The attention-weights output of the reference (need_weights=True, discarded by every caller) is
    materialised on request only: with `need_weights` False (the default) the second return value is None and nothing extra is
    launched; with True it is the head-averaged map, fp32 [B, len_a, len_b] -- the softmax average in eval, the post-dropout
    average in training (the words the forward read) -- at the cost of one omr_attn_weights launch."""

    need_weights = False

    def __init__(self, feature_dim: int, num_heads: int = 4, dropout: float = 0.1) -> None:
        super().__init__()
        self.num_heads = num_heads
        self.attention = MultiheadAttention(feature_dim, num_heads, dropout)

    def forward(self, query, len_query, key_value, len_key_value):
        blk_lq = blk_lkv = None
        if len_query is not None and len_key_value is not None:
            # create_attention_mask (model.py:329-355): block [lq:, lkv:] masked, tiled with .repeat(num_heads,1,1)
            # -> head (b, h) uses sample (b*H + h) % B (quirk 2); the kernel indexes the length vectors that way.
            blk_lq = len_query.to(query.device, torch.int32).contiguous()
            blk_lkv = len_key_value.to(query.device, torch.int32).contiguous()
        kv = self.attention.project_kv(key_value.contiguous())
        weights = {} if self.need_weights else None
        out = self.attention.cross_attention(query.contiguous(), kv, None, self.training, blk_lq, blk_lkv, weights=weights)
        return out, (weights["out"] if weights is not None else None)

    def forward_key_lengths(self, query, key_value, len_key_value):
        """The attention of `forward` over a ragged batch's packed memories: sample b sees the first len_key_value[b] (int32 [B] on the
        device) keys of key_value [B, Skv, d] and nothing else, an exact -inf key bias (float32 [B, Skv], built like
        Decoder._as_key_bias builds the decoder's) -- what b computes alone, where `forward` gets no lengths and masks nothing.  The
        block mask of `forward` is not used: it is empty at batch size 1, and at B > 1 it hands sample b another sample's lengths
        (quirk 2).  Query rows past a sample's own length give finite rows the caller drops (ConcatMemoryFn)."""
        key_bias = Decoder._as_key_bias(_pad_mask(key_value.shape[1], len_key_value))
        kv = self.attention.project_kv(key_value.contiguous())
        return self.attention.cross_attention(query.contiguous(), kv, key_bias, self.training, None, None)


class MultimodalTransformer(_Base):
    """model.py:358-726."""

    def __init__(self, max_img_height: int, max_img_width: int, max_audio_height: int, max_audio_width: int, max_seq_len: int,
                 w2i: Dict[str, int], i2w: Dict[int, str], ytest_i2w: Optional[Dict[int, str]] = None, mixer_type: str = "concat",
                 attn_window: int = -1, teacher_forcing_prob: float = 0.5, teacher_forcing_modality_prob: float = 0.5,
                 config: Optional[ModelConfig] = None) -> None:
        super().__init__()
        self.save_hyperparameters()
        self._common_init(w2i, i2w, ytest_i2w, max_seq_len, attn_window, teacher_forcing_prob, config)
        if self.ctc_weight > 0:
            raise ValueError("the CTC head reads ONE feature grid as a frame sequence: ctc_weight > 0 is for Transformer, not the mixed memory "
                             "of MultimodalTransformer")
        self.max_img_height, self.max_img_width = max_img_height, max_img_width
        self.max_audio_height, self.max_audio_width = max_audio_height, max_audio_width
        self.teacher_forcing_modality_prob = teacher_forcing_modality_prob
        c = self.config
        self.image_encoder = Encoder(in_channels=NUM_CHANNELS, dropout=c.encoder_dropout, out_channels=c.d_model)
        self.image_pos_2d = PositionalEncoding2D(c.d_model, math.ceil(max_img_height / HEIGHT_REDUCTION),
                                                 math.ceil(max_img_width / WIDTH_REDUCTION), c.dropout)
        self.audio_encoder = Encoder(in_channels=NUM_CHANNELS, dropout=c.encoder_dropout, out_channels=c.d_model)
        self.audio_pos_2d = PositionalEncoding2D(c.d_model, math.ceil(max_audio_height / HEIGHT_REDUCTION),
                                                 math.ceil(max_audio_width / WIDTH_REDUCTION), c.dropout)
        self.decoder = self._make_decoder()
        self._mixer_kind = mixer_type            # the ragged route's mixers (`_mix_ragged`) go by name
        if mixer_type == "concat":
            self.mixer = self.mixer_concat
        elif mixer_type in ("attn_img", "attn_audio", "attn_both"):
            self.cross_attn = CrossAttention(feature_dim=c.d_model, num_heads=c.nhead, dropout=c.dropout)
            self.mixer = getattr(self, "mixer_" + mixer_type)
        else:
            raise ValueError(f"Invalid mixer type: {mixer_type}")

    def _encode(self, enc: Encoder, pos: PositionalEncoding2D, x: torch.Tensor) -> torch.Tensor:
        flat = self.ensure_flat()
        f = enc.forward_nhwc(_to_dev(x, flat.device), flat.compute_dtype).permute(0, 3, 1, 2)
        return _flatten_memory(pos(f))

    def encoder_forward(self, xi, xa, xli=None, xla=None, apply_teacher_forcing_modality: bool = False):
        """model.py:485-522: BOTH encoders always run; one memory may then be returned alone.  xli and xla both integer [B, 2]
        (`_is_pixel_sizes`): the ragged route, see `forward`."""
        if _pair_route(xli, xla) == "ragged":
            x, lens_dev, _ = self._encoder_forward_ragged(xi, xli, xa, xla, apply_teacher_forcing_modality)
            return x, _pad_mask(x.shape[1], lens_dev)                            # bool [B, Smax]: True = no key
        xi = self._encode(self.image_encoder, self.image_pos_2d, xi)
        xa = self._encode(self.audio_encoder, self.audio_pos_2d, xa)
        xi, xa = self._boundary(xi, xa)
        self._touched = None           # which sub-modules get gradients this step: the optimizer skips the others (FusedAdam)
        if apply_teacher_forcing_modality:
            modality = self._draw_modality()
            if modality == "image":
                self._touched = ("image_encoder", "decoder")
                return xi, xli
            elif modality == "audio":
                self._touched = ("audio_encoder", "decoder")
                return xa, xla
            elif modality == "both":
                x, xl = self.mixer(xi=xi, xa=xa, xli=xli, xla=xla)
            else:
                raise ValueError(f"Invalid modality: {modality}")
        else:
            x, xl = self.mixer(xi=xi, xa=xa, xli=xli, xla=xla)
        return x, xl

    def _encoder_forward_ragged(self, xi, xli, xa, xla, apply_teacher_forcing_modality: bool):
        """`encoder_forward` of a padded batch of pairs of different sizes -> (memory [B, Smax, d], its per-sample lengths int32 [B] on
        the device, the same on the host): rows [0, S_b) of sample b are the memory of pair b run alone with xli = xla = None
        (validation_step's form) to rounding, the rows behind them zeros.  Same draws from `random` as the dense route."""
        if _pair_route(xli, xla) != "ragged":
            raise ValueError("per-sample pixel sizes [B, 2] are needed for both modalities")
        mi, li, di = self._pack_encode(self.image_encoder, self.image_pos_2d, xi, xli)
        ma, la, da = self._pack_encode(self.audio_encoder, self.audio_pos_2d, xa, xla)
        mi, ma = self._boundary(mi, ma)
        self._touched = None
        modality = self._draw_modality() if apply_teacher_forcing_modality else "both"
        if modality == "image":
            self._touched = ("image_encoder", "decoder")
            return mi, di, li
        if modality == "audio":
            self._touched = ("audio_encoder", "decoder")
            return ma, da, la
        if modality != "both":
            raise ValueError(f"Invalid modality: {modality}")
        return self._mix_ragged(mi, li, di, ma, la, da)

    def _mix_ragged(self, mi, li, di, ma, la, da):
        """The mixers over packed memories (mi / ma [B, S, d], host lengths li / la, device lengths di / da).  The attention mixers
        mask keys by the key memory's own lengths (CrossAttention.forward_key_lengths); ConcatMemoryFn places the rows and writes the
        zeros behind each sample's length."""
        kind = self._mixer_kind
        if kind == "concat":
            lens = [a + b for a, b in zip(li, la)]
            return Fn.ConcatMemoryFn.apply(mi, di, ma, da, max(lens)), di + da, lens
        if kind == "attn_img":                                                   # q = audio, kv = image
            x = self.cross_attn.forward_key_lengths(ma, mi, di)
            return Fn.ConcatMemoryFn.apply(x, da, None, None, x.shape[1]), da, la
        if kind == "attn_audio":                                                 # q = image, kv = audio
            x = self.cross_attn.forward_key_lengths(mi, ma, da)
            return Fn.ConcatMemoryFn.apply(x, di, None, None, x.shape[1]), di, li
        if kind == "attn_both":                                                  # model.py:723-725: the second attention's keys are the ATTENDED audio (quirk 3)
            xa2 = self.cross_attn.forward_key_lengths(ma, mi, di)
            xi2 = self.cross_attn.forward_key_lengths(mi, xa2, da)
            lens = [a + b for a, b in zip(li, la)]
            return Fn.ConcatMemoryFn.apply(xi2, di, xa2, da, max(lens)), di + da, lens
        raise ValueError(f"Invalid mixer type: {kind}")

    @torch.no_grad()
    def encode_ragged(self, xi: torch.Tensor, sizes_i: torch.Tensor, xa: torch.Tensor, sizes_a: torch.Tensor) -> List[torch.Tensor]:
        """Mixed memories [S_b, d] of a padded batch of (image, audio) pairs of different sizes (`image.collate_ragged_pairs`), one pass
        of each encoder and of the mixer for all: each equals `_encode_input` of that pair alone to rounding (not bit for bit:
        `predict` / `evaluate` keep the batch-size-1 passes)."""
        x, _, lens = self._encoder_forward_ragged(xi, sizes_i, xa, sizes_a, False)
        return [x[b, :n] for b, n in enumerate(lens)]

    def forward(self, xi, xli, xa, xla, y_in, apply_teacher_forcing_modality: bool = False) -> torch.Tensor:
        """xli / xla as the reference's forms (None, integer lengths [B], bool masks): the dense route, every sample fills the planes
        of xi and xa.  BOTH integer [B, 2], the (height, width) in pixels of each sample's content in the top-left corner of xi /
        xa: the ragged route -- sample b's logits, loss share and gradients are those of pair b run alone at its own sizes; the
        memory rows past a sample's own length are zeros and masked out (-inf).  One [B, 2] and one of another form: ValueError."""
        x, xl = self.encoder_forward(xi=xi, xa=xa, xli=xli, xla=xla, apply_teacher_forcing_modality=apply_teacher_forcing_modality)
        return self.decoder(tgt=y_in, memory=x, memory_len=xl)

    def apply_teacher_forcing(self, y: torch.Tensor) -> torch.Tensor:
        """model.py:545-559 (vectorised, torch RNG)."""
        random_mask = torch.rand_like(y, dtype=torch.float) < self.teacher_forcing_prob
        combined = random_mask & (y != self.padding_idx)
        random_indices = torch.randint(0, len(self.w2i), y.shape, device=y.device)
        return torch.where(combined, random_indices, y)

    def apply_teacher_forcing_modality(self) -> str:
        """model.py:561-575."""
        if random.random() < self.teacher_forcing_modality_prob:
            return "image" if random.random() < 0.5 else "audio"
        return "both"

    def _draw_modality(self) -> str:
        """The modality decision of a training step.  Single process: the reference's draws from the global `random` stream.
        Data parallel: the global draws are still consumed (the stream stays where the reference's would be), but the decision
        comes from the reducer's shared generator, so every rank drops the same modality and FusedAdam skips the same
        sub-modules everywhere, however each rank seeded `random` (ddp.GradReducer.broadcast_state)."""
        modality = self.apply_teacher_forcing_modality()
        rng = getattr(self._reducer, "shared_rng", None)
        if rng is not None:
            modality = ("image" if rng.random() < 0.5 else "audio") if rng.random() < self.teacher_forcing_modality_prob else "both"
        return modality

    def training_step(self, batch, batch_idx) -> torch.Tensor:
        xi, xli, xa, xla, y_in, y_out = batch
        y_in = self.apply_teacher_forcing(y_in)
        yhat = self.forward(xi=xi, xli=xli, xa=xa, xla=xla, y_in=y_in, apply_teacher_forcing_modality=True)
        loss = self.compute_loss(yhat, _to_dev(y_out, yhat.device))
        self.log("train_loss", loss, prog_bar=True, logger=True, on_epoch=True)
        if self.compute_loss.label_smoothing > 0:      # the un-smoothed mean: comparable between runs that smooth differently
            self.log("train_nll", self.compute_loss.last_nll, prog_bar=True, logger=True, on_epoch=True)
        return loss

    @torch.no_grad()
    def validation_step(self, batch, batch_idx) -> None:
        xi, xa, y = batch
        assert xi.size(0) == xa.size(0) == y.size(0) == 1, "Inference only supports batch_size = 1"
        x, _ = self.encoder_forward(xi=xi, xa=xa, xli=None, xla=None, apply_teacher_forcing_modality=False)
        yhat, _ = self._greedy(x)
        self.Y.append([self.ytest_i2w[i.item()] for i in y[0][1:]])
        self.YHat.append(yhat)

    def _encode_input(self, pair) -> torch.Tensor:
        xi, xa = pair
        assert xi.size(0) == xa.size(0) == 1, "predict takes (image, audio) pairs of batch size 1; their sizes may differ"
        x, _ = self.encoder_forward(xi=xi, xa=xa, xli=None, xla=None, apply_teacher_forcing_modality=False)
        return x

    @ctc_decode_option(1)
    @spec_option
    @grammar_option
    @refill_option
    @_beam_option
    @torch.no_grad()
    def predict(self, pairs: Iterable[Tuple[torch.Tensor, torch.Tensor]], batch_size: int = 32) -> List[List[str]]:
        """Greedy predictions of (image, audio) pairs of any size, in input order: each equals validation_step's decode of
        that pair, decoded batch_size memories at a time.  Keyword `beam` (2 .. 8, `_beam_option`): the words of `beam_search`
        of each pair's memory, batch_size // beam pairs at a time.  Keyword `refill` (default False, `refill_option`; greedy
        only): continuous batching (`_predict`), same predictions.  Keywords `draft`, `draft_len`, `draft_source`
        (evaluation.spec_option; also on `evaluate`): speculative decoding with another MultimodalTransformer on the pair, or with a
        unimodal Transformer on the pair's image / audio (`draft_source`); same predictions."""
        return self._predict(pairs, self._encode_input, batch_size)

    @ctc_decode_option(1)
    @spec_option
    @grammar_option
    @refill_option
    @_beam_option
    @torch.no_grad()
    def evaluate(self, batches: Iterable, batch_size: int = 32) -> Dict[str, float]:
        """The metrics of validation_step over `batches` ((xi, xa, y) each) followed by on_validation_epoch_end, decoded in
        batches.  Keyword `beam` (2 .. 8, `_beam_option`): the predictions are those of `beam_search`.  Keyword `refill` (default
        False, `refill_option`; greedy only): continuous batching (`_predict`), same metrics."""
        return self._evaluate(batches, lambda batch: (batch[0], batch[1]), batch_size)

    def align(self, pairs: Iterable[Tuple[torch.Tensor, torch.Tensor]], words: Optional[List[List[str]]] = None, batch_size: int = 32,
              layers=None, return_maps: bool = False) -> List[Alignment]:
        """`Transformer.align` for (image, audio) pairs.  The decoder attends over the MIXED memory: `concat` and `attn_both`
        concatenate an image-grid part and an audio-grid part, split at the image memory's length -- `source` says which part a
        token leaned on, and its cell / box are on that input's grid; `attn_img` (queries = audio) leaves the audio grid,
        `attn_audio` the image grid."""
        kind = self._mixer_kind

        def sizes_of(pair):
            img, aud = ("image", pair[0].shape[-2], pair[0].shape[-1]), ("audio", pair[1].shape[-2], pair[1].shape[-1])
            if kind == "attn_img":
                return (aud,), None
            if kind == "attn_audio":
                return (img,), None
            gh, gw = grid_of(img[1], img[2])
            return (img, aud), gh * gw

        return self._align(pairs, sizes_of, words, batch_size, layers, return_maps)

    ##### MODALITY MIXERS (model.py:644-726)

    @staticmethod
    def _len_mask(n: int, lens: torch.Tensor, device) -> torch.Tensor:
        return torch.arange(n, device=device).unsqueeze(0) >= lens.to(device).long().unsqueeze(1)

    def mixer_concat(self, xi, xa, xli=None, xla=None):
        x = torch.cat([xi, xa], dim=1)
        if xli is not None and xla is not None:
            # bool mask -> true -inf masking in the decoder (model.py:663-672)
            xl = torch.cat([self._len_mask(xi.shape[1], xli, xi.device), self._len_mask(xa.shape[1], xla, xa.device)], dim=1)
        else:
            xl = None
        return x, xl

    def mixer_attn_img(self, xi, xa, xli=None, xla=None):
        x, _ = self.cross_attn(query=xa, len_query=xla, key_value=xi, len_key_value=xli)
        return x, (xla if (xli is not None and xla is not None) else None)

    def mixer_attn_audio(self, xi, xa, xli=None, xla=None):
        x, _ = self.cross_attn(query=xi, len_query=xli, key_value=xa, len_key_value=xla)
        return x, (xli if (xli is not None and xla is not None) else None)

    def mixer_attn_both(self, xi, xa, xli=None, xla=None):
        # model.py:723-725: the second attention sees the ALREADY ATTENDED audio (variable shadowing, quirk 3)
        xa, xla = self.mixer_attn_img(xi=xi, xa=xa, xli=xli, xla=xla)
        xi, xli = self.mixer_attn_audio(xi=xi, xa=xa, xli=xli, xla=xla)
        return self.mixer_concat(xi=xi, xa=xa, xli=xli, xla=xla)
