"""Weighted late fusion (reference: src/multimodal/weighted_multimodal/test.py:21-70): an image model and an audio model --
two unimodal `Transformer`s with the same vocabulary -- decode in lock-step from the same prefix; at every step the two
next-token distributions are mixed, alpha * softmax(image logits) + (1 - alpha) * softmax(audio logits), and the argmax token
is fed back to BOTH decoders.

The reference re-runs both decoders over the whole prefix per token and reads every token back; here each model keeps its KV
cache (Decoder.init_decode: cross-attention K|V projected once, self-attention K|V appended per step), the mixing + argmax of
a step is one kernel (omr_weighted_argmax_rows) and a CHUNK of positions is one host call (omr_weighted_decode_steps_varlen:
the picked token reaches both models' next position through device memory; the host reads a chunk of tokens back at a time
and cuts the sequence after <eos>).  Same tokens as the reference (tests/golden/f15_weighted.npz).

The reference evaluates a test set one pair at a time (test.py:154-172).  `weighted_predict` / `weighted_evaluate` decode
groups of pairs of different sizes as two ragged decode states in lock-step (omr_weighted_decode_steps_varlen: per position
both models' steps for all rows, then one mixing launch for all rows); every sequence equals `weighted_prediction` of that
pair.  A sequence of alphas re-runs only the decode: encoders and cross-attention projections run once per pair.
"""
from __future__ import annotations

import ctypes
import itertools
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch

from ._lib import cur_stream, lib, ptr
from .evaluation import WINDOW_BATCHES, decode_rows, decode_stream, plan_pair_groups, refill_enabled, refill_option, stream_order
from .metrics import compute_metrics
from .synthetic import EOS_TOKEN, SOS_TOKEN

_EXHAUSTED = "weighted_prediction beyond a model's max_seq_len (positional-encoding table exhausted)"


def _decode_lockstep(st_i, st_a, img_model, audio_model, alpha: float, sync_every: int) -> List[List[str]]:
    """The lock-step loop (test.py:39-68) of every row of two decode states at position 0 -- one pair over two batch-size-1
    states, or B pairs over two ragged ones: the host reads the tokens back every `sync_every` positions and cuts each row
    after its <eos> (evaluation.decode_rows).  A dense state has no memory lengths: its pointer is NULL, which
    omr_weighted_decode_steps_varlen takes for either model (one row: what omr_weighted_decode_steps runs)."""
    assert st_i.V == st_a.V and st_i.B == st_a.B, "both models share the vocabulary (test.py:62) and decode the same rows"
    B, dev = st_i.B, st_i.tok.device
    tok = torch.full((B,), img_model.w2i[SOS_TOKEN], dtype=torch.int64, device=dev)      # the picked tokens stay here, on the device

    def step(n: int):
        n = min(n, st_i.max_len - st_i.t, st_a.max_len - st_a.t)
        if n <= 0:                                     # a live row outgrew the shorter positional table
            raise RuntimeError(_EXHAUSTED)
        toks = torch.empty((n, B), dtype=torch.int64, device=dev)
        lib().call("omr_weighted_decode_steps_varlen", ctypes.byref(st_i.desc), ptr(st_i.mem_len), ctypes.byref(st_a.desc), ptr(st_a.mem_len),
                   float(alpha), ptr(tok), st_i.t, n, ptr(toks), None, ptr(st_i.logits), ptr(st_a.logits), cur_stream())
        st_i.t += n
        st_a.t += n
        return toks.cpu().tolist(), None               # one device sync per chunk

    ids, _ = decode_rows(step, B, img_model.w2i[EOS_TOKEN], max(img_model.max_seq_len, audio_model.max_seq_len), sync_every)
    return [[img_model._i2w(t) for t in seq] for seq in ids]


def _decode_lockstep_stream(mems_i, mems_a, img_model, audio_model, alpha: float, rows: int, sync_every: int) -> List[List[str]]:
    """_decode_lockstep with continuous batching: the pairs (mems_i[k], mems_a[k]), all of which take a ragged state, stream
    through ONE slot decode state per model (Decoder.init_slot_decode); both states hold the same rows at the same positions,
    so one `pos` serves both (omr_weighted_decode_steps_rows), and a finished pair's slot goes to the next pair
    (evaluation.decode_stream).  Each sequence equals _decode_lockstep of that pair alone."""
    sos, dev = img_model.w2i[SOS_TOKEN], mems_i[0].device
    rows = min(rows, len(mems_i))
    st_i = img_model.decoder.init_slot_decode(rows, max(m.shape[0] for m in mems_i), dev, sos)
    st_a = audio_model.decoder.init_slot_decode(rows, max(m.shape[0] for m in mems_a), dev, sos)
    assert st_i.V == st_a.V, "both models share the vocabulary (test.py:62)"
    tok = torch.full((rows,), sos, dtype=torch.int64, device=dev)      # the picked tokens stay here, on the device

    def admit(slot: int, k: Optional[int]) -> None:
        st_i.admit(slot, None if k is None else mems_i[k])
        st_a.admit(slot, None if k is None else mems_a[k])
        tok[slot:slot + 1].fill_(sos)

    def step(n: int):
        n = min(n, st_i.max_len - st_i.furthest(), st_a.max_len - st_a.furthest())
        if n <= 0:                                     # a live row outgrew the shorter positional table
            raise RuntimeError(_EXHAUSTED)
        t_max = st_i.begin(n)
        st_a.begin(n)
        toks = torch.empty((n, rows), dtype=torch.int64, device=dev)
        lib().call("omr_weighted_decode_steps_rows", ctypes.byref(st_i.desc), ptr(st_i.mem_len), ctypes.byref(st_a.desc), ptr(st_a.mem_len),
                   ptr(st_i.pos), t_max, float(alpha), ptr(tok), n, ptr(toks), None, ptr(st_i.logits), ptr(st_a.logits), cur_stream())
        st_i.advance(n)
        st_a.advance(n)
        return toks.cpu().tolist(), None               # one device sync per chunk

    order = stream_order([mi.shape[0] + ma.shape[0] for mi, ma in zip(mems_i, mems_a)])
    ids, _ = decode_stream(step, admit, order, rows, img_model.w2i[EOS_TOKEN], max(img_model.max_seq_len, audio_model.max_seq_len), sync_every)
    return [[img_model._i2w(t) for t in seq] for seq in ids]


@torch.no_grad()
def weighted_prediction(xi: torch.Tensor, xa: torch.Tensor, img_model, audio_model, alpha: float = 0.5, chunk: int = 16) -> List[str]:
    """weighted_multimodal/test.py:21-70, same signature and return value (the predicted words, <eos> included when reached).
    Like the reference, the loop runs for max(img_model.max_seq_len, audio_model.max_seq_len) steps and a model whose
    positional table is shorter than that raises when the sequence outgrows it."""
    assert xi.size(0) == 1, "Inference only supports batch_size = 1"
    mem_i = img_model.encode(xi)                       # encoder -> 2-D PE -> flatten (test.py:28-37)
    mem_a = audio_model.encode(xa)
    st_i = img_model.decoder.init_decode(mem_i)
    st_a = audio_model.decoder.init_decode(mem_a)
    return _decode_lockstep(st_i, st_a, img_model, audio_model, alpha, chunk)[0]


def _check_models(img_model, audio_model) -> None:
    if img_model.w2i != audio_model.w2i:
        raise ValueError("Vocabularies do not match (weighted_multimodal/test.py:140)")


def _alphas(alpha) -> Tuple[List[float], bool]:
    if isinstance(alpha, (int, float)):
        return [float(alpha)], False
    return [float(a) for a in alpha], True


@torch.no_grad()
def _weighted_predict(pairs: Iterable, img_model, audio_model, alphas: List[float], batch_size: int, sync_every: int,
                      chunk: int = 16) -> List[List[List[str]]]:
    """-> one prediction list per alpha.  Every pair is encoded once per model and every group's (or single's) decode states
    are built once; each alpha decodes from position 0 again (DecodeState.rewind).  Called with refill=True (evaluation.refill_option): the pairs of a window that take a
    ragged state stream through one slot state per model instead (_decode_lockstep_stream), once per alpha over the kept
    memories -- the cross-attention K|V of a pair are projected again on every admission."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    if sync_every < 1:
        raise ValueError(f"sync_every must be >= 1, got {sync_every}")
    _check_models(img_model, audio_model)
    refill = refill_enabled()
    it = iter(pairs)
    preds: List[List[List[str]]] = [[] for _ in alphas]
    while True:
        window = list(itertools.islice(it, WINDOW_BATCHES * batch_size))
        if not window:
            return preds
        for xi, xa in window:                          # refuse before anything of this window is launched
            assert xi.size(0) == 1 and xa.size(0) == 1, "weighted_predict takes (image, audio) pairs of batch size 1; their sizes may differ"
        mems_i = [img_model.encode(xi) for xi, _ in window]
        mems_a = [audio_model.encode(xa) for _, xa in window]
        out: List[List[Optional[List[str]]]] = [[None] * len(window) for _ in alphas]
        singles, groups = plan_pair_groups([m.shape[1] for m in mems_i], [m.shape[1] for m in mems_a], batch_size)
        # a single: the pair alone over two batch-size-1 states, `chunk` positions per read-back like weighted_prediction
        plans = [([i], mems_i[i], mems_a[i], chunk) for i in singles]
        rest = [i for g in groups for i in g]
        if refill and rest and img_model.decoder.takes_slot_state(max(mems_i[i].shape[1] for i in rest)) and \
                audio_model.decoder.takes_slot_state(max(mems_a[i].shape[1] for i in rest)):
            mi = img_model.decoder.memory_list([mems_i[i] for i in rest])
            ma = audio_model.decoder.memory_list([mems_a[i] for i in rest])
            for k, alpha in enumerate(alphas):
                for i, seq in zip(rest, _decode_lockstep_stream(mi, ma, img_model, audio_model, alpha, batch_size, sync_every)):
                    out[k][i] = seq
            groups = []
        plans += [(g, [mems_i[i] for i in g], [mems_a[i] for i in g], sync_every) for g in groups]
        for idx, mi, ma, every in plans:
            st_i = img_model.decoder.init_decode(mi)
            st_a = audio_model.decoder.init_decode(ma)
            for k, alpha in enumerate(alphas):
                st_i.rewind()
                st_a.rewind()
                for i, seq in zip(idx, _decode_lockstep(st_i, st_a, img_model, audio_model, alpha, every)):
                    out[k][i] = seq
            del st_i, st_a
        for k in range(len(alphas)):
            preds[k] += out[k]
        del mems_i, mems_a


@refill_option
def weighted_predict(pairs: Iterable[Tuple[torch.Tensor, torch.Tensor]], img_model, audio_model, alpha: Union[float, Sequence[float]] = 0.5,
                     batch_size: int = 32, sync_every: int = 8):
    """Weighted predictions of (image, audio) pairs ([1, C, H, W] each, sizes free), in input order: each equals
    weighted_prediction(xi, xa, img_model, audio_model, alpha).  A window of WINDOW_BATCHES * batch_size pairs at a time is
    encoded at batch size 1 by each model, grouped by evaluation.plan_pair_groups and decoded group by group, both models in
    lock-step over ragged batches of up to batch_size rows.  `alpha` may be a sequence (the usual tuning sweep): the result
    is then {alpha: predictions}, with the encoders and the cross-attention projections run once, not once per alpha.
    Keyword `refill` (default False, `refill_option`): continuous batching -- a finished pair's slot goes to the next pair of the window (_decode_lockstep_stream);
    same predictions."""
    alphas, many = _alphas(alpha)
    preds = _weighted_predict(pairs, img_model, audio_model, alphas, batch_size, sync_every)
    return dict(zip(alphas, preds)) if many else preds[0]


@refill_option
def weighted_evaluate(batches: Iterable, img_model, audio_model, alpha: Union[float, Sequence[float]] = 0.5, batch_size: int = 32):
    """weighted_multimodal/test.py:154-172 over `batches` ((xi, xa, y) as the test loader yields them): compute_metrics of the
    weighted predictions against the ytest_i2w-decoded targets (without <sos>); {alpha: metrics} for a sequence of alphas.
    Keyword `refill`: as in weighted_predict."""
    _check_models(img_model, audio_model)
    truth: List[List[str]] = []

    def inputs():
        for xi, xa, y in batches:
            assert y.size(0) == 1, "weighted_evaluate takes the batches of the test loader (batch_size = 1)"
            truth.append([img_model.ytest_i2w[i] for i in y[0][1:].tolist()])
            yield xi, xa

    alphas, many = _alphas(alpha)
    preds = _weighted_predict(inputs(), img_model, audio_model, alphas, batch_size, 8)
    metrics = [compute_metrics(y_true=truth, y_pred=p) for p in preds]
    return dict(zip(alphas, metrics)) if many else metrics[0]
