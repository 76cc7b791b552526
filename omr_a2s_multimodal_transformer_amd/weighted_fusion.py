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

Beam search over the mixed distribution (`weighted_beam_search`, `weighted_beam_search_batch`, `weighted_predict(beam=)`,
`weighted_evaluate(beam=)`) is an extension: the reference decodes the fusion greedily.  It is `_Base.beam_search` of model.py
with the log of the mixed probability in place of log_softmax; beam = 1 is the weighted greedy decode.

Every entry point takes the keyword `grammar` (evaluation.grammar_option; default: img_model.decode_grammar): both models'
logits are masked by ONE automaton state per row before the mix (omr_weighted_grammar_pick, omr_weighted_beam_select_grammar).
"""
from __future__ import annotations

import contextvars
import ctypes
import functools
import itertools
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch

from . import kernels as K
from ._lib import cur_stream, lib, ptr
from .decoder import MAX_BEAM, WeightedBeamState, takes_ragged_state
from .evaluation import (WINDOW_BATCHES, active_grammar, decode_rows, decode_stream, grammar_option, no_ctc_decode_option, no_draft_option, plan_pair_groups, refill_enabled, refill_option,
                         stream_order)
from .grammar import host_mask
from .metrics import compute_metrics
from .synthetic import EOS_TOKEN, SOS_TOKEN

_EXHAUSTED = "weighted_prediction beyond a model's max_seq_len (positional-encoding table exhausted)"

_BEAM = contextvars.ContextVar("omr_weighted_beam", default=1)


def beam_option(fn):
    """Gives weighted_predict / weighted_evaluate the keyword `beam` (1 .. 8, default 1), like model._beam_option: the
    function's own parameter list stays as it is; the value is checked here, before anything is encoded; beam = 1 calls the
    function as before, a wider beam holds for the duration of the call (`_weighted_predict` asks for it).  Goes outside
    `refill_option`, so that it sees that keyword: a beam state has no slots to refill."""
    @functools.wraps(fn)
    def call(*args, beam: int = 1, **kwargs):
        if not isinstance(beam, int) or not 1 <= beam <= MAX_BEAM:
            raise ValueError(f"beam must be an integer in 1..{MAX_BEAM}, got {beam}")
        if beam == 1:
            return fn(*args, **kwargs)
        if kwargs.get("refill"):
            raise ValueError("refill=True decodes greedily: the beam state (two caches per model, a history table) has no slots to refill")
        token = _BEAM.set(beam)
        try:
            return fn(*args, **kwargs)
        finally:
            _BEAM.reset(token)
    return call


def _decode_lockstep(st_i, st_a, img_model, audio_model, alpha: float, sync_every: int) -> List[List[str]]:
    """The lock-step loop (test.py:39-68) of every row of two decode states at position 0 -- one pair over two batch-size-1
    states, or B pairs over two ragged ones: the host reads the tokens back every `sync_every` positions and cuts each row
    after its <eos> (evaluation.decode_rows).  A dense state has no memory lengths: its pointer is NULL, which
    omr_weighted_decode_steps_varlen takes for either model (one row: what omr_weighted_decode_steps runs)."""
    assert st_i.V == st_a.V and st_i.B == st_a.B, "both models share the vocabulary (test.py:62) and decode the same rows"
    B, dev = st_i.B, st_i.tok.device
    tok = torch.full((B,), img_model.w2i[SOS_TOKEN], dtype=torch.int64, device=dev)      # the picked tokens stay here, on the device
    grammar = active_grammar(img_model)
    gstate = None if grammar is None else grammar.bind(B, dev)

    def step(n: int):
        n = min(n, st_i.max_len - st_i.t, st_a.max_len - st_a.t)
        if n <= 0:                                     # a live row outgrew the shorter positional table
            raise RuntimeError(_EXHAUSTED)
        toks = torch.empty((n, B), dtype=torch.int64, device=dev)
        if gstate is not None:
            lib().call("omr_weighted_decode_steps_varlen_grammar", ctypes.byref(st_i.desc), ptr(st_i.mem_len), ctypes.byref(st_a.desc), ptr(st_a.mem_len),
                       gstate.byref(), float(alpha), ptr(tok), st_i.t, n, ptr(toks), None, ptr(st_i.logits), ptr(st_a.logits), cur_stream())
        else:
            lib().call("omr_weighted_decode_steps_varlen", ctypes.byref(st_i.desc), ptr(st_i.mem_len), ctypes.byref(st_a.desc), ptr(st_a.mem_len),
                       float(alpha), ptr(tok), st_i.t, n, ptr(toks), None, ptr(st_i.logits), ptr(st_a.logits), cur_stream())
        st_i.t += n
        st_a.t += n
        return toks.cpu().tolist(), None               # one device sync per chunk

    ids, _ = decode_rows(step, B, img_model.w2i[EOS_TOKEN], max(img_model.max_seq_len, audio_model.max_seq_len), sync_every, gstate=gstate)
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
    grammar = active_grammar(img_model)
    gstate = None if grammar is None else grammar.bind(rows, dev)

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
        if gstate is not None:
            lib().call("omr_weighted_decode_steps_rows_grammar", ctypes.byref(st_i.desc), ptr(st_i.mem_len), ctypes.byref(st_a.desc), ptr(st_a.mem_len),
                       ptr(st_i.pos), t_max, gstate.byref(), float(alpha), ptr(tok), n, ptr(toks), None, ptr(st_i.logits), ptr(st_a.logits), cur_stream())
        else:
            lib().call("omr_weighted_decode_steps_rows", ctypes.byref(st_i.desc), ptr(st_i.mem_len), ctypes.byref(st_a.desc), ptr(st_a.mem_len),
                       ptr(st_i.pos), t_max, float(alpha), ptr(tok), n, ptr(toks), None, ptr(st_i.logits), ptr(st_a.logits), cur_stream())
        st_i.advance(n)
        st_a.advance(n)
        return toks.cpu().tolist(), None               # one device sync per chunk

    order = stream_order([mi.shape[0] + ma.shape[0] for mi, ma in zip(mems_i, mems_a)])
    ids, _ = decode_stream(step, admit, order, rows, img_model.w2i[EOS_TOKEN], max(img_model.max_seq_len, audio_model.max_seq_len), sync_every,
                           gstate=gstate)
    return [[img_model._i2w(t) for t in seq] for seq in ids]


@grammar_option
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


@grammar_option
@torch.no_grad()
def weighted_beam_search(xi: torch.Tensor, xa: torch.Tensor, img_model, audio_model, alpha: float = 0.5, beam: int = 4) -> Tuple[List[str], float]:
    """Beam search of ONE pair over the weighted late fusion (an extension: the reference decodes it greedily,
    weighted_multimodal/test.py:21-70) -> (words incl. <eos> if reached, score).  `_Base.beam_search` written out for two
    models: both decode the same `beam` hypotheses, the candidates of a row are the `beam` largest
    alpha * softmax(image logits) + (1 - alpha) * softmax(audio logits) (kernels.weighted_topk_logprob) and a score is the sum
    of the logs of those mixed probabilities, without length normalisation.  beam = 1 is `weighted_prediction`.  The budget
    is max(img_model.max_seq_len, audio_model.max_seq_len); a live search that outgrows the shorter positional table raises."""
    assert xi.size(0) == 1 and xa.size(0) == 1, "Inference only supports batch_size = 1"
    return _beam_search_memories(img_model.encode(xi), audio_model.encode(xa), img_model, audio_model, alpha, beam)


@torch.no_grad()
def _beam_search_memories(mem_i: torch.Tensor, mem_a: torch.Tensor, img_model, audio_model, alpha: float, beam: int) -> Tuple[List[str], float]:
    """weighted_beam_search from the two encoded memories [1, S, d]."""
    assert beam >= 1
    grammar = active_grammar(img_model)          # both models' logits masked by each hypothesis' state; forbidden candidates dropped by the table
    gstates = [grammar.start] * beam if grammar is not None else None
    sos, eos = img_model.w2i[SOS_TOKEN], img_model.w2i[EOS_TOKEN]
    st_i, st_a = img_model.decoder.init_decode(mem_i), audio_model.decoder.init_decode(mem_a)
    st_i.share_memory_between(beam)                          # every hypothesis reads the same memory K|V; own self-attention cache rows
    st_a.share_memory_between(beam)
    assert st_i.V == st_a.V, "both models share the vocabulary (test.py:62)"
    dev = st_i.tok.device
    tok = torch.full((beam, 1), sos, dtype=torch.int64, device=dev)
    scores = [0.0] + [float("-inf")] * (beam - 1)           # only the first row is a real hypothesis before the first step
    seqs: List[List[int]] = [[] for _ in range(beam)]
    best_done: Tuple[float, Optional[List[int]]] = (float("-inf"), None)
    exhausted = True                                         # the loop ran out of positions with hypotheses still alive
    for t in range(max(img_model.max_seq_len, audio_model.max_seq_len)):
        if t >= min(st_i.max_len, st_a.max_len):            # a live hypothesis outgrew the shorter positional table
            raise RuntimeError(_EXHAUSTED)
        li, la = (m.decoder.decode_step(tok, st).view(beam, -1) for m, st in ((img_model, st_i), (audio_model, st_a)))
        if grammar is not None:
            forbidden = ~host_mask(grammar, gstates, li.device)
            li, la = li.masked_fill(forbidden, float("-inf")).contiguous(), la.masked_fill(forbidden, float("-inf")).contiguous()
        idx, val = K.weighted_topk_logprob(li, la, alpha, beam)
        idx_h, val_h = idx.cpu().tolist(), val.cpu().tolist()
        cands = [(scores[b] + val_h[b][j], b, idx_h[b][j]) for b in range(beam) if scores[b] > float("-inf") for j in range(beam)]
        if grammar is not None:
            cands = [c for c in cands if grammar.walk([c[2]], gstates[c[1]])[0] >= 0]
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        parents, new_tok, new_scores, new_seqs = [], [], [], []
        for sc, b, tk in cands:
            if tk == eos:
                if sc > best_done[0]:
                    best_done = (sc, seqs[b] + [tk])
                continue
            parents.append(b); new_tok.append(tk); new_scores.append(sc); new_seqs.append(seqs[b] + [tk])
            if len(parents) == beam:
                break
        if not parents or new_scores[0] <= best_done[0]:    # scores only fall: no live hypothesis can overtake the best finished one
            exhausted = False
            break
        while len(parents) < beam:                            # pad with dead rows
            parents.append(parents[0]); new_tok.append(new_tok[0]); new_scores.append(float("-inf")); new_seqs.append([])
        pidx = torch.tensor(parents, dtype=torch.int64, device=dev)
        st_i.reorder_rows(pidx)
        st_a.reorder_rows(pidx)
        tok = torch.tensor(new_tok, dtype=torch.int64, device=dev).view(beam, 1)
        scores, seqs = new_scores, new_seqs
        if grammar is not None:
            gstates = [grammar.walk([tk], gstates[b])[0] for b, tk in zip(parents, new_tok)]
    if exhausted and scores[0] > best_done[0]:
        best_done = (scores[0], seqs[0])                      # ran out of length: the best unfinished hypothesis wins
    return [img_model._i2w(t) for t in best_done[1]], best_done[0]


def _run_beam_state(state: WeightedBeamState, img_model, audio_model, sync_every: int) -> List[Tuple[List[str], float]]:
    """One search of a WeightedBeamState at position 0 to its end: the `done` flags are read every sync_every positions, the
    state once at the end."""
    left = max(img_model.max_seq_len, audio_model.max_seq_len)
    while left > 0:
        n = min(sync_every, left, state.max_len - state.t)
        if n <= 0:                                         # a live pair outgrew the shorter positional table
            raise RuntimeError(_EXHAUSTED)
        state.run(n)
        left -= n
        if left > 0 and all(state.done()):                 # one small device sync per chunk
            break
    return [([img_model._i2w(t) for t in seq], score) for seq, score in state.results()]


@grammar_option
@torch.no_grad()
def weighted_beam_search_batch(mems_i, mems_a, img_model, audio_model, alpha: float = 0.5, beam: int = 4,
                               sync_every: int = 8) -> List[Tuple[List[str], float]]:
    """`weighted_beam_search` of N pairs at once, on the device (decoder.WeightedBeamState; csrc/decode.hip
    omr_weighted_beam_decode_steps): -> [(words, score)] in input order, each exactly what weighted_beam_search returns for
    that pair alone.  mems_i / mems_a: each model's encoded memories, [1, S_b, d] / [S_b, d] of different lengths.  Pairs of
    which either memory has at most 64 or more than 16 384 tokens go through weighted_beam_search."""
    if not 1 <= beam <= MAX_BEAM:
        raise ValueError(f"beam must be in 1..{MAX_BEAM}, got {beam}")
    if sync_every < 1:
        raise ValueError(f"sync_every must be >= 1, got {sync_every}")
    if len(mems_i) != len(mems_a):
        raise ValueError(f"weighted_beam_search_batch: {len(mems_i)} image memories, {len(mems_a)} audio memories")
    mi = img_model.decoder.memory_list(mems_i, refuse_long=False)
    ma = audio_model.decoder.memory_list(mems_a, refuse_long=False)
    out: List[Optional[Tuple[List[str], float]]] = [None] * len(mi)
    batched = [i for i in range(len(mi)) if takes_ragged_state(mi[i].shape[0]) and takes_ragged_state(ma[i].shape[0])]
    for i in range(len(mi)):
        if i not in batched:                               # alone, such a memory takes another attention kernel: search the pair alone
            out[i] = _beam_search_memories(mi[i].unsqueeze(0), ma[i].unsqueeze(0), img_model, audio_model, alpha, beam)
    if batched:
        state = WeightedBeamState(img_model.decoder, [mi[i] for i in batched], audio_model.decoder, [ma[i] for i in batched], beam,
                                  img_model.w2i[SOS_TOKEN], img_model.w2i[EOS_TOKEN], alpha)
        state.constrain(active_grammar(img_model))
        for i, result in zip(batched, _run_beam_state(state, img_model, audio_model, sync_every)):
            out[i] = result
    return out


def _check_models(img_model, audio_model) -> None:
    if img_model.w2i != audio_model.w2i:
        raise ValueError("Vocabularies do not match (weighted_multimodal/test.py:140)")


def _alphas(alpha) -> Tuple[List[float], bool]:
    if isinstance(alpha, (int, float)):
        return [float(alpha)], False
    return [float(a) for a in alpha], True


def _beam_window(mems_i, mems_a, img_model, audio_model, alphas: List[float], batch_size: int, sync_every: int, beam: int, out) -> None:
    """out[k][i] <- the words weighted_beam_search finds for pair i of a window under alphas[k]: groups of batch_size // beam
    pairs as one WeightedBeamState each, built once and rewound per alpha; the pairs plan_pair_groups leaves alone one by one."""
    singles, groups = plan_pair_groups([m.shape[1] for m in mems_i], [m.shape[1] for m in mems_a], max(1, batch_size // beam))
    for i in singles:
        for k, alpha in enumerate(alphas):
            out[k][i] = _beam_search_memories(mems_i[i], mems_a[i], img_model, audio_model, alpha, beam)[0]
    for g in groups:
        state = WeightedBeamState(img_model.decoder, [mems_i[i] for i in g], audio_model.decoder, [mems_a[i] for i in g], beam,
                                  img_model.w2i[SOS_TOKEN], img_model.w2i[EOS_TOKEN])
        state.constrain(active_grammar(img_model))
        for k, alpha in enumerate(alphas):
            state.rewind(alpha)
            for i, (seq, _) in zip(g, _run_beam_state(state, img_model, audio_model, sync_every)):
                out[k][i] = seq
        del state


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
        beam = _BEAM.get()
        if beam > 1:                                   # beam_option: the whole window is decoded here, nothing is left for the plans below
            _beam_window(mems_i, mems_a, img_model, audio_model, alphas, batch_size, sync_every, beam, out)
            singles, groups = [], []
        else:
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


@no_ctc_decode_option
@no_draft_option
@grammar_option
@beam_option
@refill_option
def weighted_predict(pairs: Iterable[Tuple[torch.Tensor, torch.Tensor]], img_model, audio_model, alpha: Union[float, Sequence[float]] = 0.5,
                     batch_size: int = 32, sync_every: int = 8):
    """Weighted predictions of (image, audio) pairs ([1, C, H, W] each, sizes free), in input order: each equals
    weighted_prediction(xi, xa, img_model, audio_model, alpha).  A window of WINDOW_BATCHES * batch_size pairs at a time is
    encoded at batch size 1 by each model, grouped by evaluation.plan_pair_groups and decoded group by group, both models in
    lock-step over ragged batches of up to batch_size rows.  `alpha` may be a sequence (the usual tuning sweep): the result
    is then {alpha: predictions}, with the encoders and the cross-attention projections run once, not once per alpha.
    Keyword `refill` (default False, `refill_option`): continuous batching -- a finished pair's slot goes to the next pair of the window (_decode_lockstep_stream);
    same predictions.  Keyword `beam` (2 .. 8, `beam_option`; an extension: the reference decodes greedily; not with refill): each
    prediction is that of weighted_beam_search, batch_size // beam pairs at a time (decoder.WeightedBeamState); a sequence of
    alphas rewinds each group's state per alpha."""
    alphas, many = _alphas(alpha)
    preds = _weighted_predict(pairs, img_model, audio_model, alphas, batch_size, sync_every)
    return dict(zip(alphas, preds)) if many else preds[0]


@no_ctc_decode_option
@no_draft_option
@grammar_option
@beam_option
@refill_option
def weighted_evaluate(batches: Iterable, img_model, audio_model, alpha: Union[float, Sequence[float]] = 0.5, batch_size: int = 32):
    """weighted_multimodal/test.py:154-172 over `batches` ((xi, xa, y) as the test loader yields them): compute_metrics of the
    weighted predictions against the ytest_i2w-decoded targets (without <sos>); {alpha: metrics} for a sequence of alphas.
    Keywords `refill` and `beam`: as in weighted_predict."""
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
