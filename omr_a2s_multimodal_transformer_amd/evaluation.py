"""Batched evaluation over inputs of different sizes.  The reference validates one input at a time (src/train.py:34,
src/transformer/model.py:171-199, "Inference only supports batch_size = 1"); `predict` / `evaluate` of both model classes
decode groups of memories of different lengths as ONE ragged decode state (Decoder.init_decode on a list), and every
sequence equals the batch-size-1 loop's (`_greedy`) for that input.  This module holds the host side of that: the grouping,
the read-back loop of the greedy decodes and the backtrack of the batched beam search."""
from __future__ import annotations

import contextvars
import functools
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from .decoder import takes_ragged_state

WINDOW_BATCHES = 8          # inputs are encoded and sorted by memory length a window of 8 * batch_size at a time


_REFILL = contextvars.ContextVar("omr_refill", default=False)


def refill_enabled() -> bool:
    """Whether the evaluation call under way asked for continuous batching (`refill_option`)."""
    return _REFILL.get()


def refill_option(fn):
    """Gives an evaluation entry point (`predict` / `predict_with_probs` / `evaluate` of both model classes, weighted_predict /
    weighted_evaluate, sw_predict / sw_evaluate) the keyword `refill: bool = False`.  The function's own parameter list -- part
    of the public surface the tests pin -- stays as it is, like `beam` (model._beam_option); the flag holds for the duration
    of the call and the decode loops ask `refill_enabled()`.  An evaluation call made inside another one (sw_predict calls
    predict_with_probs) without the keyword keeps the outer call's choice."""
    @functools.wraps(fn)
    def call(*args, refill=None, **kwargs):
        token = _REFILL.set(_REFILL.get() if refill is None else bool(refill))
        try:
            return fn(*args, **kwargs)
        finally:
            _REFILL.reset(token)
    return call


_UNSET = object()
_GRAMMAR = contextvars.ContextVar("omr_grammar", default=_UNSET)


def grammar_option(fn):
    """Gives a decode entry point the keyword `grammar` (a grammar.Grammar, or None: unconstrained), like `refill_option`: the
    function's own parameter list stays as it is and the value holds for the duration of the call; the decode routes ask
    `active_grammar`.  Without the keyword an outer call's choice holds, and with no outer call the model's `decode_grammar`."""
    @functools.wraps(fn)
    def call(*args, grammar=_UNSET, **kwargs):
        if grammar is _UNSET:
            return fn(*args, **kwargs)
        token = _GRAMMAR.set(grammar)
        try:
            return fn(*args, **kwargs)
        finally:
            _GRAMMAR.reset(token)
    return call


def active_grammar(model):
    """The automaton the decode under way is constrained by, or None: the `grammar` keyword of the evaluation call if one was
    given (`grammar_option`), else `model.decode_grammar`; checked against the model's vocabulary."""
    from .grammar import check_grammar
    from .synthetic import EOS_TOKEN
    g = _GRAMMAR.get()
    if g is _UNSET:
        g = getattr(model, "decode_grammar", None)
    return check_grammar(g, len(model.w2i), model.w2i[EOS_TOKEN])


@dataclass
class SpecOptions:
    """What `spec_option` hands the decode routes: the draft model, the proposals per cycle, and how the draft encodes an item
    of the call (its own encoder(s); for a unimodal draft of a multimodal target, the image or the audio of the pair)."""
    draft: object
    k: int
    encode: Callable


_SPEC = contextvars.ContextVar("omr_spec", default=None)


def active_spec() -> Optional[SpecOptions]:
    """The speculative-decoding options of the evaluation call under way (`spec_option`), or None: no draft."""
    return _SPEC.get()


def check_draft(model, draft, draft_len, draft_source, others: dict) -> SpecOptions:
    """Every refusal of `draft=`, before the route or the hardware is looked at -> the options."""
    from .decoder import check_draft_len, check_row_widths
    if not hasattr(draft, "w2i") or not hasattr(draft, "decoder"):
        raise ValueError("draft must be a Transformer or a MultimodalTransformer")
    if dict(draft.w2i) != dict(model.w2i):
        raise ValueError(f"draft: its vocabulary ({len(draft.w2i)} entries) differs from the target's ({len(model.w2i)}): a proposal is "
                         "compared with the target's pick by token id")
    check_draft_len(draft_len)
    if others.get("beam", 1) != 1:
        raise ValueError("draft= decodes greedily: it does not combine with beam=")
    if others.get("grammar", None) is not None or getattr(model, "decode_grammar", None) is not None and "grammar" not in others:
        raise ValueError("draft= does not combine with a grammar (grammar= or decode_grammar): the draft's proposals are unconstrained")
    if others.get("refill", False):
        raise ValueError("draft= does not combine with refill=True: the speculative state has no slots to refill")
    if draft.max_seq_len < model.max_seq_len:
        raise ValueError(f"draft: its max_seq_len {draft.max_seq_len} is shorter than the target's {model.max_seq_len}")
    target_pair, draft_pair = hasattr(model, "image_encoder"), hasattr(draft, "image_encoder")
    if draft_pair and not target_pair:
        raise ValueError("draft: a MultimodalTransformer drafts for a MultimodalTransformer only")
    if target_pair and not draft_pair:
        if draft_source not in ("image", "audio"):
            raise ValueError('draft: a unimodal draft of a multimodal target needs draft_source="image" or "audio"')
        side = 0 if draft_source == "image" else 1
        encode = lambda pair: draft._encode_input(pair[side])                       # noqa: E731
    else:
        if draft_source is not None:
            raise ValueError("draft_source goes with a unimodal draft of a multimodal target only")
        encode = draft._encode_input
    check_row_widths("target", model.decoder)
    check_row_widths("draft", draft.decoder)
    return SpecOptions(draft=draft, k=draft_len, encode=encode)


def spec_option(fn):
    """Gives an evaluation entry point (`predict` / `predict_with_probs` / `evaluate` of both model classes) the keywords
    `draft` (a model with the target's vocabulary, or None: no speculation), `draft_len` (proposals per cycle, 1..31, default 4) and
    `draft_source` ("image" / "audio": what a unimodal draft of a multimodal target reads), like `refill_option`: the function's
    own parameter list stays as it is and the options hold for the duration of the call; `_predict` asks `active_spec()`.  It is the
    outermost option, so it sees -- without consuming them -- the `beam`, `grammar` and `refill` keywords it does not combine with.
    Without a draft nothing is allocated or launched.  The statistics of the call are left in `model.last_spec_stats`."""
    @functools.wraps(fn)
    def call(self, *args, draft=None, draft_len=4, draft_source=None, **kwargs):
        if draft is None:
            if draft_source is not None:
                raise ValueError("draft_source goes with draft=")
            return fn(self, *args, **kwargs)
        opts = check_draft(self, draft, draft_len, draft_source, kwargs)
        self.last_spec_stats = {"cycles": 0, "drafted": 0, "accepted": 0, "tokens": 0}
        token = _SPEC.set(opts)
        try:
            return fn(self, *args, **kwargs)
        finally:
            _SPEC.reset(token)
    return call


def no_draft_option(fn):
    """For the late-fusion entry points (weighted_predict / weighted_evaluate, sw_predict / sw_evaluate): `draft=` (and `draft_len=`,
    `draft_source=`) is refused with ValueError before anything is encoded -- two models decode in lock-step there, and a draft for
    the pair is a later change.  draft=None passes, so a caller may hand the keyword through."""
    @functools.wraps(fn)
    def call(*args, draft=None, draft_len=None, draft_source=None, **kwargs):
        if draft is not None or draft_len is not None or draft_source is not None:
            raise ValueError(f"{fn.__name__} does not take draft=: speculative decoding covers predict / predict_with_probs / evaluate of one model")
        return fn(*args, **kwargs)
    return call


_CTC_DECODE = contextvars.ContextVar("omr_ctc_decode", default=None)


def active_ctc_decode() -> Optional[float]:
    """The CTC weight of the joint CTC / attention beam search the call under way asked for (`ctc_decode_option`), or None: the beam
    search ranks by the attention log-probabilities alone."""
    return _CTC_DECODE.get()


def check_ctc_decode_call(model, weight, beam, others: dict) -> float:
    """Every refusal of `ctc_decode=`, before anything is encoded -> the weight."""
    from .decoder import MAX_BEAM
    from .kernels import check_ctc_decode
    weight = check_ctc_decode(weight)
    if hasattr(model, "image_encoder"):
        raise ValueError("ctc_decode= is for Transformer: the CTC head reads ONE feature grid as a frame sequence, not the mixed memory of "
                         "MultimodalTransformer")
    if getattr(model, "ctc_weight", 0.0) <= 0:
        raise ValueError("ctc_decode= needs the CTC head: build the model with ModelConfig(ctc_weight > 0)")
    if isinstance(beam, bool) or not isinstance(beam, int) or not 2 <= beam <= MAX_BEAM:
        raise ValueError(f"ctc_decode= re-ranks the candidates of a beam search: beam must be an integer in 2..{MAX_BEAM}, got {beam!r}")
    if others.get("grammar", None) is not None or getattr(model, "decode_grammar", None) is not None and "grammar" not in others:
        raise ValueError("ctc_decode= does not combine with a grammar (grammar= or decode_grammar) yet")
    if others.get("refill", False):
        raise ValueError("ctc_decode= does not combine with refill=True: refill decodes greedily")
    if others.get("draft", None) is not None:
        raise ValueError("ctc_decode= does not combine with draft=: speculative decoding is greedy")
    return weight


def ctc_decode_option(beam_default: int, beam_at: Optional[int] = None):
    """Gives a decode entry point of a model the keyword `ctc_decode` (the CTC weight, strictly between 0 and 1; None: off), like
    `grammar_option`: the function's own parameter list stays as it is, and the weight holds for the duration of the call; `beam_search`
    and the batched beam state ask `active_ctc_decode`.  It is the outermost option, so it sees -- without consuming them -- the `beam`,
    `grammar`, `refill` and `draft` keywords it checks (`check_ctc_decode_call`).  beam_default: the beam of a call that names none;
    beam_at: where a positional beam sits behind `self`.  Without the keyword nothing is allocated or launched."""
    def wrap(fn):
        @functools.wraps(fn)
        def call(self, *args, ctc_decode=None, **kwargs):
            if ctc_decode is None:
                return fn(self, *args, **kwargs)
            beam = args[beam_at] if beam_at is not None and len(args) > beam_at else kwargs.get("beam", beam_default)
            token = _CTC_DECODE.set(check_ctc_decode_call(self, ctc_decode, beam, kwargs))
            try:
                return fn(self, *args, **kwargs)
            finally:
                _CTC_DECODE.reset(token)
        return call
    return wrap


def no_ctc_decode_option(fn):
    """For the late-fusion entry points, like `no_draft_option`: `ctc_decode=` is refused with ValueError before anything is encoded -- two
    models decode in lock-step there, and a CTC score for the pair is a later change.  ctc_decode=None passes."""
    @functools.wraps(fn)
    def call(*args, ctc_decode=None, **kwargs):
        if ctc_decode is not None:
            raise ValueError(f"{fn.__name__} does not take ctc_decode=: the joint CTC / attention search covers beam_search / beam_search_batch / "
                             "predict / evaluate of one Transformer")
        return fn(*args, **kwargs)
    return call


def plan_groups(lengths: Sequence[int], batch_size: int, window: int = 0) -> Tuple[List[int], List[List[int]]]:
    """-> (singles, groups) over the indices of `lengths` (memory lengths in tokens).  singles: memories decoded alone at batch
    size 1 -- at most MIN_RAGGED_MEMORY tokens (such a row alone takes another attention kernel than the ragged batch) or
    more than MAX_RAGGED_MEMORY (decoder.takes_ragged_state).  groups: the other indices, sorted by decreasing length (ties:
    input order) within consecutive windows of `window` inputs (0: one window) and cut into groups of at most batch_size, so
    that the rows of a group have similar lengths.  Every index appears exactly once.  This is plan_pair_groups of pairs
    whose two memories are the same one: 2 * length orders like length."""
    return plan_pair_groups(lengths, lengths, batch_size, window)


def plan_pair_groups(len_a: Sequence[int], len_b: Sequence[int], batch_size: int,
                     window: int = 0) -> Tuple[List[int], List[List[int]]]:
    """plan_groups for PAIRS of memories decoded by two models in lock-step (weighted late fusion): pair i has len_a[i] tokens
    for one model and len_b[i] for the other.  singles: pairs of which EITHER memory has at most MIN_RAGGED_MEMORY or more
    than MAX_RAGGED_MEMORY tokens (decoded alone, through the batch-size-1 path).  groups: the other indices, sorted by
    decreasing len_a + len_b (ties: input order; the key affects speed only, never results) within consecutive windows of
    `window` pairs (0: one window) and cut into groups of at most batch_size.  Every index appears exactly once."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    if len(len_a) != len(len_b):
        raise ValueError(f"plan_pair_groups: {len(len_a)} lengths for one model, {len(len_b)} for the other")

    def ragged(i: int) -> bool:
        return takes_ragged_state(len_a[i]) and takes_ragged_state(len_b[i])

    n = len(len_a)
    window = window if window > 0 else max(n, 1)
    singles: List[int] = []
    groups: List[List[int]] = []
    for w0 in range(0, n, window):
        idx = range(w0, min(n, w0 + window))
        singles += [i for i in idx if not ragged(i)]
        rest = sorted((i for i in idx if ragged(i)), key=lambda i: (-(len_a[i] + len_b[i]), i))
        groups += [rest[g:g + batch_size] for g in range(0, len(rest), batch_size)]
    return singles, groups


def decode_rows(step: Callable, rows: int, eos: int, budget: int, sync_every: int,
                want_probs: bool = False, gstate=None) -> Tuple[List[List[int]], List[List[float]]]:
    """THE chunked read-back loop of every greedy decode (one model or two in lock-step, one row or a ragged batch): ->
    (token ids, top-1 values) per row, each row cut after its <eos> (`eos`, kept) or after `budget` positions.
    step(n) runs up to n further positions of all rows and returns (tokens, values) as host lists [m][rows], 1 <= m <= n
    -- values only with want_probs, else None; it raises when it cannot advance.  The chosen tokens reach the next position
    on the device, so the loop handles host lists only: the caller's `step` does the one read-back (two with values) per
    chunk.  What a finished row computed after its <eos> is dropped (at most sync_every - 1 positions in vain); `step` is
    not asked again once every row is done.  Without want_probs the value lists stay empty.
    gstate (grammar.GrammarState, or None): the automaton state `step` decodes under; every row is put to the start state here,
    before the first position, and the device advances it from then on (a finished row sits in the sink state)."""
    if gstate is not None:
        gstate.reset()
    out: List[List[int]] = [[] for _ in range(rows)]
    values: List[List[float]] = [[] for _ in range(rows)]
    done = [False] * rows
    left = budget
    while left > 0 and not all(done):
        toks, top1 = step(min(sync_every, left))
        for s, row in enumerate(toks):
            for b, t in enumerate(row):
                if not done[b]:
                    out[b].append(t)
                    if want_probs:
                        values[b].append(float(top1[s][b]))
                    done[b] = t == eos
        left -= len(toks)
    return out, values


def decode_spec(first, cycles: Callable, plain: Callable, rows: int, eos: int, budget: int, R: int, sync_every: int,
                want_probs: bool = False) -> Tuple[List[List[int]], List[List[float]]]:
    """The read-back loop of a speculative greedy decode (decoder.SpecDecodeState), next to `decode_rows` and with its result:
    (token ids, top-1 values) per row, each cut after its <eos> (kept) or after `budget` positions.
    first: (tokens [rows], values [rows] or None) of position 0, which the caller ran with the plain step.
    cycles(n, t_max) enqueues n cycles of R = k + 1 positions each and returns, per row, the tokens (and values, or None) the
    cycles appended to that row's run -- between 1 and R per cycle for a live row, none for a finished one; t_max is the furthest
    live row's position, and n is bounded here so that t_max + n * R <= budget: a cycle advances a row by at most R.
    plain(n, pos) runs n plain positions of every row, row b from pos[b] (0 for a finished row), and returns (tokens, values) as
    host lists [n][rows]: the last fewer-than-R positions before `budget`, where a cycle no longer fits.  Once the plain steps
    have begun the rows stay with them.  Touches host lists and the two callbacks only."""
    if rows < 1 or sync_every < 1 or R < 2:
        raise ValueError(f"decode_spec: rows {rows}, sync_every {sync_every} must be >= 1 and R {R} >= 2")
    out: List[List[int]] = [[] for _ in range(rows)]
    values: List[List[float]] = [[] for _ in range(rows)]
    if budget <= 0:
        return out, values
    done = [False] * rows

    def append(b: int, t: int, v) -> None:
        out[b].append(int(t))
        if want_probs:
            values[b].append(float(v))
        done[b] = int(t) == eos or len(out[b]) >= budget

    for b in range(rows):
        append(b, first[0][b], first[1][b] if want_probs else None)
    while not all(done):
        t_max = max(len(out[b]) for b in range(rows) if not done[b])
        n = min(sync_every, (budget - t_max) // R)
        if n < 1:
            break
        new_t, new_v = cycles(n, t_max)
        for b in range(rows):
            if done[b]:
                continue
            if not len(new_t[b]):
                raise RuntimeError("decode_spec: a live row did not advance")
            for i, t in enumerate(new_t[b]):
                append(b, t, new_v[b][i] if want_probs else None)
                if done[b]:
                    break
    while not all(done):
        pos = [0 if done[b] else len(out[b]) for b in range(rows)]
        toks, top1 = plain(min(sync_every, budget - max(pos)), pos)
        for s, row in enumerate(toks):
            for b in range(rows):
                if pos[b] and not done[b]:
                    append(b, row[b], top1[s][b] if want_probs else None)
    return out, values


def stream_order(lengths: Sequence[int]) -> List[int]:
    """Admission order of decode_stream: the indices of `lengths` by decreasing length (ties: input order), so that the rows
    running side by side have similar memories.  The order affects speed only, never results."""
    return sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))


def decode_stream(step: Callable, admit: Callable, order: Sequence[int], rows: int, eos: int, budget: int, sync_every: int,
                  want_probs: bool = False, gstate=None) -> Tuple[List[List[int]], List[List[float]]]:
    """decode_rows with a QUEUE (continuous batching): `rows` slots decode the inputs `order` (a permutation of
    0 .. len(order) - 1, admitted in that order) -> (token ids, top-1 values) per INPUT index, each cut after its <eos> (kept)
    or after `budget` positions of that input.  After every chunk the finished rows are cut, and each freed slot goes to the
    next waiting input; the loop ends when the queue is empty and every slot is done.
    admit(slot, index) hands `slot` to input `index`, which starts at position 0; admit(slot, None) leaves it idle (nothing
    waits; whatever it computes is dropped).  step(n) runs n further positions of all slots and returns (tokens, values) as host
    lists [m][rows], 1 <= m <= n -- values only with want_probs, else None; it raises when it cannot advance.  n never takes a
    live row past its budget.  Like decode_rows this touches host lists and the two callbacks only -- and gstate
    (grammar.GrammarState, or None), the automaton state `step` decodes under: a slot's entry is put to the start state at the
    read-back that admits its next input, where `admit` sets its token."""
    n_in = len(order)
    if sorted(order) != list(range(n_in)):
        raise ValueError("decode_stream: `order` must be a permutation of the input indices")
    if rows < 1 or sync_every < 1:
        raise ValueError(f"decode_stream: rows {rows} and sync_every {sync_every} must be >= 1")
    out: List[List[int]] = [[] for _ in range(n_in)]
    values: List[List[float]] = [[] for _ in range(n_in)]
    if budget <= 0:
        return out, values
    waiting = list(order)[::-1]
    holds: List = [None] * rows                       # the input each slot decodes
    used = [0] * rows                                  # positions of that input so far

    def refill(b: int) -> None:
        holds[b] = waiting.pop() if waiting else None
        used[b] = 0
        admit(b, holds[b])
        if gstate is not None:
            gstate.reset_row(b)

    for b in range(rows):
        refill(b)
    while any(i is not None for i in holds):
        live = [b for b in range(rows) if holds[b] is not None]
        toks, top1 = step(min(sync_every, min(budget - used[b] for b in live)))
        for b in live:
            i = holds[b]
            for s, row in enumerate(toks):
                out[i].append(row[b])
                if want_probs:
                    values[i].append(float(top1[s][b]))
                used[b] += 1
                if row[b] == eos or used[b] >= budget:
                    refill(b)
                    break
    return out, values


def beam_backtrack(hist_parent, hist_token, row: int, position: int) -> List[int]:
    """The tokens of the hypothesis that sat in row `row` of ONE input after `position` positions of a beam search, from that
    input's history tables: hist_parent[p][r] is the row (of position p - 1) that row r of position p continued, hist_token[p][r]
    the token it took.  position 0: the empty prefix."""
    out: List[int] = []
    for p in range(position - 1, -1, -1):
        out.append(int(hist_token[p][row]))
        row = int(hist_parent[p][row])
    return out[::-1]


def beam_results(beam: int, positions: int, eos: int, scores, best_score, best_row, best_pos, done, hist_parent,
                 hist_token, dead_end=None) -> List[Tuple[List[int], float]]:
    """(token ids, score) of every input of a batched beam search from its device state read back (BeamDecodeState.snapshot;
    rows n * beam .. n * beam + beam - 1 belong to input n), after `positions` positions.  The finished hypothesis
    (best_score, best_row, best_pos) is the prefix of row best_row before position best_pos, plus <eos>.  An input that is not
    done ran out of positions: its best unfinished hypothesis (row 0) wins iff its score is greater than the best finished
    one -- the last two lines of _Base.beam_search.  dead_end (the joint CTC / attention search only: per input the position at which it
    stopped): an input that is done with nothing finished met candidates of -inf alone; its result is row 0 of the last position it
    survived, whose score its frozen state still holds."""
    out: List[Tuple[List[int], float]] = []
    for n in range(len(best_score)):
        r0 = n * beam
        hp = [row[r0:r0 + beam] for row in hist_parent[:positions]]
        ht = [row[r0:r0 + beam] for row in hist_token[:positions]]
        score, seq = float(best_score[n]), None
        if score > float("-inf"):
            seq = beam_backtrack(hp, ht, int(best_row[n]), int(best_pos[n])) + [eos]
        if not done[n] and float(scores[r0]) > score:
            score, seq = float(scores[r0]), beam_backtrack(hp, ht, 0, positions)
        if seq is None and dead_end is not None and done[n]:
            score, seq = float(scores[r0]), beam_backtrack(hp, ht, 0, int(dead_end[n]))
        if seq is None:
            raise RuntimeError(f"beam search: input {n} has neither a finished nor a live hypothesis")
        out.append((seq, score))
    return out


# ------------------------------------------------------------------------------------------------ alignment (attention maps)

ALIGN_MAP_BYTES = 1 << 30   # `align` cuts its groups so that the fp32 map buffer B * Tmax * Smax * 4 of a group stays under this
GRID_ROW_PIXELS, GRID_COL_PIXELS = 16, 8      # encoder.HEIGHT_REDUCTION / WIDTH_REDUCTION: one memory row covers 16 x 8 input pixels


@dataclass
class Alignment:
    """Where the decoder looked for each token of one input (`Transformer.align` / `MultimodalTransformer.align`): token t of
    `words` leaned most on memory row index[t], with head- and layer-averaged cross-attention weight weight[t]; that row is
    cell[t] = (row, column) of the encoder grid of its source[t] ("image" / "audio") and covers box[t] = (top, left, bottom,
    right) input pixels (bottom / right exclusive, clipped to the input).  maps: the whole distributions, fp32 [n, S] on the
    device, when asked for."""
    words: List[str]
    index: np.ndarray            # int64 [n]
    weight: np.ndarray           # float32 [n]
    cell: np.ndarray             # int64 [n, 2]
    box: np.ndarray              # int64 [n, 4]
    source: List[str]
    maps: Optional[object] = None


def grid_of(height: int, width: int) -> Tuple[int, int]:
    """The encoder grid (h', w') = (ceil(h / 16), ceil(w / 8)) of an input of height x width pixels."""
    return -(-int(height) // GRID_ROW_PIXELS), -(-int(width) // GRID_COL_PIXELS)


def cells_and_boxes(index, sizes, split: Optional[int] = None):
    """Memory row -> encoder cell, input pixels and source.  index: the memory rows, int [n].  sizes: one (source, height, width)
    per grid the memory is made of, in memory order -- one entry for a single encoder's memory (or an attention mixer's, whose
    memory lives on the query grid), two for a concatenated memory, whose first grid holds rows [0, split) and whose second
    grid starts at row `split` (the image memory's length; checked against the first grid).  -> (cell int64 [n, 2] = (s // w',
    s % w') on that grid, box int64 [n, 4] = (top, left, bottom, right) in that input's pixels clipped to its size, source
    [n]).  Pure host arithmetic."""
    idx = np.asarray(index, dtype=np.int64).reshape(-1)
    sizes = [(str(src), int(h), int(w)) for src, h, w in sizes]
    if len(sizes) not in (1, 2):
        raise ValueError(f"a memory is one grid or two concatenated ones, got {len(sizes)} sizes")
    grids = [grid_of(h, w) for _, h, w in sizes]
    if len(sizes) == 2:
        first = grids[0][0] * grids[0][1]
        if split is None:
            split = first
        if split != first:
            raise ValueError(f"split {split} is not the length {first} of the first grid {grids[0]}")
    elif split is not None:
        raise ValueError("split belongs to a memory of two grids")
    starts = [0, split] if len(sizes) == 2 else [0]
    total = sum(gh * gw for gh, gw in grids)
    if idx.size and (idx.min() < 0 or idx.max() >= total):
        raise ValueError(f"memory rows must lie in [0, {total}), got {int(idx.min())} .. {int(idx.max())}")
    part = (idx >= split).astype(np.int64) if len(sizes) == 2 else np.zeros_like(idx)
    cell = np.zeros((idx.size, 2), dtype=np.int64)
    box = np.zeros((idx.size, 4), dtype=np.int64)
    for g, ((_, h, w), (gh, gw)) in enumerate(zip(sizes, grids)):
        sel = part == g
        s = idx[sel] - starts[g]
        r, c = s // gw, s % gw
        cell[sel] = np.stack([r, c], axis=1)
        box[sel] = np.stack([r * GRID_ROW_PIXELS, c * GRID_COL_PIXELS, np.minimum((r + 1) * GRID_ROW_PIXELS, h),
                             np.minimum((c + 1) * GRID_COL_PIXELS, w)], axis=1)
    return cell, box, [sizes[g][0] for g in part.tolist()]


def plan_align_groups(targets: Sequence[int], memories: Sequence[int], batch_size: int, limit_bytes: Optional[int] = None) -> List[List[int]]:
    """Consecutive groups of input indices for `align`: at most batch_size rows each, cut further so that the group's fp32 map
    buffer rows * max(targets) * max(memories) * 4 stays within limit_bytes (default ALIGN_MAP_BYTES, read at call time); an input
    that exceeds the limit alone is a group of its own."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    limit = ALIGN_MAP_BYTES if limit_bytes is None else limit_bytes
    groups: List[List[int]] = []
    cur: List[int] = []
    tmax = smax = 0
    for i, (t, s) in enumerate(zip(targets, memories)):
        t2, s2 = max(tmax, t), max(smax, s)
        if cur and (len(cur) >= batch_size or (len(cur) + 1) * t2 * s2 * 4 > limit):
            groups.append(cur)
            cur, t2, s2 = [], t, s
        cur.append(i)
        tmax, smax = t2, s2
    if cur:
        groups.append(cur)
    return groups
