"""Token automata for grammar-constrained decoding (an extension: the reference picks over the whole vocabulary at every
position, src/transformer/model.py:182-193, so nothing keeps a transcript inside the token stream its own encoder produces,
src/data/encoding.py `encode`).

A `Grammar` is a deterministic automaton over token ids, compressed by token class: `token_class[v]` names the class of
vocabulary entry v and `next[s][c]` the state after a token of class c in state s, or -1 where that token is forbidden.  The
decode kernels (include/omr_hip.h "grammar-constrained decoding") read a forbidden token's logit as -inf and advance one
int32 state per row on the device; this module is the host side: the checked tables, their device copies, the host walk the
tests compare against, and `kern_grammar`, the automaton of the reference's **kern token stream.

A constrained decode that reaches its length budget before an accepting state returns a VALID PREFIX (`prefix_ok`), not a
complete sequence (`accepts`): forcing completion is not attempted.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np

MAX_CLASSES = 256          # OMR_GRAMMAR_MAX_CLASSES: a state's `next` row is staged in 256 ints of LDS, classes are bytes


class _GrammarDesc(ctypes.Structure):
    """omr_grammar_desc of include/omr_hip.h."""
    _fields_ = [("cls", ctypes.c_void_p), ("next", ctypes.c_void_p), ("S", ctypes.c_int), ("C", ctypes.c_int), ("state", ctypes.c_void_p)]


class Grammar:
    """Grammar(token_class, next, start, eos=1).  token_class: one class id per vocabulary entry [V], C <= 256 classes; next:
    int [S, C], -1 = forbidden; start: the state before the first predicted token; eos: the id of <eos> (default: the id layout of
    synthetic.make_vocab).  <eos> must have a class of its own; a state ACCEPTS iff <eos> is allowed in it.  The constructor
    appends a sink state S in which only <eos> is allowed and points every <eos> transition there, so a finished row that keeps
    running keeps a valid state; `self.next` is the [S + 1, C] table the device reads, `self.sink` = S.
    Refused (ValueError): a class id >= C (or < 0), more than 256 classes, a table target outside [-1, S), a start outside
    [0, S), <eos> sharing its class, a reachable state with no allowed token, a reachable state from which no accepting state
    can be reached.  (A class without a vocabulary entry allows nothing.)  Hence no row ever meets a state in which everything
    is forbidden."""

    def __init__(self, token_class, next, start: int, eos: int = 1):
        cls = np.asarray(token_class)
        nxt = np.asarray(next)
        if cls.ndim != 1 or cls.size < 1 or nxt.ndim != 2 or nxt.shape[0] < 1 or nxt.shape[1] < 1:
            raise ValueError(f"grammar: token_class must be [V] and next [S, C], got {cls.shape} and {nxt.shape}")
        if not (np.issubdtype(cls.dtype, np.integer) and np.issubdtype(nxt.dtype, np.integer)):
            raise ValueError("grammar: token_class and next hold integers")
        S, C = int(nxt.shape[0]), int(nxt.shape[1])
        if C > MAX_CLASSES:
            raise ValueError(f"grammar: {C} classes, at most {MAX_CLASSES}")
        if cls.min() < 0 or cls.max() >= C:
            raise ValueError(f"grammar: class ids must lie in [0, {C}), got {int(cls.min())} .. {int(cls.max())}")
        if nxt.min() < -1 or nxt.max() >= S:
            raise ValueError(f"grammar: table targets must lie in [-1, {S}), got {int(nxt.min())} .. {int(nxt.max())}")
        if not 0 <= int(start) < S:
            raise ValueError(f"grammar: start state {start} outside [0, {S})")
        V = int(cls.size)
        if not 0 <= int(eos) < V:
            raise ValueError(f"grammar: <eos> id {eos} outside the vocabulary of {V}")
        eos_class = int(cls[eos])
        if int((cls == eos_class).sum()) != 1:
            raise ValueError("grammar: <eos> must have a class of its own")
        full = np.full((S + 1, C), -1, dtype=np.int32)
        full[:S] = nxt
        full[:, eos_class] = np.where(full[:, eos_class] >= 0, S, -1)
        full[S, eos_class] = S
        self.V, self.S, self.C, self.sink = V, S + 1, C, S
        self.start, self.eos, self.eos_class = int(start), int(eos), eos_class
        self.token_class = cls.astype(np.uint8)
        self.next = full
        self._device: Dict[str, Tuple] = {}
        self._check_reachable()

    def _check_reachable(self) -> None:
        used = np.zeros(self.C, dtype=bool)
        used[self.token_class] = True                       # classes that have a vocabulary entry
        allowed = (self.next >= 0) & used[None, :]
        seen, todo = {self.start}, [self.start]
        while todo:
            s = todo.pop()
            for c in np.nonzero(allowed[s])[0]:
                n = int(self.next[s, c])
                if n not in seen:
                    seen.add(n)
                    todo.append(n)
        for s in sorted(seen):
            if not allowed[s].any():
                raise ValueError(f"grammar: reachable state {s} allows no token")
        good = {s for s in seen if allowed[s, self.eos_class]}          # accepting; grown backwards to a fixed point
        grew = True
        while grew:
            grew = False
            for s in seen - good:
                if any(int(self.next[s, c]) in good for c in np.nonzero(allowed[s])[0]):
                    good.add(s)
                    grew = True
        stuck = sorted(seen - good)
        if stuck:
            raise ValueError(f"grammar: no accepting state can be reached from reachable state {stuck[0]}")

    # ---- host walk
    def walk(self, ids: Iterable[int], state: int = None) -> List[int]:
        """The state after each token of `ids`, from `state` (default: start); -1 from the first forbidden token on."""
        s = self.start if state is None else int(state)
        out: List[int] = []
        for t in ids:
            if s >= 0:
                s = int(self.next[s, self.token_class[int(t)]]) if 0 <= int(t) < self.V else -1
            out.append(s)
        return out

    def prefix_ok(self, ids: Sequence[int]) -> bool:
        """Whether every token of `ids` is allowed where it stands (the empty sequence is)."""
        ids = list(ids)
        return not ids or self.walk(ids)[-1] >= 0

    def accepts(self, ids: Sequence[int]) -> bool:
        """Whether `ids` is a complete sequence: a valid prefix whose only <eos> is its last token."""
        ids = list(ids)
        return bool(ids) and ids[-1] == self.eos and ids.count(self.eos) == 1 and self.prefix_ok(ids)

    def allowed(self, state: int) -> np.ndarray:
        """bool [V]: the tokens allowed in `state`."""
        return self.next[int(state)][self.token_class] >= 0

    # ---- constructors
    @classmethod
    def permissive(cls, V: int, eos: int, forbid: Iterable[int] = ()) -> "Grammar":
        """One state in which everything is allowed except the ids `forbid` (plus the sink behind <eos>)."""
        tc = np.zeros(V, dtype=np.int64)
        tc[eos] = 1
        forbid = sorted(set(int(f) for f in forbid))
        if eos in forbid:
            raise ValueError("grammar: <eos> cannot be forbidden")
        tc[forbid] = 2
        return cls(tc, np.array([[0, 0, -1]] if forbid else [[0, 0]], dtype=np.int32), 0, eos)

    # ---- device side
    def to(self, device):
        """(token_class uint8 [V], next int32 [S, C]) as tensors on `device`, uploaded once per device."""
        import torch
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = (torch.from_numpy(self.token_class.copy()).to(device), torch.from_numpy(self.next.copy()).to(device))
        return self._device[key]

    def bind(self, rows: int, device) -> "GrammarState":
        """The per-row device state of one decode (`rows` int32 entries, all at `start`) with its descriptor."""
        return GrammarState(self, rows, device)


class GrammarState:
    """One decode's automaton state: int32 [rows] on the device, advanced by the kernels, plus the omr_grammar_desc the
    *_grammar entries take.  The decode loop (evaluation.decode_rows / decode_stream) resets it: every row at the start of a
    decode, one row when its slot is handed to the next input."""

    def __init__(self, grammar: Grammar, rows: int, device):
        import torch
        self.grammar, self.rows = grammar, rows
        self.cls, self.next = grammar.to(device)
        self.state = torch.full((rows,), grammar.start, dtype=torch.int32, device=device)
        self.desc = _GrammarDesc()
        self.desc.cls, self.desc.next, self.desc.state = self.cls.data_ptr(), self.next.data_ptr(), self.state.data_ptr()
        self.desc.S, self.desc.C = grammar.S, grammar.C

    def byref(self):
        return ctypes.byref(self.desc)

    def reset(self) -> None:
        self.state.fill_(self.grammar.start)

    def reset_row(self, row: int) -> None:
        self.state[row:row + 1].fill_(self.grammar.start)


def host_mask(grammar: Grammar, states: Sequence[int], device):
    """bool [len(states), V] on `device`: the tokens allowed in each of the host-held `states` (the host-driven beam loops)."""
    import torch
    return torch.from_numpy(np.stack([grammar.allowed(s) for s in states])).to(device)


def check_grammar(grammar, V: int, eos: int):
    """`grammar` (None passes) against the model that is to decode under it."""
    if grammar is None:
        return None
    if not isinstance(grammar, Grammar):
        raise TypeError(f"grammar must be a Grammar or None, got {type(grammar).__name__}")
    if grammar.V != V or grammar.eos != eos:
        raise ValueError(f"grammar: built for a vocabulary of {grammar.V} with <eos> = {grammar.eos}, the model has {V} and {eos}")
    return grammar


# ------------------------------------------------------------------------------------------------ the **kern token stream

EOS_TOKEN = "<eos>"
CON_TOKEN, COC_TOKEN, COR_TOKEN = "<con>", "<coc>", "<cor>"        # src/data/encoding.py:8-10
OPEN_SPINE, CLOSE_SPINE = "*^", "*v"                              # src/data/encoding.py:36-37
SYMBOL, CON, COC, COR, OPEN, CLOSE, EOS, FORBIDDEN = range(8)     # the classes of kern_grammar


def kern_grammar(w2i: Dict[str, int], max_spines: int = 8, spines: bool = True) -> Grammar:
    """The automaton of the reference's token stream (src/data/encoding.py `encode`): rows separated by <cor>, the voices of a row
    by <coc>, the symbols of a voice by <con>.  Classes: symbol (everything else), <con>, <coc>, <cor>, *^, *v, <eos>, forbidden
    (<pad> / <PAD>, <sos>).  Any of these tokens but <eos> may be missing from w2i.

    Level 1, always:
      * symbols (classes symbol, *^, *v) and separators (<con>, <coc>, <cor>) alternate, and a sequence begins with a symbol;
      * <eos> comes only directly after a symbol;
      * <pad> / <sos> never appear.
    Level 2, with spines=True.  A row is a maximal run of tokens without <cor> or <eos>; its voices are the runs between <coc>.
    A voice is an OPEN voice when `*^` is its only symbol, a CLOSE voice when `*v` is its only symbol, else ordinary.
      * The first row has n voices for some 1 <= n <= max_spines: its max_spines-th <coc> is forbidden.
      * Every later row has exactly the n of its predecessor's SUCCESSOR WIDTH: <coc> is forbidden after voice n, <cor> and <eos>
        before voice n is complete.  (<eos> ends the last row, which must be complete as well.)
      * The successor width of a row is: 2 per open voice, 1 per ordinary voice, 1 per maximal run of adjacent close voices
        (that is n, plus one per *^, minus k - 1 per maximal run of k *v).
      * The <cor> after a row whose successor width lies outside [1, max_spines] is forbidden -- <cor> is the token that would
        begin a row of that width (until then a <con> can still turn the last voice into an ordinary one).  <eos> is not:
        nothing follows the last row."""
    if EOS_TOKEN not in w2i:
        raise ValueError("kern_grammar: the vocabulary has no <eos>")
    if max_spines < 1:
        raise ValueError(f"kern_grammar: max_spines must be >= 1, got {max_spines}")
    V = max(w2i.values()) + 1
    tc = np.full(V, SYMBOL, dtype=np.int64)
    named = {CON_TOKEN: CON, COC_TOKEN: COC, COR_TOKEN: COR, OPEN_SPINE: OPEN, CLOSE_SPINE: CLOSE, EOS_TOKEN: EOS,
             "<pad>": FORBIDDEN, "<PAD>": FORBIDDEN, "<sos>": FORBIDDEN}
    for word, c in named.items():
        if word in w2i:
            tc[w2i[word]] = c
    if not spines:
        table = np.full((2, 8), -1, dtype=np.int32)
        table[0, [SYMBOL, OPEN, CLOSE]] = 1              # state 0: a symbol is due; state 1: directly after a symbol
        table[1, [CON, COC, COR]] = 0
        table[1, EOS] = 0                                  # any target: the constructor points <eos> at the sink
        return Grammar(tc, table, 0, w2i[EOS_TOKEN])
    # state = (n, j, m, prev_close, cur): n the row's width (0: the first row), j voices finished, m their successor width
    # (saturating at max_spines + 1), prev_close whether the last finished voice was a close voice, cur the voice under way:
    DUE, ONLY_OPEN, ONLY_CLOSE, ORDINARY, MORE = range(5)      # no symbol yet | *^ alone | *v alone | ordinary, after a symbol | after <con>
    start = (0, 0, 0, 0, DUE)
    index, rows, todo = {start: 0}, [], [start]

    def state_id(st):
        if st not in index:
            index[st] = len(index)
            todo.append(st)
        return index[st]

    while todo:
        st = todo.pop(0)
        n, j, m, prev_close, cur = st
        row = [-1] * 8
        if cur in (DUE, MORE):
            for c, kind in ((SYMBOL, ORDINARY), (OPEN, ONLY_OPEN), (CLOSE, ONLY_CLOSE)):
                row[c] = state_id((n, j, m, prev_close, kind if cur == DUE else ORDINARY))
        else:
            row[CON] = state_id((n, j, m, prev_close, MORE))
            width = m + (2 if cur == ONLY_OPEN else (0 if prev_close else 1) if cur == ONLY_CLOSE else 1)
            width = min(width, max_spines + 1)
            if (j + 1 < max_spines) if n == 0 else (j + 1 < n):
                row[COC] = state_id((n, j + 1, width, int(cur == ONLY_CLOSE), DUE))
            if n == 0 or j + 1 == n:
                if 1 <= width <= max_spines:
                    row[COR] = state_id((width, 0, 0, 0, DUE))
                row[EOS] = 0
        rows.append((index[st], row))
    table = np.full((len(index), 8), -1, dtype=np.int32)
    for i, row in rows:
        table[i] = row
    return Grammar(tc, table, 0, w2i[EOS_TOKEN])

