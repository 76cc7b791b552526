"""Numpy restatements for grammar-constrained decoding: what the constrained kernels and drivers must compute, written without
them.  `allowed` is always a bool mask over the vocabulary; a forbidden logit is replaced by -inf BEFORE anything else looks at it
(so NaN / +inf there vanish), which is the whole definition of the masked load."""
import numpy as np

NINF = float("-inf")


def mask_logits(x, allowed):
    """fp32 copy of x with -inf where `allowed` is False (x, allowed broadcastable over rows)."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(np.asarray(allowed, dtype=bool), x, np.float32(NINF)).astype(np.float32)


def masked_argmax(x, allowed):
    """-> (index, value) per row: the first index of the largest allowed logit (torch.argmax's tie rule) and that logit."""
    m = np.atleast_2d(mask_logits(x, allowed))
    idx = np.array([int(np.flatnonzero(row == row.max())[0]) for row in m], dtype=np.int64)
    return idx, m[np.arange(m.shape[0]), idx]


def log_softmax32(m):
    """log_softmax of fp32 rows, computed in fp32: x - (max + log(sum(exp(x - max))))."""
    m = np.atleast_2d(np.asarray(m, dtype=np.float32))
    mx = m.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        lse = mx + np.log(np.exp(m - mx, dtype=np.float32).sum(axis=1, keepdims=True, dtype=np.float32), dtype=np.float32)
        return (m - lse).astype(np.float32)


def topk_ordered(values, k):
    """Indices of the k largest entries per row, by (value descending, index ascending); -inf entries rank last, by index."""
    values = np.atleast_2d(values)
    return np.stack([np.lexsort((np.arange(row.size), -row))[:k] for row in values]).astype(np.int64)


def masked_topk_log_softmax(x, allowed, k):
    """-> (indices [rows, k], log-probabilities [rows, k]): the k best of log_softmax over the ALLOWED tokens (renormalised),
    ties towards the smaller index.  Where fewer than k tokens are allowed the rest are forbidden tokens at -inf, by index."""
    lp = log_softmax32(mask_logits(x, allowed))
    idx = topk_ordered(lp, k)
    return idx, np.take_along_axis(lp, idx, axis=1)


def masked_weighted_mix(la, lb, allowed, alpha):
    """alpha * softmax(mask(la)) + (1 - alpha) * softmax(mask(lb)) per row in fp32: two rounded products and one add, the weights
    rounded to fp32 once each (torch's `alpha * p + (1 - alpha) * q` on fp32 tensors)."""
    def softmax(m):
        m = np.atleast_2d(m)
        e = np.exp(m - m.max(axis=1, keepdims=True), dtype=np.float32)
        return (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)
    wa, wb = np.float32(alpha), np.float32(1.0 - float(alpha))
    return (wa * softmax(mask_logits(la, allowed))).astype(np.float32) + (wb * softmax(mask_logits(lb, allowed))).astype(np.float32)


def masked_weighted_topk(la, lb, allowed, alpha, k):
    """-> (indices [rows, k], log of the mixed probability [rows, k]) of masked_weighted_mix, ties towards the smaller index."""
    p = masked_weighted_mix(la, lb, allowed, alpha)
    idx = topk_ordered(p, k)
    with np.errstate(divide="ignore"):
        return idx, np.log(np.take_along_axis(p, idx, axis=1), dtype=np.float32)


def state_walk(next_table, token_class, start, ids):
    """The states after each token of ids from `start`; -1 from the first forbidden token on."""
    s, out = int(start), []
    for t in ids:
        if s >= 0:
            s = int(next_table[s][token_class[int(t)]])
        out.append(s)
    return out


def allowed_mask(next_table, token_class, state):
    """bool [V]: the tokens allowed in `state`."""
    return np.asarray(next_table)[int(state)][np.asarray(token_class)] >= 0


def select_body(idx, val, beam, eos, scores, best_done, t, next_table=None, token_class=None, states=None):
    """The body of the position loop of _Base.beam_search on the top-k lists (idx, val [beam][beam]) of ONE input's rows, with the
    liveness rule of the constrained selection: a candidate (parent b, token) counts only if its parent is live
    (scores[b] > -inf) AND next[states[b]][class[token]] >= 0 -- by the table, whatever its value.  states None: no grammar.
    best_done: (score, parent row, position).  -> (stopped, best_done, parents, tokens, scores, states); on `stopped` the last
    four are the inputs' (nothing is reordered)."""
    cands = []
    for b in range(beam):
        if not scores[b] > NINF:
            continue
        for j in range(beam):
            tk = int(idx[b][j])
            ns = -2 if states is None else int(next_table[states[b]][token_class[tk]])
            if states is None or ns >= 0:
                cands.append((float(scores[b]) + float(val[b][j]), b, tk, ns))
    cands.sort(key=lambda c: (-c[0], c[1], c[2]))
    parents, new_tok, new_scores, new_states = [], [], [], []
    for sc, b, tk, ns in cands:
        if tk == eos:
            if sc > best_done[0]:
                best_done = (sc, b, t)
            continue
        parents.append(b); new_tok.append(tk); new_scores.append(sc); new_states.append(ns)
        if len(parents) == beam:
            break
    if not parents or new_scores[0] <= best_done[0]:
        return True, best_done, None, None, None, None
    while len(parents) < beam:                      # dead padding rows: copies of the first survivor
        parents.append(parents[0]); new_tok.append(new_tok[0]); new_scores.append(NINF); new_states.append(new_states[0])
    return False, best_done, parents, new_tok, new_scores, (None if states is None else new_states)


def host_beam_loop(step, topk, beam, sos, eos, max_len, next_table, token_class, start):
    """The host beam loop of _Base.beam_search under an automaton, for ONE input.  step(tokens [beam], parents [beam] or None) ->
    the fp32 logits [beam, V] (per model: a tuple of them) of the next position after reordering the hypotheses by `parents`;
    topk(masked logits ...) -> (idx, val) [beam][beam], the k best log-probabilities of the masked rows.  -> (token ids, score):
    the best finished hypothesis, or the best live one if the positions ran out and it scores higher."""
    scores = [0.0] + [NINF] * (beam - 1)
    states = [int(start)] * beam
    seqs = [[] for _ in range(beam)]
    tokens, parents = [sos] * beam, None
    best = (NINF, None)
    exhausted = True
    for t in range(max_len):
        logits = step(tokens, parents)
        allowed = np.stack([allowed_mask(next_table, token_class, s) for s in states])
        many = isinstance(logits, tuple)
        masked = tuple(mask_logits(x, allowed) for x in logits) if many else (mask_logits(logits, allowed),)
        idx, val = topk(*masked)
        stopped, bd, par, tok, sc, st = select_body(idx, val, beam, eos, scores, (best[0], 0, 0), t, next_table, token_class, states)
        if bd[0] > best[0]:
            best = (bd[0], seqs[bd[1]] + [eos])
        if stopped:
            exhausted = False
            break
        seqs = [seqs[p] + [k] if s > NINF else [] for p, k, s in zip(par, tok, sc)]
        scores, states, tokens, parents = sc, st, tok, par
    if exhausted and scores[0] > best[0]:
        best = (scores[0], seqs[0])
    return best[1], best[0]
