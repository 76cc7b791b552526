"""Batched evaluation over inputs of different sizes.  The reference validates one input at a time (src/train.py:34,
src/transformer/model.py:171-199, "Inference only supports batch_size = 1"); `predict` / `evaluate` of both model classes
decode groups of memories of different lengths as ONE ragged decode state (Decoder.init_decode on a list), and every
sequence equals the batch-size-1 loop's (`_greedy`) for that input.  This module holds the host-side grouping."""
from __future__ import annotations

from typing import List, Sequence, Tuple

from .decoder import MAX_RAGGED_MEMORY, MIN_RAGGED_MEMORY

WINDOW_BATCHES = 8          # inputs are encoded and sorted by memory length a window of 8 * batch_size at a time


def plan_groups(lengths: Sequence[int], batch_size: int, window: int = 0) -> Tuple[List[int], List[List[int]]]:
    """-> (singles, groups) over the indices of `lengths` (memory lengths in tokens).  singles: memories decoded alone at batch
    size 1 -- at most MIN_RAGGED_MEMORY tokens (such a row alone takes another attention kernel than the ragged batch) or
    more than MAX_RAGGED_MEMORY.  groups: the other indices, sorted by decreasing length (ties: input order) within
    consecutive windows of `window` inputs (0: one window) and cut into groups of at most batch_size, so that the rows of a
    group have similar lengths.  Every index appears exactly once."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    n = len(lengths)
    window = window if window > 0 else max(n, 1)
    singles: List[int] = []
    groups: List[List[int]] = []
    for w0 in range(0, n, window):
        idx = range(w0, min(n, w0 + window))
        singles += [i for i in idx if not MIN_RAGGED_MEMORY < lengths[i] <= MAX_RAGGED_MEMORY]
        rest = sorted((i for i in idx if MIN_RAGGED_MEMORY < lengths[i] <= MAX_RAGGED_MEMORY), key=lambda i: (-lengths[i], i))
        groups += [rest[g:g + batch_size] for g in range(0, len(rest), batch_size)]
    return singles, groups
