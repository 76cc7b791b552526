"""CPU-only checks of batched evaluation over inputs of different sizes: the new entry points of the C ABI, the native edit
distance against the Python reference, the grouping of memories into ragged batches, and the read-back loop of the greedy
decodes against a scripted step."""
import ctypes
import random
import subprocess

import numpy as np
import pytest

from omr_a2s_multimodal_transformer_amd import _lib, metrics
from omr_a2s_multimodal_transformer_amd.decoder import MAX_RAGGED_MEMORY, MIN_RAGGED_MEMORY
from omr_a2s_multimodal_transformer_amd.evaluation import decode_rows, plan_groups, plan_pair_groups

NEW = ("omr_attn_fwd_split_varlen", "omr_decode_steps_varlen", "omr_edit_distance_batch")


def test_new_entry_points_are_declared_and_exported():
    protos = _lib.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T omr_" in line}
    for name in NEW:
        assert name in protos, name
        assert name in exported, name
    assert protos["omr_attn_fwd_split_varlen"][1][19:21] == ["const float* key_bias", "const int* kv_len"]
    assert protos["omr_decode_steps_varlen"][1][:2] == ["const omr_decode_desc* desc", "const int* mem_len"]


def _native(pairs):
    return metrics.edit_distances(pairs)


def test_native_edit_distance_equals_python_reference():
    rng = random.Random(2026)
    pairs = []
    for i in range(500):
        alpha = rng.choice([2, 3, 5, 40])
        la = 0 if i % 50 == 0 else rng.randint(0, 600)
        lb = 0 if i % 70 == 1 else rng.randint(0, 600)
        a = [f"t{rng.randrange(alpha)}" for _ in range(la)]
        b = [f"t{rng.randrange(alpha)}" for _ in range(lb)]
        pairs.append((a, b))
    pairs += [([], []), (["x"], []), ([], ["y", "z"])]
    got = _native(pairs)
    want = [metrics.edit_distance(a, b) for a, b in pairs]
    assert got == want


def test_ed_counts_maps_tokens_of_both_lists_per_call():
    # the same token string on both sides matches whatever ids the vocabularies gave it
    t = [["a", "b", "c"], ["d"], []]
    p = [["b", "c"], ["d"], ["e"]]
    assert metrics.ed_counts(t, p) == [2, 4, 2, 3]
    assert metrics.ed_counts([], []) == [0, 0, 0, 0]


def test_edit_distance_batch_rejects_bad_offsets():
    lib = _lib.lib()
    a = np.array([1, 2], dtype=np.int32)
    off = np.array([2, 0], dtype=np.int64)                 # decreasing offsets
    dist = np.zeros(1, dtype=np.int64)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)
    assert lib.query("omr_edit_distance_batch", vp(a), vp(off), vp(a), vp(off), 1, vp(dist)) != 0


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("batch_size,window", [(4, 0), (4, 32), (3, 5), (1, 0), (32, 256)])
def test_plan_groups_covers_every_input_once(seed, batch_size, window):
    rng = random.Random(seed)
    n = rng.randint(0, 90)
    lengths = [rng.choice([1, 30, 64, 65, 200, 256, 257, 1024, 5000, 12696, MAX_RAGGED_MEMORY, MAX_RAGGED_MEMORY + 1,
                           rng.randint(1, 20000)]) for _ in range(n)]
    singles, groups = plan_groups(lengths, batch_size, window)
    order = singles + [i for g in groups for i in g]
    assert sorted(order) == list(range(n))                 # restoring input order is a scatter by these indices
    assert all(1 <= len(g) <= batch_size for g in groups)
    for i in singles:
        assert lengths[i] <= MIN_RAGGED_MEMORY or lengths[i] > MAX_RAGGED_MEMORY
    for g in groups:
        assert all(MIN_RAGGED_MEMORY < lengths[i] <= MAX_RAGGED_MEMORY for i in g)
        assert [lengths[i] for i in g] == sorted((lengths[i] for i in g), reverse=True)
        if window:
            assert len({i // window for i in g}) == 1       # a group never reaches across windows
    # the permutation round trip: predictions scattered by the plan come back in input order
    preds = [None] * n
    for i in order:
        preds[i] = f"p{i}"
    assert preds == [f"p{i}" for i in range(n)]


def test_plan_groups_rejects_a_bad_batch_size():
    with pytest.raises(ValueError):
        plan_groups([100], 0)


def test_plan_groups_on_a_literal_and_as_pairs_of_one_memory():
    # 64 and 20000 tokens are decoded alone; 65 and 16384 are the ends of the ragged range; ties keep input order
    assert plan_groups([100, 64, 300, 20000, 300, 65, 16384], 2) == ([1, 3], [[6, 2], [4, 0], [5]])
    rng = random.Random(11)
    for _ in range(200):
        lengths = [rng.choice([1, 64, 65, 300, 300, 5000, MAX_RAGGED_MEMORY, MAX_RAGGED_MEMORY + 1, rng.randint(1, 20000)])
                   for _ in range(rng.randint(0, 40))]
        bs, window = rng.randint(1, 9), rng.choice([0, 3, 16])
        assert plan_groups(lengths, bs, window) == plan_pair_groups(lengths, lengths, bs, window)


# ---- evaluation.decode_rows against a step that replays a fixed table: TABLE[position][row], <eos> = 1.  Row 0 ends on
#      position 3 (the last of a chunk of 4), row 1 on position 4 (the first of the next), row 2 on position 6; what a row
#      "computes" after its <eos> -- further <eos> included -- must be dropped.
EOS = 1
TABLE = [[5, 6, 7], [8, 9, 3], [4, 4, 4], [EOS, 2, 9], [EOS, EOS, 5], [7, 7, 6], [3, EOS, EOS], [9, 9, 9], [EOS, 2, 2], [4, 5, 6],
         [6, 5, 4], [2, 2, 2]]
WANT = [[5, 8, 4, EOS], [6, 9, 4, 2, EOS], [7, 3, 4, 9, 5, 6, EOS]]


def _value(position, row):
    return position * 10 + row + 0.25


def _scripted(table, limit=None, want_probs=False):
    """-> (step, the list of n it was asked for).  step(n) replays the next min(n, limit) positions of `table`."""
    asked = []
    cursor = [0]

    def step(n):
        asked.append(n)
        m = n if limit is None else min(n, limit)
        if cursor[0] + m > len(table):
            raise RuntimeError("scripted step: the table is exhausted")
        p0 = cursor[0]
        cursor[0] += m
        toks = [list(table[p]) for p in range(p0, p0 + m)]
        vals = [[_value(p, r) for r in range(len(table[p]))] for p in range(p0, p0 + m)] if want_probs else None
        return toks, vals

    return step, asked


def test_decode_rows_cuts_each_row_after_its_eos_and_stops_asking():
    step, asked = _scripted(TABLE)
    ids, values = decode_rows(step, 3, EOS, 12, 4)
    assert ids == WANT
    assert values == [[], [], []]
    assert asked == [4, 4]                                 # every row is done after position 6: no third request


def test_decode_rows_without_eos_spends_exactly_the_budget():
    table = [[2 + (p + r) % 5 for r in range(3)] for p in range(16)]
    step, asked = _scripted(table)
    ids, _ = decode_rows(step, 3, EOS, 10, 4)
    assert asked == [4, 4, 2]                              # the last request is the short remainder
    assert ids == [[table[p][r] for p in range(10)] for r in range(3)]
    step, asked = _scripted(table)
    assert decode_rows(step, 3, EOS, 8, 4)[0] == [[table[p][r] for p in range(8)] for r in range(3)] and asked == [4, 4]


def test_decode_rows_keeps_the_values_of_the_kept_positions():
    step, _ = _scripted(TABLE, want_probs=True)
    ids, values = decode_rows(step, 3, EOS, 12, 4, want_probs=True)
    assert ids == WANT
    assert values == [[_value(p, r) for p in range(len(WANT[r]))] for r in range(3)]
    assert all(isinstance(v, float) for row in values for v in row)


def test_decode_rows_takes_a_step_that_returns_fewer_positions_than_asked():
    table = [[2 + (p + r) % 5 for r in range(2)] for p in range(12)]
    step, asked = _scripted(table, limit=3)
    ids, _ = decode_rows(step, 2, EOS, 10, 4)
    assert asked == [4, 4, 4, 1]                           # 3 + 3 + 3 positions issued, then the one that is left
    assert ids == [[table[p][r] for p in range(10)] for r in range(2)]
    step, asked = _scripted(TABLE, limit=3, want_probs=True)
    ids, values = decode_rows(step, 3, EOS, 12, 4, want_probs=True)
    assert ids == WANT and asked == [4, 4, 4]
    assert values == [[_value(p, r) for p in range(len(WANT[r]))] for r in range(3)]


def test_decode_rows_lets_the_error_of_a_step_that_cannot_advance_through():
    step, asked = _scripted(TABLE[:3])
    with pytest.raises(RuntimeError, match="exhausted"):
        decode_rows(step, 3, EOS, 12, 2)
    assert asked == [2, 2]


@pytest.mark.parametrize("budget", [5, 7, 12])
def test_decode_rows_does_not_depend_on_sync_every(budget):
    want = [seq[:budget] for seq in WANT]
    for sync_every in range(1, budget + 1):
        step, asked = _scripted(TABLE, want_probs=True)
        ids, values = decode_rows(step, 3, EOS, budget, sync_every, want_probs=True)
        assert ids == want, sync_every
        assert values == [[_value(p, r) for p in range(len(want[r]))] for r in range(3)], sync_every
        assert sum(asked) <= budget and all(1 <= n <= sync_every for n in asked)
    step, _ = _scripted([row[:1] for row in TABLE])
    assert decode_rows(step, 1, EOS, 12, 16)[0] == [WANT[0]]       # one row: the batch-size-1 loop
