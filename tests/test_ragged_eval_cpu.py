"""CPU-only checks of batched evaluation over inputs of different sizes: the new entry points of the C ABI, the native edit
distance against the Python reference, and the grouping of memories into ragged batches."""
import ctypes
import random
import subprocess

import numpy as np
import pytest

from omr_a2s_multimodal_transformer_amd import _lib, metrics
from omr_a2s_multimodal_transformer_amd.decoder import MAX_RAGGED_MEMORY, MIN_RAGGED_MEMORY
from omr_a2s_multimodal_transformer_amd.evaluation import plan_groups

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
