"""Batched late-fusion evaluation, the parts that need no GPU: the grouping of (image, audio) pairs, the two new entry points
in the header, and the public signatures."""
import inspect
import random

import pytest

from omr_a2s_multimodal_transformer_amd._lib import parse_header
from omr_a2s_multimodal_transformer_amd.decoder import MAX_RAGGED_MEMORY, MIN_RAGGED_MEMORY
from omr_a2s_multimodal_transformer_amd.evaluation import plan_pair_groups


def _ragged(n):
    return MIN_RAGGED_MEMORY < n <= MAX_RAGGED_MEMORY


def _lengths(n, seed):
    r = random.Random(seed)
    pool = [1, 24, MIN_RAGGED_MEMORY, MIN_RAGGED_MEMORY + 1, 100, 256, 257, 1000, 12696, MAX_RAGGED_MEMORY, MAX_RAGGED_MEMORY + 1]
    return [r.choice(pool) for _ in range(n)], [r.choice(pool) for _ in range(n)]


@pytest.mark.parametrize("n,batch_size,window", [(0, 4, 0), (1, 1, 0), (37, 4, 0), (37, 4, 8), (64, 32, 16), (50, 1, 7), (23, 100, 0)])
def test_plan_pair_groups_partitions_the_indices(n, batch_size, window):
    la, lb = _lengths(n, 100 + n + window)
    singles, groups = plan_pair_groups(la, lb, batch_size, window)
    assert sorted(singles + [i for g in groups for i in g]) == list(range(n))             # every index exactly once
    assert sorted(singles) == [i for i in range(n) if not (_ragged(la[i]) and _ragged(lb[i]))]
    assert all(1 <= len(g) <= batch_size for g in groups)
    w = window if window > 0 else max(n, 1)
    for g in groups:
        assert len({i // w for i in g}) == 1                                              # a group never spans two windows
        key = [la[i] + lb[i] for i in g]
        assert key == sorted(key, reverse=True)                                           # similar lengths side by side


def test_plan_pair_groups_on_the_table_of_the_gpu_test():
    la = [100, 260, 240, 24, 600, 180, 75, 250]
    lb = [150, 130, 270, 130, 76, 330, 24, 200]
    singles, groups = plan_pair_groups(la, lb, 4)
    assert singles == [3, 6]                                # 24 image tokens / 24 audio tokens: either side short -> alone
    assert groups == [[4, 2, 5, 7], [1, 0]]
    assert plan_pair_groups(la, lb, 8) == ([3, 6], [[4, 2, 5, 7, 1, 0]])
    assert plan_pair_groups(la, lb, 1)[1] == [[4], [2], [5], [7], [1], [0]]


def test_plan_pair_groups_refuses_bad_arguments():
    with pytest.raises(ValueError, match="batch_size"):
        plan_pair_groups([100], [100], 0)
    with pytest.raises(ValueError):
        plan_pair_groups([100, 200], [100], 4)


def test_header_declares_the_batched_entry_points():
    protos = parse_header()
    ret, args = protos["omr_weighted_argmax_rows"]
    assert ret == "int" and "long* tokens_out" in args and "long* idx_out" in args and "float* prob_out" in args
    assert args.count("long") == 2 and len(args) == 11     # lda, ldb
    ret, args = protos["omr_weighted_decode_steps_varlen"]
    assert ret == "int" and "const int* mem_len_a" in args and "const int* mem_len_b" in args
    assert args.count("const omr_decode_desc* desc_a") == 1 and args.count("const omr_decode_desc* desc_b") == 1 and len(args) == 13
    # the entry points they generalise keep their prototypes
    assert protos["omr_weighted_argmax"][1] == ["const float* logits_a", "const float* logits_b", "int", "float", "long* idx_out", "float* prob_out",
                                                "void* stream"]
    assert len(protos["omr_weighted_decode_steps"][1]) == 11


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_public_signatures():
    from omr_a2s_multimodal_transformer_amd import late_fusion, weighted_fusion
    from omr_a2s_multimodal_transformer_amd.decoder import DecodeState
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    E = inspect.Parameter.empty
    assert _params(weighted_fusion.weighted_predict) == [("pairs", E), ("img_model", E), ("audio_model", E), ("alpha", 0.5), ("batch_size", 32),
                                                         ("sync_every", 8)]
    assert _params(weighted_fusion.weighted_evaluate) == [("batches", E), ("img_model", E), ("audio_model", E), ("alpha", 0.5), ("batch_size", 32)]
    assert _params(late_fusion.sw_predict) == [("pairs", E), ("img_model", E), ("audio_model", E), ("batch_size", 32), ("match", 2),
                                               ("mismatch", -1), ("gap_penalty", -1)]
    assert _params(late_fusion.sw_evaluate)[:4] == [("batches", E), ("img_model", E), ("audio_model", E), ("batch_size", 32)]
    assert _params(Transformer.predict_with_probs) == [("self", E), ("xs", E), ("batch_size", 32)]
    assert _params(Transformer.predict) == [("self", E), ("xs", E), ("batch_size", 32)]
    assert _params(DecodeState.rewind) == [("self", E)]
    # weighted_prediction keeps the reference's signature (+ chunk)
    assert _params(weighted_fusion.weighted_prediction) == [("xi", E), ("xa", E), ("img_model", E), ("audio_model", E), ("alpha", 0.5), ("chunk", 16)]
