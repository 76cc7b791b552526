"""CPU-only checks of continuous batching for greedy evaluation: the read-back loop with a queue (evaluation.decode_stream)
against scripted `step` / `admit` callbacks, the positions it asks for against the grouped plan, and the new entry points of
the C ABI."""
import subprocess

import pytest
import torch

from omr_a2s_multimodal_transformer_amd import _lib
from omr_a2s_multimodal_transformer_amd.evaluation import decode_rows, decode_stream, plan_groups, stream_order

EOS = 1
NEW = ("omr_attn_fwd_split_rows", "omr_decode_steps_rows", "omr_weighted_decode_steps_rows")


class Script:
    """`rows` slots over scripted inputs: input i emits tokens 100 * i + position and <eos> as its lengths[i]-th token (never
    when lengths[i] is None); the value of a token is token + 0.5.  An idle slot emits -7."""

    def __init__(self, lengths, rows):
        self.lengths, self.rows = lengths, rows
        self.holds, self.pos = [None] * rows, [0] * rows
        self.admitted, self.asked = [], []

    def admit(self, slot, i):
        self.holds[slot], self.pos[slot] = i, 0
        if i is not None:
            self.admitted.append(i)

    def token(self, slot):
        i, p = self.holds[slot], self.pos[slot]
        if i is None:
            return -7
        return EOS if self.lengths[i] is not None and p == self.lengths[i] - 1 else 100 * (i + 1) + p

    def step(self, n):
        self.asked.append(n)
        toks, vals = [], []
        for _ in range(n):
            toks.append([self.token(b) for b in range(self.rows)])
            vals.append([t + 0.5 for t in toks[-1]])
            self.pos = [p + 1 for p in self.pos]
        return toks, vals

    def expected(self, i, budget):
        n = self.lengths[i]
        if n is not None and n <= budget:
            return [100 * (i + 1) + p for p in range(n - 1)] + [EOS]
        return [100 * (i + 1) + p for p in range(budget)]


LENGTHS = [5, 1, None, 3, 12, 2, None, 7, 1, 4, 9]


@pytest.mark.parametrize("rows", [1, 2, 4, 16])
@pytest.mark.parametrize("sync_every", [1, 3, 8, 100])
def test_stream_returns_every_input_once_cut_at_eos_or_budget(rows, sync_every):
    budget = 10
    sc = Script(LENGTHS, rows)
    order = stream_order([50, 300, 70, 70, 900, 65, 66, 300, 1000, 80, 81])
    out, vals = decode_stream(sc.step, sc.admit, order, rows, EOS, budget, sync_every, want_probs=True)
    assert sc.admitted == order == [8, 4, 1, 7, 10, 9, 2, 3, 6, 5, 0]          # decreasing length, ties in input order
    assert out == [sc.expected(i, budget) for i in range(len(LENGTHS))]         # by input index, whatever the chunk
    assert vals == [[t + 0.5 for t in seq] for seq in out]                      # values of the kept positions only
    assert all(n >= 1 for n in sc.asked)
    out2, vals2 = decode_stream(Script(LENGTHS, rows).step, Script(LENGTHS, rows).admit, order, rows, EOS, budget, sync_every)
    assert vals2 == [[] for _ in LENGTHS]


def test_stream_keeps_no_row_past_its_budget():
    """Every live row may run `n` more positions: n never exceeds the budget left of the row that is furthest along."""
    sc = Script([None, 2, None], 2)
    budget = 7

    def step(n):
        for b in range(2):
            if sc.holds[b] is not None:
                assert sc.pos[b] + n <= budget, (b, sc.pos[b], n)
        return sc.step(n)

    out, _ = decode_stream(step, sc.admit, [0, 1, 2], 2, EOS, budget, 4)
    assert [len(s) for s in out] == [7, 2, 7]


def test_stream_asks_for_fewer_positions_than_the_grouped_plan():
    lengths = [5, 1, 1, 1, 1]
    sc = Script(lengths, 2)
    out, _ = decode_stream(sc.step, sc.admit, list(range(5)), 2, EOS, 16, 1)
    assert [len(s) for s in out] == lengths
    assert sum(sc.asked) == 5
    # the grouped plan on the same lengths: every group runs until its longest row ends
    singles, groups = plan_groups([100] * 5, 2)
    assert singles == [] and [len(g) for g in groups] == [2, 2, 1]
    asked = 0
    for g in groups:
        gs = Script([lengths[i] for i in g], len(g))
        for b in range(len(g)):
            gs.admit(b, b)
        got, _ = decode_rows(lambda n: tuple(x[:n] for x in gs.step(n)), len(g), EOS, 16, 1)
        assert [len(s) for s in got] == [lengths[i] for i in g]
        asked += sum(gs.asked)
    assert asked == 7


def test_stream_passes_an_error_of_step_through_and_refuses_bad_plans():
    sc = Script([3, 3], 2)

    def step(n):
        raise RuntimeError("decode_step beyond max_seq_len")

    with pytest.raises(RuntimeError, match="beyond max_seq_len"):
        decode_stream(step, sc.admit, [0, 1], 2, EOS, 8, 4)
    with pytest.raises(ValueError, match="permutation"):
        decode_stream(sc.step, sc.admit, [0, 0], 2, EOS, 8, 4)
    with pytest.raises(ValueError, match="rows"):
        decode_stream(sc.step, sc.admit, [0, 1], 0, EOS, 8, 4)
    assert decode_stream(step, sc.admit, [0, 1], 2, EOS, 0, 4) == ([[], []], [[], []])      # no budget: nothing is asked


def _cpu_model(cls):
    from omr_a2s_multimodal_transformer_amd import model as M
    from omr_a2s_multimodal_transformer_amd import synthetic as syn
    from omr_a2s_multimodal_transformer_amd.config import ModelConfig
    w2i, i2w = syn.make_vocab(30)
    cfg = ModelConfig(num_layers=1)
    if cls == "Transformer":
        return M.Transformer(64, 256, 16, w2i, i2w, config=cfg)
    return M.MultimodalTransformer(64, 256, 64, 256, 16, w2i, i2w, config=cfg)


@pytest.mark.parametrize("cls", ["Transformer", "MultimodalTransformer"])
def test_refill_with_a_beam_is_refused_before_anything_runs(cls):
    m = _cpu_model(cls)
    x = torch.zeros(1, 1, 32, 32)
    item = x if cls == "Transformer" else (x, x)
    y = torch.tensor([[2, 5, 1]])
    batch = (x, y) if cls == "Transformer" else (x, x, y)
    with pytest.raises(ValueError, match="refill"):
        m.predict([item], beam=2, refill=True)
    with pytest.raises(ValueError, match="refill"):
        m.evaluate([batch], beam=4, refill=True)


def test_new_entry_points_are_declared_and_exported():
    protos = _lib.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T omr_" in line}
    for name in NEW:
        assert name in protos, name
        assert name in exported, name
    # omr_attn_fwd_split_varlen's arguments plus kv_start
    varlen, rows = protos["omr_attn_fwd_split_varlen"][1], protos["omr_attn_fwd_split_rows"][1]
    assert rows[:21] == varlen[:21] and rows[21] == "const int* kv_start" and rows[22:] == varlen[21:]
    assert protos["omr_decode_steps_rows"][1] == ["const omr_decode_desc* desc", "const int* mem_len", "const int* pos", "int", "long* tokens", "int",
                                                  "long* out_tokens", "float* out_top1", "float* last_logits", "void* stream"]
    w = protos["omr_weighted_decode_steps_rows"][1]
    assert w[:6] == ["const omr_decode_desc* desc_a", "const int* mem_len_a", "const omr_decode_desc* desc_b", "const int* mem_len_b", "const int* pos", "int"]
    assert len(w) == len(protos["omr_weighted_decode_steps_varlen"][1]) + 1        # pos / t_max replace t0
