"""Conv3x3Fn.backward's routes without a GPU: the launches of every ConvBlock case equal the recorded ones
(tests/golden/conv_bwd_routes.json, written by gen_conv_bwd_routes.py on the commit before the planner), the planner's invariants over
its whole input space, and the behaviour of the hand-on link."""
import gc
import itertools
import json
import os
import random
import weakref

import pytest
import torch

import conv_route_trace as T
from omr_a2s_multimodal_transformer_amd import conv_plan as P
from omr_a2s_multimodal_transformer_amd import functional as Fn
from omr_a2s_multimodal_transformer_amd.kernels import conv3x3_bwd_fused_covers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_bwd_routes.json")
DGRADS = ("none", "conv", "conv_stat2", "two_pass", "fused", "fused_apply", "fused_xn", "fused_s2")
FINISHES = ("none", "apply", "hand_on")


# ------------------------------------------------------------------------------------------------ A. same launches as recorded

def test_seeds_reach_the_three_dropout_positions():
    for pos, seed in T.SEED_OF_POSITION.items():
        random.seed(seed)
        assert random.randint(1, 3) == pos


def test_every_case_issues_the_recorded_launches(monkeypatch):
    """Names, order, scalar arguments and tensor dataflow of forward + backward, for every case of the fixture; and every data-gradient
    route and every finish of the plan is taken by some case, so none goes unpinned."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    want_cases = T.cases()
    assert len(want_cases) == len(doc["cases"])
    plans = []
    inner = Fn.plan_conv3x3_bwd
    monkeypatch.setattr(Fn, "plan_conv3x3_bwd", lambda *a: plans.append(inner(*a)) or plans[-1])
    for case, row in zip(want_cases, doc["cases"]):
        want = [doc["calls"][i] for i in doc["traces"][row]]
        got = json.loads(json.dumps(T.run_case(case)))
        if got != want:
            k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            pytest.fail(f"{case}: call {k} differs\n got  {got[k:k + 1]}\n want {want[k:k + 1]}\n got  {T.names(got)}\n want {T.names(want)}")
    assert {p.dgrad for p in plans} == set(DGRADS) and {p.finish for p in plans} == set(FINISHES)
    assert any(p.pre_apply for p in plans)                  # the fallback: a FUSED_NORM_CHANNELS width the kernel does not cover
    assert any(p.own_relu for p in plans) and any(not p.wgrad_separate for p in plans)


def test_the_examples_of_the_three_routes():
    """bf16, 16 -> 16 stride 1, dropout behind conv1: the backward launches under FUSED_BWD = 15, 3 and 0."""
    bwd = {fb: T.names(T.run_case(T.Case(5, "bf16", fb, False, 16, "16,32", True, True, True, 1, True, False)))[4:] for fb in (15, 3, 0)}
    assert bwd[15] == ["conv3x3_bwd_fused", "instnorm_reduce_sums", "conv3x3_bwd_fused", "conv3x3_bwd_fused"]
    assert bwd[3] == ["conv3x3_wgrad", "conv3x3", "instnorm_reduce_sums", "conv3x3_bwd_fused", "conv3x3_bwd_fused"]
    assert bwd[0] == ["conv3x3_wgrad", "conv3x3", "instnorm_bwd_apply", "conv3x3_wgrad", "conv3x3", "conv3x3_wgrad", "conv3x3"]


# ------------------------------------------------------------------------------------------------ B. planner invariants

def test_planner_invariants_over_its_whole_input_space():
    widths = ((1, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128))
    flags = (False, True)
    n = 0
    for bf16, (cin, cout), stride, normalised, needs_dx, relu, mask_own, role, taken_mask, fb, min_cout, two_pass in itertools.product(
            flags, widths, ((1, 1), (2, 2), (2, 1)), flags, flags, flags, flags, (P.NO_LINK, P.GIVES, P.TAKES), flags, range(16), (16, 32), flags):
        p = P.plan_conv3x3_bwd(bf16, cin, cout, stride, normalised, needs_dx, relu, mask_own, role, taken_mask, fb, min_cout, two_pass)
        what = (p, bf16, cin, cout, stride, normalised, needs_dx, relu, mask_own, role, taken_mask, fb, min_cout, two_pass)
        n += 1
        assert p.dgrad in DGRADS and p.finish in FINISHES, what
        # weight and bias gradients are accumulated exactly once
        assert p.wgrad_separate != (p.dgrad in P.FUSED_DGRADS), what
        # a taken hand-on is applied exactly once; nothing is applied that was not taken
        assert (p.pre_apply + (p.dgrad == "fused_apply")) == (role == P.TAKES), what
        # only the giving role hands on, and it does whenever it has a gradient to hand on
        assert (p.finish == "hand_on") == (role == P.GIVES and normalised and needs_dx), what
        # the conv's own InstanceNorm backward is applied exactly once: by the apply pass, the two-pass epilogue or the producer
        norm_family = p.dgrad in ("conv_stat2", "two_pass", "fused_xn", "fused_s2")
        assert norm_family == (normalised and needs_dx), what
        assert (p.finish != "none") == (norm_family and p.dgrad != "two_pass"), what
        # fused routes: bf16 and the shapes the kernels cover
        if p.dgrad in ("fused", "fused_apply", "fused_xn"):
            assert conv3x3_bwd_fused_covers(bf16, cin, cout, stride), what
        if p.dgrad == "fused_s2":
            assert bf16 and (cin, cout, stride) == (32, 32, (2, 2)), what
        if p.dgrad in ("fused", "fused_apply"):
            assert not normalised, what
        # no data gradient asked, none computed
        if not needs_dx:
            assert p.dgrad == "none" and p.finish == "none", what
        assert p.own_relu == (relu and mask_own), what
    assert n == 2 * 8 * 3 * 2 ** 4 * 3 * 2 * 16 * 2 * 2


def test_the_hand_on_predicate():
    for bf16, ch, grad, fb in itertools.product((False, True), (16, 32, 64), (False, True), range(16)):
        assert P.hands_on(bf16, ch, grad, fb, (16, 32)) == (bool(fb & 2) and bf16 and grad and ch in (16, 32))
    assert P.hands_on(True, 64, True, 2, (16, 32, 64))


# ------------------------------------------------------------------------------------------------ C. the link

def _conv2_conv3(blk, x, link):
    y, mean, rstd = Fn.conv3x3(x, blk.conv2, stride=(1, 1), relu=True, mask_own=False, mask_input=True, in_scale=1.0, want_stats=True, link=link)
    z = Fn.conv3x3(y, blk.conv3, stride=(1, 1), relu=True, in_stats=(mean, rstd), mask_own=True, mask_input=True, in_scale=1.0, link=link)
    return y, z


def _block_and_input():
    blk = T.make_block(16, 16, (1, 1), True)
    return blk, torch.empty((T.B, *T.PLANE, 16), dtype=torch.bfloat16).requires_grad_(True)


def _stop(g):
    raise RuntimeError("stop")


def test_a_backward_that_raises_leaves_no_record_behind():
    """The pass raises between conv3's backward and conv2's: the record is on the link, and link and record go with the graph -- by
    reference counting alone: the record holds no tensor with a history, so no cycle through the graph waits for the collector."""
    gc.collect()
    gc.disable()
    try:
        _raise_then_drop()
    finally:
        gc.enable()


def _raise_then_drop():
    with T.recording(fused_bwd=15) as rec:
        blk, x = _block_and_input()
        link = Fn.NormLink()
        y, z = _conv2_conv3(blk, x, link)
        y.register_hook(_stop)
        with pytest.raises(RuntimeError, match="stop"):
            z.backward(torch.empty_like(z))
        assert link.record is not None and link.record.y.data_ptr() == y.data_ptr()
        dead = [weakref.ref(link), weakref.ref(link.record.y), weakref.ref(link.record.ws)]
    del link, y, z, rec.keep[:]
    assert [r() for r in dead] == [None, None, None]


def test_conv2_refuses_a_gradient_the_record_does_not_belong_to():
    with T.recording(fused_bwd=15):
        blk, x = _block_and_input()
        y, z = _conv2_conv3(blk, x, Fn.NormLink())
        y.register_hook(lambda g: g.clone())
        with pytest.raises(RuntimeError, match="not the one the handed-on InstanceNorm record belongs to"):
            z.backward(torch.empty_like(z))


def test_conv2_raises_when_nothing_was_handed_on():
    with T.recording(fused_bwd=15):
        blk, x = _block_and_input()
        y, _, _ = Fn.conv3x3(x, blk.conv2, stride=(1, 1), relu=True, mask_own=False, mask_input=True, in_scale=1.0, want_stats=True, link=Fn.NormLink())
        with pytest.raises(RuntimeError, match="did not hand on its InstanceNorm gradient"):
            y.backward(torch.empty_like(y))


def test_two_graphs_alive_at_once_take_their_own_records():
    """The window-chain pattern: forward A, forward B, backward B, backward A through one block."""
    with T.recording(fused_bwd=15) as rec:
        blk = T.make_block(16, 16, (1, 1), True)
        blk.eval()
        outs = [blk.nhwc(torch.empty((T.B, *T.PLANE, 16), dtype=torch.bfloat16).requires_grad_(True), True, 1.0, True)[0] for _ in range(2)]
        conv2_out = [e[2] for e in rec.trace if e[0] == "conv3x3" and e[1].get("stat_mode") == 1]
        for out in reversed(outs):
            out.backward(torch.empty_like(out))
    applied = [e[1]["norm"][0] for e in rec.trace if e[0] == "conv3x3_bwd_fused" and "norm" in e[1]]
    assert len(set(conv2_out)) == 2 and applied == conv2_out[::-1]
