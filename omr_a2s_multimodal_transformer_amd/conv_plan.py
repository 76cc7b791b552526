"""Which kernels the backward pass of a dense 3x3 conv runs (functional.Conv3x3Fn), decided once and from plain values, and the link
over which a ConvBlock's conv3 hands its InstanceNorm gradient to conv2.

The encoder's routes by layer and FUSED_BWD (bf16; DESIGN.md has the whole table): with the shipped 15, conv1 and conv2 of
ConvBlocks 0 and 1 run `fused` / `fused_apply`, their conv3 `fused_xn` / `fused_s2` and hand on; ConvBlocks 2-4 and fp32 run the
separate kernels (`conv`, or `conv_stat2` + `apply`) with the weight gradient on the side stream; the ragged route has no
normalise-on-load conv and no hand-on, the convs the one-pass kernel covers still run `fused`.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .kernels import conv3x3_bwd_fused_covers

Tensor = torch.Tensor

NO_LINK, GIVES, TAKES = 0, 1, 2        # a conv's role in a hand-on: conv3 (normalises on load) gives, conv2 (its producer) takes
FUSED_DGRADS = ("fused", "fused_apply", "fused_xn", "fused_s2")      # the one-pass kernels: they accumulate dW and db themselves


class ConvBwdPlan(NamedTuple):
    """The steps of Conv3x3Fn.backward, in the order they run."""
    pre_apply: bool         # stand-alone instnorm_bwd_apply of a taken hand-on that nobody applies on load
    own_relu: bool          # relu_bwd with the conv's stored output
    wgrad_separate: bool    # conv3x3_wgrad (+ bias gradient) on the side stream
    dgrad: str              # none | conv | conv_stat2 | two_pass | fused | fused_apply | fused_xn | fused_s2
    finish: str             # none | apply (instnorm_bwd_apply of the conv's own input norm) | hand_on (leave it to the producer)


def plan_conv3x3_bwd(bf16: bool, cin: int, cout: int, stride, normalised: bool, needs_dx: bool, relu: bool, mask_own: bool, role: int,
                     taken_mask: bool, fused_bwd: int, min_cout: int, two_pass: bool) -> ConvBwdPlan:
    """bf16: the compute dtype; normalised: the conv normalised its input on load; role: NO_LINK / GIVES / TAKES; taken_mask: the
    record a TAKES conv received carries a ReLU mask; fused_bwd, min_cout, two_pass: functional.FUSED_BWD, FUSED_MIN_COUT,
    TWO_PASS_NORM_BWD.  Quirks that are behaviour:
    * a taken hand-on is applied on load wherever the one-pass kernel covers the conv, whatever bit 1 and `min_cout` say (they gate
      only the plain one-pass route); elsewhere (a width in FUSED_NORM_CHANNELS the kernel does not cover, or a record without a
      ReLU mask) it is applied by the stand-alone pass first;
    * `two_pass` is ignored on a conv that hands on, and wherever bit 4 / 8 picks a one-pass kernel;
    * bit 8 does not ask conv3x3_bwd_fused_covers (the stride-2 entry has its own shape: bf16, 32 -> 32, stride (2, 2)); bit 4 does,
      on top of 16 -> 16;
    * without a data gradient there is no one-pass route: the weight gradient runs alone."""
    stride = tuple(stride)
    covered = conv3x3_bwd_fused_covers(bf16, cin, cout, stride)
    one_pass = not normalised and needs_dx and covered
    apply_on_load = role == TAKES and one_pass and taken_mask
    pre_apply = role == TAKES and not apply_on_load
    own_relu = relu and mask_own
    if apply_on_load or (one_pass and bool(fused_bwd & 1) and cout >= min_cout):
        return ConvBwdPlan(pre_apply, own_relu, False, "fused_apply" if apply_on_load else "fused", "none")
    if not needs_dx:
        return ConvBwdPlan(pre_apply, own_relu, True, "none", "none")
    if not normalised:
        return ConvBwdPlan(pre_apply, own_relu, True, "conv", "none")
    finish = "hand_on" if role == GIVES else "apply"
    if fused_bwd & 8 and bf16 and stride == (2, 2) and (cin, cout) == (32, 32):
        return ConvBwdPlan(pre_apply, own_relu, False, "fused_s2", finish)
    if fused_bwd & 4 and covered and (cin, cout) == (16, 16):
        return ConvBwdPlan(pre_apply, own_relu, False, "fused_xn", finish)
    if two_pass and role != GIVES:
        return ConvBwdPlan(pre_apply, own_relu, True, "two_pass", "none")
    return ConvBwdPlan(pre_apply, own_relu, True, "conv_stat2", finish)


def hands_on(bf16: bool, channels: int, grad: bool, fused_bwd: int, norm_channels) -> bool:
    """ConvBlock: conv3 hands its un-applied InstanceNorm gradient to conv2 (FUSED_BWD bit 2, bf16, a conv2 width named in
    FUSED_NORM_CHANNELS).  Whether conv2 then applies it on load is plan_conv3x3_bwd's `fused_apply`; a named width that the
    one-pass kernel does not cover takes `pre_apply` instead."""
    return bool(fused_bwd & 2) and grad and bf16 and channels in norm_channels


class NormRecord(NamedTuple):
    """What the InstanceNorm backward of y needs besides dL/dxhat (the arguments of kernels.instnorm_bwd_apply, and
    kernels.conv3x3_bwd_fused's `norm`)."""
    y: Tensor
    mean: Tensor
    rstd: Tensor
    ws: Tensor
    slots: int
    relu_mask: bool
    relu_scale: float


class NormLink:
    """One hand-on, ConvBlock conv3 -> conv2, made per forward pass and held by the two autograd nodes: it lives and dies with their
    graph, so a backward pass that raises leaves nothing behind, and two graphs alive at once cannot take each other's record.  The
    record holds no tensor with an autograd history (no cycle through the graph)."""
    def __init__(self):
        self.record = self.grad_key = None

    def give(self, grad: Tensor, record: NormRecord) -> None:
        self.record, self.grad_key = record, (grad.data_ptr(), tuple(grad.shape))

    def take(self, grad: Tensor) -> NormRecord:
        record, key = self.record, self.grad_key
        self.record = self.grad_key = None
        if record is None:
            raise RuntimeError("Conv3x3Fn: the consumer's backward did not hand on its InstanceNorm gradient")
        if key != (grad.data_ptr(), tuple(grad.shape)):
            raise RuntimeError("Conv3x3Fn: the gradient received is not the one the handed-on InstanceNorm record belongs to")
        return record
