"""Launch traces of the encoder's ConvBlock on the CPU: `functional` sees a recorder in place of the `kernels` module, so every kernel
wrapper call of a forward + backward pass is logged -- its name, its scalar arguments and, for every tensor operand, a label given at
the tensor's first appearance -- and answered with an uninitialised tensor of the right shape.  Two runs that log the same trace issue
the same launches, in the same order, over the same dataflow.  Shared by tests/golden/gen_conv_bwd_routes.py (which records the
traces of the commit it is run on) and tests/test_conv_routes_cpu.py (which replays every case and requires equal traces).

Only `ConvBlock.nhwc`, the four route flags of `functional` and the `kernels` wrappers' signatures are relied on."""
from __future__ import annotations

import contextlib
import inspect
import itertools
import random
from typing import List, NamedTuple, Tuple

import torch

from omr_a2s_multimodal_transformer_amd import functional as Fn
from omr_a2s_multimodal_transformer_amd import kernels as real_K
from omr_a2s_multimodal_transformer_amd.encoder import ConvBlock
from omr_a2s_multimodal_transformer_amd.runtime import seed_dropout

B, PLANE = 2, (9, 33)
# every ConvBlock of the encoder, plus the two square stride-1 shapes
SHAPES = ((1, 16, (1, 1)), (16, 32, (2, 2)), (32, 64, (2, 2)), (64, 128, (2, 2)), (128, 128, (2, 1)), (16, 16, (1, 1)), (32, 32, (1, 1)))
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
SEED_OF_POSITION = {1: 1, 2: 0, 3: 5}        # random.seed(s); random.randint(1, 3) -> the dropout position (checked by the test)
STAT_SLOTS = 3                               # what the recorder answers for conv_stat_ws


class Case(NamedTuple):
    shape: int              # index into SHAPES
    dtype: str
    fused_bwd: int
    two_pass: bool
    min_cout: int
    norm_channels: str
    in_mask: bool
    defer_out: bool
    train: bool
    position: int
    x_grad: bool
    ragged: bool


def cases() -> List[Case]:
    """The flag grid in full at one block configuration per dropout position; then the block's own arguments on the flag values
    that change a route there: masks, every position and the input gradient in training mode on the dense and the ragged route
    (which ignores the masks), and eval mode, where no dropout is placed, at one position."""
    out = []
    for i, (shape, dtype, fb, tp, mc, nc) in enumerate(itertools.product(range(len(SHAPES)), DTYPES, range(16), (False, True), (16, 32), ("16,32", "16,32,64"))):
        out.append(Case(shape, dtype, fb, tp, mc, nc, True, True, True, 1 + i % 3, True, False))
    for shape, dtype, fb, x_grad, train, ragged in itertools.product(range(len(SHAPES)), DTYPES, (0, 15), (False, True), (True, False), (False, True)):
        masks = ((False, False),) if ragged else tuple(itertools.product((False, True), (False, True)))
        for (in_mask, defer_out), pos in itertools.product(masks, (1, 2, 3) if train else (2,)):
            if not (SHAPES[shape][0] == 1 and in_mask):      # the image is no ReLU output
                out.append(Case(shape, dtype, fb, False, 16, "16,32", in_mask, defer_out, train, pos, x_grad, ragged))
    return list(dict.fromkeys(out))


def _is_default(v, default) -> bool:
    return not isinstance(v, torch.Tensor) and type(v) is type(default) and v == default


class Recorder:
    """Stands in for the `kernels` module.  `trace` is a list of [name, arguments, result]: the arguments by the wrapper's parameter
    names, those at their default left out, tensors as labels ("t0", "t1", ...: first appearance, keyed by address, shape and dtype, so
    a view that aliases a tensor is that tensor); every labelled tensor is kept alive so that no address is seen twice."""

    PASS_THROUGH = ("conv_out_hw", "conv3x3_bwd_fused_ok")

    def __init__(self):
        self.trace, self.labels, self.keep = [], {}, []

    def label(self, v):
        if isinstance(v, torch.Tensor):
            key = (v.data_ptr(), tuple(v.shape), v.dtype)
            if key not in self.labels:
                self.labels[key] = f"t{len(self.labels)}"
                self.keep.append(v)
            return self.labels[key]
        if isinstance(v, (tuple, list)):
            return [self.label(e) for e in v]
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        return str(v)                                    # dtype, device

    def __getattr__(self, name):
        real = getattr(real_K, name)
        if name in self.PASS_THROUGH:
            return real
        answer = getattr(self, "_" + name)

        def call(*args, **kwargs):
            sig = inspect.signature(real)
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            a = bound.arguments
            entry = [name, {k: self.label(v) for k, v in a.items() if not _is_default(v, sig.parameters[k].default)}, None]
            self.trace.append(entry)                     # before the answer: the operands are labelled before the result
            out = answer(a)
            entry[2] = self.label(out)
            return out

        return call

    # ---- what each wrapper returns (shapes and dtypes of kernels.py)

    @staticmethod
    def _like(t):
        return torch.empty_like(t)

    def _conv_stat_ws(self, a):
        return torch.empty(STAT_SLOTS * a["B"] * a["C"] * 2 + 2 * a["B"] * a["C"], dtype=torch.float64), STAT_SLOTS

    def _conv3x3(self, a):
        x = a["x"]
        Ho, Wo = a["out_hw"] if a["out_hw"] is not None else real_K.conv_out_hw(x.shape[1], x.shape[2], a["stride"])
        return torch.empty((x.shape[0], Ho, Wo, a["w_phys"].shape[0]), dtype=x.dtype)

    def _instnorm_finalize(self, a):
        return torch.empty((a["B"], a["C"])), torch.empty((a["B"], a["C"]))

    def _conv3x3_weight_flip(self, a):
        w = a["w_phys"]
        return torch.empty((w.shape[3], 3, 3, w.shape[0]), dtype=w.dtype)

    def _instnorm_extent_fwd(self, a):
        x = a["x"]
        return torch.empty_like(x), torch.empty((x.shape[0], x.shape[3])), torch.empty((x.shape[0], x.shape[3]))

    def _none(self, a):
        return None

    _conv3x3_wgrad = _instnorm_reduce_sums = _none
    _instnorm_bwd_apply = _conv3x3_bwd_fused = _conv3x3_bwd_fused_s2 = _instnorm_extent_bwd = lambda self, a: self._like(a["x"])
    _relu_bwd = lambda self, a: self._like(a["dy"])
    _dropout = lambda self, a: self._like(a["x"])
    _extent_zero = lambda self, a: a["x"]


def make_block(cin: int, cout: int, stride: Tuple[int, int], lowp: bool) -> ConvBlock:
    """A ConvBlock whose parameters carry what params.FlatParams attaches: the physical [COUT, 3, 3, CIN] weights, their bf16 copy
    and the fp32 gradient views (no `omr_flat`: the data-gradient weights are re-laid per call, which the trace shows)."""
    blk = ConvBlock(cin, cout, stride=stride, dropout=0.5)
    for p in blk.parameters():
        p.omr_phys = torch.empty(p.shape).permute(0, 2, 3, 1).contiguous() if p.dim() == 4 else torch.empty(p.shape)
        p.omr_lowp = p.omr_phys.to(torch.bfloat16) if lowp else None
        p.omr_grad = torch.empty(p.omr_phys.shape)
    return blk


@contextlib.contextmanager
def recording(fused_bwd=None, two_pass=None, min_cout=None, norm_channels=None):
    """`functional` sees a fresh Recorder (yielded) instead of `kernels`, and the given route flags; all restored on exit."""
    saved = (Fn.K, Fn.FUSED_BWD, Fn.TWO_PASS_NORM_BWD, Fn.FUSED_MIN_COUT, Fn.FUSED_NORM_CHANNELS)
    rec = Recorder()
    try:
        Fn.K = rec
        Fn.FUSED_BWD = saved[1] if fused_bwd is None else fused_bwd
        Fn.TWO_PASS_NORM_BWD = saved[2] if two_pass is None else two_pass
        Fn.FUSED_MIN_COUT = saved[3] if min_cout is None else min_cout
        Fn.FUSED_NORM_CHANNELS = saved[4] if norm_channels is None else tuple(int(v) for v in norm_channels.split(","))
        yield rec
    finally:
        Fn.K, Fn.FUSED_BWD, Fn.TWO_PASS_NORM_BWD, Fn.FUSED_MIN_COUT, Fn.FUSED_NORM_CHANNELS = saved


def run_case(c: Case) -> list:
    """The trace of one forward + backward pass of a ConvBlock under the case's flags."""
    cin, cout, stride = SHAPES[c.shape]
    dt = DTYPES[c.dtype]
    with recording(c.fused_bwd, c.two_pass, c.min_cout, c.norm_channels) as rec:
        blk = make_block(cin, cout, stride, dt == torch.bfloat16)
        blk.train(c.train)
        x = torch.empty((B, PLANE[0], PLANE[1], cin), dtype=dt).requires_grad_(c.x_grad)
        ext = None
        if c.ragged:
            e_in = torch.tensor([[PLANE[0], PLANE[1]], [5, 17]], dtype=torch.int32)
            st = torch.tensor(stride, dtype=torch.int32)
            ext = (e_in, (e_in + st - 1) // st)
        seed_dropout(11)
        random.seed(SEED_OF_POSITION[c.position])
        y, scale = blk.nhwc(x, c.in_mask, 1.25 if c.in_mask else 1.0, c.defer_out, extents=ext)
        rec.trace.append(["returned", {"y": rec.label(y), "scale": scale}, None])
        y.backward(torch.empty_like(y))
    return rec.trace


def names(trace: list, skip=("conv3x3_weight_flip", "conv_stat_ws", "returned")) -> List[str]:
    return [e[0] for e in trace if e[0] not in skip]
