"""Flat parameter storage sized for one HBM-resident model replica + fused Adam.

All parameters of a model live in ONE fp32 buffer (master weights) with parallel flat buffers for
gradients, Adam moments and (bf16 mode) the bf16 compute copy.  nn.Parameters are views into the master
buffer that keep the reference's logical shapes (state-dict contract) while the memory
is laid out for the kernels: conv weights [Cout,Cin,kh,kw] are stored [Cout,kh,kw,Cin] (the logical
tensor is the channels_last-strided permutation), so MFMA B-fragments are 16-byte k-contiguous loads.
One flat buffer means: Adam is a single kernel launch (kernels.adam_step), zero_grad is one memset and the
data-parallel gradient all-reduce runs over a few large contiguous buckets (ddp.py).
"""
from __future__ import annotations

import contextlib
from typing import Dict, Iterable, List, Optional, Tuple

import torch
import torch.nn as nn

from . import kernels as K
from .config import OptimConfig, lr_at

ALIGN = 64  # elements; keeps every view 256-byte aligned in fp32 and 128-byte aligned in bf16


def _phys_perm(ndim: int) -> Optional[Tuple[int, ...]]:
    """logical dims -> physical order: channel dim 1 moves last for conv weights (ndim >= 3)."""
    if ndim < 3:
        return None
    return (0,) + tuple(range(2, ndim)) + (1,)


def _inverse(perm: Tuple[int, ...]) -> Tuple[int, ...]:
    inv = [0] * len(perm)
    for i, p in enumerate(perm):
        inv[p] = i
    return tuple(inv)


# Parameters that are placed back to back (in layer order) so that one GEMM can run over all of them through a row-group
# view (omr_gemm row_group_*): the packed cross-attention in_proj matrices / biases of all decoder layers, whose K|V rows
# project the SAME encoder memory in every layer (functional.FusedCrossKVFn).  Placement is a memory-layout choice only:
# names, shapes and state-dict order are untouched.
_GROUPED_SUFFIXES = ("multihead_attn.in_proj_weight", "multihead_attn.in_proj_bias")


def _placement_order(named_params: List[Tuple[str, nn.Parameter]]) -> List[Tuple[str, nn.Parameter]]:
    order: List[Tuple[str, nn.Parameter]] = []
    done = set()
    for n, p in named_params:
        if n in done:
            continue
        suffix = next((s for s in _GROUPED_SUFFIXES if n.endswith(s)), None)
        if suffix is None:
            order.append((n, p))
            done.add(n)
            continue
        for n2, p2 in named_params:             # pull every member of the family here, in model (layer) order
            if n2.endswith(suffix) and n2 not in done and p2.shape == p.shape:
                order.append((n2, p2))
                done.add(n2)
    return order


class FlatParams:
    def __init__(self, named_params: List[Tuple[str, nn.Parameter]], device: torch.device, compute_dtype: torch.dtype):
        self.names = [n for n, _ in named_params]
        self.params = [p for _, p in named_params]
        self.device = device
        self.compute_dtype = compute_dtype
        self.offsets: Dict[str, Tuple[int, int]] = {}
        off = 0
        for n, p in _placement_order(named_params):
            self.offsets[n] = (off, p.numel())
            off += (p.numel() + ALIGN - 1) // ALIGN * ALIGN
        self.total = off
        self.master = torch.zeros(off, dtype=torch.float32, device=device)
        self.grad = torch.zeros(off, dtype=torch.float32, device=device)
        self.lowp = torch.zeros(off, dtype=torch.bfloat16, device=device) if compute_dtype == torch.bfloat16 else None
        self.exp_avg: Optional[torch.Tensor] = None
        self.exp_avg_sq: Optional[torch.Tensor] = None
        self.ema: Optional[torch.Tensor] = None          # EMA of the masters, same layout (FusedAdam.enable_ema)
        with torch.no_grad():
            for n, p in named_params:
                o, cnt = self.offsets[n]
                perm = _phys_perm(p.dim())
                phys_shape = tuple(p.shape) if perm is None else tuple(p.shape[i] for i in perm)

                def views(buf):
                    phys = buf[o:o + cnt].view(phys_shape)
                    logical = phys if perm is None else phys.permute(_inverse(perm))
                    return phys, logical

                phys, logical = views(self.master)
                logical.copy_(p.detach().to(device=device, dtype=torch.float32))
                p.data = logical
                p.omr_phys = phys
                gphys, glogical = views(self.grad)
                p.omr_grad = gphys
                p.grad = glogical
                p.omr_lowp = views(self.lowp)[0] if self.lowp is not None else None
        # Data-gradient weights of the dense 3x3 convs ([CIN,3,3,COUT], taps mirrored: the transposed conv's operand) in the
        # compute dtype: refreshed once per optimizer step by ONE launch (refresh_flips) instead of one re-layout launch in front
        # of every data gradient of the backward pass.  A per-parameter (torch version, update count) stamp guards manual edits.
        convs = [p for p in self.params if p.dim() == 4 and tuple(p.shape[2:]) == (3, 3) and p.shape[1] > 1]
        self.flip = torch.empty(sum(p.numel() for p in convs), dtype=compute_dtype, device=device)
        self.updates = 0                 # weight updates that bypass torch's version counter (the step kernel writes through raw pointers)
        self._flip_table = None
        self._flip_params = convs
        pairs, off = [], 0
        for p in convs:
            cout, cin = p.shape[0], p.shape[1]
            p.omr_flip = self.flip[off:off + p.numel()].view(cin, 3, 3, cout)
            p.omr_flat = self
            p.omr_flip_stamp = None
            off += p.numel()
            pairs.append((p.omr_phys if compute_dtype == torch.float32 else p.omr_lowp, p.omr_flip))
        self._flip_pairs = pairs
        self.sync_lowp()

    def sync_lowp(self) -> None:
        """Refresh the bf16 compute copy from the fp32 masters (after load_state_dict / manual edits)."""
        if self.lowp is not None:
            K.cast(self.master, torch.bfloat16, out=self.lowp)
        self.refresh_flips()

    def refresh_flips(self) -> None:
        """Re-lay the data-gradient weights of all dense 3x3 convs from the current compute weights (one launch)."""
        if not self._flip_pairs or not self.master.is_cuda:
            return
        if self._flip_table is None:
            self._flip_table = K.conv3x3_weight_flip_table(self._flip_pairs)
        K.conv3x3_weight_flip_grouped(self._flip_table)
        for p in self._flip_params:
            p.omr_flip_stamp = (p._version, self.updates)

    def flipped(self, p: nn.Parameter, dtype: torch.dtype) -> torch.Tensor:
        """Data-gradient weights of conv parameter p.  Current by construction after FusedAdam.step / sync_lowp; an in-place
        edit of the parameter through torch (copy_, a sub-module's load_state_dict) bumps its version counter and triggers a
        refresh here.  (In bf16 mode such an edit needs sync_compute_weights() anyway: the forward reads the bf16 copy.)"""
        if dtype != self.compute_dtype:
            return K.conv3x3_weight_flip(p.omr_phys if dtype == torch.float32 else p.omr_lowp)
        if p.omr_flip_stamp != (p._version, self.updates):
            self.refresh_flips()
        return p.omr_flip

    def zero_grad(self) -> None:
        from .runtime import WgradStream
        WgradStream.reset()         # also drops what a failed backward pass left collected
        self.grad.zero_()

    def slice_of(self, names: Iterable[str]) -> Tuple[int, int]:
        """[begin, end) element range of the flat buffers that covers the given parameters."""
        offs = [self.offsets[n] for n in names]
        b = min(o for o, _ in offs)
        e = max((o + c + ALIGN - 1) // ALIGN * ALIGN for o, c in offs)
        return b, e

    def module_ranges(self) -> "Dict[str, Tuple[int, int]]":
        """{top-level sub-module name: [begin, end)}: the contiguous range of the flat buffers each top-level sub-module
        (encoder, image_encoder, audio_encoder, decoder, cross_attn) owns.  Placement keeps every sub-module contiguous (the
        grouped cross-attention in_proj family lies inside `decoder`); checked here."""
        groups: Dict[str, List[str]] = {}
        for n in self.names:
            groups.setdefault(n.split(".", 1)[0], []).append(n)
        ranges = {g: self.slice_of(ns) for g, ns in groups.items()}
        spans = sorted(ranges.values())
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "top-level sub-modules overlap in the flat buffer"
        return ranges


class StepLedger:
    """Step counts of the guarded optimizer step when the apply / skip decision of a step arrives AFTER the next one is due:
    host values only (no tensors, no events), in the spirit of evaluation.decode_rows, so a CPU test can script it.

    count(names) counts a step TENTATIVELY for the sub-modules it touches and returns its index k; settle(k, applied) closes it:
    a step that was not applied gives its +1 back to exactly those sub-modules and raises `skipped`.  At most one step is open:
    the caller settles step k - 1 before it counts step k, so the counts it reads for step k's bias corrections are exact -- a
    skipped step never counts, whichever sub-modules it touched."""

    def __init__(self, names: Iterable[str]):
        self.steps: Dict[str, int] = {n: 0 for n in names}
        self.skipped = 0
        self.issued = 0                                    # index of the next step
        self._open: Optional[Tuple[int, Tuple[str, ...]]] = None

    @property
    def open(self) -> Optional[int]:
        """Index of the step whose record has not been settled (None: every step is settled)."""
        return None if self._open is None else self._open[0]

    def count(self, names: Iterable[str]) -> int:
        if self._open is not None:
            raise RuntimeError(f"StepLedger: step {self._open[0]} has to be settled before the next one is counted")
        names = tuple(names)
        for n in names:
            self.steps[n] += 1
        k = self.issued
        self.issued += 1
        self._open = (k, names)
        return k

    def settle(self, k: int, applied: bool) -> None:
        """Record k says applied / not applied.  Settling a step that is not open (again, or never counted) changes nothing."""
        if self._open is None or self._open[0] != k:
            return
        if not applied:
            for n in self._open[1]:
                self.steps[n] -= 1
            self.skipped += 1
        self._open = None


class _Guard:
    """Device side of FusedAdam's guard: the reduction workspace, ONE omr_step_ctl on the device, and a two-deep ring of pinned host
    copies with an event each (step k's copy goes to slot k % 2, so the last settled record stays readable while the next copy
    is in flight)."""

    def __init__(self, flat: FlatParams, max_norm: Optional[float]):
        self.max_norm = max_norm
        self.ws = torch.empty(K.grad_norm_workspace_bytes(flat.total, K.GRAD_NORM_MAX_RANGES), dtype=torch.uint8, device=flat.device)
        self.ctl = K.new_step_ctl(flat.device)
        self.ring = torch.zeros((2, self.ctl.numel()), dtype=torch.uint8)
        if self.ctl.is_cuda:
            self.ring = self.ring.pin_memory()
        self.events: List[Optional[torch.cuda.Event]] = [None, None]
        self.meta: List[Optional[Tuple[Tuple[str, ...], float]]] = [None, None]     # (range names, grad_scale) of the step in each slot
        self.settled = None               # (StepCtl, names, grad_scale) of the newest settled record

    def push(self, k: int, names: Tuple[str, ...], grad_scale: float) -> None:
        self.ring[k % 2].copy_(self.ctl, non_blocking=True)
        if self.events[k % 2] is None:
            self.events[k % 2] = torch.cuda.Event()
        self.events[k % 2].record()
        self.meta[k % 2] = (names, grad_scale)

    def pull(self, k: int) -> bool:
        """Wait for step k's copy (one whole forward and backward old in steady state: no wait) and decode it -> applied."""
        self.events[k % 2].synchronize()
        rec = K.read_step_ctl(self.ring[k % 2])
        self.settled = (rec,) + self.meta[k % 2]
        return bool(rec.apply)


def decays(name: str, ndim: int, no_decay: Iterable[str]) -> bool:
    """Does weight decay apply to this parameter?  Never to one with fewer than two dimensions (biases, norm gains), nor to one
    whose name holds one of the `no_decay` substrings (OptimConfig.no_decay)."""
    return ndim >= 2 and not any(s in name for s in no_decay)


def decay_block_map(offsets: Dict[str, Tuple[int, int]], ndims: Dict[str, int], total: int, no_decay: Iterable[str]) -> List[int]:
    """One entry per K.DECAY_BLOCK elements of a flat buffer of `total` elements (omr_adamw_ema's decay_blocks): 1 where the block
    belongs to a parameter that decays, else 0.  Every parameter starts on a multiple of ALIGN, which the block size divides, so a
    block never holds two parameters; the unused end of a parameter's last block shares its entry (nothing reads those elements),
    and blocks no parameter touches count as "no decay".  Host values only: a CPU test checks it against a hand-made table."""
    B = K.DECAY_BLOCK
    assert ALIGN % B == 0
    no_decay = tuple(no_decay)
    blocks = [0] * ((total + B - 1) // B)
    for name, (off, count) in offsets.items():
        if off % ALIGN:
            raise ValueError(f"decay_block_map: {name} starts at {off}, not on a multiple of {ALIGN}")
        if decays(name, ndims[name], no_decay):
            for k in range(off // B, (off + count + B - 1) // B):
                blocks[k] = 1
    return blocks


class FusedAdam:
    """torch.optim.Adam(lr=1e-4, amsgrad=False) semantics (model.py:134-139,475-483) as one kernel launch per top-level
    sub-module over the flat buffers (one launch in the common case that every sub-module has gradients).
    Interface subset of torch.optim.Optimizer: step / zero_grad / param_groups / state_dict.

    optim (config.OptimConfig, optional): the recipe around that update -- decoupled weight decay (torch.optim.AdamW) that leaves
    biases and norm gains alone, a learning-rate schedule (config.lr_at, indexed by step() CALLS) and an exponential moving
    average of the weights (enable_ema / ema_weights).  Every range goes through the one step kernel (kernels.adam_step,
    omr_adamw_ema), behind the guard's record when the guard is on; what a config does not ask for is passed as its neutral value
    (weight_decay 0, no average, no record), which leaves torch.optim.Adam's update.

    Parameters WITHOUT a gradient are skipped like torch.optim.Adam skips `p.grad is None` (Lightning zeroes with
    set_to_none): no update from stale momentum, no moment decay, no step count.  In MultimodalTransformer the modality-drop
    steps (model.py:510-519) leave one encoder and cross_attn without gradients; the model reports the sub-modules that took
    part in the step through `touched_fn` and each sub-module keeps its own step count for the bias correction.  (Under data
    parallelism every rank takes the same branch BY CONSTRUCTION: the modality decision is drawn from a generator all ranks
    seed with rank 0's value -- model.MultimodalTransformer._draw_modality, ddp.GradReducer.broadcast_state -- so all ranks
    skip the same slices; tests/test_ddp_cpu.py runs it with ranks seeded differently.)"""

    def __init__(self, flat: FlatParams, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8, touched_fn=None,
                 optim: Optional[OptimConfig] = None):
        self.flat = flat
        self.param_groups = [dict(params=flat.params, lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False)]
        self.ranges = flat.module_ranges()
        self._ledger = StepLedger(self.ranges)             # owns `steps` and `skipped`
        self.touched_fn = touched_fn
        self._guard: Optional[_Guard] = None
        if flat.exp_avg is None:
            flat.exp_avg = torch.zeros_like(flat.master)
            flat.exp_avg_sq = torch.zeros_like(flat.master)
        self.calls = 0                                     # step() calls so far: the schedule's index (a skipped step counts)
        self.optim: Optional[OptimConfig] = None
        self.ema_decay: Optional[float] = None
        self._decay_blocks: Optional[torch.Tensor] = None
        self._in_ema = False
        if optim is not None:
            self._configure(optim)

    # ---- recipe: decoupled weight decay, schedule, EMA weights (config.OptimConfig; omr_adamw_ema in csrc/optim.hip)
    def _configure(self, optim: OptimConfig) -> None:
        f, g = self.flat, self.param_groups[0]
        self.optim = optim
        g.update(lr=optim.lr, betas=optim.betas, eps=optim.eps, weight_decay=optim.weight_decay)
        self._decay_blocks = None
        if optim.weight_decay != 0:                        # built once: the placement never changes
            ndims = {n: p.dim() for n, p in zip(f.names, f.params)}
            self._decay_blocks = torch.tensor(decay_block_map(f.offsets, ndims, f.total, optim.no_decay), dtype=torch.uint8).to(f.device)
        if optim.ema_decay is not None:
            self.enable_ema(optim.ema_decay)

    @property
    def _recipe(self) -> bool:
        """Does the recipe ask for anything?  Not with a config that asks for nothing new and no EMA: then step() reads the learning
        rate from param_groups and leaves it alone, exactly as without a config.  (The kernel is the same either way.)"""
        return self.flat.ema is not None or (self.optim is not None and not self.optim.plain)

    def enable_ema(self, decay: float) -> None:
        """Keep an exponential moving average of the weights in `flat.ema` (fp32, laid out like `flat.master`):
        ema = decay * ema + (1 - decay) * p after every applied step, inside the step kernel.
        The average starts as a COPY of the current `flat.master` -- torch.optim.swa_utils.AveragedModel's first update.
        Only the ranges a step touches are averaged: a sub-module the modality drop left without gradients keeps its average,
        as it keeps its moments and its step count; so does everything when the guard skips the step.
        Calling it again changes the decay and keeps the average."""
        if not 0 <= decay <= 1:
            raise ValueError(f"enable_ema: decay must lie in [0, 1] (got {decay})")
        if self._in_ema:
            raise RuntimeError("enable_ema: not inside ema_weights()")
        self.ema_decay = float(decay)
        if self.flat.ema is None:
            self.flat.ema = self.flat.master.clone()

    @contextlib.contextmanager
    def ema_weights(self):
        """Scope in which the model computes with the averaged weights: settles the last guarded step, exchanges `flat.master`
        and `flat.ema` in place (omr_swap_f32: no third buffer) and refreshes the bf16 copy and the conv flips; on exit -- also
        when the body raised -- exchanges them back and refreshes again, which restores every buffer to the bit.  Inside,
        the parameters (state_dict, save_checkpoint) ARE the averaged weights.  Not nestable; step() inside is refused."""
        if self.flat.ema is None:
            raise RuntimeError("ema_weights: no average is kept -- call enable_ema(decay) or give OptimConfig(ema_decay=...)")
        if self._in_ema:
            raise RuntimeError("ema_weights: already inside the scope (it does not nest)")
        self.settle()
        self._swap_ema()
        self._in_ema = True
        try:
            yield self
        finally:
            self._in_ema = False
            self._swap_ema()

    def _swap_ema(self) -> None:
        f = self.flat
        K.swap_f32(f.master, f.ema)
        f.updates += 1              # a weight update torch's version counter does not see
        f.sync_lowp()

    @property
    def steps(self) -> Dict[str, int]:
        """{top-level sub-module: optimizer steps applied to it}; with the guard on, the last step's count is tentative until
        settle()."""
        return self._ledger.steps

    @steps.setter
    def steps(self, value: Dict[str, int]) -> None:
        self._ledger.steps = value

    @property
    def step_count(self) -> int:
        self.settle()
        return max(self.steps.values())

    def zero_grad(self, set_to_none: bool = False) -> None:
        self.flat.zero_grad()

    # ---- guard: global gradient norm, clipping and the skip of a non-finite step, decided on the device (csrc/optim.hip)
    def enable_guard(self, max_norm: Optional[float] = None, skip_nonfinite: bool = True) -> None:
        """From the next step() on: one omr_grad_norm over the touched sub-modules' ranges, then the step kernel behind the
        record it filled.  max_norm: clip the gradient to this global L2 norm (torch.nn.utils.clip_grad_norm_; None = no clipping).
        A step whose gradient holds inf / NaN (or whose sum of squares overflows) writes nothing and does not count.  That
        holds whenever the guard is on -- a clip factor computed from a non-finite norm has no meaning -- so skip_nonfinite only
        says whether a guard WITHOUT clipping is wanted; enable_guard(None, False) asks for nothing and is refused.
        The host learns of a step's outcome one step late (settle())."""
        if max_norm is None and not skip_nonfinite:
            raise ValueError("enable_guard: nothing to guard -- give max_norm and / or skip_nonfinite=True")
        if max_norm is not None and not max_norm > 0:
            raise ValueError(f"enable_guard: max_norm must be positive (got {max_norm}); None switches clipping off")
        self.settle()
        self._guard = _Guard(self.flat, max_norm)

    def disable_guard(self) -> None:
        """Back to the unguarded path (the step kernel without a record); the step counts and `skipped` stay."""
        self.settle()
        self._guard = None

    def settle(self) -> None:
        """Close the last guarded step: wait for the copy of its record and, if the device skipped it, take its step count back."""
        k = self._ledger.open
        if k is not None:
            self._ledger.settle(k, self._guard.pull(k))

    @property
    def skipped(self) -> int:
        """Guarded steps the device did not apply."""
        self.settle()
        return self._ledger.skipped

    @property
    def last_grad_norm(self) -> Optional[float]:
        """Global L2 norm of the last guarded step's gradient, times its grad_scale, before clipping (waits for that step)."""
        self.settle()
        return self.settled_grad_norm

    @property
    def settled_grad_norm(self) -> Optional[float]:
        """The same for the newest step that is ALREADY settled -- one step behind right after step(); never waits."""
        s = None if self._guard is None else self._guard.settled
        return None if s is None else float(s[0].norm)

    @property
    def last_range_norms(self) -> Optional[Dict[str, float]]:
        """{sub-module: L2 norm of its gradient range, times grad_scale} of the last guarded step (waits for that step)."""
        self.settle()
        s = None if self._guard is None else self._guard.settled
        return None if s is None else {n: float(s[0].range_sumsq[r]) ** 0.5 * s[2] for r, n in enumerate(s[1])}

    def step(self, grad_scale: float = 1.0, touched=None) -> None:
        """touched: names of the top-level sub-modules that received gradients this step (None = all; default: ask the model)."""
        g = self.param_groups[0]
        f = self.flat
        if self._in_ema:
            raise RuntimeError("FusedAdam.step: inside ema_weights() the masters hold the averaged weights; leave the scope first")
        if touched is None and self.touched_fn is not None:
            touched = self.touched_fn()
        names = list(self.ranges) if touched is None else [n for n in self.ranges if n in set(touched)]
        guard = self._guard if names else None
        if guard is None:
            for n in names:
                self.steps[n] += 1
        else:
            # The previous step's outcome first (its copy is a whole forward and backward old: no wait in steady state), only
            # then this step's count: the bias corrections below are exact although the decision is taken on the device.
            self.settle()
            k = self._ledger.count(names)
        from .runtime import WgradStream
        WgradStream.join()
        # merge neighbouring ranges that share a step count: one launch over the whole buffer in the common case
        runs: List[List[int]] = []
        names = sorted(names, key=lambda nm: self.ranges[nm][0])
        for n in names:
            b, e = self.ranges[n]
            if runs and runs[-1][1] == b and runs[-1][2] == self.steps[n]:
                runs[-1][1] = e
            else:
                runs.append([b, e, self.steps[n]])
        if guard is not None:
            K.grad_norm(f.grad, [self.ranges[n] for n in names], grad_scale, guard.max_norm, guard.ws, guard.ctl)
        cfg = self.optim
        if cfg is not None and self._recipe:
            # The schedule is indexed by CALLS: a step the device skips still advances it, so no host decision waits for the guard.
            g["lr"] = lr_at(cfg, self.calls)
        self.calls += 1
        for b, e, st in runs:
            K.adam_step(f.master[b:e], f.grad[b:e], f.exp_avg[b:e], f.exp_avg_sq[b:e], st, g["lr"], g["betas"], g["eps"], grad_scale,
                        p_lowp=None if f.lowp is None else f.lowp[b:e], weight_decay=0.0 if cfg is None else cfg.weight_decay,
                        decay_blocks=None if self._decay_blocks is None else self._decay_blocks[b // K.DECAY_BLOCK:],
                        ema=None if f.ema is None else f.ema[b:e], ema_decay=self.ema_decay or 0.0,
                        ctl=None if guard is None else guard.ctl)
        if guard is not None:
            guard.push(k, tuple(names), grad_scale)
        f.updates += 1
        f.refresh_flips()           # the next backward pass finds its data-gradient weights ready (harmless after a skipped step)

    def state_dict(self):
        sd = dict(step=self.step_count, steps=dict(self.steps), exp_avg=self.flat.exp_avg, exp_avg_sq=self.flat.exp_avg_sq, param_groups=[
            {k: v for k, v in self.param_groups[0].items() if k != "params"}])
        if self._guard is not None:
            sd["skipped"] = self.skipped
        sd["calls"] = self.calls
        if self.optim is not None:
            sd["optim"] = self.optim.to_dict()
        if self.flat.ema is not None:
            # inside ema_weights() the two buffers are exchanged: the average is what `master` holds there
            sd["ema"] = self.flat.master.clone() if self._in_ema else self.flat.ema
            sd["ema_decay"] = self.ema_decay
        return sd

    def load_state_dict(self, sd) -> None:
        """Also takes a dict written before the recipe existed (no `calls`, `optim`, `ema`): the schedule then starts at the
        number of applied steps, and configuration and average stay as they are."""
        if self._in_ema:
            raise RuntimeError("FusedAdam.load_state_dict: not inside ema_weights()")
        self.settle()
        self.steps = {g: int(sd.get("steps", {}).get(g, sd["step"])) for g in self.ranges}
        self._ledger.skipped = int(sd.get("skipped", 0))
        self.flat.exp_avg.copy_(sd["exp_avg"])
        self.flat.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.calls = int(sd.get("calls", sd["step"]))
        if sd.get("optim") is not None:
            self._configure(OptimConfig.from_dict(sd["optim"]))
        if sd.get("ema") is not None:
            self.enable_ema(sd["ema_decay"])
            self.flat.ema.copy_(sd["ema"])
        if self._recipe and self.optim is not None and self.calls > 0:
            self.param_groups[0]["lr"] = lr_at(self.optim, self.calls - 1)      # what the last step() left there
