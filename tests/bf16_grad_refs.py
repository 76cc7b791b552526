"""References and the bound for the gradients of the bf16 training step (tests/test_bf16_grad_refs_cpu.py checks the method on the CPU,
tests/test_bf16_grad_parity_gpu.py applies it to the HIP path; DESIGN.md "bf16 gradient parity" has the storage-point mapping).

The fp64 oracle (oracle/ref_cpu.py with the run's own dropout and ReLU masks injected, `oracle_grads`) differentiates the same
piecewise-linear function as the HIP run.  A bf16 run differs from it by the rounding of every tensor it STORES in bf16, and how much that
moves each parameter gradient is measured on the reference alone: `emulate` runs the same oracle forward and backward and rounds
straight-through to bf16 -- the value in forward, the gradient in backward -- at the tensors the HIP path stores in bf16, accumulating in
the oracle's dtype between them.  Two realisations (fp64 and fp32 accumulation) give the yardstick

    e_ref[n] = max over the two of ||g_emul[n] - g64[n]|| / ||g64[n]||

per parameter, for the whole flat gradient ("<all>") and for the logits ("<logits>"); `check_gradients` holds an implementation to
max(2 e_ref[n], 1e-3) per parameter, 1.5 e_ref on the whole gradient and 2 e_ref on the logits.  The factors are margins over a
reference-only measurement: two correct implementations draw independent rounding noise.  Nothing here reads the code under test.

Rounding points of the FULL set, all from outside the oracle (whose results are pinned by tests/golden):
  * matrices (dim >= 2: conv, depthwise, linear, in_proj, embedding, head): value only -- the bf16 compute copies; their gradients are
    accumulated in fp32 and never rounded;
  * F.conv2d / F.linear: input 0 and the output, value and gradient (every conv / depthwise / pointwise / GEMM reads and writes bf16
    tensors; rounding the input also covers the cast image, the residual adds, +PE and the normalise-on-load of conv3);
  * torch.softmax output: value only (P as the P.V product reads it; dP stays in registers);
  * torch.matmul: the scores get a gradient-only rounding (dS is bf16 for the dQ / dK products, S itself never leaves registers), the
    P.V product is rounded in value and gradient (the stored attention output and its gradient);
  * DropPlan.apply: "attn" rounds the dropped probabilities in value; "nhwc" / "rows" round input and output in value and gradient (the
    fused epilogues store round(round(v) * scale), add+LayerNorm rounds the dropped branch, embed+PE is stored before its dropout);
  * instance_norm / layer_norm outputs, value and gradient.
Not rounded (fp32 in the HIP path): biases, LayerNorm weights, statistics, the sum dropout(x) + res inside add+LayerNorm, the scores and
dP, every parameter gradient.  The conv/linear-only set rounds the outputs of F.conv2d and F.linear and nothing else.
"""
import contextlib
import statistics

import torch
import torch.nn.functional as F
from torch.overrides import TorchFunctionMode

from oracle import ref_cpu as R

ALL, LOGITS = "<all>", "<logits>"
FLOOR, PER_TENSOR, WHOLE, LOGIT_FACTOR = 1e-3, 2.0, 1.5, 2.0      # check_gradients' margins (module docstring)


# ------------------------------------------------------------------------------------------------ shared with the fp32 parity test

def materialise(trace, relu_trace, dev="cuda:0"):
    """The HIP run's dropout masks (from (kind, p, seed, mode), through omr_dropout / omr_attn_dropout_mask) and ReLU masks
    as CPU tensors in the oracle's layouts; dropout masks are built lazily because their shapes come from the oracle."""
    from omr_a2s_multimodal_transformer_amd import kernels as K
    cache = {}

    def drop_mask(site, kind, p, shape, channel):
        tkind, tp, seed, tch = trace[site]
        assert tkind == kind and abs(tp - p) < 1e-12 and tch == channel, (site, trace[site], kind, p, channel)
        if site not in cache:
            if kind == "attn":
                B, H, T, S = shape
                m = K.attn_dropout_mask(B, H, T, S, p, seed, dev).float() / (1.0 - p)
            elif kind == "nhwc":
                B, C, Hh, W = shape
                m = K.dropout(torch.ones((B, Hh, W, C), device=dev, dtype=torch.float32), p, seed, channel).permute(0, 3, 1, 2)
            else:
                m = K.dropout(torch.ones(shape, device=dev, dtype=torch.float32), p, seed, False)
            cache[site] = m.cpu().contiguous()
        return cache[site]

    relu_masks = [(m.permute(0, 3, 1, 2) if m.dim() == 4 else m).cpu().contiguous() for m in relu_trace]      # NHWC -> NCHW
    return drop_mask, relu_masks


def oracle_grads(fwd, sd32, dtype, drop_mask, relu_masks):
    sd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd32.items()}
    plan = R.DropPlan(lambda *a: drop_mask(*a).to(dtype), relu_fn=lambda site, shape: relu_masks[site].to(dtype))
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)          # the oracle's sinusoid tables follow the default dtype
    try:
        logits, loss = fwd(sd, plan)
        loss.backward()
    finally:
        torch.set_default_dtype(prev)
    assert plan.relu_sites == len(relu_masks)
    return {k: v.grad for k, v in sd.items()}


def load(module, shapes, seed):
    from omr_a2s_multimodal_transformer_amd import synthetic as syn
    sd = syn.seeded_state_dict(shapes, seed)
    missing, unexpected = module.load_state_dict(sd, strict=False)
    assert not unexpected and all(m.endswith("pe") or m.endswith("pe_hwc") for m in missing)
    return sd


# ------------------------------------------------------------------------------------------------ straight-through bf16 rounding

def bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


class _Round(torch.autograd.Function):
    """value: round in forward; grad: round in backward; the other direction is the identity (straight through)."""

    @staticmethod
    def forward(ctx, x, value, grad):
        ctx.grad = grad
        return bf16(x) if value else x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return (bf16(g) if ctx.grad else g), None, None


def rnd(x):
    return _Round.apply(x, True, True)


def rnd_value(x):
    return _Round.apply(x, True, False)


def rnd_grad(x):
    return _Round.apply(x, False, True)


class RoundingMode(TorchFunctionMode):
    """Rounds around F.conv2d, F.linear, torch.matmul and torch.softmax as the module docstring lists.  full = False: the conv/linear-only
    set.  The oracle's attention calls torch.matmul twice, scores first, then P.V."""

    def __init__(self, full=True):
        super().__init__()
        self.full, self.matmuls = full, 0

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is F.conv2d or func is F.linear:
            if self.full:
                args = (rnd(args[0]) if args[0].requires_grad else bf16(args[0]),) + tuple(args[1:])
            return rnd(func(*args, **kwargs))
        if not self.full:
            return func(*args, **kwargs)
        if func is torch.matmul:
            self.matmuls += 1
            out = func(*args, **kwargs)
            return rnd_grad(out) if self.matmuls % 2 else rnd(out)
        if func is torch.softmax:
            return rnd_value(func(*args, **kwargs))
        return func(*args, **kwargs)


class RoundingPlan(R.DropPlan):
    """DropPlan whose dropout sites store what the HIP epilogues store (module docstring).  full = False rounds nothing here."""

    def __init__(self, mask_fn, relu_fn=None, full=True):
        super().__init__(mask_fn, relu_fn)
        self.full = full

    def drop(self, x, m, site):
        """x * m of dropout site `site` (the hook the wrong-gradient plans of the CPU test override)."""
        return x * m

    def apply(self, x, kind, p, channel=False):
        if p <= 0.0:
            return x
        site = self.sites
        m = self.mask_fn(site, kind, float(p), tuple(x.shape), channel)
        self.sites += 1
        if not self.full:
            return self.drop(x, m, site)
        if kind == "attn":
            return rnd_value(self.drop(x, m, site))
        return rnd(self.drop(rnd(x), m, site))

    def mask(self, x, m, site):
        """x * m of ReLU site `site` (overridden like `drop`)."""
        return x * m

    def relu(self, x):
        if self.relu_fn is None:
            return F.relu(x)
        m = self.relu_fn(self.relu_sites, tuple(x.shape))
        self.relu_sites += 1
        return self.mask(x, m, self.relu_sites - 1)


@contextlib.contextmanager
def rounded_norms(instance_norm=None):
    """oracle.ref_cpu's instance_norm and layer_norm with rounded outputs while the block runs.  instance_norm(call index, x, plain):
    replaces the plain function for the calls it answers (not None) -- the CPU test's wrong InstanceNorm backward."""
    inorm, lnorm, calls = R.instance_norm, R.layer_norm, [0]

    def instance(x, eps=1e-3):
        i, calls[0] = calls[0], calls[0] + 1
        y = instance_norm(i, x, inorm) if instance_norm is not None else None
        return rnd(inorm(x, eps) if y is None else y)

    R.instance_norm, R.layer_norm = instance, lambda *a, **k: rnd(lnorm(*a, **k))
    try:
        yield
    finally:
        R.instance_norm, R.layer_norm = inorm, lnorm


class Result:
    """Parameter gradients by state-dict name (None: no gradient), the logits and the loss of one pass."""

    def __init__(self, grads, logits, loss, sites=(0, 0)):
        self.grads, self.logits, self.loss, self.sites = grads, logits, float(loss), tuple(sites)      # sites: (dropout, ReLU) calls of the pass


def reference(fwd, sd32, drop_mask, relu_masks):
    """The fp64 oracle on the run's piecewise-linear region: what every gradient is compared with."""
    return emulate(fwd, sd32, torch.float64, drop_mask, relu_masks, rounding=None)


def emulate(fwd, sd32, dtype, drop_mask, relu_masks, rounding="full", plan_cls=RoundingPlan, instance_norm=None):
    """One oracle forward + backward with the injected masks, accumulating in `dtype`.  rounding: None (the plain oracle), "full" or
    "conv_linear".  relu_masks None: the oracle's own ReLUs.  fwd(sd, plan) -> (logits, loss)."""
    full = rounding == "full"
    sd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd32.items()}
    used = {k: (rnd_value(v) if full and v.dim() >= 2 else v) for k, v in sd.items()}
    relu_fn = None if relu_masks is None else (lambda site, shape: relu_masks[site].to(dtype))
    mask_fn = lambda *a: drop_mask(*a).to(dtype)      # noqa: E731
    plan = R.DropPlan(mask_fn, relu_fn) if rounding is None else plan_cls(mask_fn, relu_fn, full=full)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)          # the oracle's sinusoid tables follow the default dtype
    try:
        with contextlib.ExitStack() as stack:
            if rounding is not None:
                mode = stack.enter_context(RoundingMode(full))
                if full:
                    stack.enter_context(rounded_norms(instance_norm))
            logits, loss = fwd(used, plan)
        if rounding is not None and full:
            assert mode.matmuls % 2 == 0, "the oracle's attention calls torch.matmul in pairs"
        loss.backward()
    finally:
        torch.set_default_dtype(prev)
    assert relu_masks is None or plan.relu_sites == len(relu_masks)
    return Result({k: v.grad for k, v in sd.items()}, logits.detach(), loss.detach(), (plan.sites, plan.relu_sites))


# ------------------------------------------------------------------------------------------------ yardstick and check

def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _flat(grads, names):
    return torch.cat([grads[n].detach().double().reshape(-1) for n in names])


def errors(got, g64):
    """Relative L2 error of `got` against the fp64 reference: per parameter that has an oracle gradient, ALL (the flat gradient over
    those parameters) and LOGITS.  A parameter the oracle gives a gradient and `got` does not is an error of 1."""
    names = [n for n, g in g64.grads.items() if g is not None]
    out = {}
    for n in names:
        g = got.grads.get(n)
        out[n] = 1.0 if g is None else _rel(g.detach().cpu(), g64.grads[n])
    zeros = {n: (got.grads[n] if got.grads.get(n) is not None else torch.zeros_like(g64.grads[n])).cpu() for n in names}
    out[ALL] = _rel(_flat(zeros, names), _flat(g64.grads, names))
    out[LOGITS] = _rel(got.logits.detach().cpu(), g64.logits)
    return out


def yardstick(g64, emulations):
    """e_ref: the largest error of the reference's own bf16-storage emulations, per key of `errors`."""
    errs = [errors(e, g64) for e in emulations]
    return {k: max(e[k] for e in errs) for k in errs[0]}


def bounds(e_ref):
    return {k: (WHOLE * v if k == ALL else LOGIT_FACTOR * v if k == LOGITS else max(PER_TENSOR * v, FLOOR)) for k, v in e_ref.items()}


def measure(got, g64, e_ref):
    """-> (ratios error / bound by key, the parameters without an oracle gradient whose gradient in `got` is not exactly zero)."""
    err, bnd = errors(got, g64), bounds(e_ref)
    nonzero = [n for n, g in g64.grads.items() if g is None and got.grads.get(n) is not None and float(got.grads[n].abs().max()) != 0.0]
    return {k: err[k] / bnd[k] for k in err}, nonzero


def check_gradients(got, g64, e_ref, label=""):
    """Every parameter with an oracle gradient within max(2 e_ref[n], 1e-3), the whole gradient within 1.5 x and the logits within 2 x
    their yardsticks; parameters without an oracle gradient exactly zero; nothing left out.  Prints and returns the figures."""
    ratios, nonzero = measure(got, g64, e_ref)
    per = {k: v for k, v in ratios.items() if k not in (ALL, LOGITS)}
    have = [n for n, g in g64.grads.items() if g is not None]
    worst = max(per, key=per.get)
    e = [e_ref[n] for n in have]
    report = dict(worst=per[worst], worst_name=worst, whole=ratios[ALL], logits=ratios[LOGITS], e_min=min(e), e_med=statistics.median(e),
                  e_max=max(e), e_all=e_ref[ALL], e_logits=e_ref[LOGITS], checked=len(per))
    print(f"{label} worst {per[worst]:.3f} x bound ({worst}); whole gradient {ratios[ALL]:.3f} x, logits {ratios[LOGITS]:.3f} x; "
          f"e_ref min {min(e):.2e} median {report['e_med']:.2e} max {max(e):.2e}, whole {e_ref[ALL]:.2e}, logits {e_ref[LOGITS]:.2e}; "
          f"{len(per)} tensors")
    assert len(per) == len(have) and set(per) == set(have), (len(per), len(have))
    assert set(got.grads) >= set(g64.grads), sorted(set(g64.grads) - set(got.grads))
    assert not nonzero, f"gradient where the oracle has none: {nonzero}"
    over = sorted(((v, k) for k, v in ratios.items() if not v <= 1.0), reverse=True)
    assert not over, f"{label} above the bound (ratio, tensor): {over[:8]}"
    return report
