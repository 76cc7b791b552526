"""The CTC loss kernels (omr_ctc_fwd / omr_ctc_bwd) against the fp64 reference, bounds and case table of tests/ctc_refs.py: label counts around
one wave of threads and at 1 025 states, repeated labels down to a single path, one frame, infeasible samples, the long thin precision case, a
ragged batch with padded columns, the scalar row pass, three vocabulary widths, 70 samples; both dtypes."""
import ctypes
import functools

import pytest
import torch

import ctc_refs as R
from oracle import kernel_refs as KR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ids = lambda cases: [c.name for c in cases]  # noqa: E731


def K():
    from omr_a2s_multimodal_transformer_amd import kernels
    return kernels


def run(case):
    """The case through the entries -> the dict ctc_refs.check takes; dlogits is the whole [B, Fmax, ldv] buffer."""
    inp = R.inputs(case)
    x = inp["buf"].to(DEV)[:, :, :case.V]
    flen, tgt = inp["frame_len"].to(DEV), inp["targets"].to(DEV)
    loss, rows, infeasible, acc2, ws = K().ctc_fwd(x, flen, tgt, case.V, R.BLANK, R.EOS)
    dl = K().ctc_bwd(x, flen, tgt, ws, case.V, R.BLANK, grad_scale=R.GRAD_SCALE, grad_out=torch.tensor([R.GRAD_OUT], device=DEV))
    dl = dl if dl._base is None else dl._base
    torch.cuda.synchronize()
    lse = K().ctc_workspace_lse(ws, case.B, case.Fmax).cpu()
    for b, n in enumerate(case.frames):
        lse[b, n:] = 0.0                                                    # frames >= F_b are skipped: the workspace holds nothing there
    return dict(loss=float(loss.cpu()[0]), rows=rows.cpu(), infeasible=int(infeasible.cpu()[0]), acc2=acc2.cpu(), lse=lse, dlogits=dl.cpu())


@functools.lru_cache(maxsize=None)
def result(case):
    return run(case)


@pytest.mark.parametrize("case", R.CASES, ids=ids(R.CASES))
def test_ctc_loss_and_gradient(case):
    """lse, the per-sample nll, the loss, the infeasible count, dlogits and its row sums within their bounds; what must be +0 is, bit for bit;
    acc2 holds the sum the mean was formed from."""
    out = result(case)
    R.check(case, out)
    R.check_zero_bits(case, out["dlogits"], out["rows"])
    assert float(out["acc2"][1]) == case.B
    assert float(torch.tensor(float(out["acc2"][0]) / case.B, dtype=torch.float64).float()) == out["loss"]


def test_the_long_case_beats_torch_fp32():
    """The offset scheme: on F = 2048 the kernel's nll is closer to fp64 than torch's own fp32 recursion is, whose |log alpha| has grown to ~1e4."""
    case = [c for c in R.CASES if c.name == "f32-long-thin"][0]
    out, r = result(case), R.reference(case)
    _, rows32, _ = R.torch_ctc(case, torch.float32)
    mine, theirs = abs(float(out["rows"][0]) - r["rows"][0]), abs(rows32[0] - r["rows"][0])
    print(f"long-thin nll error: kernel {mine:.3e}, torch fp32 {theirs:.3e}, fp32 rounding of the result {R.U * r['rows'][0]:.3e}")
    assert mine <= theirs + R.U * r["rows"][0]


@pytest.mark.parametrize("case", [c for c in R.CASES if c.name in ("f32-ragged", "bf16-repeats", "f32-L512", "bf16-infeasible")], ids=lambda c: c.name)
def test_two_runs_give_the_same_bits(case):
    a, b = result(case), run(case)
    for k in ("rows", "lse", "dlogits"):
        KR.assert_bit_equal(b[k], a[k], f"ctc {case.name} {k}")
    assert a["loss"] == b["loss"] and a["infeasible"] == b["infeasible"]


def test_bad_arguments_are_refused_and_nothing_is_written():
    from omr_a2s_multimodal_transformer_amd._lib import lib
    B, Fm, T, V = 2, 4, 3, 10
    x = torch.zeros((B, Fm, V), device=DEV)
    flen = torch.full((B,), Fm, dtype=torch.int32, device=DEV)
    tgt = torch.full((B, T), 3, dtype=torch.int64, device=DEV)
    ws = torch.full((K().ctc_workspace_bytes(B, Fm, T, V),), 77, dtype=torch.uint8, device=DEV)
    outs = dict(acc2=torch.full((2,), KR.SENTINEL, dtype=torch.float64, device=DEV), loss=torch.full((1,), KR.SENTINEL, device=DEV),
                rows=torch.full((B,), KR.SENTINEL, device=DEV), inf=torch.full((1,), 99, dtype=torch.int32, device=DEV),
                dl=torch.full((B, Fm, V), KR.SENTINEL, device=DEV))
    before = {k: v.clone() for k, v in outs.items()}
    p = lambda t: t.data_ptr()  # noqa: E731

    def fwd(B=B, Fm=Fm, T=T, V=V, ldv=V, blank=0, eos=2, logits=p(x), ws_=p(ws)):
        return lib().fns["omr_ctc_fwd"](0, logits, ldv, p(flen), p(tgt), ws_, p(outs["acc2"]), p(outs["loss"]), p(outs["rows"]), p(outs["inf"]),
                                        B, Fm, T, V, blank, eos, None)

    def bwd(B=B, Fm=Fm, T=T, V=V, ldv=V, blank=0, dl=p(outs["dl"])):
        return lib().fns["omr_ctc_bwd"](0, p(x), ldv, p(flen), p(tgt), p(ws), dl, B, Fm, T, V, blank, ctypes.c_float(1.0), None, None)

    for rc in (fwd(B=0), fwd(Fm=0), fwd(T=0), fwd(T=1024), fwd(V=0), fwd(ldv=V - 1), fwd(blank=V), fwd(blank=-1), fwd(eos=V), fwd(eos=-2),
               fwd(logits=None), fwd(ws_=None), bwd(B=0), bwd(T=1024), bwd(ldv=V - 1), bwd(blank=V), bwd(dl=None)):
        assert rc == -1
    assert K().ctc_workspace_bytes(B, Fm, T, V) > 0 and lib().query("omr_ctc_workspace_bytes", B, Fm, 1024, V) == -1
    torch.cuda.synchronize()
    for k, v in outs.items():
        KR.assert_bit_equal(v.cpu(), before[k].cpu(), f"refused call wrote {k}")
    assert bool((ws == 77).all())
