"""The CTC prefix-score kernels (omr_ctc_prefix_init / omr_ctc_prefix_scores / omr_ctc_prefix_advance) against the fp64 reference, the float32
yardstick and the case table of tests/ctc_prefix_refs.py: one and two frames, frame counts around one and two LDS tiles, ragged inputs with an
empty one, the empty hypothesis, the repeat rule, <eos> / blank / <sos> / out-of-vocabulary candidates, beam 3 and 8, vocabularies that are
no multiple of 8, chains of positions through advance -> score; fp32 and bf16 logits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ctc_prefix_refs as R
from oracle import kernel_refs as KR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 256
SENT = 0xA5


def K():
    from omr_a2s_multimodal_transformer_amd import kernels
    return kernels


def guarded(shape, dtype):
    """A tensor of `shape` with a 256-byte band of SENT bytes behind it -> (tensor, the band)."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((n + GUARD,), SENT, dtype=torch.uint8, device=DEV)
    return raw[:n].view(dtype).view(*shape), raw[n:]


def block(case, weight=0.3):
    """The case's CtcPrefixBlock, its workspace moved into a buffer with a guard band behind it and initialised again -> (block, band)."""
    from omr_a2s_multimodal_transformer_amd._lib import cur_stream, lib
    inp = R.inputs(case)
    x = inp["buf"].to(DEV)[:, :, :case.V]
    blk = K().CtcPrefixBlock(x, inp["frame_len"].to(DEV), case.V, case.beam, R.BLANK, R.SOS, R.EOS, weight)
    n = blk.ws.numel()
    raw = torch.full((n + GUARD,), SENT, dtype=torch.uint8, device=DEV)
    blk.ws = raw[:n]
    blk.desc.ws = raw.data_ptr()
    assert lib().query("omr_ctc_beam_workspace_bytes", blk.byref()) == n
    lib().call("omr_ctc_prefix_init", blk.byref(), cur_stream())
    return blk, raw[n:]


def run(case):
    """The chain of tests/ctc_prefix_refs.run_chain through the entries -> the same structure, plus what the bit checks need."""
    blk, band = block(case)
    rows, beam, frames = case.N * case.beam, case.beam, case.frames
    bands = [band]
    out = []
    lasts = blk.last(0).cpu().tolist()
    assert lasts == [R.SOS] * rows and blk.logpsi().cpu().tolist() == [0.0] * rows
    for pos in range(case.positions):
        par = pos & 1
        cand, parents, tokens = R.plan(case, pos, lasts)
        delta, dband = guarded((rows, beam), torch.float32)
        bands.append(dband)
        blk.scores(par, torch.from_numpy(cand).to(DEV), out=delta)
        old_logpsi = blk.logpsi().cpu().numpy().copy()
        blk.state(par ^ 1).fill_(float("nan"))                                 # what the advance does not write stays NaN
        blk.advance(par, torch.from_numpy(parents).to(DEV), torch.from_numpy(tokens).to(DEV))
        torch.cuda.synchronize()
        st = blk.state(par ^ 1).cpu().numpy()
        for i in range(rows):
            assert np.isnan(st[i, :, frames[i // beam]:]).all(), "the advance wrote behind a sample's frames"
        lasts = blk.last(par ^ 1).cpu().tolist()
        out.append(dict(cand=cand, parents=parents, tokens=tokens, delta=delta.cpu().numpy().copy(), gn=st[:, 0].copy(), gb=st[:, 1].copy(),
                        logpsi=blk.logpsi().cpu().numpy().copy(), last=np.array(lasts), old_logpsi=old_logpsi))
    for b in bands:
        assert bool((b == SENT).all()), "a guard band was written"
    lse = blk.lse().cpu().numpy().copy()
    for n, F in enumerate(frames):
        lse[n, F:] = 0.0
    return dict(lse=lse, positions=out)


@functools.lru_cache(maxsize=None)
def result(case):
    return run(case)


@functools.lru_cache(maxsize=None)
def reference(case):
    ref = R.run_chain(case)
    return ref, R.bounds(case, ref)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_scores_and_stored_rows(case):
    """delta, the stored gn / gb rows and logpsi of every position within 4 x the float32 yardstick's error (+ half a bf16 ulp of the logits);
    -inf exactly where the reference has it; the survivors' last tokens; lse within the project's fp32 tolerance."""
    got = result(case)
    ref, (bound, e32) = reference(case)
    err = R.errors(got, ref)
    for k in R.KINDS:
        ratio = err[k] / e32[k] if e32[k] > 0 else float("inf") if err[k] > 0 else 0.0
        print(f"{case.name} {k}: kernel error {err[k]:.3e}, float32 yardstick {e32[k]:.3e}, ratio {ratio:.2f}, bound {bound[k]:.3e}")
    for k in R.KINDS:
        assert err[k] <= bound[k], (case.name, k, err[k], bound[k])
    for g, r in zip(got["positions"], ref["positions"]):
        assert g["last"].tolist() == r["last"].tolist()
    assert np.allclose(got["lse"], ref["lse"], **KR.tol(KR.F32))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_a_survivor_keeps_its_candidates_bits(case):
    """Score and advance run one row body: wherever a survivor (parent, token) was also a candidate of that parent, the candidate's delta is
    min(stored logpsi - the parent's logpsi, 0) formed in float32 from the STORED bits -- at position 0, where the parent's logpsi is 0, the
    stored logpsi itself."""
    got = result(case)
    checked = 0
    for t, pos in enumerate(got["positions"]):
        for i in range(len(pos["tokens"])):
            r = (i // case.beam) * case.beam + int(pos["parents"][i])
            for j in np.nonzero(pos["cand"][r] == pos["tokens"][i])[0]:
                new, old = np.float32(pos["logpsi"][i]), np.float32(pos["old_logpsi"][r])
                with np.errstate(invalid="ignore"):
                    want = np.float32(-np.inf) if new == -np.inf else min(np.float32(new - old), np.float32(0))
                assert np.float32(pos["delta"][r, j]).tobytes() == np.float32(want).tobytes(), (case.name, t, i, r, j)
                if t == 0 and new <= 0:
                    assert np.float32(pos["delta"][r, j]).tobytes() == new.tobytes()
                checked += 1
    assert checked >= case.positions


@pytest.mark.parametrize("case", [c for c in R.CASES if c.name in ("fp32-ragged", "bf16-ragged8", "fp32-2chunk+1", "bf16-chunk")], ids=lambda c: c.name)
def test_two_runs_give_the_same_bits(case):
    a, b = result(case), run(case)
    for pa, pb in zip(a["positions"], b["positions"]):
        for k in ("delta", "gn", "gb", "logpsi"):
            KR.assert_bit_equal(torch.from_numpy(pb[k]), torch.from_numpy(pa[k]), f"{case.name} {k}")


def test_the_long_case_against_plain_float32():
    """What the (maximum, sum) accumulation of logpsi buys on F = 1500: printed, and never worse than the float32 yardstick's own error."""
    case = [c for c in R.CASES if c.name == "fp32-long"][0]
    ref, (bound, e32) = reference(case)
    err = R.errors(result(case), ref)
    print(f"long case: kernel / float32 yardstick errors -- delta {err['delta']:.3e} / {e32['delta']:.3e}, rows {err['rows']:.3e} / "
          f"{e32['rows']:.3e}, logpsi {err['logpsi']:.3e} / {e32['logpsi']:.3e}")
    assert all(err[k] <= bound[k] for k in R.KINDS)


def test_dead_rows_and_done_inputs_are_skipped():
    case = [c for c in R.CASES if c.name == "fp32-ragged"][0]
    blk, band = block(case)
    rows, beam = case.N * case.beam, case.beam
    _, parents, tokens = R.plan(case, 0, [R.SOS] * rows)
    scores = torch.zeros(rows, dtype=torch.float64, device=DEV)
    scores[1] = float("-inf")                                                  # a dead padding row of input 0
    done = torch.tensor([0, 0, 1], dtype=torch.int32, device=DEV)              # input 2 has stopped
    blk.state(1).fill_(float("nan"))
    blk.last(1).fill_(-9)
    blk.advance(0, torch.from_numpy(parents).to(DEV), torch.from_numpy(tokens).to(DEV), scores=scores, done=done)
    torch.cuda.synchronize()
    st, last = blk.state(1).cpu().numpy(), blk.last(1).cpu().tolist()
    F0 = case.frames[0]
    for i in range(rows):
        skipped = i == 1 or i // beam == 2
        assert (last[i] == -9) == skipped, i
        if i // beam == 0:
            assert np.isnan(st[i, :, :F0]).all() == skipped, i
        if i // beam == 2:
            assert np.isnan(st[i]).all()
    assert bool((band == SENT).all())


def test_bad_arguments_are_refused_and_nothing_is_written():
    from omr_a2s_multimodal_transformer_amd._lib import lib
    case = [c for c in R.CASES if c.name == "fp32-F2"][0]
    blk, band = block(case)
    rows, beam = case.N * case.beam, case.beam
    torch.cuda.synchronize()
    before = blk.ws.clone()
    cand = torch.full((rows, beam), 3, dtype=torch.int64, device=DEV)
    delta, dband = guarded((rows, beam), torch.float32)
    delta.fill_(KR.SENTINEL)
    par = torch.zeros(rows, dtype=torch.int32, device=DEV)
    tok = torch.full((rows,), 3, dtype=torch.int64, device=DEV)
    d = blk.desc

    def calls():
        p = lambda t: t.data_ptr()  # noqa: E731
        return [lib().fns["omr_ctc_prefix_init"](blk.byref(), None), lib().fns["omr_ctc_prefix_scores"](blk.byref(), 0, p(cand), p(delta), None),
                lib().fns["omr_ctc_prefix_advance"](blk.byref(), 0, p(par), p(tok), None, None, None)]

    def with_field(name, value):
        keep = getattr(d, name)
        setattr(d, name, value)
        try:
            return calls()
        finally:
            setattr(d, name, keep)

    for name, value in [("lam", 0.0), ("lam", 1.0), ("lam", -0.5), ("lam", float("nan")), ("beam", 0), ("beam", 9), ("V", 0), ("ldv", case.V - 1),
                        ("blank", case.V), ("sos", -1), ("eos", R.SOS), ("N", 0), ("Fmax", 0), ("logits", None), ("frame_len", None), ("ws", None),
                        ("ws_bytes", 8), ("lse", None), ("state1", d.state0), ("dtype", 7)]:
        got = with_field(name, value)
        assert all(rc in (-1, -3) for rc in got), (name, value, got)
    p = lambda t: t.data_ptr()  # noqa: E731
    assert lib().fns["omr_ctc_prefix_scores"](blk.byref(), 2, p(cand), p(delta), None) == -1
    assert lib().fns["omr_ctc_prefix_scores"](blk.byref(), 0, None, p(delta), None) == -1
    assert lib().fns["omr_ctc_prefix_advance"](blk.byref(), -1, p(par), p(tok), None, None, None) == -1
    assert lib().fns["omr_ctc_prefix_advance"](blk.byref(), 0, None, p(tok), None, None, None) == -1
    bad = K()._CtcBeamDesc()
    bad.N, bad.beam, bad.Fmax = 1, 9, 4
    assert lib().query("omr_ctc_beam_workspace_bytes", ctypes.byref(bad)) == -1
    torch.cuda.synchronize()
    assert torch.equal(blk.ws, before) and bool((delta == KR.SENTINEL).all()) and bool((band == SENT).all()) and bool((dband == SENT).all())
    with pytest.raises(ValueError, match="ctc_decode"):
        K().CtcPrefixBlock(blk.logits, blk.frame_len, case.V, beam, R.BLANK, R.SOS, R.EOS, 1.0)
