"""Joint CTC / attention beam search: beam_search_batch(ctc_decode=) and predict(beam=, ctc_decode=) against the per-input host loop
beam_search(ctc_decode=) (words identical, scores `==`), a planted case at the omr_beam_select_ctc level on which the CTC score changes the
outcome, and the unchanged default (no new entry is called without the keyword)."""
import ctypes

import numpy as np
import pytest
import torch

import spec_refs

pytestmark = pytest.mark.gpu

from omr_a2s_multimodal_transformer_amd import kernels as K  # noqa: E402
from omr_a2s_multimodal_transformer_amd import synthetic as syn  # noqa: E402
from omr_a2s_multimodal_transformer_amd._lib import cur_stream, lib, ptr  # noqa: E402
from omr_a2s_multimodal_transformer_amd.config import ModelConfig  # noqa: E402
from omr_a2s_multimodal_transformer_amd.decoder import BeamSearchBlock  # noqa: E402

DEV = "cuda:0"
NO_DROP = dict(dropout=0.0, encoder_dropout=0.0)
LAM = 0.3
# image sizes -> memory lengths ceil(H/16) * ceil(W/8) = 128, 250, 400, 450 (all above 64: every input takes the batched state) and
# CTC frame counts (ctc_pool = 1) of the same numbers: four to fifteen LDS tiles of the score kernel
SIZES = [(32, 512), (32, 1000), (64, 800), (48, 1200)]


def rnd(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _transformer(cfg, win=-1, max_seq=24, hw=(64, 1600), V=30, seed=61):
    """The small model of tests/test_beam_batch_gpu.py; the CTC head (not part of the seeded weights) is drawn from its own seed."""
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    w2i, i2w = syn.make_vocab(V)
    torch.manual_seed(seed)
    m = Transformer(hw[0], hw[1], max_seq, w2i, i2w, attn_window=win, config=cfg)
    sd = syn.seeded_state_dict(syn.transformer_shapes(V, cfg.d_model, cfg.ff_dim, cfg.num_layers), seed)
    m.load_state_dict(sd, strict=False)
    m.flatten_parameters()
    m.eval()
    return m


def _images(seed):
    return [rnd((1, 1, h, w), seed + i).to(DEV) for i, (h, w) in enumerate(SIZES)]


BLANK_BIAS = 8.0
EOS_BIAS_STEPS = [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 5.0, 6.0, 8.0]


def _search_biases(m, mems, beam=4):
    """A random head spreads every frame over the whole vocabulary, so P(no label at all) is e^-hundreds and no hypothesis ever takes <eos>:
    all inputs would run out of positions and the comparison would say little.  The CTC head's blank bias is raised by BLANK_BIAS (frames are
    mostly blank, as a trained head's are), then the decoder's <eos> bias over a fixed list of increments until the HOST LOOP's joint results
    end by <eos> at two different lengths below max_seq_len.  Fails, never skips, when no increment does."""
    m.ctc_head.bias.omr_phys[m.w2i["<PAD>"]] += BLANK_BIAS
    bias, eos = m.decoder.out_layer.bias.omr_phys, m.w2i["<eos>"]
    base = bias[eos].item()
    seen = []
    for add in EOS_BIAS_STEPS:
        bias[eos] = base + add
        res = [m.beam_search(x, beam, ctc_decode=LAM) for x in mems]
        ended = sorted({len(r[0]) for r in res if r[0][-1] == "<eos>" and len(r[0]) < m.max_seq_len})
        seen.append((add, [len(r[0]) for r in res]))
        if len(ended) >= 2:
            print(f"<eos> bias +{add}: joint lengths {[len(r[0]) for r in res]}")
            return add
    raise AssertionError(f"no <eos> bias increment gave joint results that end at two different lengths: {seen}")


@pytest.mark.parametrize("dtype,win", [("fp32", -1), ("bf16", -1), ("fp32", 4), ("bf16", 4)])
def test_joint_batched_search_equals_the_host_loop(dtype, win):
    m = _transformer(ModelConfig(compute_dtype=dtype, ctc_weight=0.3, **NO_DROP), win)
    xs = _images(800)
    mems = [m.encode(x) for x in xs]
    assert [x.shape[1] for x in mems] == [128, 250, 400, 450]
    _search_biases(m, mems)
    differs = 0
    for beam in (2, 4, 8):
        want = [m.beam_search(x, beam, ctc_decode=LAM) for x in mems]
        got = m.beam_search_batch(mems, beam, ctc_decode=LAM)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g[0] == w[0], (beam, i)
            assert g[1] == w[1], (beam, i, g[1], w[1])
        assert m.predict(xs, beam=beam, ctc_decode=LAM, batch_size=16) == [w[0] for w in want], beam
        plain = [m.beam_search(x, beam) for x in mems]
        differs += sum(p != w for p, w in zip(plain, want))
        print(f"beam {beam}: joint lengths {[len(w[0]) for w in want]}, plain lengths {[len(p[0]) for p in plain]}, "
              f"joint scores {[round(w[1], 3) for w in want]}")
    assert differs > 0, "the CTC score changed no result: the comparison says nothing about it"
    assert m.beam_search_batch(list(reversed(mems)), 4, ctc_decode=LAM) == [m.beam_search(x, 4, ctc_decode=LAM) for x in reversed(mems)]


# ------------------------------------------------------------------------------------------------------------ planted case
class _Search:
    """One input's search driven entry by entry: omr_beam_select / omr_beam_select_ctc + omr_ctc_prefix_advance on the SAME attention logits
    at every position."""

    def __init__(self, att, beam, eos, sos, max_len, ctc=None):
        self.att, self.V, self.beam, self.max_len, self.ctc = att, att.shape[1], beam, max_len, ctc
        self.block = BeamSearchBlock(1, beam, sos, eos, max_len, DEV)

    def run(self):
        b = self.block
        for t in range(self.max_len):
            if self.ctc is None:
                lib().call("omr_beam_select", ptr(self.att), self.att.stride(0), self.V, ctypes.byref(b.bdesc), t, cur_stream())
            else:
                lib().call("omr_beam_select_ctc", ptr(self.att), self.att.stride(0), self.V, ctypes.byref(b.bdesc), self.ctc.byref(), t, cur_stream())
            torch.cuda.synchronize()
            s = b.snapshot()
            if s["done"][0]:
                return b.results(t + 1, None if self.ctc is None else self.ctc.advanced().cpu().tolist())[0]
            if self.ctc is not None:
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
                self.ctc.advance(t & 1, up(s["parents"]), up(s["tokens"]), scores=up(s["scores"]), done=up(s["done"]))
        return b.results(self.max_len)[0]


def test_planted_case_the_ctc_score_carries_the_search_past_a_premature_eos():
    """The attention logits put <eos> on top at every position; the CTC frames spell 5 6 7 with margins of 30.  The plain search ends at once
    with <eos>; the joint search returns 5 6 7 <eos>.  Without omr_beam_select_ctc this test cannot run."""
    V, beam, blank, sos, eos, max_len = 12, 4, 0, 2, 1, 8
    att = torch.zeros((beam, V), device=DEV)
    att[:, eos] = 5.0
    att[:, 5:8] = 4.0
    frames = [5, 5, blank, 6, blank, 7, 7]
    ctc_logits = torch.zeros((1, len(frames), 16), device=DEV)
    for f, v in enumerate(frames):
        ctc_logits[0, f, v] = 30.0
    plain = _Search(att, beam, eos, sos, max_len).run()
    assert plain[0] == [eos]
    blk = K.CtcPrefixBlock(ctc_logits[:, :, :V], torch.tensor([len(frames)], dtype=torch.int32, device=DEV), V, beam, blank, sos, eos, LAM)
    joint = _Search(att, beam, eos, sos, max_len, ctc=blk).run()
    assert joint[0] == [5, 6, 7, eos], joint
    # its score: four positions of the mix, the CTC deltas all within 1e-9 of 0 (margins of 30 over 12 columns)
    lp = torch.log_softmax(att[0].double(), 0)
    wa, wc = K.ctc_mix_weights(LAM)
    want = wa * float(lp[5] + lp[6] + lp[7] + lp[eos])
    assert abs(joint[1] - want) < 1e-5


def test_planted_dead_end_returns_the_last_hypothesis_that_lived():
    """Two frames spell 5 6; the attention never offers <eos>.  At position 2 every candidate is a third label in two frames: all at -inf,
    nothing finished.  The result is row 0 of position 1, 5 6, with the score it had."""
    V, beam, blank, sos, eos, max_len = 12, 2, 0, 2, 1, 8
    att = torch.zeros((beam, V), device=DEV)
    att[:, 5], att[:, 6], att[:, eos] = 4.0, 3.9, -20.0
    ctc_logits = torch.zeros((1, 2, 16), device=DEV)
    ctc_logits[0, 0, 5] = ctc_logits[0, 1, 6] = 30.0
    blk = K.CtcPrefixBlock(ctc_logits[:, :, :V], torch.tensor([2], dtype=torch.int32, device=DEV), V, beam, blank, sos, eos, LAM)
    seq, score = _Search(att, beam, eos, sos, max_len, ctc=blk).run()
    assert seq == [5, 6] and blk.advanced().cpu().tolist() == [2]
    lp = torch.log_softmax(att[0].double(), 0)
    assert abs(score - K.ctc_mix_weights(LAM)[0] * float(lp[5] + lp[6])) < 1e-5


# ------------------------------------------------------------------------------------------------------------ the unchanged default
def test_without_the_keyword_no_new_entry_is_called():
    m = _transformer(ModelConfig(ctc_weight=0.3, **NO_DROP))
    xs = _images(900)
    new = ("omr_ctc_beam_workspace_bytes", "omr_ctc_prefix_init", "omr_ctc_prefix_scores", "omr_ctc_prefix_advance", "omr_beam_select_ctc",
           "omr_beam_decode_steps_ctc")
    out = {}
    called = spec_refs.record_entries(lambda: out.setdefault("plain", m.predict(xs, beam=4)))
    assert called and not [n for n in called if n in new or "ctc" in n]
    assert out["plain"] == [m.beam_search(m._encode_input(x), 4)[0] for x in xs]
    called = spec_refs.record_entries(lambda: out.setdefault("joint", m.predict(xs, beam=4, ctc_decode=LAM)))
    assert {"omr_ctc_frames_fwd", "omr_ctc_beam_workspace_bytes", "omr_ctc_prefix_init", "omr_beam_decode_steps_ctc"} <= set(called)
    assert "omr_beam_decode_steps" not in called
    called = spec_refs.record_entries(lambda: m.beam_search(m._encode_input(xs[0]), 4, ctc_decode=LAM))
    assert {"omr_ctc_prefix_init", "omr_ctc_prefix_scores", "omr_ctc_prefix_advance"} <= set(called)
    # a model without the head attaches nothing to its memories
    m0 = _transformer(ModelConfig(**NO_DROP))
    assert not hasattr(m0.encode(xs[0]), "ctc_grid") and hasattr(m.encode(xs[0]), "ctc_grid")
