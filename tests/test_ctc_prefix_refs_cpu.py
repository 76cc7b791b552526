"""CPU-only: the references of tests/ctc_prefix_refs.py against brute-force enumeration of all V^F alignments (V = 3: the blank and two
labels; F <= 5), and the case table's own claims."""
import itertools

import numpy as np
import pytest

import ctc_prefix_refs as R

V = 3
SOS_, EOS_ = -1, -2            # outside the vocabulary: all three columns are emitting symbols


def probs(F, seed):
    rng = np.random.RandomState(seed)
    x = rng.randn(F, V) * 1.5
    y = x - R.lse_rows(x)[:, None]
    return y, np.exp(y)


def hyp_of(y, labels):
    h = R.empty_hyp(y, SOS_)
    for c in labels:
        h, _ = R.extend(y, h, c, SOS_, EOS_)
    return h


def prefixes(max_len):
    for n in range(max_len + 1):
        yield from itertools.product((1, 2), repeat=n)


@pytest.mark.parametrize("F,seed", [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5)])
def test_prefix_scores_against_all_alignments(F, seed):
    y, p = probs(F, seed)
    mass = R.brute_masses(p)
    assert abs(sum(mass.values()) - 1.0) < 1e-12
    starts = lambda h: sum(w for k, w in mass.items() if k[:len(h)] == h)  # noqa: E731
    for g in prefixes(3):
        hg = hyp_of(y, g)
        # psi(g): the mass of the alignments whose collapse starts with g
        assert np.exp(hg.logpsi) == pytest.approx(starts(g), rel=1e-11, abs=1e-15), (g, "psi")
        # the <eos> value: the mass that collapses to exactly g
        _, p_eos = R.extend(y, hg, EOS_, SOS_, EOS_)
        assert np.exp(p_eos) == pytest.approx(mass.get(g, 0.0), rel=1e-11, abs=1e-15), (g, "eos")
        # gn + gb at the last frame is the same mass, split by the last frame's symbol
        last_label = sum(w for path in itertools.product(range(V), repeat=F) if R.collapse(path) == g and path[-1] != R.BLANK
                         for w in [np.prod([p[f, v] for f, v in enumerate(path)])])
        assert np.exp(hg.gn[F - 1]) == pytest.approx(last_label, rel=1e-11, abs=1e-15), (g, "gn")
        # sum_c psi(g c) + P(g) = psi(g)
        total = np.exp(p_eos)
        for c in (1, 2):
            _, psi = R.extend(y, hg, c, SOS_, EOS_)
            assert np.exp(psi) == pytest.approx(starts(g + (c,)), rel=1e-11, abs=1e-15), (g, c)
            total += np.exp(psi)
            assert R.delta_of(psi, hg.logpsi) <= 0.0
        assert total == pytest.approx(np.exp(hg.logpsi), rel=1e-11, abs=1e-15), (g, "sum rule")
        # blank and <sos> extend nothing
        assert R.extend(y, hg, R.BLANK, SOS_, EOS_)[1] == R.NINF and R.extend(y, hg, SOS_, SOS_, EOS_)[1] == R.NINF


def test_no_frames():
    y = np.zeros((0, 5))
    g = R.empty_hyp(y)
    assert R.extend(y, g, R.EOS)[1] == 0.0 and R.extend(y, g, 3)[1] == R.NINF
    h, _ = R.extend(y, g, 3)
    assert R.extend(y, h, R.EOS)[1] == R.NINF and R.delta_of(R.extend(y, h, 4)[1], h.logpsi) == R.NINF


def test_case_table_covers_what_it_says():
    names = {c.name for c in R.CASES}
    for dt in (R.F32, R.BF16):
        assert {f"{dt}-{n}" for n in ("F1", "F2", "chunk-1", "chunk", "chunk+1", "2chunk+1", "ragged", "ragged8")} <= names
    assert {c.beam for c in R.CASES} >= {3, 8} and any(c.V % 8 for c in R.CASES) and any(0 in c.frames for c in R.CASES)
    case = [c for c in R.CASES if c.name == "fp32-ragged"][0]
    ref = R.run_chain(case)
    assert len(ref["positions"]) == 4
    seen = dict(repeat=False, eos=False, blank=False, sos=False, outside=False)
    lasts = [R.SOS] * (case.N * case.beam)
    for pos in ref["positions"]:
        for r, row in enumerate(pos["cand"]):
            for j, c in enumerate(row):
                c = int(c)
                seen["repeat"] |= R.is_label(c, case.V) and c == lasts[r]
                seen["eos"] |= c == R.EOS
                seen["blank"] |= c == R.BLANK
                seen["sos"] |= c == R.SOS
                if not R.is_label(c, case.V) and c != R.EOS:
                    assert pos["delta"][r, j] == R.NINF
        assert all(R.is_label(int(t), case.V) for t in pos["tokens"])
        lasts = pos["last"].tolist()
    assert seen["repeat"] and seen["eos"] and seen["blank"] and seen["sos"]
    # a survivor that repeats its parent's last token (new row 0 from position 1 on)
    assert int(ref["positions"][1]["tokens"][0]) == int(ref["positions"][0]["last"][int(ref["positions"][1]["parents"][0])])
    # the fp32 yardstick errs, and by less than 1e-3 on these sizes
    b, e32 = R.bounds(case, ref)
    assert all(0.0 < e32[k] < 1e-3 for k in R.KINDS), e32
