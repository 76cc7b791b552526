"""The loss kernels' shared steps (csrc/loss_rows.h) pinned to the bit: every case of tools/record_loss_bits.py -- the plain, the
label-smoothed and the distillation entries, forward and backward, on the seeded case tables with V <= 2101 -- hashes to what the commit
before the steps were written once (e871648) computed (tests/golden/loss_bits.json, recorded with a checkout of that commit)."""
import functools
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_loss_bits", os.path.join(ROOT, "tools", "record_loss_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


with open(os.path.join(ROOT, "tests", "golden", "loss_bits.json")) as _fh:
    GOLDEN = json.load(_fh)


@functools.lru_cache(maxsize=None)
def hashes():
    """All cases, computed once."""
    from omr_a2s_multimodal_transformer_amd import kernels
    return _recorder().compute(kernels)


def test_the_recorder_covers_exactly_the_golden_cases():
    """plain: 2 + 6 of oracle/kernel_refs and the 6 smoothing inputs; smooth: 8 and the 6 again at eps = 0; distill: 14 and 9 at lam = 0."""
    assert sorted(hashes()) == sorted(GOLDEN)
    assert len(GOLDEN) == (2 + 6) + 6 + 8 + 6 + 14 + 9 == 51


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_bits_equal_the_parent(case):
    assert hashes()[case] == GOLDEN[case], f"{case}: the output bytes differ from those of e871648"
