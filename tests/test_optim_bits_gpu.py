"""The one optimizer kernel (csrc/optim.hip) pinned to the bit: every case of tools/record_optim_bits.py -- omr_adam, omr_adam_guarded and
omr_adamw_ema in all eight combinations, three consecutive steps at nine sizes -- hashes to what the commit that still had three kernels
(79e5dd9) computed (tests/golden/optim_bits.json, recorded with a checkout of that commit)."""
import functools
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_optim_bits", os.path.join(ROOT, "tools", "record_optim_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


with open(os.path.join(ROOT, "tests", "golden", "optim_bits.json")) as _fh:
    GOLDEN = json.load(_fh)


@functools.lru_cache(maxsize=None)
def hashes():
    """All cases, computed once."""
    from omr_a2s_multimodal_transformer_amd import _lib
    return _recorder().compute(_lib)


def test_the_recorder_covers_exactly_the_golden_cases():
    """Per size: omr_adam without / with the bf16 copy, omr_adam_guarded, omr_adamw_ema {plain, decay, ema, decay+ema} x {free, guarded}."""
    import test_optim_recipe_gpu as T
    from oracle import kernel_refs as KR
    assert sorted(_recorder().SIZES) == sorted(T.SIZES + [KR.ADAM_N])
    assert sorted(hashes()["cases"]) == sorted(GOLDEN["cases"])
    assert len(GOLDEN["cases"]) == (2 + 1 + 4 * 2) * 9 == 99


@pytest.mark.parametrize("case", sorted(GOLDEN["cases"]))
def test_bits_equal_the_parent(case):
    size = case.rsplit("/", 1)[1]
    assert hashes()["inputs"][size] == GOLDEN["inputs"][size], f"{size}: the INPUTS differ from those the golden was recorded with"
    assert hashes()["cases"][case] == GOLDEN["cases"][case], f"{case}: the output bytes differ from those of 79e5dd9"
