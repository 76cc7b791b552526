"""The GEMM family (csrc/gemm.hip, gemm_panel.hip, gemm_tall.hip) pinned to the bit: every case of tools/record_gemm_bits.py -- the
generic kernel's product, epilogue, fused-dropout and one-split column-sum cases, the non-split row-group cases, the real-valued
panel and tall cases and the fp8 calls -- hashes to what the commit before the family's shared steps were written once (d747dd0)
computed (tests/golden/gemm_bits.json, recorded with a checkout of that commit, twice, in two processes, with equal results).  No
atomic reaches a pinned output; the split-K and grouped weight-gradient routes stay under tests/test_gemm_branches_gpu.py."""
import functools
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_gemm_bits", os.path.join(ROOT, "tools", "record_gemm_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


with open(os.path.join(ROOT, "tests", "golden", "gemm_bits.json")) as _fh:
    GOLDEN = json.load(_fh)


@functools.lru_cache(maxsize=None)
def hashes():
    """All cases, computed once."""
    from omr_a2s_multimodal_transformer_amd import kernels
    return _recorder().compute(kernels)


def test_the_recorder_covers_exactly_the_golden_cases():
    """40 calls of the generic kernel (24 products, 9 epilogues, 4 one-split column sums, 3 fused dropouts), 6 row-group calls, P4, T4
    and 8 fp8 calls."""
    from oracle import decode_refs as DR
    from oracle import kernel_refs as KR
    rec = _recorder()
    assert len(rec.tile_cases()) == 24 + 9 + 4 + 3 and len(rec.ref_cases()) == 6 + 2
    assert sorted(hashes()["cases"]) == sorted(GOLDEN["cases"]) == sorted(GOLDEN["inputs"])
    assert len(GOLDEN["cases"]) == 40 + 8 + len(KR.DTYPES) * len(DR.FP8_CASES) == 56


@pytest.mark.parametrize("case", sorted(GOLDEN["cases"]))
def test_bits_equal_the_parent(case):
    assert hashes()["inputs"][case] == GOLDEN["inputs"][case], f"{case}: the INPUTS differ from those the golden was recorded with"
    assert hashes()["cases"][case] == GOLDEN["cases"][case], f"{case}: the output bytes differ from those of d747dd0"
