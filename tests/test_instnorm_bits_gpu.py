"""The InstanceNorm slot protocol (csrc/instnorm_slots.h) pinned to the bit: every case of tools/record_instnorm_bits.py -- the dense
entries, the extent entries, the two fused conv backwards that reduce into the slots -- hashes to what the commit before the protocol
was written once (76405df) computed (tests/golden/instnorm_bits.json, recorded with a checkout of that commit), and the dense and the
extent statistics, which share one stage 1 and one stage 2, agree to the bit on a batch whose extents are the whole plane."""
import functools
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _recorder():
    spec = importlib.util.spec_from_file_location("record_instnorm_bits", os.path.join(ROOT, "tools", "record_instnorm_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


with open(os.path.join(ROOT, "tests", "golden", "instnorm_bits.json")) as _fh:
    GOLDEN = json.load(_fh)


@functools.lru_cache(maxsize=None)
def hashes():
    """All cases, computed once."""
    from omr_a2s_multimodal_transformer_amd import kernels
    return _recorder().compute(kernels)


def test_the_recorder_covers_exactly_the_golden_cases():
    assert sorted(hashes()) == sorted(GOLDEN)
    assert len(GOLDEN) == 2 * 3 * 6 + 2 * 4 * 3 + 2


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_bits_equal_the_parent(case):
    assert hashes()[case] == GOLDEN[case], f"{case}: the output bytes differ from those of 76405df"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [16, 128])
def test_extent_statistics_of_the_whole_plane_are_the_dense_statistics(dtype, C):
    """Real-valued input (the order of the sums matters), 37 x 50 (1 / n is not exact, the last block has a partial slab): mean and rstd
    of omr_instnorm_extent_fwd with every extent equal to the plane are bit-equal to omr_instnorm_stats.  (Not so the backward: the
    dense apply multiplies by 1 / HW rounded to float, the extent apply by 1 / n in double -- instnorm_slots.h.)"""
    from omr_a2s_multimodal_transformer_amd import kernels as K
    B, H, W = 3, 37, 50
    x = (torch.randn((B, H, W, C), generator=torch.Generator().manual_seed(900 + C)) * 1.7 + 0.4).to(dtype).to(DEV)
    ext = torch.tensor([[H, W]] * B, dtype=torch.int32, device=DEV)
    mean, rstd = K.instnorm_stats(x)
    _, emean, erstd = K.instnorm_extent_fwd(x, ext)
    assert torch.equal(mean.view(torch.int32), emean.view(torch.int32)), "mean"
    assert torch.equal(rstd.view(torch.int32), erstd.view(torch.int32)), "rstd"
