"""CPU-only: every `*_grammar` entry of include/omr_hip.h is declared with the descriptor in its prototype and refuses a bad
omr_grammar_desc (NULL, NULL tables or state, C outside 1..256, S < 1) with OMR_ERR_ARG before it looks at anything else --
nothing is launched, so no GPU is needed.  The struct mirror has the C layout's size."""
import ctypes

import pytest

from omr_a2s_multimodal_transformer_amd import _lib
from omr_a2s_multimodal_transformer_amd.decoder import _BeamDesc, _DecodeDesc
from omr_a2s_multimodal_transformer_amd.grammar import MAX_CLASSES, _GrammarDesc

ARG = -1
P = 4096            # a non-NULL pointer value that is never dereferenced: the descriptor is refused first
ENTRIES = ("omr_grammar_pick", "omr_weighted_grammar_pick", "omr_beam_select_grammar", "omr_weighted_beam_select_grammar",
           "omr_decode_steps_grammar", "omr_decode_steps_varlen_grammar", "omr_decode_steps_rows_grammar",
           "omr_weighted_decode_steps_varlen_grammar", "omr_weighted_decode_steps_rows_grammar", "omr_beam_decode_steps_grammar",
           "omr_weighted_beam_decode_steps_grammar")


def _row_kernel_desc():
    d = _DecodeDesc()
    d.dtype, d.B, d.L, d.d, d.nhead, d.ff, d.V, d.ldv, d.max_len, d.S = 1, 2, 1, 256, 4, 256, 30, 32, 16, 128      # widths the row kernel takes
    return d


def _args(entry, g):
    a, b, bd = ctypes.byref(_row_kernel_desc()), ctypes.byref(_row_kernel_desc()), ctypes.byref(_BeamDesc())
    return {
        "omr_grammar_pick": (P, 32, 2, 30, g, P, None, None, None),
        "omr_weighted_grammar_pick": (P, 32, P, 32, 2, 30, 0.5, g, P, None, None, None),
        "omr_beam_select_grammar": (P, 32, 30, bd, g, 0, None),
        "omr_weighted_beam_select_grammar": (P, 32, P, 32, 30, 0.5, bd, g, 0, None),
        "omr_decode_steps_grammar": (a, g, P, 0, 1, P, None, None, None),
        "omr_decode_steps_varlen_grammar": (a, P, g, P, 0, 1, P, None, None, None),
        "omr_decode_steps_rows_grammar": (a, None, P, 0, g, P, 1, P, None, None, None),
        "omr_weighted_decode_steps_varlen_grammar": (a, None, b, None, g, 0.5, P, 0, 1, P, None, P, P, None),
        "omr_weighted_decode_steps_rows_grammar": (a, None, b, None, P, 0, g, 0.5, P, 1, P, None, P, P, None),
        "omr_beam_decode_steps_grammar": (a, bd, None, g, 0, 1, None),
        "omr_weighted_beam_decode_steps_grammar": (a, None, b, None, bd, P, g, 0.5, 0, 1, None),
    }[entry]


def _desc(**change):
    d = _GrammarDesc()
    d.cls, d.next, d.state, d.S, d.C = P, P, P, 3, 7
    for k, v in change.items():
        setattr(d, k, v)
    return d


def test_every_grammar_entry_is_declared_with_its_descriptor():
    protos = _lib.parse_header()
    for entry in ENTRIES:
        ret, types = protos[entry]
        assert ret == "int" and types.count("const omr_grammar_desc* grammar") == 1 and types[-1] == "void* stream", entry
        assert len(types) == len(_args(entry, None)), entry
    assert {n for n in protos if n.endswith("_grammar") or "grammar_pick" in n} == set(ENTRIES)
    assert ctypes.sizeof(_GrammarDesc) == 3 * 8 + 2 * 4 and _lib.header_constant("OMR_GRAMMAR_MAX_CLASSES") == MAX_CLASSES == 256
    # the existing entries and descriptors are as they were
    assert len(protos["omr_decode_steps"][1]) == 8 and len(protos["omr_beam_select"][1]) == 6 and ctypes.sizeof(_BeamDesc) == 4 * 4 + 14 * 8


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_descriptors_are_refused_before_anything_else(entry):
    q = _lib.lib().query
    assert q(entry, *_args(entry, None)) == ARG
    for change in (dict(cls=None), dict(next=None), dict(state=None), dict(C=0), dict(C=257), dict(C=-1), dict(S=0)):
        assert q(entry, *_args(entry, ctypes.byref(_desc(**change)))) == ARG, change
