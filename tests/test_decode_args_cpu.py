"""CPU-only: the native decode executor's entries, put to calls they must refuse, without a GPU.

One table for the eight decode / fusion / beam entries plus omr_decode_workspace_bytes, omr_beam_workspace_bytes, omr_beam_select and
omr_weighted_beam_select.  Every device pointer INSIDE a descriptor stays NULL, so the furthest any case can get is the
NULL-pointer refusal of the descriptor check -- never a launch -- and the file is safe to run on a machine with a GPU too.  The
pointers passed beside the descriptors (tokens, outputs, logits) are never dereferenced by a refused call; they point into a
host buffer.

What the table can and cannot show follows from that rule.  The fault-free case (`null_device_pointers`, a beam descriptor
without a state block) is itself refused with OMR_ERR_ARG = -1, so a row that expects -1 shows that the named fault is met
without a crash (no NULL descriptor dereferenced, no division by a zero width, no launch) and with no OTHER code -- it does
not show that the check it names exists: deleting that check would leave the row passing.  The same holds for the selection and
workspace tables below.  What the table does pin is the precedence of OMR_ERR_UNSUPPORTED = -3: only the two
per-row-position entries answer it, for every descriptor the row kernel does not take, and before they look at any pointer
(Decoder.takes_slot_state asks that way).  The codes are those of the executor before its host half was restructured."""
import ctypes
import types

import pytest

from omr_a2s_multimodal_transformer_amd import _lib
from omr_a2s_multimodal_transformer_amd.decoder import _BeamDesc, _DecodeDesc

ARG, UNSUPPORTED = -1, -3
_HOST = ctypes.create_string_buffer(4096)
P = ctypes.addressof(_HOST)                      # a non-NULL stand-in for the pointers beside the descriptors

GREEDY = ("omr_decode_steps", "omr_decode_steps_varlen", "omr_decode_steps_rows")
WEIGHTED = ("omr_weighted_decode_steps", "omr_weighted_decode_steps_varlen", "omr_weighted_decode_steps_rows")
BEAM = ("omr_beam_decode_steps", "omr_weighted_beam_decode_steps")
PAIR = WEIGHTED + BEAM[1:]
ENTRIES = GREEDY + WEIGHTED + BEAM


def desc(**kw):
    """Widths of a model the row kernel takes; every pointer NULL."""
    d = _DecodeDesc()
    vals = dict(dtype=_lib.BF16, B=6, L=2, d=128, nhead=4, ff=256, V=100, ldv=104, max_len=64, S=100, window=-1, fp8=0, cross_ld=512,
                cross_bs=51200)
    vals.update(kw)
    for k, v in vals.items():
        setattr(d, k, v)
    return d


def beam_desc(**kw):
    b = _BeamDesc()
    vals = dict(beam=3, N=2, eos=2, max_len=64)
    vals.update(kw)
    for k, v in vals.items():
        setattr(b, k, v)
    return b


def case(**kw):
    """A call no check but the NULL pointers in the descriptors stops: B = 6 rows = 2 inputs x beam 3, 4 positions from 0."""
    c = types.SimpleNamespace(a=desc(), b=desc(), bd=beam_desc(), t0=0, n=4, out=True, pos=True, null=())
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def call(entry, c):
    ref = lambda name: None if name in c.null else ctypes.byref(getattr(c, name))
    a, b, bd, out, pos = ref("a"), ref("b"), ref("bd"), (P if c.out else None), (P if c.pos else None)
    if entry == "omr_weighted_decode_steps":      # the B = 1 wrapper: one row where the case has its usual six
        for d in (c.a, c.b):
            d.B = 1 if d.B == 6 else d.B
    args = {
        "omr_decode_steps": (a, P, c.t0, c.n, out, None, None, None),
        "omr_decode_steps_varlen": (a, P, P, c.t0, c.n, out, None, None, None),
        "omr_decode_steps_rows": (a, None, pos, c.t0, P, c.n, out, None, None, None),
        "omr_weighted_decode_steps": (a, b, 0.5, P, c.t0, c.n, out, None, P, P, None),
        "omr_weighted_decode_steps_varlen": (a, None, b, None, 0.5, P, c.t0, c.n, out, None, P, P, None),
        "omr_weighted_decode_steps_rows": (a, None, b, None, pos, c.t0, 0.5, P, c.n, out, None, P, P, None),
        "omr_beam_decode_steps": (a, bd, None, c.t0, c.n, None),
        "omr_weighted_beam_decode_steps": (a, None, b, None, bd, None, 0.5, c.t0, c.n, None),
    }[entry]
    return _lib.lib().query(entry, *args)


def _set(which, **kw):
    def change(c):
        for k, v in kw.items():
            setattr(getattr(c, which), k, v)
    return change


def _call_field(**kw):
    def change(c):
        for k, v in kw.items():
            setattr(c, k, v)
    return change


# fault -> (what it changes in the fault-free case, the entries it is put to, the code)
FAULTS = {
    "null_device_pointers": (lambda c: None, ENTRIES, ARG),
    "null_descriptor": (_call_field(null=("a",)), ENTRIES, ARG),
    "null_descriptor_b": (_call_field(null=("b",)), PAIR, ARG),
    "null_beam_descriptor": (_call_field(null=("bd",)), BEAM, ARG),
    "n_steps_0": (_call_field(n=0), ENTRIES, ARG),
    "t0_negative": (_call_field(t0=-1), ENTRIES, ARG),
    "d_not_a_multiple_of_nhead": (_set("a", nhead=3), ENTRIES, ARG),
    "d_not_a_multiple_of_nhead_b": (_set("b", nhead=3), PAIR, ARG),
    "ldv_below_V": (_set("a", ldv=96), ENTRIES, ARG),
    "ldv_not_a_multiple_of_8": (_set("a", ldv=100), ENTRIES, ARG),
    "steps_beyond_max_len": (_call_field(t0=61), ENTRIES, ARG),
    "steps_beyond_max_len_of_a": (_set("a", max_len=3), PAIR, ARG),
    "steps_beyond_max_len_of_b": (_set("b", max_len=3), PAIR, ARG),
    "several_steps_without_out_tokens": (_call_field(out=False), GREEDY + WEIGHTED, ARG),
    "B_differs_between_the_models": (_set("b", B=4), PAIR, ARG),
    "V_differs_between_the_models": (_set("b", V=99), PAIR, ARG),
    "beam_0": (_set("bd", beam=0), BEAM, ARG),
    "beam_9": (_set("bd", beam=9), BEAM, ARG),
    "B_is_not_N_times_beam": (_set("bd", N=3), BEAM, ARG),
    "beam_max_len_differs": (_set("bd", max_len=32), BEAM[:1], ARG),
    "steps_beyond_beam_max_len": (_set("bd", max_len=3), BEAM, ARG),
    "eos_negative": (_set("bd", eos=-1), BEAM, ARG),
    "eos_beyond_V": (_set("bd", eos=100), BEAM, ARG),
    "beam_beyond_V": (_set("a", V=2, ldv=8), BEAM, ARG),
    # per-row positions: whether the descriptor takes the entry is answered before any pointer is looked at
    "width_96": (_set("a", d=96), ("omr_decode_steps_rows", "omr_weighted_decode_steps_rows"), UNSUPPORTED),
    "width_96_b": (_set("b", d=96), ("omr_weighted_decode_steps_rows",), UNSUPPORTED),
    "width_96_and_every_pointer_null": (lambda c: (_set("a", d=96)(c), _call_field(pos=False, out=False)(c)),
                                        ("omr_decode_steps_rows", "omr_weighted_decode_steps_rows"), UNSUPPORTED),
    "ff_beyond_the_row_kernel": (_set("a", ff=2304), ("omr_decode_steps_rows", "omr_weighted_decode_steps_rows"), UNSUPPORTED),
    "width_256_null_pos": (lambda c: (_set("a", d=256)(c), _set("b", d=256)(c), _call_field(pos=False)(c)),
                           ("omr_decode_steps_rows", "omr_weighted_decode_steps_rows"), ARG),
    "null_descriptor_before_the_width": (lambda c: (_set("b", d=96)(c), _call_field(null=("a",))(c)), ("omr_weighted_decode_steps_rows",), ARG),
}
TABLE = [(entry, fault) for fault, (_, entries, _) in FAULTS.items() for entry in entries]


@pytest.mark.parametrize("entry,fault", TABLE, ids=[f"{e}-{f}" for e, f in TABLE])
def test_refused_call(entry, fault):
    change, _, code = FAULTS[fault]
    c = case()
    change(c)
    assert call(entry, c) == code


def test_the_b1_wrapper_refuses_other_batch_sizes():
    assert call("omr_weighted_decode_steps", case(a=desc(B=2), b=desc(B=2))) == ARG
    assert call("omr_weighted_decode_steps", case(a=desc(B=1), b=desc(B=2))) == ARG


def test_varlen_wants_mem_len():
    assert _lib.lib().query("omr_decode_steps_varlen", ctypes.byref(desc()), None, P, 0, 1, P, None, None, None) == ARG


WORKSPACE = [("null", None, ARG), ("B_0", dict(B=0), ARG), ("d_0", dict(d=0), ARG), ("ff_0", dict(ff=0), ARG), ("ldv_below_V", dict(ldv=96), ARG)]


@pytest.mark.parametrize("name,kw,code", WORKSPACE, ids=[w[0] for w in WORKSPACE])
def test_decode_workspace_bytes_refusals(name, kw, code):
    assert _lib.lib().query("omr_decode_workspace_bytes", None if kw is None else ctypes.byref(desc(**kw))) == code


def test_beam_workspace_bytes_refusals_and_offsets():
    q = _lib.lib().query
    assert q("omr_beam_workspace_bytes", None) == ARG
    for kw in (dict(beam=0), dict(beam=9), dict(N=0), dict(max_len=0)):
        assert q("omr_beam_workspace_bytes", ctypes.byref(beam_desc(**kw))) == ARG
    bd = beam_desc()                              # state NULL: the ten fields become offsets, each 256-byte aligned, in order
    nbytes = q("omr_beam_workspace_bytes", ctypes.byref(bd))
    offs = [int(getattr(bd, n) or 0) for n in _BeamDesc.STATE_FIELDS]
    assert offs == sorted(offs) and offs[0] == 0 and all(o % 256 == 0 for o in offs) and offs[-1] < nbytes
    assert nbytes >= 6 * 8 * 2 + 2 * 8 + 2 * 4 * 4 + 6 * 4 + 2 * 64 * 6 * 4


SELECT = [  # name, beam descriptor changes, V, ld, t
    ("state_null", {}, 100, 104, 0),
    ("beam_0", dict(beam=0), 100, 104, 0),
    ("beam_9", dict(beam=9), 100, 104, 0),
    ("N_0", dict(N=0), 100, 104, 0),
    ("eos_negative", dict(eos=-1), 100, 104, 0),
    ("eos_beyond_V", dict(eos=100), 100, 104, 0),
    ("V_below_beam", {}, 2, 104, 0),
    ("ld_below_V", {}, 100, 96, 0),
    ("t_negative", {}, 100, 104, -1),
    ("t_beyond_max_len", {}, 100, 104, 64),
]


@pytest.mark.parametrize("name,kw,V,ld,t", SELECT, ids=[s[0] for s in SELECT])
def test_beam_select_refusals(name, kw, V, ld, t):
    q = _lib.lib().query
    bd = beam_desc(**kw)                          # state stays NULL: refused there at the latest
    assert q("omr_beam_select", P, ld, V, ctypes.byref(bd), t, None) == ARG
    assert q("omr_weighted_beam_select", P, ld, P, ld, V, 0.5, ctypes.byref(bd), t, None) == ARG
    assert q("omr_beam_select", None, ld, V, ctypes.byref(bd), t, None) == ARG
    assert q("omr_weighted_beam_select", P, ld, None, ld, V, 0.5, ctypes.byref(bd), t, None) == ARG
    assert q("omr_beam_select", P, ld, V, None, t, None) == ARG
    assert q("omr_weighted_beam_select", P, ld, P, ld, V, 0.5, None, t, None) == ARG
