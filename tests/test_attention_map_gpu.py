"""The attention map kernel (csrc/attention_map.hip, omr_attn_weights) through ctypes against the fp64 reference and the derived
bound of tests/attention_map_refs.py ("Attention maps").  Every case runs in fp32 and bf16; `lse` comes from the
forward entry on the same operands (omr_attn_fwd_ws; omr_attn_fwd_split_varlen for the kv_len case, the forward entry that takes
per-row key counts); operands are views into NaN-filled buffers (K rows past a row's kv_len are NaN), every output buffer is
NaN-filled with a pitch wider than S and its tail columns must stay NaN.  Each test prints its largest error / bound ratio
before it asserts <= 1."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_map_refs as M  # noqa: E402
from omr_a2s_multimodal_transformer_amd import kernels as K  # noqa: E402
from omr_a2s_multimodal_transformer_amd._lib import cur_stream, dtype_code, lib, ptr  # noqa: E402
from oracle import attention_refs as R  # noqa: E402
from oracle.kernel_refs import TAG  # noqa: E402

DEV = "cuda:0"
TAIL = 7          # columns of every map buffer past S: pitches S + 7 are 12, 72, 136 (16-byte rows: vector stores) and 71, 107, 157, 307 (not)


def _strides(*ts):
    assert all(t.stride(2) == 1 for t in ts)
    return tuple(t.stride(1) for t in ts) + tuple(t.stride(0) for t in ts)


class MapRun:
    """Device side of one (case, dtype): the operands, the forward's lse, NaN-filled map buffers."""

    def __init__(self, case, dtype):
        self.case, self.dtype = case, dtype
        inp = self.inp = R.attn_inputs(case, dtype)
        B, H, T, S, d, slot = case.B, case.H, case.T, case.S, case.d, inp["slot"]
        bufs = {n: t.to(DEV) for n, t in inp["bufs"].items()}
        if case.causal:
            g = bufs["qkv"]
            self.q, self.k, self.v = g[:, :T, :d], g[:, :T, d:2 * d], g[:, :T, 2 * d:]
        else:
            self.q, self.k, self.v = bufs["q"][:, :T, :d], bufs["k"][:, :slot, :d], bufs["v"][:, :slot, :d]
        self.bias = None if inp["bias"] is None else inp["bias"].to(DEV)
        self.blk = (None, None) if case.blk is None else tuple(torch.tensor(x, dtype=torch.int32, device=DEV) for x in case.blk)
        self.kv_len = None if case.kv_len is None else torch.tensor(case.kv_len, dtype=torch.int32, device=DEV)
        self.p, self.seed = case.drop or (0.0, 0)
        self.words = None
        if case.drop:       # the words the kernels read and the byte mask of the same (p, seed); the reference uses the latter
            self.words = K.attn_dropout_words(B, H, T, S, self.p, self.seed, DEV)
            mask = K.attn_dropout_mask(B, H, T, S, self.p, self.seed, DEV)
            assert torch.equal(mask.cpu().bool(), inp["keep"]), "omr_attn_dropout_mask differs from the hash restated in oracle/attention_refs.py"
        self.o = torch.empty((B, T, d), dtype=dtype, device=DEV)
        self.lse = torch.empty((B, H, T), dtype=torch.float32, device=DEV)
        self.forward()

    def forward(self, q=None):
        """lse (and O) of the forward entry for these operands."""
        c, q = self.case, self.q if q is None else q
        args = (dtype_code(self.dtype), ptr(q), ptr(self.k), ptr(self.v), ptr(self.o), ptr(self.lse), *_strides(q, self.k, self.v, self.o),
                c.B, c.H, c.T, c.S, c.hd)
        if c.entry == "varlen":
            n = lib().query("omr_attn_split_workspace_floats", c.B, c.H, c.T, c.S, c.hd)
            ws = torch.empty(max(n, 1), dtype=torch.float32, device=DEV)
            lib().call("omr_attn_fwd_split_varlen", *args, ptr(self.bias), ptr(self.kv_len), ptr(ws), n, cur_stream())
        else:
            n = lib().query("omr_attn_workspace_floats", c.B, c.H, c.T, c.S, c.hd, int(c.causal), 0)
            ws = torch.empty(max(n, 1), dtype=torch.float32, device=DEV)
            lib().call("omr_attn_fwd_ws", *args, int(c.causal), c.window, ptr(self.bias), ptr(self.blk[0]), ptr(self.blk[1]), float(self.p), self.seed,
                       ptr(self.words), ptr(ws) if n else None, n, cur_stream())
        torch.cuda.synchronize()

    def buffer(self):
        c = self.case
        return torch.full((c.B, c.T + 1, c.S + TAIL), float("nan"), dtype=torch.float32, device=DEV)

    def weights(self, buf, q=None, out_scale=None, accumulate=0, code=None, hd=None, words="own", ldq=None):
        """The raw entry on the [B, T, S] view of `buf`; returns its status."""
        c, q = self.case, self.q if q is None else q
        w = buf[:, :c.T, :c.S]
        rc = lib().query("omr_attn_weights", dtype_code(self.dtype) if code is None else code, ptr(q), ptr(self.k), ptr(self.lse), ptr(w),
                         q.stride(1) if ldq is None else ldq, self.k.stride(1), w.stride(1), q.stride(0), self.k.stride(0), w.stride(0), c.B, c.H,
                         c.T, c.S, c.hd if hd is None else hd, int(c.causal), c.window, ptr(self.bias), ptr(self.blk[0]), ptr(self.blk[1]),
                         ptr(self.kv_len), float(self.p), ptr(self.words if words == "own" else words),
                         float(1.0 / c.H if out_scale is None else out_scale), accumulate, cur_stream())
        torch.cuda.synchronize()
        return rc

    def view(self, buf):
        return buf[:, :self.case.T, :self.case.S].cpu()

    def outside_is_nan(self, buf) -> bool:
        rest = buf.clone()
        rest[:, :self.case.T, :self.case.S] = float("nan")
        return bool(torch.isnan(rest).all())


def _planned_range(case) -> int:
    return lib().query("omr_attn_weights_range", case.B, case.T, case.S)


def _check_case(case, dtype, tag=""):
    """One case through the entry, twice: inside the bound, nothing outside the view written, the two runs bit-equal."""
    run = MapRun(case, dtype)
    buf, again = run.buffer(), run.buffer()
    assert run.weights(buf) == 0 and run.weights(again) == 0
    ref, bound = M.map_case_ref(case, dtype)
    got = run.view(buf)
    M.map_check(f"{tag}{case.name}-{TAG[dtype]}", got, ref, bound)
    assert run.outside_is_nan(buf), f"{case.name}: columns S .. ldw - 1 or the row past T were written"
    assert torch.equal(buf.view(torch.int32), again.view(torch.int32)), f"{case.name}: two runs differ"
    if not case.drop:                        # a distribution per row, except the rows without a visible key: exactly 0
        sums = got.double().sum(dim=-1)
        dead = ref.sum(dim=-1) == 0
        assert bool((got[dead] == 0).all()) and float((sums[~dead] - 1.0).abs().max()) <= float(bound.sum(dim=-1).max())
    return buf


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.case_id)
@pytest.mark.parametrize("case", M.MAP_CASES, ids=R.case_id)
def test_attention_map(case, dtype):
    assert _planned_range(case) == M.expected_range(case.B, case.T, case.S) == 64      # tiny batches: one tile per workgroup
    _check_case(case, dtype)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.case_id)
@pytest.mark.parametrize("case", M.RANGE_CASES, ids=R.case_id)
def test_attention_map_default_plan_with_two_tiles_per_workgroup(case, dtype):
    """Batches large enough that the launcher's own plan hands a workgroup two 64-key tiles: the step from one tile to the next
    (`it / H`, the reset of the head sum, the reuse of the wave's LDS patch), zero-filled beside computed tiles in one range, and
    the kv_len / -inf tail / causal band / window edges that fall inside a range."""
    assert _planned_range(case) == M.expected_range(case.B, case.T, case.S) == 128 < case.S
    _check_case(case, dtype)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.case_id)
@pytest.mark.parametrize("case,ranges", [(c, r) for c in M.MAP_CASES for r in (1, 2) if ((c.S + 63) // 64 + r - 1) // r > 1],
                         ids=lambda v: R.case_id(v) if isinstance(v, R.AttnCase) else f"{v}range")
def test_attention_map_long_ranges_give_the_same_bits(case, ranges, dtype, monkeypatch):
    """Every case of more than one tile again with the plan asked for `ranges` key ranges per query block (OMR_ATTN_MAP_MIN_WG):
    one workgroup walks all S keys, or half of them -- 2 to 5 tiles in a row, the masks' edges inside.  Inside the bound, and
    bit-equal to the default plan's result: one owner per element, the same head order, whatever the ranges."""
    base = _check_case(case, dtype)
    blocks = case.B * ((case.T + 127) // 128)
    monkeypatch.setenv("OMR_ATTN_MAP_MIN_WG", str(ranges * blocks))
    ntile = (case.S + 63) // 64
    want = (ntile + ranges - 1) // ranges * 64
    assert _planned_range(case) == M.expected_range(case.B, case.T, case.S, ranges * blocks) == want > 64
    long = _check_case(case, dtype, tag=f"{ranges}-range ")
    assert torch.equal(base.view(torch.int32), long.view(torch.int32)), f"{case.name}: the result depends on the key ranges"


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.case_id)
def test_accumulate_adds_a_second_call(dtype):
    """Two calls with out_scale = 1 / (2 H) on different Q, the second with accumulate = 1: the sum of the two references."""
    case = M.MAP_CASE["map-t33-s65-hd32-plus1"]
    run = MapRun(case, dtype)
    inp = run.inp
    half = 1.0 / (2 * case.H)
    buf = run.buffer()
    assert run.weights(buf, out_scale=half) == 0
    q2_host = inp["q"].flip(1).contiguous()
    q2 = q2_host.to(DEV)
    run.forward(q2)                          # the lse of the second Q
    assert run.weights(buf, q=q2, out_scale=half, accumulate=1) == 0
    r1, b1 = M.weights_ref(inp["q"], inp["k"], case.H, case=case, dtype=dtype, key_bias=inp["bias"], out_scale=half)
    r2, b2 = M.weights_ref(q2_host, inp["k"], case.H, case=case, dtype=dtype, key_bias=inp["bias"], out_scale=half)
    M.map_check(f"accumulate-{TAG[dtype]}", run.view(buf), r1 + r2, b1 + b2)
    assert run.outside_is_nan(buf)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.case_id)
def test_single_head_map_times_v_is_the_forward_output(dtype):
    """H = 1, no dropout: w is P itself, and w @ V (fp64, on the host) is the forward's O within the forward's own bound."""
    case = R.AttnCase("map-h1-t33-s65-hd64", "fwd", 2, 1, 33, 65, 64, family="needles", bias="plus1")
    run = MapRun(case, dtype)
    buf = run.buffer()
    assert run.weights(buf) == 0
    o_ref, o_bound = R.attention_ref(run.inp["q"], run.inp["k"], run.inp["v"], 1, case=case, dtype=dtype, key_bias=run.inp["bias"])["o"]
    wv = run.view(buf).double() @ run.inp["v"].double()
    r_fwd, r_map = R.ratio(run.o.cpu(), o_ref, o_bound), R.ratio(wv, run.o.cpu().double(), o_bound)
    print(f"map-h1-{TAG[dtype]}: forward O against its reference {r_fwd:.4f}, w @ V against the forward's O {r_map:.4f}")
    assert r_fwd <= 1.0 and r_map <= 1.0


def test_refusals_write_nothing():
    case = M.MAP_CASE["map-drop-t33-s65-hd64"]
    run = MapRun(case, torch.float32)
    buf = run.buffer()
    assert run.weights(buf, hd=48) == -3                     # head_dim 48: unsupported
    assert run.weights(buf, code=7) == -3                    # no such dtype
    assert run.weights(buf, words=None) == -1                # dropout_p > 0 without the keep words
    assert run.weights(buf, ldq=run.q.stride(1) + 1) == -1   # rows of q are read as 16-byte fragments
    assert bool(torch.isnan(buf).all())
    with pytest.raises(RuntimeError):                        # the wrapper: GPU tensors only, no CPU fall-back
        K.attn_weights(run.q.cpu(), run.k, run.lse, case.H, dropout_p=run.p, drop_words=run.words)


def test_wrapper_pads_its_own_buffer_and_averages_the_heads():
    case = M.MAP_CASE["map-blk-b3-h4-t40-s100-hd32"]
    run = MapRun(case, torch.bfloat16)
    w = K.attn_weights(run.q, run.k, run.lse, case.H, blk_lq=run.blk[0], blk_lkv=run.blk[1])
    torch.cuda.synchronize()
    assert tuple(w.shape) == (case.B, case.T, case.S) and w.dtype == torch.float32 and w.stride(1) % 4 == 0
    M.map_check("wrapper-blk-bf16", w.cpu(), *M.map_case_ref(case, torch.bfloat16))
