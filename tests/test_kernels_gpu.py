"""Per-kernel parity: each C-ABI entry point (through the ctypes binding) vs torch CPU fp32 / the oracle.
fp32 runs are held to ~1e-4 (exact-f32 MFMA chain, different summation order); bf16 runs to bf16 rounding."""
import math

import numpy as np

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16]


def dev():
    return torch.device("cuda:0")


def K():
    from omr_a2s_multimodal_transformer_amd import kernels
    return kernels


def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def q(t, dtype):
    """Quantise a CPU fp32 tensor to the test dtype and back (the reference sees what the kernel sees)."""
    return t.to(dtype).float()


def tol(dtype, scale=1.0):
    return dict(rtol=2e-4, atol=2e-4 * scale) if dtype == torch.float32 else dict(rtol=3e-2, atol=3e-2 * scale)


def check(got, ref, dtype, scale=1.0, what=""):
    got = got.detach().float().cpu()
    ref = ref.detach().float()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    torch.testing.assert_close(got, ref, **tol(dtype, scale), msg=lambda m: f"{what}: {m}")


# ------------------------------------------------------------------------------------------------ GEMM

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K_", [(200, 100, 72), (128, 128, 32), (257, 300, 264), (64, 6997, 256)])
def test_gemm_nt_bias_relu(dtype, M, N, K_):
    a, b, bias = q(rnd((M, K_), 1), dtype), q(rnd((N, K_), 2), dtype), rnd((N,), 3)
    ref = F.relu(a @ b.t() + bias)
    out = K().gemm(a.to(dev(), dtype), b.to(dev(), dtype), bias=bias.to(dev()), relu=True)
    check(out, ref, dtype, scale=math.sqrt(K_) / 4, what="gemm NT")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_trans_b(dtype):
    M, N, K_ = 150, 96, 200
    a, b = q(rnd((M, K_), 4), dtype), q(rnd((K_, N), 5), dtype)
    out = K().gemm(a.to(dev(), dtype), b.to(dev(), dtype), trans_b=True)
    check(out, a @ b, dtype, scale=4, what="gemm transB")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", [1, 4])
def test_gemm_tn_accumulate(dtype, split):
    Mred, N, K_ = 700, 72, 136  # dW[N,K] = dY[Mred,N]^T X[Mred,K]
    dy, x = q(rnd((Mred, N), 6), dtype), q(rnd((Mred, K_), 7), dtype)
    init = rnd((N, K_), 8)
    out = init.to(dev()).clone()
    db = torch.ones(N, device=dev())
    K().gemm(dy.to(dev(), dtype), x.to(dev(), dtype), trans_a=True, trans_b=True, out=out, accumulate=True, split_k=split, colsum_a=db)
    check(out, init + dy.t() @ x, dtype, scale=8, what="gemm TN")
    check(db, 1.0 + dy.sum(0), dtype, scale=8, what="gemm TN fused column sums")


def test_gemm_rejects_unaligned():
    a = torch.zeros((8, 30), device=dev())
    with pytest.raises(RuntimeError):
        K().gemm(a, a)


# ------------------------------------------------------------------------------------------------ elementwise

@pytest.mark.parametrize("dtype", DTYPES)
def test_add_relu_bwd(dtype):
    a, b = q(rnd((3, 1001), 9), dtype), q(rnd((3, 1001), 10), dtype)
    check(K().add(a.to(dev(), dtype), b.to(dev(), dtype)), a + b, dtype, what="add")
    check(K().relu_bwd(a.to(dev(), dtype), b.to(dev(), dtype), 2.0), a * (b > 0) * 2.0, dtype, what="relu_bwd")


@pytest.mark.parametrize("dtype", DTYPES)
def test_embed_pe_fwd_bwd(dtype):
    V, d, B, T = 50, 64, 3, 7
    table = q(rnd((V, d), 11), dtype)
    table[0] = 0
    pe = R.pe1d_table(12, d)[0]
    g = torch.Generator().manual_seed(1)
    tok = torch.randint(0, V, (B, T), generator=g)
    tok[1, 4:] = 0
    out = K().embed_pe(tok.to(dev()), table.to(dev(), dtype), pe.to(dev()))
    check(out, table[tok] + pe[:T], dtype, what="embed+pe")
    dout = q(rnd((B, T, d), 12), dtype)
    dtab = torch.zeros((V, d), device=dev())
    K().embed_bwd(tok.to(dev()), dout.to(dev(), dtype), dtab, 0)
    ref = torch.zeros(V, d)
    ref.index_add_(0, tok.flatten(), dout.reshape(-1, d))
    ref[0] = 0
    check(dtab, ref, torch.float32, what="embed bwd")


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_pe2d(dtype):
    pe = R.pe2d_table(64, 5, 9)  # [1,C,h,w]
    x = q(rnd((2, 3, 7, 64), 13), dtype)  # NHWC
    out = K().add_pe2d(x.to(dev(), dtype), pe[0].permute(1, 2, 0).contiguous().to(dev()))
    ref = x + pe[0, :, :3, :7].permute(1, 2, 0)
    check(out, ref, dtype, what="pe2d")
    with pytest.raises(AssertionError):
        K().add_pe2d(torch.zeros((1, 6, 7, 64), device=dev()), pe[0].permute(1, 2, 0).contiguous().to(dev()))


def test_colsum_adam_argmax():
    x = rnd((1000, 70), 14)
    db = torch.zeros(70, device=dev())
    K().colsum_into(x.to(dev()), db)
    check(db, x.sum(0), torch.float32, scale=10, what="colsum")
    p, g = rnd((5000,), 15), rnd((5000,), 16)
    pr, m, v = p.clone(), torch.zeros(5000), torch.zeros(5000)
    pg, mg, vg = p.to(dev()), torch.zeros(5000, device=dev()), torch.zeros(5000, device=dev())
    lp = torch.empty(5000, dtype=torch.bfloat16, device=dev())
    for step in (1, 2, 3):
        R.adam_step([pr], [g], [m], [v], step, lr=1e-3)
        K().adam_step(pg, g.to(dev()), mg, vg, step, 1e-3, p_lowp=lp)
    torch.testing.assert_close(pg.cpu(), pr, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(lp.float().cpu(), pr.bfloat16().float(), rtol=1e-2, atol=1e-3)
    z = rnd((6997,), 17)
    z[4000] = z[123] = 5.0
    idx, val = K().argmax(z.to(dev()))
    assert int(idx) == 123 and float(val) == 5.0


def test_dropout_statistics():
    x = torch.ones((4, 16, 32, 8), device=dev())
    y = K().dropout(x, 0.5, seed=7)
    keep = (y > 0).float().mean().item()
    assert abs(keep - 0.5) < 0.02 and torch.allclose(y[y > 0], torch.tensor(2.0, device=dev()))
    y2 = K().dropout(x, 0.25, seed=9, channel_mode=True)
    per = (y2 > 0).float().mean(dim=(1, 2))  # [B, C]: whole channels kept or dropped
    assert set(per.flatten().tolist()) <= {0.0, 1.0}
    assert torch.equal(K().dropout(x, 0.5, seed=7), y)


# ------------------------------------------------------------------------------------------------ norms

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [16, 128, 256])
def test_instnorm_stats_and_bwd(dtype, C):
    B, H, W = 2, 9, 37
    x = q(F.relu(rnd((B, H, W, C), 18) + 0.3), dtype)  # NHWC
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = R.instance_norm(xn)
    mean, rstd = K().instnorm_stats(x.to(dev(), dtype))
    check(mean, xn.detach().mean((2, 3)), torch.float32, what="in mean")
    check(rstd, 1 / torch.sqrt(xn.detach().var((2, 3), unbiased=False) + 1e-3), torch.float32, scale=5, what="in rstd")
    g = q(rnd((B, H, W, C), 19), dtype)
    y.backward(g.permute(0, 3, 1, 2))
    dx = K().instnorm_bwd(g.to(dev(), dtype), x.to(dev(), dtype), mean, rstd, relu_mask=False)
    check(dx, xn.grad.permute(0, 2, 3, 1), dtype, scale=3, what="in bwd")
    dxm = K().instnorm_bwd(g.to(dev(), dtype), x.to(dev(), dtype), mean, rstd, relu_mask=True, relu_scale=2.0)
    check(dxm, (xn.grad * (xn.detach() > 0) * 2.0).permute(0, 2, 3, 1), dtype, scale=6, what="in bwd masked")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [128, 256])
def test_add_layernorm(dtype, d):
    M = 70
    x, res = q(rnd((M, d), 20), dtype), q(rnd((M, d), 21), dtype)
    gamma, beta = rnd((d,), 22) + 1.5, rnd((d,), 23)
    xs = [t.clone().requires_grad_(True) for t in (x, res, gamma, beta)]
    ref = R.layer_norm(xs[0] + xs[1], xs[2], xs[3])
    out, mean, rstd = K().add_layernorm_fwd(x.to(dev(), dtype), res.to(dev(), dtype), gamma.to(dev()), beta.to(dev()))
    check(out, ref, dtype, scale=3, what="ln fwd")
    g = q(rnd((M, d), 24), dtype)
    ref.backward(g)
    dg, db = torch.zeros(d, device=dev()), torch.zeros(d, device=dev())
    ds = K().add_layernorm_bwd(g.to(dev(), dtype), x.to(dev(), dtype), res.to(dev(), dtype), gamma.to(dev()), mean, rstd, dg, db)
    check(ds, xs[0].grad, dtype, scale=4, what="ln ds")
    check(dg, xs[2].grad, dtype, scale=8, what="ln dgamma")
    check(db, xs[3].grad, dtype, scale=8, what="ln dbeta")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_fused_dropout_matches_gemm_then_dropout(dtype):
    """FFN dropout in the GEMM epilogue = omr_dropout applied to the activated output, to the bit."""
    M, N, Kd, p, seed = 200, 320, 96, 0.25, 99
    k = K()
    a = q(rnd((M, Kd), 90, -1, 1), dtype).to(dev(), dtype)
    w = q(rnd((N, Kd), 91, -1, 1), dtype).to(dev(), dtype)
    bias = rnd((N,), 92, -1, 1).to(dev())
    plain = k.gemm(a, w, bias=bias, relu=True)
    fused = k.gemm(a, w, bias=bias, relu=True, drop=(p, seed))
    assert torch.equal(fused, k.dropout(plain, p, seed))


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_layernorm_fused_dropout_matches_dropout_then_add_ln(dtype):
    """The sublayer dropout fused into the add+LayerNorm kernels uses omr_dropout's mask: both routes agree exactly."""
    M, d, p, seed = 70, 256, 0.3, 1234
    k = K()
    x, res = q(rnd((M, d), 25), dtype).to(dev(), dtype), q(rnd((M, d), 26), dtype).to(dev(), dtype)
    gamma, beta = (rnd((d,), 27) + 1.5).to(dev()), rnd((d,), 28).to(dev())
    xd = k.dropout(x, p, seed)
    ref, mean0, rstd0 = k.add_layernorm_fwd(xd, res, gamma, beta)
    out, mean, rstd = k.add_layernorm_fwd(x, res, gamma, beta, drop_p=p, drop_seed=seed)
    assert torch.equal(out, ref) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
    g = q(rnd((M, d), 29), dtype).to(dev(), dtype)
    dg0, db0 = torch.zeros(d, device=dev()), torch.zeros(d, device=dev())
    ds0 = k.add_layernorm_bwd(g, xd, res, gamma, mean0, rstd0, dg0, db0)
    dg, db = torch.zeros(d, device=dev()), torch.zeros(d, device=dev())
    ds, dx = k.add_layernorm_bwd(g, x, res, gamma, mean, rstd, dg, db, drop_p=p, drop_seed=seed)
    assert torch.equal(ds, ds0)
    assert torch.equal(dx, k.dropout(ds0, p, seed))
    torch.testing.assert_close(dg, dg0, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(db, db0, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ convolutions

def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


CONV_CASES = [  # CIN, COUT, stride, H, W
    (1, 16, (1, 1), 13, 45), (16, 16, (1, 1), 11, 37), (16, 32, (1, 1), 9, 33), (32, 32, (2, 2), 13, 41), (64, 64, (2, 2), 12, 70),
    (64, 128, (1, 1), 7, 35), (128, 128, (2, 1), 9, 34), (128, 128, (2, 2), 8, 36),
    (32, 32, (1, 1), 17, 70), (32, 64, (1, 1), 9, 40), (64, 32, (1, 1), 10, 33), (128, 128, (1, 1), 19, 65),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout,stride,H,W", CONV_CASES)
def test_conv3x3_fwd_bwd(dtype, cin, cout, stride, H, W):
    B = 2
    x = q(rnd((B, cin, H, W), 30), dtype).requires_grad_(True)
    w = q(rnd((cout, cin, 3, 3), 31) / math.sqrt(cin * 9) * 2, dtype).requires_grad_(True)
    bias = rnd((cout,), 32).requires_grad_(True)
    y = F.relu(F.conv2d(x, w, bias, stride=stride, padding=1))
    k = K()
    xg = nhwc(x.detach()).to(dev(), dtype)
    wg = w.detach().permute(0, 2, 3, 1).contiguous().to(dev(), dtype)
    yg = k.conv3x3(xg, wg, bias.detach().to(dev()), stride=stride, relu=True)
    check(yg, nhwc(y), dtype, what="conv fwd")
    # backward: g = dL/d(pre-activation) (the ReLU mask is applied by the caller protocol)
    g = q(rnd(tuple(y.shape), 33), dtype)
    pre = F.conv2d(x, w, bias, stride=stride, padding=1)
    pre.backward(g)
    gg = nhwc(g).to(dev(), dtype)
    dw, db = torch.zeros((cout, 3, 3, cin), device=dev()), torch.zeros(cout, device=dev())
    k.conv3x3_wgrad(xg, gg, dw, stride=stride, db=db)
    check(dw, w.grad.permute(0, 2, 3, 1), dtype, scale=math.sqrt(B * H * W) / 2, what="conv wgrad")
    check(db, bias.grad, dtype, scale=math.sqrt(B * H * W) / 2, what="conv bias grad")
    if cin > 1:
        wd = k.conv3x3_weight_flip(wg)
        dx = k.conv3x3(gg, wd, None, stride=(1, 1), dil=stride, out_hw=(H, W))
        check(dx, nhwc(x.grad), dtype, scale=2, what="conv dgrad")
        dxm = k.conv3x3(gg, wd, None, stride=(1, 1), dil=stride, out_hw=(H, W), out_mask=xg, mask_scale=2.0)
        check(dxm, nhwc(x.grad * (x.detach() > 0) * 2.0), dtype, scale=4, what="conv dgrad masked")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,stride,H,W", [(32, (2, 2), 10, 40), (64, (2, 2), 12, 70), (128, (2, 1), 9, 34), (16, (1, 1), 19, 45), (128, (2, 2), 7, 33)])
def test_conv3x3_fused_instnorm(dtype, C, stride, H, W):
    B = 2
    x = q(F.relu(rnd((B, C, H, W), 34)), dtype).requires_grad_(True)
    w = q(rnd((C, C, 3, 3), 35) / 12, dtype).requires_grad_(True)
    xh = R.instance_norm(x)
    xh.retain_grad()
    pre = F.conv2d(xh, w, None, stride=stride, padding=1)
    k = K()
    xg = nhwc(x.detach()).to(dev(), dtype)
    wg = w.detach().permute(0, 2, 3, 1).contiguous().to(dev(), dtype)
    stats = k.instnorm_stats(xg)
    yg = k.conv3x3(xg, wg, None, stride=stride, in_stats=stats)
    check(yg, nhwc(pre), dtype, scale=2, what="norm+conv fwd")
    g = q(rnd(tuple(pre.shape), 36), dtype)
    pre.backward(g)
    dw = torch.zeros((C, 3, 3, C), device=dev())
    k.conv3x3_wgrad(xg, nhwc(g).to(dev(), dtype), dw, stride=stride, in_stats=stats)
    check(dw, w.grad.permute(0, 2, 3, 1), dtype, scale=8, what="norm+conv wgrad")
    dxh = k.conv3x3(nhwc(g).to(dev(), dtype), k.conv3x3_weight_flip(wg), None, dil=stride, out_hw=(H, W))
    check(dxh, nhwc(xh.grad), dtype, scale=2, what="norm+conv dgrad")
    dx = k.instnorm_bwd(dxh, xg, stats[0], stats[1], relu_mask=False)
    check(dx, nhwc(x.grad), dtype, scale=8, what="norm bwd chain")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [128, 256])
def test_dwconv3x3(dtype, C):
    B, H, W = 2, 6, 19
    x = q(rnd((B, C, H, W), 37), dtype).requires_grad_(True)
    w = q(rnd((C, 1, 3, 3), 38) / 3, dtype).requires_grad_(True)
    bias = rnd((C,), 39).requires_grad_(True)
    y = F.conv2d(x, w, bias, padding=1, groups=C)
    k = K()
    xg, wg = nhwc(x.detach()).to(dev(), dtype), w.detach().reshape(C, 9).to(dev(), dtype)
    check(k.dwconv3x3(xg, wg, bias.detach().to(dev())), nhwc(y), dtype, what="dw fwd")
    g = q(rnd((B, C, H, W), 40), dtype)
    y.backward(g)
    gg = nhwc(g).to(dev(), dtype)
    check(k.dwconv3x3(gg, wg, None, flip=True), nhwc(x.grad), dtype, what="dw dgrad")
    dw, db = torch.zeros((C, 9), device=dev()), torch.zeros(C, device=dev())
    k.dwconv3x3_wgrad(xg, gg, dw, db)
    check(dw, w.grad.reshape(C, 9), dtype, scale=6, what="dw wgrad")
    check(db, bias.grad, dtype, scale=6, what="dw bgrad")
    # fused InstanceNorm on the input
    x2 = q(F.relu(rnd((B, C, H, W), 41)), dtype)
    stats = k.instnorm_stats(nhwc(x2).to(dev(), dtype))
    ref = F.conv2d(R.instance_norm(x2), w.detach(), bias.detach(), padding=1, groups=C)
    check(k.dwconv3x3(nhwc(x2).to(dev(), dtype), wg, bias.detach().to(dev()), in_stats=stats), nhwc(ref), dtype, scale=2, what="dw norm fwd")


# Which depthwise kernel a shape reaches (dispatch rules of omr_dwconv3x3 / omr_dwconv3x3_wgrad, csrc/dwconv.hip).  With
# cv = C / (8 for bf16, 4 for fp32) 16-byte channel groups, tc = 256 / cv tile columns and a halo tile of 10 x (tc + 2) x C elements:
#   forward / data gradient
#     dwconv3x3_tile_kernel         tc >= 2, H >= 4, tile <= 64 KB, w 16-byte aligned: all four cases of test_dwconv3x3
#     dwconv3x3_walk_kernel         H >= 4 otherwise: DW_PATH_CASES[0] (tile too large) and [1] (w not aligned) below
#     dwconv3x3_kernel              H < 4: DW_PATH_CASES[2] below
#   weight gradient
#     dwconv3x3_wgrad_tile_kernel   NLD = 12 (10 (tc + 2) cv <= 3072): bf16 C = 128 in test_dwconv3x3
#                                   NLD = 16: bf16 C = 256 in test_dwconv3x3
#                                   "wide" fold (cv >= 64): fp32 C = 256 in test_dwconv3x3
#     dwconv3x3_wgrad_kernel        cv not in {16, 32, 64..256} or H < 4: bf16 C = 64 in test_fuzz_depthwise_walkers, DW_PATH_CASES[2] below
#     unsupported                   no tile and cv > 64: DW_PATH_CASES[0] below
DW_PATH_CASES = [  # dtype, C, H, weight offset in bytes, weight gradient supported
    # dwconv3x3_walk_kernel: the tile is 10 x 4 x 512 x 4 B = 80 KB > 64 KB; weight gradient: cv = 128 fits neither the tile nor a wave -> unsupported
    (torch.float32, 512, 6, 0, False),
    # dwconv3x3_walk_kernel: the weight starts 8 bytes into its buffer, the tile kernel reads taps as aligned 16-byte fragments;
    # weight gradient: dwconv3x3_wgrad_tile_kernel<bf16, 12> (it does not read w)
    (torch.bfloat16, 128, 6, 8, True),
    # dwconv3x3_kernel (per pixel): H = 3 < 4; weight gradient: dwconv3x3_wgrad_kernel (row walker, cv = 16)
    (torch.bfloat16, 128, 3, 0, True),
]


@pytest.mark.parametrize("dtype,C,H,w_off,has_wgrad", DW_PATH_CASES)
def test_dwconv3x3_every_kernel(dtype, C, H, w_off, has_wgrad):
    """The depthwise kernels test_dwconv3x3's shapes do not reach, against F.conv2d with test_dwconv3x3's tolerances; each with the
    fused InstanceNorm on the input and the producer's mask on the output.  mask_scale = 2 doubles the data gradient, hence scale=2."""
    B, W = 2, 19
    x = q(rnd((B, C, H, W), 37), dtype).requires_grad_(True)
    w = q(rnd((C, 1, 3, 3), 38) / 3, dtype).requires_grad_(True)
    bias = rnd((C,), 39).requires_grad_(True)
    y = F.conv2d(x, w, bias, padding=1, groups=C)
    k = K()
    xg = nhwc(x.detach()).to(dev(), dtype)
    off = w_off // xg.element_size()
    wbuf = torch.zeros(C * 9 + off, device=dev(), dtype=dtype)
    wg = wbuf[off:].view(C, 9)                                  # a view `w_off` bytes into a larger buffer
    wg.copy_(w.detach().reshape(C, 9))
    assert wbuf.data_ptr() % 16 == 0 and wg.data_ptr() % 16 == w_off and wg.is_contiguous()
    check(k.dwconv3x3(xg, wg, bias.detach().to(dev())), nhwc(y), dtype, what="dw fwd")
    g = q(rnd((B, C, H, W), 40), dtype)
    y.backward(g)
    gg = nhwc(g).to(dev(), dtype)
    check(k.dwconv3x3(gg, wg, None, flip=True), nhwc(x.grad), dtype, what="dw dgrad")
    m = q(F.relu(rnd((B, C, H, W), 42)), dtype)                 # the producer's ReLU output: about half of it is 0
    check(k.dwconv3x3(gg, wg, None, flip=True, out_mask=nhwc(m).to(dev(), dtype), mask_scale=2.0), nhwc(x.grad * (m > 0) * 2.0), dtype, scale=2,
          what="dw masked dgrad")
    # fused InstanceNorm on the input
    x2 = q(F.relu(rnd((B, C, H, W), 41)), dtype).requires_grad_(True)
    x2g = nhwc(x2.detach()).to(dev(), dtype)
    stats = k.instnorm_stats(x2g)
    w2 = w.detach().clone().requires_grad_(True)
    b2 = bias.detach().clone().requires_grad_(True)
    ref = F.conv2d(R.instance_norm(x2), w2, b2, padding=1, groups=C)
    check(k.dwconv3x3(x2g, wg, bias.detach().to(dev()), in_stats=stats), nhwc(ref), dtype, scale=2, what="dw norm fwd")
    dw, db = torch.zeros((C, 9), device=dev()), torch.zeros(C, device=dev())
    if not has_wgrad:
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            k.dwconv3x3_wgrad(xg, gg, dw, db)
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            k.dwconv3x3_wgrad(x2g, gg, dw, db, in_stats=stats)
        return
    k.dwconv3x3_wgrad(xg, gg, dw, db)
    check(dw, w.grad.reshape(C, 9), dtype, scale=6, what="dw wgrad")
    check(db, bias.grad, dtype, scale=6, what="dw bgrad")
    ref.backward(g)
    dw.zero_(), db.zero_()
    k.dwconv3x3_wgrad(x2g, gg, dw, db, in_stats=stats)
    # the kernel rounds the normalised input to the compute dtype and unit-variance values are sqrt(3) x the uniform ones above:
    # twice the plain bound, the factor test_fuzz_depthwise_walkers uses for its normalised cases
    check(dw, w2.grad.reshape(C, 9), dtype, scale=12, what="dw norm wgrad")
    check(db, b2.grad, dtype, scale=6, what="dw norm bgrad")


# ------------------------------------------------------------------------------------------------ attention

def ref_attention(qh, kh, vh, nhead, bias):
    """[B,T,d] x [B,S,d]: softmax(QK^T/sqrt(hd) + bias[B,H,T,S]) V, heads = contiguous channel slices."""
    B, T, d = qh.shape
    S = kh.shape[1]
    hd = d // nhead
    qq = qh.view(B, T, nhead, hd).transpose(1, 2)
    kk = kh.view(B, S, nhead, hd).transpose(1, 2)
    vv = vh.view(B, S, nhead, hd).transpose(1, 2)
    s = qq @ kk.transpose(-1, -2) / math.sqrt(hd)
    if bias is not None:
        s = s + bias
    return (torch.softmax(s, -1) @ vv).transpose(1, 2).reshape(B, T, d)


ATTN_CASES = [  # name, T, S, d, nhead, causal, window, key_bias kind, blk
    ("self_causal_pad", 70, 70, 256, 4, True, -1, "plus1", False),
    ("self_window", 150, 150, 256, 4, True, 20, None, False),
    ("self_window_ge_T", 33, 33, 128, 4, True, 100, "plus1", False),
    ("cross_bool", 40, 200, 256, 4, False, -1, "neginf", False),
    ("cross_plus1", 129, 77, 128, 4, False, -1, "plus1", False),
    ("cross_blk_quirk", 50, 90, 256, 4, False, -1, None, True),
    ("decode_one_query", 1, 700, 256, 4, False, -1, "plus1", False),      # T <= 32: the forward splits the keys over the waves
    ("decode_few_queries", 20, 333, 128, 4, False, -1, "neginf", False),
    ("decode_blk_quirk", 8, 130, 256, 4, False, -1, None, True),
    # T > 32 and S >= 1024: forward and dQ split the keys over workgroups (2 x 768).  Rows 1 and 2 have 733 and 366 valid keys, so
    # their whole second split is -inf: the weight-0 path of the merge
    ("cross_key_split", 40, 1100, 256, 4, False, -1, "neginf", False),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,T,S,d,nhead,causal,window,kb,blk", ATTN_CASES)
def test_attention_fwd_bwd(dtype, name, T, S, d, nhead, causal, window, kb, blk):
    B = 3
    packed = T == S and causal
    qv, kv, vv = (q(rnd((B, n, d), 50 + i), dtype).requires_grad_(True) for i, n in enumerate((T, S, S)))
    bias = torch.zeros(B, nhead, T, S)
    key_bias = None
    lens = torch.tensor([S, (2 * S) // 3, S // 3])
    if kb is not None:
        key_bias = torch.zeros(B, S)
        for i, l in enumerate(lens.tolist()):
            key_bias[i, l:] = 1.0 if kb == "plus1" else float("-inf")
        bias = bias + key_bias.view(B, 1, 1, S)
    if causal:
        bias = bias + R.tgt_attn_mask(T, window).view(1, 1, T, T)
    lq = lkv = None
    if blk:
        lq = torch.tensor([T, T // 2, T // 4], dtype=torch.int32)
        lkv = torch.tensor([S, S // 2, S // 5], dtype=torch.int32)
        m = torch.zeros(B, T, S)
        for i in range(B):
            m[i, int(lq[i]):, int(lkv[i]):] = float("-inf")
        bias = bias + m[torch.arange(B * nhead) % B].view(B, nhead, T, S)
    ref = ref_attention(qv, kv, vv, nhead, bias)
    g = q(rnd((B, T, d), 60), dtype)
    ref.backward(g)
    k = K()
    if name == "cross_key_split":  # the case must keep covering the key split
        from omr_a2s_multimodal_transformer_amd._lib import lib
        assert lib().query("omr_attn_workspace_floats", B, nhead, T, S, d // nhead, 0, 0) > 0
    if packed:  # q|k|v packed [B,T,3d] views, as the decoder's self-attention uses them
        qkv = torch.cat([qv, kv, vv], dim=-1).detach().to(dev(), dtype)
        qg, kg, vg = qkv[:, :, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = dqkv[:, :, :d], dqkv[:, :, d:2 * d], dqkv[:, :, 2 * d:]
    else:
        qg, kg, vg = (t.detach().to(dev(), dtype) for t in (qv, kv, vv))
        dq, dk, dv = torch.empty_like(qg), torch.empty_like(kg), torch.empty_like(vg)
    kw = dict(causal=causal, window=window, key_bias=None if key_bias is None else key_bias.to(dev()),
              blk_lq=None if lq is None else lq.to(dev()), blk_lkv=None if lkv is None else lkv.to(dev()))
    o, lse = k.attn_fwd(qg, kg, vg, nhead, **kw)
    check(o, ref, dtype, what=f"attn fwd {name}")
    k.attn_bwd(qg, kg, vg, o, g.to(dev(), dtype), lse, dq, dk, dv, nhead, **kw)
    check(dq, qv.grad, dtype, what=f"attn dq {name}")
    check(dk, kv.grad, dtype, what=f"attn dk {name}")
    check(dv, vv.grad, dtype, what=f"attn dv {name}")


def test_attention_dropout_consistency():
    """Forward and backward regenerate the same mask: check dV against a reference built from the
    kernel's own dropped probabilities (recovered with V = identity)."""
    B, T, S, d, nhead = 1, 64, 64, 64, 1
    k = K()
    qg = rnd((B, T, d), 70).to(dev())
    kg = rnd((B, S, d), 71).to(dev())
    eye = torch.eye(S, d, device=dev()).view(1, S, d).contiguous()
    pd, lse = k.attn_fwd(qg, kg, eye, nhead, dropout_p=0.3, seed=5)  # = dropped, rescaled probabilities
    p_full, _ = k.attn_fwd(qg, kg, eye, nhead)
    kept = pd > 0
    assert abs(kept.float().mean().item() - 0.7) < 0.05
    torch.testing.assert_close(pd[kept], (p_full / 0.7)[kept], rtol=1e-4, atol=1e-6)
    vg = rnd((B, S, d), 72).to(dev())
    o, lse = k.attn_fwd(qg, kg, vg, nhead, dropout_p=0.3, seed=5)
    torch.testing.assert_close(o, pd @ vg, rtol=1e-3, atol=1e-4)
    g = rnd((B, T, d), 73).to(dev())
    dq, dk, dv = torch.empty_like(qg), torch.empty_like(kg), torch.empty_like(vg)
    k.attn_bwd(qg, kg, vg, o, g, lse, dq, dk, dv, nhead, dropout_p=0.3, seed=5)
    torch.testing.assert_close(dv[0], pd[0].t() @ g[0], rtol=1e-3, atol=1e-4)
    # dQ / dK of both backward kernels against autograd through softmax -> (recovered mask) -> 1/(1-p) -> @ V
    qa, ka = qg.cpu().clone().requires_grad_(True), kg.cpu().clone().requires_grad_(True)
    mask = kept.cpu().float() / 0.7
    (((torch.softmax(qa @ ka.transpose(1, 2) / math.sqrt(d), dim=-1) * mask) @ vg.cpu()) * g.cpu()).sum().backward()
    torch.testing.assert_close(dq.cpu(), qa.grad, rtol=2e-3, atol=2e-4)
    torch.testing.assert_close(dk.cpu(), ka.grad, rtol=2e-3, atol=2e-4)


# ------------------------------------------------------------------------------------------------ loss

@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_entropy(dtype):
    M, V = 37, 6997
    Vp = K().round_up(V, 8)
    logits = q(rnd((M, V), 80, -4, 4), dtype).requires_grad_(True)
    g = torch.Generator().manual_seed(2)
    tgt = torch.randint(1, V, (M,), generator=g)
    tgt[5:9] = 0
    ref = F.cross_entropy(logits, tgt, ignore_index=0)
    ref.backward()
    buf = torch.zeros((M, Vp), dtype=dtype, device=dev())
    buf[:, :V] = logits.detach().to(dev(), dtype)
    loss, lse, acc2 = K().ce_fwd(buf[:, :V], tgt.to(dev()), V, 0)
    torch.testing.assert_close(loss.cpu()[0], ref.detach(), rtol=1e-4 if dtype == torch.float32 else 1e-2, atol=1e-4)
    dl = K().ce_bwd(buf[:, :V], tgt.to(dev()), lse, acc2, V, 0)
    check(dl, logits.grad, dtype, scale=0.01, what="ce bwd")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("channel_mode", [False, True])
def test_conv3x3_fused_dropout_and_instnorm_reductions(dtype, channel_mode):
    """The conv epilogue's fused MixDropout uses the same counter-based mask as omr_dropout, and its fused
    per-(image, channel) reductions equal the stand-alone InstanceNorm statistics / backward kernels."""
    B, C, H, W = 3, 32, 21, 45          # several tiles per image, ragged edges
    k = K()
    x = q(rnd((B, H, W, C), 90), dtype).to(dev(), dtype)
    w = q(rnd((C, 3, 3, C), 91) / 12, dtype).to(dev(), dtype)
    bias = rnd((C,), 92).to(dev())
    y_plain = k.conv3x3(x, w, bias, relu=True)
    ws, slots = k.conv_stat_ws(B, H, W, C, dev())
    y = k.conv3x3(x, w, bias, relu=True, drop=(0.5, 77, channel_mode), stat_mode=1, stat_ws=ws, stat_slots=slots)
    ref = k.dropout(y_plain, 0.5, 77, channel_mode)
    torch.testing.assert_close(y.float(), ref.float(), **tol(dtype))
    mean, rstd = k.instnorm_finalize(ws, slots, B, C, H * W)
    mean_ref, rstd_ref = k.instnorm_stats(y)
    torch.testing.assert_close(mean, mean_ref, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(rstd, rstd_ref, rtol=1e-4, atol=1e-4)
    # mode 2: backward sums fused into the data-gradient conv == stand-alone reduction + apply
    g = q(rnd((B, H, W, C), 93), dtype).to(dev(), dtype)
    wd = k.conv3x3_weight_flip(w)
    dxh_ref = k.conv3x3(g, wd, None, out_hw=(H, W))
    dx_ref = k.instnorm_bwd(dxh_ref, y, mean, rstd, relu_mask=True, relu_scale=2.0)
    ws2, slots2 = k.conv_stat_ws(B, H, W, C, dev())
    dxh = k.conv3x3(g, wd, None, out_hw=(H, W), stat_mode=2, stat_ws=ws2, stat_slots=slots2, stat_x=y, stat_stats=(mean, rstd))
    assert torch.equal(dxh, dxh_ref)
    dx = k.instnorm_bwd_apply(dxh, y, mean, rstd, ws2, slots2, relu_mask=True, relu_scale=2.0)
    torch.testing.assert_close(dx.float(), dx_ref.float(), **tol(dtype, 2))
    # the statistics are a fixed-order reduction (no atomics): repeated launches agree to the bit, also with fewer slots
    # than the launch would like to use (the grid is clamped to the slot count)
    for s_use in (slots, 2):
        runs = []
        for _ in range(3):
            wsr = torch.full_like(ws, float("nan"))        # the launch writes every slot it is given (unused ones as zeros)
            k.conv3x3(x, w, bias, relu=True, drop=(0.5, 77, channel_mode), stat_mode=1, stat_ws=wsr, stat_slots=s_use)
            runs.append(k.instnorm_finalize(wsr, s_use, B, C, H * W))
        assert all(torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1]) for r in runs[1:])
        torch.testing.assert_close(runs[0][0], mean_ref, rtol=1e-4, atol=1e-5)
    a1, a2 = k.instnorm_stats(y), k.instnorm_stats(y)
    assert torch.equal(a1[0], a2[0]) and torch.equal(a1[1], a2[1])
    d1 = k.instnorm_bwd(dxh_ref, y, mean, rstd, relu_mask=True, relu_scale=2.0)
    assert torch.equal(d1, dx_ref)


# ------------------------------------------------------------------------------------------------ audio front end

@pytest.mark.parametrize("n", [22050 * 3 + 137, 5000])
def test_log_stft_matches_oracle(n):
    """GPU log-STFT (one fp32 GEMM + dB kernels) vs the numpy restatement of the reference's librosa pipeline
    (preprocessing.py:17-30).  librosa is absent in this image: parity with librosa itself is unpinned (see oracle)."""
    from omr_a2s_multimodal_transformer_amd import audio
    t = torch.arange(n, dtype=torch.float64) / 22050
    g = torch.Generator().manual_seed(3)
    y = (0.6 * torch.sin(2 * math.pi * 440 * t) + 0.3 * torch.sin(2 * math.pi * 1318.5 * t * (1 + 0.01 * t)) + 0.02 * torch.randn(n, generator=g, dtype=torch.float64)).float()
    ref = R.log_stft(y.numpy())
    out = audio.log_stft(y.to(dev()))
    assert tuple(out.shape) == (1, 195, 1 + n // 512) and ref.shape == tuple(out.shape[1:])
    got = out[0].cpu().numpy()
    assert got.min() >= 0.0 and got.max() == pytest.approx(1.0, abs=1e-6)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-3)


def test_resample_poly_matches_scipy_golden(golden):
    """GPU polyphase resampler (one fp32 GEMM over strided frames x filter phases) vs scipy.signal.resample_poly outputs
    (fixture F18 = librosa.resample(res_type="polyphase"), preprocessing.py:19; the reference's default "soxr_hq" backend is
    absent here: against the reference's own samples this step is parity unpinned) -- and the resampled signal through the
    spectrogram front end keeps its shape contract."""
    from omr_a2s_multimodal_transformer_amd import audio
    g = golden("f18_resample")
    for k in range(6):
        o, t, n = (int(v) for v in g[f"c{k}_meta"])
        x = torch.from_numpy(g[f"c{k}_x"]).to(dev())
        y = audio.resample_poly(x, o, t)
        ref = g[f"c{k}_y"]
        assert tuple(y.shape) == ref.shape == (-(-n * (t // math.gcd(o, t)) // (o // math.gcd(o, t))),)
        np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=0, atol=5e-6)
    spec = audio.log_stft(audio.resample_poly(torch.from_numpy(g["c1_x"]).to(dev()), 48000))
    assert tuple(spec.shape) == (1, 195, 1 + g["c1_y"].shape[0] // 512)
