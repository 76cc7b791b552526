"""Audio front end (audio.log_stft, audio.resample_poly, omr_log_stft_post): case tables, inputs, fp64 references, bounds and the
CPU stand-ins of tests/test_audio_branches_gpu.py and tests/test_audio_refs_cpu.py.  Derivations: DESIGN.md, "Audio front end
coverage".  Every check prints and returns its largest error / bound ratio before it asserts <= 1; no constant is fitted.

The dB stage out = max(L(m) - L(M), -80) / 80 + 1, L(m) = 20 log10(max(amin, m)), M = max m, is monotone in every input, so
magnitude intervals [m_lo, m_hi] give out in [f(m_lo, M_hi), f(m_hi, M_lo)], widened by DELTA for its fp32 evaluation."""
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import ref_cpu

U = 2.0 ** -24
LOG10_ULPS = 3.0                            # OpenCL's figure for log10 (the ROCm device library's own table is not at hand)
AMIN = float(np.float32(1e-5))              # amin as the kernel holds it: 1e-5 rounded to fp32 (2.5e-8 below 1e-5, 2.7e-9 in the output)
TOP_DB = 80.0
N_FFT, HOP, BINS, SR = 2048, 512, 195, 22050
SENTINEL = 1234.5
SWEEP = 2048 * 256                          # threads of the largest element-wise launch (ew_grid): element SWEEP is the first of a second sweep


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the dB stage as intervals
def _L(m):
    return 20.0 * np.log10(np.maximum(AMIN, m))


DbBox = namedtuple("DbBox", "lo hi delta zero all_one")


def db_box(m_lo: np.ndarray, m_hi: np.ndarray) -> DbBox:
    """Output interval of every element from its magnitude interval.  delta: log10f at LOG10_ULPS ulp (<= 2 u LOG10_ULPS |l|) and the
    rounding of x20, for L(m) and for L(M), each relative to |L| <= l_max; the subtraction relative to |d| <= 2 l_max; then the
    roundings of /80 (|x| <= 1) and of +1 (result <= 1).  zero: the whole interval, delta included, at or under the floor, where
    the clamp makes the result -80 / 80 + 1 = 0 exactly.  all_one: every magnitude under amin, so L(m) = L(M) for every element."""
    M_lo, M_hi = float(m_lo.max()), float(m_hi.max())
    l_max = max(100.0, abs(float(_L(M_lo))), abs(float(_L(M_hi))))
    d_db = (2.0 * (2.0 * LOG10_ULPS + 1.0) + 2.0) * U * l_max
    delta = d_db / TOP_DB + 2.0 * U
    d_lo = _L(m_lo) - _L(M_hi)
    d_hi = np.minimum(_L(m_hi) - _L(M_lo), 0.0)                       # no magnitude exceeds the maximum
    lo = np.maximum(d_lo, -TOP_DB) / TOP_DB + 1.0
    hi = np.maximum(d_hi, -TOP_DB) / TOP_DB + 1.0
    return DbBox(lo, hi, delta, d_hi + d_db <= -TOP_DB, M_hi < AMIN)


def db_check(got: np.ndarray, m_lo: np.ndarray, m_hi: np.ndarray, who: str = "") -> float:
    """got, m_lo, m_hi: the same shape.  -> largest |got - centre| / (half width + delta)."""
    assert got.dtype == np.float32 and got.shape == m_lo.shape == m_hi.shape, f"{who}: {got.dtype} {got.shape} vs {m_lo.shape}"
    assert np.isfinite(got).all(), f"{who}: {int((~np.isfinite(got)).sum())} non-finite outputs for finite magnitudes"
    box = db_box(m_lo, m_hi)
    if box.all_one:
        assert (got == 1.0).all(), f"{who}: every magnitude is under amin, {int((got != 1.0).sum())} outputs are not exactly 1.0 (min {got.min()!r})"
        print(f"{who}: all under amin, every output exactly 1.0")
        return 0.0
    assert (got[box.zero] == 0.0).all(), f"{who}: {int((got[box.zero] != 0.0).sum())} of {int(box.zero.sum())} elements under the floor are not exactly 0.0"
    assert got.min() >= 0.0 and got.max() == 1.0, f"{who}: range [{got.min()!r}, {got.max()!r}], the maximum must be exactly 1.0"
    top = int(np.argmax(m_lo))
    rest = np.delete(m_hi.reshape(-1), top)
    if rest.size == 0 or m_lo.reshape(-1)[top] > rest.max():          # the maximum is known: that element is 0 dB
        assert got.reshape(-1)[top] == 1.0, f"{who}: the element holding the maximum is {got.reshape(-1)[top]!r}"
    mid, half = 0.5 * (box.lo + box.hi), 0.5 * (box.hi - box.lo) + box.delta
    r = np.abs(got.astype(np.float64) - mid) / half
    worst = int(np.argmax(r))
    ratio = float(r.reshape(-1)[worst])
    print(f"{who}: dB stage largest |got - centre| / (half width + delta) = {ratio:.4f} at {np.unravel_index(worst, got.shape)}, "
          f"delta = {box.delta:.3e}, {int(box.zero.sum())} of {got.size} exactly 0")
    assert ratio <= 1.0, f"{who}: output {got.reshape(-1)[worst]!r} outside [{box.lo.reshape(-1)[worst]!r}, {box.hi.reshape(-1)[worst]!r}] -+ {box.delta:.3e}"
    return ratio


# ------------------------------------------------------------------------------------------------ omr_log_stft_post alone
PostCase = namedtuple("PostCase", "name frames bins r_lo r_hi peak")
POST_CASES = [
    PostCase("post-wrap", 2690, 195, 1.1e-6, 9e2, 1e3),                # 524 550 elements: 262 in the second sweep of both kernels
    PostCase("post-tiny", 3, 7, 1.1e-6, 9e2, 1e3),                     # less than one block, bins != 195
    PostCase("post-one", 1, 195, 1.1e-6, 9e2, 1e3),
    PostCase("post-silent", 4, 195, 0.0, 0.0, 0.0),
    PostCase("post-under-amin", 4, 195, 1.1e-6, 9e-6, 0.0),
    PostCase("post-quiet", 4, 195, 1.1e-6, 1e-2, 0.0125),              # the floor (1.25e-6) is under amin: amin is what the quiet bins get
]
DIRTY_LOUD = PostCase("post-dirty-ws", 5, 195, 1.1e-3, 9e2, 1e3)       # the second run is this times 1e-3: 60 dB quieter
POST = {c.name: c for c in POST_CASES + [DIRTY_LOUD]}


def post_spec(case: PostCase) -> np.ndarray:
    """fp32 [frames, 2 bins] = (re | im): magnitudes log-uniform over [r_lo, r_hi], angle 0.1 .. pi/2 - 0.1 (so that both parts
    stay within [1e-7, 1e3]: neither square underflows or overflows), random signs.  peak > r_hi: the LAST element is
    peak (0.6 - 0.8i), above every other; 600 - 800i has magnitude 1000 exactly."""
    f, b = case.frames, case.bins
    if case.r_hi == 0.0:
        return np.zeros((f, 2 * b), dtype=np.float32)
    rng = np.random.default_rng(1000 + sum(map(ord, case.name)))
    r = np.exp(rng.uniform(math.log(case.r_lo), math.log(case.r_hi), (f, b)))
    th = rng.uniform(0.1, math.pi / 2 - 0.1, (f, b))
    s = rng.choice([-1.0, 1.0], (2, f, b))
    spec = np.concatenate([r * np.cos(th) * s[0], r * np.sin(th) * s[1]], axis=1).astype(np.float32)
    if case.peak:
        spec[f - 1, b - 1], spec[f - 1, 2 * b - 1] = 0.6 * case.peak, -0.8 * case.peak
    a = np.abs(spec)
    assert a.min() >= 1e-7 and a.max() <= 1e3
    return spec


def post_mag_ref(spec: np.ndarray) -> np.ndarray:
    b = spec.shape[1] // 2
    return np.hypot(spec[:, :b].astype(np.float64), spec[:, b:].astype(np.float64))


def post_check(before: np.ndarray, after: np.ndarray, out: np.ndarray, who: str = "") -> float:
    """before / after: spec [frames, 2 bins] as given / as left; out [bins, frames].  The re half holds m within 3 u of hypot in
    fp64 (two squares, an add and a square root; a contracted re*re + im*im has one rounding fewer), the im half is unchanged,
    and the dB stage is judged on the magnitudes pass 1 stored: pass 2 reads exactly those, so the interval is delta alone."""
    f, b = before.shape[0], before.shape[1] // 2
    assert after.shape == before.shape and out.shape == (b, f) and out.dtype == np.float32, f"{who}: shapes {after.shape} {out.shape}"
    assert np.array_equal(bits(after[:, b:]), bits(before[:, b:])), f"{who}: the im half of spec changed"
    m_ref = post_mag_ref(before)
    m = after[:, :b].astype(np.float64)
    assert np.isfinite(m).all() and (m >= 0).all(), f"{who}: stored magnitudes not finite"
    assert (m[m_ref == 0] == 0).all()
    r_m = float(np.max(np.abs(m - m_ref) / np.where(m_ref > 0, 3.0 * U * m_ref, 1.0)))
    print(f"{who}: magnitude largest error / (3 u m) = {r_m:.4f}")
    assert r_m <= 1.0, f"{who}: stored magnitude off by {r_m:.3f} x 3 u m"
    r_db = db_check(np.ascontiguousarray(out.T), m, m, who)
    return max(r_m, r_db)


def post_floor_fractions(before: np.ndarray):
    """(fraction of elements whose whole interval is at the floor, fraction under amin), on the reference."""
    m = post_mag_ref(before)
    box = db_box(m * (1 - 3 * U), m * (1 + 3 * U))
    return float(box.zero.mean()), float((m * (1 + 3 * U) < AMIN).mean())


POST_DAMAGES = ("max_first_sweep", "db_second_sweep_dropped", "amin_1e-10", "amin_1e-4", "clamp_absolute", "natural_log", "stale_max", "nan_dropped")


def post_standin(before: np.ndarray, damage: str = None, ws: int = 0):
    """torch CPU fp32 in the kernels' place: sqrt(re*re + im*im), the max, log10.  ws: what the maximum workspace held before the
    call (only the `stale_max` damage looks at it).  -> (spec after, out [bins, frames], workspace after)."""
    assert damage is None or damage in POST_DAMAGES
    f, b = before.shape[0], before.shape[1] // 2
    spec = torch.from_numpy(before.copy())
    re, im = spec[:, :b], spec[:, b:]
    m = torch.sqrt(re * re + im * im)
    spec[:, :b] = m
    flat = m.reshape(-1)
    if damage == "max_first_sweep":
        flat = flat[:SWEEP]
    if damage == "nan_dropped":                                        # fmaxf(x, NaN) = x, in both passes
        flat = torch.nan_to_num(flat, nan=0.0)
        m = torch.nan_to_num(m, nan=0.0)
    mx = flat.max() if flat.numel() else torch.zeros(())               # torch's max, maximum and clamp keep a NaN, as numpy's do
    if damage == "stale_max":
        mx = torch.maximum(mx, torch.tensor([ws], dtype=torch.int32).view(torch.float32)[0])
    amin = torch.tensor({"amin_1e-10": 1e-10, "amin_1e-4": 1e-4}.get(damage, 1e-5), dtype=torch.float32)
    log = torch.log if damage == "natural_log" else torch.log10
    mc, mxc = torch.maximum(m, amin), torch.maximum(mx, amin)
    if damage == "clamp_absolute":
        db = torch.maximum(20.0 * log(mc), torch.tensor(-80.0)) - 20.0 * log(mxc)
    else:
        db = 20.0 * log(mc) - 20.0 * log(mxc)
        db = torch.where(mc == mxc, torch.zeros(()), db)               # the maximum is 0 dB, also when it is +inf
        db = torch.maximum(db, torch.tensor(-80.0))
    out = (db / 80.0 + 1.0).t().contiguous()
    if damage == "db_second_sweep_dropped":
        out.view(-1)[SWEEP:] = SENTINEL                                # pass 2 is output-major: element i = bin * frames + frame
    return spec.numpy(), out.numpy(), int(mx.view(torch.int32))


def nonfinite_specs():
    """{"nan": (spec, where), "inf": (spec, where)}: post-tiny's shape, and one with a second sweep's worth left out -- small."""
    out = {}
    for kind, val in (("nan", np.nan), ("inf", np.inf)):
        spec = post_spec(POST["post-tiny"])
        spec[1, 3] = val                                               # re of frame 1, bin 3
        out[kind] = (spec, (1, 3))
    return out


def nonfinite_check(kind: str, where, out: np.ndarray, who: str = "") -> None:
    """A NaN magnitude: every output NaN (numpy's maximum keeps it, so does the device).  A +inf magnitude: that element is the
    maximum, 1.0, and every finite one is infinitely far under it: 0.0."""
    if kind == "nan":
        assert np.isnan(out).all(), f"{who}: {int((~np.isnan(out)).sum())} of {out.size} outputs are not NaN after a NaN magnitude"
    else:
        fr, k = where
        want = np.zeros_like(out)
        want[k, fr] = 1.0
        assert np.array_equal(bits(out), bits(want)), f"{who}: +inf magnitude: element {out[k, fr]!r}, others in [{np.delete(out.reshape(-1), k * out.shape[1] + fr).min()!r}, {np.delete(out.reshape(-1), k * out.shape[1] + fr).max()!r}]"


# ------------------------------------------------------------------------------------------------ audio.log_stft end to end
StftCase = namedtuple("StftCase", "name n samples tight all_one")
STFT_CASES = [
    # n = 3172: 7 frames.  Sparse signals: a product with a zero sample is an exact zero and adding it is exact, so the GEMM bound
    # holds with K_eff = the largest number of non-zero samples in a frame instead of K = 2048.
    StftCase("impulse-mid", 3172, {1028: 0.9}, True, False),           # window index 1540 / 1028 / 516 / 4 in frames 1..4, none elsewhere
    StftCase("impulse-edge", 3172, {4: 0.9}, True, False),             # window index 4 in frame 2: under the floor of frames 0, 1
    StftCase("impulses-five", 3172, {4: 0.9, 700: -0.5, 1500: 0.25, 2300: 0.7, 3171: -0.33}, True, False),
    StftCase("n0", 0, {}, False, True),
    StftCase("n1", 1, {0: 0.5}, False, False),
    StftCase("n511", 511, {510: 0.5}, False, False),
    StftCase("n512", 512, {511: -0.5}, False, False),
    StftCase("silent-5000", 5000, {}, False, True),
    StftCase("amplitude-1e-9", 5000, "noise", False, True),
]
STFT = {c.name: c for c in STFT_CASES}
WIDE, WIDE_SHARE, WIDEST = 1e-5, 0.01, 1e-3                            # a tight case: at most WIDE_SHARE of intervals wider than WIDE, none than WIDEST


def stft_signal(case: StftCase) -> np.ndarray:
    y = np.zeros(case.n, dtype=np.float32)
    if case.samples == "noise":
        y[:] = 1e-9 * np.random.default_rng(7).uniform(-1, 1, case.n)
    else:
        for i, v in case.samples.items():
            y[i] = v
    return y


def basis64(symmetric: bool = False) -> np.ndarray:
    """[2 bins, n_fft] fp64: hann[n] cos(2 pi k n / N) over -hann[n] sin(2 pi k n / N), the periodic Hann window
    0.5 - 0.5 cos(2 pi n / N) (scipy's fftbins=True; `symmetric` has N - 1 there: the damage)."""
    n = np.arange(N_FFT, dtype=np.float64)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / (N_FFT - 1 if symmetric else N_FFT))
    ang = 2.0 * np.pi * np.arange(BINS, dtype=np.float64)[:, None] * n[None, :] / N_FFT
    return np.concatenate([np.cos(ang) * win, -np.sin(ang) * win], axis=0)


def stft_frames(y: np.ndarray, hop: int = HOP, centre: bool = True, frames: int = None) -> np.ndarray:
    """[frames, n_fft] of the zero-padded signal, frames = 1 + n // 512 (the count does not follow a damaged hop)."""
    n = y.shape[0]
    frames = 1 + n // HOP if frames is None else frames
    padded = np.zeros(n + N_FFT + HOP * frames, dtype=y.dtype)
    off = N_FFT // 2 if centre else 0
    padded[off:off + n] = y
    return np.stack([padded[i * hop:i * hop + N_FFT] for i in range(frames)])


def stft_mag_box(y: np.ndarray, basis32: np.ndarray):
    """(m_lo, m_hi) [frames, bins]: the fp64 product of the fp32 frames with the fp32 basis, and per element
    E = 4 (K_eff + 2) u sum |a||b| for re and for im, E_m = hypot(E_re, E_im) + 3 u (m + hypot(E_re, E_im))."""
    a = stft_frames(y).astype(np.float64)
    b = basis32.astype(np.float64)
    k_eff = int((a != 0).sum(axis=1).max())
    s, s_abs = a @ b.T, np.abs(a) @ np.abs(b).T
    e = 4.0 * (k_eff + 2) * U * s_abs
    m = np.hypot(s[:, :BINS], s[:, BINS:])
    e_h = np.hypot(e[:, :BINS], e[:, BINS:])
    e_m = e_h + 3.0 * U * (m + e_h)
    return np.maximum(m - e_m, 0.0), m + e_m, k_eff


def stft_check(case: StftCase, out, basis32: np.ndarray, who: str = "") -> float:
    """out: what audio.log_stft returned for stft_signal(case), a torch tensor [1, 195, 1 + n // 512] fp32."""
    frames = 1 + case.n // HOP
    assert tuple(out.shape) == (1, BINS, frames) and out.dtype == torch.float32, f"{who}: {tuple(out.shape)} {out.dtype}"
    got = out[0].detach().cpu().numpy()
    m_lo, m_hi, k_eff = stft_mag_box(stft_signal(case), basis32)
    box = db_box(m_lo, m_hi)
    width = box.hi - box.lo + 2.0 * box.delta
    print(f"{who}: K_eff = {k_eff}, interval width median {np.median(width):.3e}, share > {WIDE:g}: {float((width > WIDE).mean()):.4%}, widest {width.max():.3e}")
    if case.tight:
        assert float((width > WIDE).mean()) <= WIDE_SHARE and width.max() <= WIDEST, f"{who}: the reference intervals have gone slack"
    assert bool(box.all_one) == case.all_one
    return db_check(np.ascontiguousarray(got.T), m_lo, m_hi, who)


def basis_check(basis32: np.ndarray) -> float:
    """The fp32 basis is one rounding of the fp64 periodic-Hann basis: |b32 - b64| <= u |b64| (1 + 2^-20 for the last bit of
    another libm's cos).  -> the largest error / bound."""
    b64 = basis64()
    assert basis32.dtype == np.float32 and basis32.shape == b64.shape
    err, bound = np.abs(basis32.astype(np.float64) - b64), U * np.abs(b64) * (1 + 2.0 ** -20) + 2.0 ** -150
    return float((err / bound).max())


STFT_DAMAGES = ("symmetric_hann", "no_centre_padding", "hop_511", "last_frame_dropped", "not_transposed")


def stft_standin(y: np.ndarray, damage: str = None):
    """torch CPU fp32 matmul of the strided frames with the fp32 basis, then post_standin.  -> [1, 195, frames] torch fp32."""
    assert damage is None or damage in STFT_DAMAGES
    frames = 1 + y.shape[0] // HOP
    basis = torch.from_numpy(basis64(symmetric=damage == "symmetric_hann").astype(np.float32))
    a = torch.from_numpy(stft_frames(y, hop=511 if damage == "hop_511" else HOP, centre=damage != "no_centre_padding"))
    if damage == "last_frame_dropped":
        a = a.clone()
        a[frames - 1] = 0.0
    spec = (a @ basis.t()).numpy()
    out = post_standin(spec)[1]
    if damage == "not_transposed":
        out = np.ascontiguousarray(out.T).reshape(BINS, frames)        # [frame][bin] memory read as [bin][frame]
    return torch.from_numpy(np.ascontiguousarray(out)).unsqueeze(0)


# ------------------------------------------------------------------------------------------------ audio.resample_poly
RESAMPLE_CASES = [
    # (orig, target, n)
    (11025, 22050, 301),       # g = 4 (odd down), G = 8, K = 32, 76 rows
    (11025, 22050, 4),         # n_out = G: one full row
    (11025, 22050, 5),         # two rows, the last holding 2 of 8
    (66150, 22050, 50),        # G = 4
    (22050, 16000, 1500),      # G = 1280, K = 1800, one row
    (22050, 8000, 999),
    (24000, 22050, 1000),
    (12000, 22050, 333),
    (44100, 22050, 1), (44100, 22050, 2),      # n_out = 1
    (48000, 22050, 3),
    (16000, 22050, 1),
    (22050, 22050, 64),        # up == down: a clone, not an alias
]


def resample_id(case) -> str:
    return "%d-%d-n%d" % case


def up_down(orig: int, target: int):
    g = math.gcd(orig, target)
    return target // g, orig // g


def resample_input(case) -> np.ndarray:
    orig, target, n = case
    return np.random.default_rng(orig % 1000 + target % 1000 + n).standard_normal(n).astype(np.float32)


def resample_ref(case):
    """(ref, sum |x||h|) in fp64: scipy.signal.resample_poly as oracle.ref_cpu.resample_poly restates it (pinned by fixture F18),
    kept in fp64 here with the sum of absolute terms next to it."""
    orig, target, n = case
    x = resample_input(case).astype(np.float64)
    up, down = up_down(orig, target)
    if up == down:
        return x.copy(), np.zeros(n)
    h, r0 = ref_cpu.resample_filter(up, down)
    n_out = -(-n * up // down)
    ref, mag = np.zeros(n_out), np.zeros(n_out)
    for j in range(n_out):
        t = (j + r0) * down
        i_lo, i_hi = max(0, -(-(t - len(h) + 1) // up)), min(n - 1, t // up)
        if i_hi >= i_lo:
            i = np.arange(i_lo, i_hi + 1)
            ref[j], mag[j] = np.dot(x[i], h[t - i * up]), np.dot(np.abs(x[i]), np.abs(h[t - i * up]))
    return ref, mag


def resample_check(case, got, k_pad: int, who: str = "") -> float:
    """got: torch fp32 [ceil(n up / down)], contiguous.  |got - ref| <= (4 (K_ + 2) + 1) u sum |x||h|: the GEMM bound over the
    plan's padded window K_ (= k_pad), + 1 for the rounding of H to fp32."""
    orig, target, n = case
    up, down = up_down(orig, target)
    assert got.dtype == torch.float32 and got.dim() == 1 and got.is_contiguous() and got.numel() == -(-n * up // down), \
        f"{who}: {got.dtype} {tuple(got.shape)} contiguous={got.is_contiguous()}, want length {-(-n * up // down)}"
    ref, mag = resample_ref(case)
    g = got.detach().cpu().numpy()
    if up == down:
        assert np.array_equal(bits(g), bits(ref.astype(np.float32))), f"{who}: up == down is a copy"
        return 0.0
    assert np.array_equal(ref.astype(np.float32), ref_cpu.resample_poly(resample_input(case), orig, target)), "the fp64 reference left the oracle"
    bound = (4.0 * (k_pad + 2) + 1.0) * U * mag
    assert np.isfinite(g).all() and (bound > 0).all()
    ratio = float((np.abs(g.astype(np.float64) - ref) / bound).max())
    print(f"{who}: resample {resample_id(case)} K_ = {k_pad}: largest error / bound = {ratio:.5f}")
    assert ratio <= 1.0, f"{who}: resample {resample_id(case)}: error / bound = {ratio:.3f}"
    return ratio


RESAMPLE_DAMAGES = ("phase_plus_one", "lo_not_rounded", "last_row_dropped")


def plan_restated(up: int, down: int, damage: str = None):
    """audio._resample_plan in fp64, written from the same derivation (y[q G + p] = sum_i' x[q g down + i'] h[(p + r0) down - i' up])
    -> (H [G, K_] fp64, lo the frames start at, g).  Damages: the phase one output late (r0 + 1); the columns of H starting at the
    first tap while the frames start at the 16-byte-aligned sample below it."""
    h, r0 = ref_cpu.resample_filter(up, down)
    if damage == "phase_plus_one":
        r0 += 1
    g = 1
    while (g * down) % 4:
        g += 1
    G = g * up
    lo_tap = -((len(h) - 1 - r0 * down) // up)
    hi = ((G - 1 + r0) * down) // up
    lo = lo_tap - lo_tap % 4
    col0 = lo_tap if damage == "lo_not_rounded" else lo
    K_ = (hi - lo + 1 + 7) // 8 * 8
    H = np.zeros((G, K_))
    for p in range(G):
        ip = np.arange(col0, hi + 1)
        j = (p + r0) * down - ip * up
        ok = (j >= 0) & (j < len(h))
        H[p, (ip - col0)[ok]] = h[j[ok]]
    return H, lo, g


def resample_standin(case, plan, damage: str = None):
    """plan = (H, lo, g) with H [G, K_] (fp32 values) times the strided frames of the zero-padded fp32 signal, in fp64, rounded
    once to fp32; the framing is audio.resample_poly's.  -> torch fp32."""
    assert damage is None or damage in RESAMPLE_DAMAGES
    orig, target, n = case
    up, down = up_down(orig, target)
    x = resample_input(case)
    if up == down:
        return torch.from_numpy(x.copy())
    H, lo, g = plan
    H = np.asarray(H, dtype=np.float64)
    G, K_ = H.shape
    n_out = -(-n * up // down)
    rows = -(-n_out // G)
    stride, front = g * down, -lo
    padded = np.zeros(front + (rows - 1) * stride + K_ + 8)
    padded[front:front + n] = x
    frames = np.stack([padded[q * stride:q * stride + K_] for q in range(rows)])
    out = frames @ H.T
    if damage == "last_row_dropped":
        out[rows - 1] = 0.0
    return torch.from_numpy(out.reshape(-1)[:n_out].astype(np.float32))
