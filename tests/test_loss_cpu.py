"""The photometric loss (include/gsplat.h, gs_photometric_loss*) without a GPU: `loss_reference`, the float64 restatement of
the header's definition that tests/test_loss_gpu.py holds the kernels to, checked here against central differences and
against a direct 121-tap loop; the seeded inputs of both files, those of more than 1024 tiles with their precondition and
their float32 guard; and the two symbols in the header, the binding and the library."""
import functools

import numpy as np
import pytest

from vk3dgaussiansplatting_amd import _lib

C1, C2 = 0.01 ** 2, 0.03 ** 2

# The cases of tests/test_loss_gpu.py (tools/loss_cost.py reports the same ones).  W x H: smaller than the window radius
# (1 x 1, 5 x 3); one tile whose window leaves the image on all sides; one-pixel partial tiles right and below (a halo with a
# single valid column / row); partial tiles both ways; a centre tile that takes its whole halo from eight neighbours
SHAPES = [(1, 1), (5, 3), (16, 16), (33, 17), (37, 21), (48, 48)]
TOL = {"noise": 2e-5, "near": 2e-5, "flat": 4e-3}
LAMBDAS = (0.2, 0.0, 1.0)
BG = (0.2, 0.5, 0.9)
BGS = (None, (1.0, 1.0, 1.0), BG)
SEED = 4

# More than 1024 tiles: k_loss_reduce gives each of its 1024 threads per = ceil(tiles / 1024) consecutive tiles.  W x H, each
# the smallest that reaches its edge: 1024 tiles (per = 1, every thread busy, one valid row per tile); 1025 (per = 2, 513
# threads, the last owns a single tile); the same with grid_w = 1; 2049 (per = 3, ragged tail); 8193 (per = 9, as a 1080p
# frame's 8160 tiles with per = 8; 911 threads busy).  MANY_TILES_2D: 33 x 32 = 1056 tiles, interior tiles with full halos.
STRIPS = [(16384, 1), (16385, 1), (1, 16385), (32769, 2), (131073, 1)]
MANY_TILES_2D = (528, 512)
APART_KINDS = ("noise_apart", "near_apart")         # held to TOL["noise"], the project's own 2e-5
# (kind, w, h, lambda, bg) of tests/test_loss_gpu.py::test_by_value_many_tiles
MANY_TILE_CASES = [(kind, w, h, lam, bg) for w, h in STRIPS for kind in APART_KINDS for lam in (0.2, 1.0) for bg in (None, BG)]
MANY_TILE_CASES.append(("noise_apart",) + MANY_TILES_2D + (0.2, BG))
# (kind, w, h) of the float32 guard: lambda = 0.2, no background
MANY_TILE_GUARD = [(kind, w, h) for w, h in STRIPS for kind in APART_KINDS] + [("noise_apart",) + MANY_TILES_2D]


@functools.lru_cache(maxsize=None)
def window():
    """The eleven weights: exp(-k^2 / (2 * 1.5^2)) normalised in double, rounded once to float32 (returned as float64)."""
    k = np.arange(-5, 6, dtype=np.float64)
    w = np.exp(-k * k / (2.0 * 1.5 ** 2))
    w = (w / w.sum()).astype(np.float32).astype(np.float64)
    w.setflags(write=False)
    return w


def _loss_torch(rgba, target, lam, bg, dtype, separable):
    """The definition in torch at `dtype`: (numbers [3], gradient [H][W][4]) as numpy arrays of that dtype.  separable: the
    window as a row pass then a column pass; else one 11 x 11 window."""
    import torch
    import torch.nn.functional as F
    x = torch.tensor(np.asarray(rgba), dtype=dtype, requires_grad=True)             # [H, W, 4]
    g = torch.tensor(np.asarray(target), dtype=dtype).permute(2, 0, 1)[None]        # [1, 3, H, W]
    lam_t = torch.tensor(float(lam), dtype=dtype)
    img = x[..., :3]
    if bg is not None:
        img = img + (1.0 - x[..., 3:4]) * torch.tensor(np.asarray(bg, np.float32).astype(np.float64), dtype=dtype)
    img = img.permute(2, 0, 1)[None]
    w1 = torch.tensor(window(), dtype=dtype)
    if separable:
        wx, wy = w1.reshape(1, 1, 1, 11).repeat(3, 1, 1, 1), w1.reshape(1, 1, 11, 1).repeat(3, 1, 1, 1)
        conv = lambda t: F.conv2d(F.conv2d(t, wx, padding=(0, 5), groups=3), wy, padding=(5, 0), groups=3)
    else:
        w2 = (w1[:, None] * w1[None, :]).reshape(1, 1, 11, 11).repeat(3, 1, 1, 1)
        conv = lambda t: F.conv2d(t, w2, padding=5, groups=3)
    mu1, mu2 = conv(img), conv(g)
    s1 = conv(img * img) - mu1 * mu1
    s2 = conv(g * g) - mu2 * mu2
    s12 = conv(img * g) - mu1 * mu2
    ssim = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    l1 = (img - g).abs().mean()
    dssim = 1.0 - ssim.mean()
    loss = (1.0 - lam_t) * l1 + lam_t * dssim
    loss.backward()
    numbers = torch.stack([loss, l1, dssim]).detach().numpy()
    return numbers, x.grad.numpy()


def loss_reference(rgba, target, lam=0.2, bg=None):
    """float64: numbers = {loss, L1, DSSIM} and dloss/d(rgba) [H][W][4] by autograd, of the definition in include/gsplat.h."""
    import torch
    return _loss_torch(rgba, target, lam, bg, torch.float64, separable=False)


def loss_float32(rgba, target, lam=0.2, bg=None, separable=True):
    """The same formulas evaluated in float32 by torch on the CPU: what the tolerance of the GPU test is derived from."""
    import torch
    return _loss_torch(rgba, target, lam, bg, torch.float32, separable)


def make_inputs(kind, w, h, seed, alpha):
    """Seeded float32 (rgba [H][W][4], target [H][W][3]).  noise: I uniform in [-0.1, 1.1], G uniform in [0, 1]; near:
    I = G + 0.02 N(0, 1); flat: G = 0.7, I = 0.69, both + 1e-3 N(0, 1) (conv(I^2) - mu^2 cancels).  alpha: random in [0, 1] (for a background: rgb
    is then chosen so that the composited image over `alpha` = bg is the I above), else 0.  For any number of values, where
    noise and near come as close as float32 rounding (|I - G| of 6e-8 and 0 among 1e5 values), two kinds apart by
    construction, s = +-1 at random: noise_apart: I = G + s U(1e-3, 0.6); near_apart: I = G + s (1e-3 + 0.02 |N(0, 1)|)."""
    rng = np.random.default_rng([seed, w, h, {"noise": 0, "near": 1, "flat": 2, "noise_apart": 3, "near_apart": 4}[kind]])
    g = rng.uniform(0.0, 1.0, (h, w, 3))
    if kind == "noise":
        i = rng.uniform(-0.1, 1.1, (h, w, 3))
    elif kind == "near":
        i = g + 0.02 * rng.standard_normal((h, w, 3))
    elif kind in APART_KINDS:
        s = rng.choice((-1.0, 1.0), (h, w, 3))
        i = g + s * (rng.uniform(1e-3, 0.6, (h, w, 3)) if kind == "noise_apart"
                     else 1e-3 + 0.02 * np.abs(rng.standard_normal((h, w, 3))))
    else:
        g = 0.7 + 1e-3 * rng.standard_normal((h, w, 3))
        i = 0.69 + 1e-3 * rng.standard_normal((h, w, 3))
    rgba = np.zeros((h, w, 4), np.float32)
    if alpha is not None:
        a = rng.uniform(0.0, 1.0, (h, w))
        rgba[..., 3] = a
        i = i - (1.0 - a)[..., None] * np.asarray(alpha, np.float64)
    rgba[..., :3] = i
    return rgba, g.astype(np.float32)


def composited_float32(rgba, bg):
    """I = rgb + (1 - a) * bg in float32, in the kernels' order of operations."""
    i = rgba[..., :3].astype(np.float32)
    if bg is not None:
        i = i + (np.float32(1.0) - rgba[..., 3:4]) * np.asarray(bg, np.float32)
    assert i.dtype == np.float32
    return i


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def many_tile_case(kind, w, h, lam, bg):
    """(rgba, target, reference numbers, reference gradient) of one many-tile case: computed once per process, shared by
    the tests that need it, read-only."""
    rgba, target = make_inputs(kind, w, h, SEED, bg)
    return _frozen(rgba, target, *loss_reference(rgba, target, lam, bg))


@functools.lru_cache(maxsize=None)
def float32_torch_errors(kind, w, h):
    """What float32 torch (both summation orders, lambda = 0.2, no background) is wrong by on make_inputs(kind, w, h, SEED):
    (|loss - ref| / |ref|, max |gradient - ref| / max |ref|), the worse of the two orders."""
    rgba, target, ref_n, ref_g = many_tile_case(kind, w, h, 0.2, None)
    worst_l = worst_g = 0.0
    for separable in (True, False):
        n, g = loss_float32(rgba, target, 0.2, None, separable)
        worst_l = max(worst_l, abs(float(n[0]) - ref_n[0]) / abs(ref_n[0]))
        worst_g = max(worst_g, float(np.abs(g - ref_g).max() / np.abs(ref_g).max()))
    return worst_l, worst_g


def direct_numbers(rgba, target, lam, bg):
    """{loss, L1, DSSIM} by a direct, non-separable 121-tap loop in numpy float64: no convolution routine, no torch."""
    rgba, target = np.asarray(rgba, np.float64), np.asarray(target, np.float64)
    h, w = target.shape[:2]
    img = rgba[..., :3].copy()
    if bg is not None:
        img += (1.0 - rgba[..., 3:4]) * np.asarray(bg, np.float32).astype(np.float64)
    wt = window()
    total = 0.0
    for y in range(h):
        for x in range(w):
            acc = np.zeros((5, 3))
            for dy in range(-5, 6):
                for dx in range(-5, 6):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w:
                        wgt = wt[dy + 5] * wt[dx + 5]
                        a, b = img[yy, xx], target[yy, xx]
                        acc += wgt * np.stack([a, b, a * a, b * b, a * b])
            m1, m2 = acc[0], acc[1]
            s1, s2, s12 = acc[2] - m1 * m1, acc[3] - m2 * m2, acc[4] - m1 * m2
            total += np.sum(((2 * m1 * m2 + C1) * (2 * s12 + C2)) / ((m1 * m1 + m2 * m2 + C1) * (s1 + s2 + C2)))
    l1 = np.abs(img - target).mean()
    dssim = 1.0 - total / (3 * h * w)
    return np.array([(1.0 - lam) * l1 + lam * dssim, l1, dssim])


@pytest.mark.parametrize("bg", [None, BG], ids=["black", "bg"])
def test_reference_gradient_against_central_differences(bg):
    """9 x 7, float64, every one of the 252 inputs moved by +-1e-6: max |difference quotient - gradient| <= 1e-6 of the
    gradient's largest magnitude (truncation ~1e-12, rounding ~1e-10 of it; no |I - G| of the noise input is below 1e-4)."""
    pytest.importorskip("torch")
    w, h, lam, step = 9, 7, 0.2, 1e-6
    rgba, target = make_inputs("noise", w, h, 1, bg)
    rgba = rgba.astype(np.float64)
    img = rgba[..., :3] + ((1.0 - rgba[..., 3:4]) * np.asarray(bg) if bg is not None else 0.0)
    assert np.abs(img - target).min() > 1e-4
    _, grad = loss_reference(rgba, target, lam, bg)
    fd = np.zeros_like(grad)
    for idx in np.ndindex(*rgba.shape):
        hi, lo = rgba.copy(), rgba.copy()
        hi[idx] += step
        lo[idx] -= step
        fd[idx] = (loss_reference(hi, target, lam, bg)[0][0] - loss_reference(lo, target, lam, bg)[0][0]) / (2 * step)
    if bg is None:
        assert not grad[..., 3].any()
    assert np.abs(fd - grad).max() <= 1e-6 * np.abs(grad).max()


@pytest.mark.parametrize("w,h", [(5, 3), (16, 16)])
def test_reference_numbers_against_a_direct_loop(w, h):
    """loss, L1 and DSSIM of the reference equal a 121-tap loop in numpy to 1e-12 (relative), with and without a background."""
    pytest.importorskip("torch")
    for kind, bg, lam in (("noise", None, 0.2), ("near", BG, 0.7)):
        rgba, target = make_inputs(kind, w, h, 2, bg)
        got, _ = loss_reference(rgba, target, lam, bg)
        want = direct_numbers(rgba, target, lam, bg)
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (kind, got, want)


def test_float32_orders_agree_with_the_reference():
    """The two float32 evaluations (separable, 2-D) of a 16 x 16 noise input are within 2e-6 of the reference: the figure
    the GPU test's tolerance of 2e-5 is ten times."""
    pytest.importorskip("torch")
    rgba, target = make_inputs("noise", 16, 16, 3, None)
    ref_n, ref_g = loss_reference(rgba, target)
    for separable in (True, False):
        n, g = loss_float32(rgba, target, separable=separable)
        assert np.abs(n - ref_n).max() <= 2e-6 * np.abs(ref_n).max()
        assert np.abs(g - ref_g).max() <= 2e-6 * np.abs(ref_g).max()


@pytest.mark.parametrize("w,h", STRIPS + [MANY_TILES_2D], ids=[f"{w}x{h}" for w, h in STRIPS + [MANY_TILES_2D]])
def test_apart_kinds_are_apart(w, h):
    """The precondition of the by-value tests on the many-tile inputs, every kind with and without a background:
    min |composited I - G| > 5e-7 with the composite and the difference in float32 (1.0e-3 by construction), so that no
    sign(I - G) hangs on float32 rounding; both signs occur, and alpha is random under a background and 0 without."""
    for kind in APART_KINDS:
        for bg in (None, BG):
            rgba, target = make_inputs(kind, w, h, SEED, bg)
            assert rgba.dtype == target.dtype == np.float32 and rgba.shape == (h, w, 4) and target.shape == (h, w, 3)
            d = composited_float32(rgba, bg) - target
            assert d.dtype == np.float32
            gap = float(np.abs(d).min())
            print(f"{kind} {w}x{h} bg={bg}: min |I - G| {gap:.3e}")
            assert gap > 5e-7 and gap > 0.99e-3, (kind, bg, gap)
            assert (d > 0).any() and (d < 0).any()
            assert rgba[..., 3].any() == (bg is not None)


@pytest.mark.parametrize("kind,w,h", MANY_TILE_GUARD, ids=[f"{k}-{w}x{h}" for k, w, h in MANY_TILE_GUARD])
def test_float32_torch_stays_within_a_fraction_of_tol_many_tiles(kind, w, h):
    """The guard of tests/test_loss_gpu.py::test_float32_torch_stays_within_a_fraction_of_tol on the many-tile inputs, where
    no GPU is needed for it: float32 torch stays within tol / 5 = 4e-6 of the float64 reference.  Worst when written: loss
    1.7e-6 (near_apart, 131073 x 1), gradient 9.9e-7 of its scale (noise_apart, 528 x 512)."""
    pytest.importorskip("torch")
    tol = TOL["noise"]
    worst_l, worst_g = float32_torch_errors(kind, w, h)
    print(f"float32 torch, {kind} {w}x{h}: loss {worst_l:.3e}, gradient {worst_g:.3e} of its scale (tol {tol})")
    assert worst_l <= tol / 5 and worst_g <= tol / 5


def test_loss_symbols_are_exported():
    """The two entry points are in the binding's list and in the library (on a tree without the feature: neither)."""
    for name in ("gs_photometric_loss", "gs_photometric_loss_device"):
        assert name in _lib.EXPORTS
    assert hasattr(_lib.lib(), "gs_photometric_loss")
    assert hasattr(_lib.lib(), "gs_photometric_loss_device")
