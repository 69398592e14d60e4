"""The photometric loss (include/gsplat.h, gs_photometric_loss*) without a GPU: `loss_reference`, the float64 restatement of
the header's definition that tests/test_loss_gpu.py holds the kernels to, checked here against central differences and
against a direct 121-tap loop; the seeded inputs of both files; and the two symbols in the header, the binding and the
library."""
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
    is then chosen so that the composited image over `alpha` = bg is the I above), else 0."""
    rng = np.random.default_rng([seed, w, h, {"noise": 0, "near": 1, "flat": 2}[kind]])
    g = rng.uniform(0.0, 1.0, (h, w, 3))
    if kind == "noise":
        i = rng.uniform(-0.1, 1.1, (h, w, 3))
    elif kind == "near":
        i = g + 0.02 * rng.standard_normal((h, w, 3))
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


def test_loss_symbols_are_exported():
    """The two entry points are in the binding's list and in the library (on a tree without the feature: neither)."""
    for name in ("gs_photometric_loss", "gs_photometric_loss_device"):
        assert name in _lib.EXPORTS
    assert hasattr(_lib.lib(), "gs_photometric_loss")
    assert hasattr(_lib.lib(), "gs_photometric_loss_device")
