"""The photometric loss on the MI355X (include/gsplat.h, gs_photometric_loss*; csrc/gs_loss.hip) against `loss_reference`
of tests/test_loss_cpu.py (float64), by value (also past 1024 tiles), by bits, by known answers, through the zero-copy
path, the refusals and torch autograd.  A one-splat scene exists only so that a resolution can be set; rgba and target are
passed explicitly."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_parity_gpu import make_renderer, make_scene
from test_backward_cpu import small_scene
from test_loss_cpu import (BG, BGS, LAMBDAS, MANY_TILE_CASES, MANY_TILE_GUARD, SEED, SHAPES, TOL,
                           composited_float32, float32_torch_errors, loss_reference, make_inputs, many_tile_case)

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def contexts():
    """One renderer per resolution (a one-splat scene), made on first use, shared by the tests and cleaned up at the end."""
    made = {}

    def get(w, h, **kw):
        key = (w, h) + tuple(sorted(kw.items()))
        if key not in made:
            aos = gs.makeGaussian((0.0, 0.0, 2.0), (0.1, 0.1, 0.1), sh0=(0.5, 0.5, 0.5, 0.8))[None].astype(np.float32)
            made[key] = make_renderer(make_scene(aos, w, h), w, h, **kw)
        return made[key]

    yield get
    for r in made.values():
        r.cleanup()


def composited(rgba, bg):
    i = rgba[..., :3].astype(np.float64)
    if bg is not None:
        i = i + (1.0 - rgba[..., 3:4].astype(np.float64)) * np.asarray(bg, np.float32).astype(np.float64)
    return i


def number_bounds(ref, tol):
    """tol relative for each of loss, L1, DSSIM; absolute for a DSSIM below 1e-3."""
    b = tol * np.abs(ref)
    if ref[2] < 1e-3:
        b[2] = tol
    return b


def plane_errors(got, ref):
    """max |got - ref| and max |ref| of each of the four channel planes."""
    return (np.abs(got.astype(np.float64) - ref).reshape(-1, 4).max(0), np.abs(ref).reshape(-1, 4).max(0))


# ---- 1. by value ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(TOL))
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_by_value(contexts, w, h, kind):
    """Every lambda in {0.2, 0, 1} and bg in {NULL, (1, 1, 1), (0.2, 0.5, 0.9)} (alpha random in [0, 1] under a bg):
    per channel plane max |gpu - ref| <= tol * max |ref|; loss, L1 and DSSIM to tol relative (absolute for a DSSIM below
    1e-3).  tol = 2e-5 for noise and near, 4e-3 for flat: ten times what the same formulas evaluated in float32 by torch on
    the CPU, separable and 2-D, are wrong by on these kinds at lambda = 0.2 without a background -- at most 2.2e-6 of the
    gradient's scale and 1.7e-6 of the loss for noise and near, 1.8e-4 and 3.8e-4 for flat, when the tolerance was set; on
    these inputs float32 torch is wrong by 9.3e-7 / 1.0e-7 (noise), 2.1e-6 / 2.2e-6 (near), 1.6e-4 / 3.2e-4 (flat).  The
    kernels on an MI355X, worst over every case here: gradient 6.4e-7 (noise), 6.4e-6 (near), 7.4e-5 (flat) of the plane's
    scale; numbers 2.0e-7, 2.7e-6 and 4.1e-6 relative, a DSSIM below 1e-3 included (profiles/loss_cost.txt)."""
    tol = TOL[kind]
    r = contexts(w, h)
    worst_g = worst_n = 0.0
    for lam in LAMBDAS:
        for bg in BGS:
            rgba, target = make_inputs(kind, w, h, SEED, bg)
            assert np.abs(composited(rgba, bg) - target).min() > 5e-7      # no sign(I - G) hangs on float32 rounding
            ref_n, ref_g = loss_reference(rgba, target, lam, bg)
            got_n, got_g = r.photometricLoss(rgba, target, lam, bg)
            err, scale = plane_errors(got_g, ref_g)
            nerr, nb = np.abs(got_n.astype(np.float64) - ref_n), number_bounds(ref_n, tol)
            worst_g = max(worst_g, float((err / np.where(scale > 0, scale, 1.0)).max()))
            worst_n = max(worst_n, float((nerr / nb).max()) * tol)
            print(f"{kind} {w}x{h} lam={lam} bg={bg}: grad err/scale {err / np.where(scale > 0, scale, 1.0)} numbers err {nerr} bounds {nb}")
            assert np.all(err <= tol * scale), (lam, bg, err, scale)
            assert np.all(nerr <= nb), (lam, bg, got_n, ref_n)
    print(f"WORST {kind} {w}x{h}: gradient {worst_g:.3e} of the plane's scale, numbers {worst_n:.3e} (tol {tol})")


def case_id(kind, w, h, lam, bg):
    return f"{kind}-{w}x{h}-lam{lam}-{'bg' if bg else 'black'}"


@pytest.mark.parametrize("kind,w,h,lam,bg", MANY_TILE_CASES, ids=[case_id(*c) for c in MANY_TILE_CASES])
def test_by_value_many_tiles(contexts, kind, w, h, lam, bg):
    """More than 1024 tiles, where k_loss_reduce gives a thread `per` > 1 tiles, a ragged last slice or none at all
    (test_loss_cpu.STRIPS, MANY_TILES_2D): the assertions of test_by_value at its tol of 2e-5, every number relative (each
    DSSIM here exceeds 1e-3, which is asserted).  The kinds are noise_apart and near_apart, whose |I - G| is at least 1e-3 by
    construction: the precondition, evaluated in float32, holds for every case.  Strips: both kinds x lambda in {0.2, 1} x
    bg in {NULL, (0.2, 0.5, 0.9)}; 528 x 512: noise_apart, lambda 0.2, with the background.  A reduce that drops or doubles a
    tile moves the numbers by about 1 / tiles (6e-5 for the single pixel of the 1025th tile) and no gradient value.
    The kernels on an MI355X, worst over these cases: gradient 1.1e-6 of the plane's scale (near_apart, 1 x 16385, lambda 1,
    with the background; noise_apart at most 3.0e-7), numbers 5.3e-8 relative (noise_apart, 16384 x 1)."""
    tol = TOL["noise"]
    rgba, target, ref_n, ref_g = many_tile_case(kind, w, h, lam, bg)
    assert np.abs(composited_float32(rgba, bg) - target).min() > 5e-7       # no sign(I - G) hangs on float32 rounding
    assert np.abs(composited(rgba, bg) - target).min() > 5e-7
    assert ref_n[2] >= 1e-3
    got_n, got_g = contexts(w, h).photometricLoss(rgba, target, lam, bg)
    err, scale = plane_errors(got_g, ref_g)
    nerr, nb = np.abs(got_n.astype(np.float64) - ref_n), tol * np.abs(ref_n)
    worst_g, worst_n = float((err / np.where(scale > 0, scale, 1.0)).max()), float((nerr / np.abs(ref_n)).max())
    print(f"WORST {case_id(kind, w, h, lam, bg)}: gradient {worst_g:.3e} of the plane's scale, numbers {worst_n:.3e} (tol {tol})")
    assert np.all(err <= tol * scale), (err, scale)
    assert np.all(nerr <= nb), (got_n, ref_n)


GUARD_CASES = ([pytest.param(kind, SHAPES, id=kind) for kind in TOL] +
               [pytest.param(kind, [(w, h)], id=f"{kind}-{w}x{h}") for kind, w, h in MANY_TILE_GUARD])


@pytest.mark.parametrize("kind,shapes", GUARD_CASES)
def test_float32_torch_stays_within_a_fraction_of_tol(kind, shapes):
    """The guard on the margin: the float32 evaluation by torch (both summation orders, lambda = 0.2, no background: what
    the tolerance was derived from) on every shape.  The figures the tolerance was set from, 2.2e-6 and 1.7e-6, are 0.11
    and 0.085 of 2e-5, and on these inputs torch's float32 gradient reaches 0.10 to 0.17 of it for `near` whatever the
    seed: `a tenth of tol` cannot hold for that figure, so the guard is tol / 5 -- a margin of five, twice the worst figure
    measured (0.108 with this seed).  A torch whose float32 convolution is wrong by more than that fails here.  The
    many-tile inputs of test_by_value_many_tiles, one shape per case: at worst 1.7e-6 of the loss (near_apart, 131073 x 1)
    and 9.9e-7 of the gradient's scale (noise_apart, 528 x 512) against 4e-6.  near_apart is left out at 528 x 512: the
    near kind reaches 3.4e-6 there, 0.84 of the guard."""
    tol = TOL.get(kind, TOL["noise"])              # the many-tile kinds are held to the same 2e-5
    worst_l = worst_g = 0.0
    for w, h in shapes:
        err_l, err_g = float32_torch_errors(kind, w, h)
        worst_l, worst_g = max(worst_l, err_l), max(worst_g, err_g)
    print(f"float32 torch, {kind}: loss {worst_l:.3e}, gradient {worst_g:.3e} of its scale (tol {tol})")
    assert worst_l <= tol / 5 and worst_g <= tol / 5


# ---- 2. the alpha gradient ------------------------------------------------------------------------------------------------

def test_alpha_gradient(contexts):
    """bg == NULL: exactly 0.0f everywhere.  With a bg: -sum_c bg_c dI_c recomputed in float32 from the returned rgb
    gradients, to 2 ulp."""
    for w, h in ((5, 3), (37, 21)):
        r = contexts(w, h)
        rgba, target = make_inputs("noise", w, h, SEED, BG)
        _, g = r.photometricLoss(rgba, target, 0.2, None)
        assert not bits(g[..., 3]).any() and np.any(g[..., :3] != 0)
        for bg in BGS[1:]:
            _, g = r.photometricLoss(rgba, target, 0.2, bg)
            b = np.asarray(bg, np.float32)
            want = -((b[0] * g[..., 0] + b[1] * g[..., 1]) + b[2] * g[..., 2])
            assert want.dtype == np.float32 and np.any(want != 0)
            assert np.all(np.abs(g[..., 3] - want) <= 2 * np.spacing(np.abs(want)))


# ---- 3. bits --------------------------------------------------------------------------------------------------------------

def device_call(r, rgba, target, lam, bg, want_grad=True):
    """The device form on torch tensors: (numbers, gradient or None) back on the host."""
    import torch
    t_rgba = None if rgba is None else torch.tensor(rgba, device="cuda")
    t_target = torch.tensor(target, device="cuda")
    numbers = torch.zeros(3, device="cuda")
    grad = torch.zeros(target.shape[0], target.shape[1], 4, device="cuda") if want_grad else None
    torch.cuda.synchronize()
    r.photometricLossDevice(None if t_rgba is None else t_rgba.data_ptr(), t_target.data_ptr(), lam, bg, numbers.data_ptr(),
                            None if grad is None else grad.data_ptr())
    r.synchronize()
    return numbers.cpu().numpy(), None if grad is None else grad.cpu().numpy()


def test_bits_are_reproducible(contexts):
    """Two calls, the host form and the device form, and a call after gs_set_resolution to another size and back (the
    scratch is freed and allocated again): identical uint32 views of loss_out and of the gradient."""
    pytest.importorskip("torch")
    w, h = 37, 21
    r = contexts(w, h)
    rgba, target = make_inputs("noise", w, h, SEED, BG)
    n0, g0 = r.photometricLoss(rgba, target, 0.2, BG)
    n1, g1 = r.photometricLoss(rgba, target, 0.2, BG)
    assert np.array_equal(bits(n0), bits(n1)) and np.array_equal(bits(g0), bits(g1))
    n2, g2 = device_call(r, rgba, target, 0.2, BG)
    assert np.array_equal(bits(n0), bits(n2)) and np.array_equal(bits(g0), bits(g2))
    L = _lib.lib()
    assert L.gs_set_resolution(r._ctx.handle, 48, 48) == _lib.GS_OK
    big = make_inputs("near", 48, 48, SEED, None)
    r.photometricLoss(big[0], big[1], 1.0, None)
    assert L.gs_set_resolution(r._ctx.handle, w, h) == _lib.GS_OK
    n3, g3 = r.photometricLoss(rgba, target, 0.2, BG)
    assert np.array_equal(bits(n0), bits(n3)) and np.array_equal(bits(g0), bits(g3))


def test_bits_are_reproducible_many_tiles(contexts):
    """16385 x 1 (1025 tiles: two per thread of the reduce, the last thread's slice ragged): the host form twice and the
    device form once give identical uint32 views of loss_out and of the gradient."""
    pytest.importorskip("torch")
    w, h = 16385, 1
    r = contexts(w, h)
    rgba, target = many_tile_case("noise_apart", w, h, 0.2, BG)[:2]
    n0, g0 = r.photometricLoss(rgba, target, 0.2, BG)
    n1, g1 = r.photometricLoss(rgba, target, 0.2, BG)
    assert n0.all() and np.any(g0 != 0)
    assert np.array_equal(bits(n0), bits(n1)) and np.array_equal(bits(g0), bits(g1))
    n2, g2 = device_call(r, rgba, target, 0.2, BG)
    assert np.array_equal(bits(n0), bits(n2)) and np.array_equal(bits(g0), bits(g2))


# ---- 4. known answers -----------------------------------------------------------------------------------------------------

ODD_TILES = {"first": lambda tiles, per: 0, "last": lambda tiles, per: tiles - 1, "per-1": lambda tiles, per: per - 1,
             "per": lambda tiles, per: per, "tiles-2": lambda tiles, per: tiles - 2}


@pytest.mark.parametrize("odd", list(ODD_TILES))
@pytest.mark.parametrize("w,h", [(16385, 1), (32769, 2)], ids=["16385x1", "32769x2"])
def test_l1_exact_many_tiles(contexts, w, h, odd):
    """A known answer for the sum over the tiles, with no reference and no tolerance beyond the last rounding: lambda = 0,
    no background, G = 0.5 everywhere, I - G = 0.25 everywhere but in one whole tile, where it is 0.5.  Every |I - G|, every
    tile's sum (12 or 24 per 16 pixels) and every partial sum of them is exact in float and in double, so L1 is
    float32(sum / (3 W H)) to 1 ulp (the kernel multiplies by the rounded reciprocal) and the loss is L1.  The odd tile is
    the first, the last (one pixel wide), the last of the first thread's slice of `per` tiles, the first of the second
    thread's, and the last but one: a dropped or doubled tile is 0.25 or 0.5 per value of it away, and which one says where."""
    grid_w, grid_h = (w + 15) // 16, (h + 15) // 16
    tiles = grid_w * grid_h
    per = (tiles + 1023) // 1024
    assert tiles > 1024 and per > 1
    tile = ODD_TILES[odd](tiles, per)
    tx, ty = tile % grid_w, tile // grid_w
    diff = np.full((h, w, 3), 0.25, np.float32)
    diff[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16] = 0.5
    in_tile = int(np.count_nonzero(diff == 0.5))
    assert in_tile == 3 * min(16, w - tx * 16) * min(16, h - ty * 16) > 0
    target = np.full((h, w, 3), 0.5, np.float32)
    rgba = np.zeros((h, w, 4), np.float32)
    rgba[..., :3] = target + diff                                   # 0.75 and 1.0: exact
    expected_sum = 0.25 * (3 * w * h - in_tile) + 0.5 * in_tile
    want = np.float32(expected_sum / (3 * w * h))
    n, g = contexts(w, h).photometricLoss(rgba, target, 0.0, None)
    print(f"{w}x{h} tile {tile} of {tiles} (per {per}): L1 {n[1]!r}, expected {want!r}")
    assert abs(np.float64(n[1]) - np.float64(want)) <= np.spacing(want), (tile, n, want)
    assert bits(n[:1]) == bits(n[1:2])
    assert np.array_equal(g[..., :3], np.full((h, w, 3), np.float32(1.0 / (3 * w * h)))) and not bits(g[..., 3]).any()


def test_identical_images(contexts):
    """I == G, lambda = 0.2: all three numbers <= 1e-6 and an rgb gradient of at most 1e-6 / (3 H W) in magnitude, with and
    without a background (the kernel gives zeros exactly without one)."""
    for w, h in ((5, 3), (33, 17)):
        r = contexts(w, h)
        _, target = make_inputs("noise", w, h, SEED, None)
        rgba = np.zeros((h, w, 4), np.float32)
        rgba[..., :3] = target
        n, g = r.photometricLoss(rgba, target, 0.2, None)
        assert np.all(np.abs(n) <= 1e-6) and np.abs(g[..., :3]).max() <= 1e-6 / (3 * h * w)
        assert not bits(n).any() and not (bits(g) & 0x7FFFFFFF).any()
        rgba[..., 3] = 1.0                                           # opaque: the background does not show
        n, g = r.photometricLoss(rgba, target, 0.2, BG)
        assert np.all(np.abs(n) <= 1e-6) and np.abs(g[..., :3]).max() <= 1e-6 / (3 * h * w)


def test_lambda_zero_gives_the_sign(contexts):
    """lambda = 0: the rgb gradient is exactly +-1 / (3 H W) or 0, the sign of I - G; L1 is the loss."""
    for w, h in ((5, 3), (33, 17)):
        r = contexts(w, h)
        rgba, target = make_inputs("noise", w, h, SEED, None)
        rgba[0, 0, :3] = target[0, 0]                                # one pixel with I == G
        n, g = r.photometricLoss(rgba, target, 0.0, None)
        unit = np.float32(1.0 / (3 * h * w))
        want = np.sign(rgba[..., :3] - target).astype(np.float32) * unit
        assert np.array_equal(g[..., :3], want) and not g[0, 0].any() and not bits(g[..., 3]).any()
        assert n[0] == n[1]


def test_loss_only_writes_no_gradient(contexts):
    """grad_rgba32f == NULL: the same loss_out bits, and nothing but the three numbers is written -- they sit in the middle
    of a canary-filled buffer; a call with a gradient writes exactly H * W * 4 floats of its canary-filled buffer."""
    torch = pytest.importorskip("torch")
    w, h = 33, 17
    r = contexts(w, h)
    rgba, target = make_inputs("near", w, h, SEED, None)
    n0, g0 = r.photometricLoss(rgba, target, 0.2, None)
    n1, none = r.photometricLoss(rgba, target, 0.2, None, want_grad=False)
    assert none is None and np.array_equal(bits(n0), bits(n1))
    canary, guard, px4 = -12345.5, 64, h * w * 4
    t_rgba, t_target = torch.tensor(rgba, device="cuda"), torch.tensor(target, device="cuda")
    numbers = torch.full((guard + 3 + guard,), canary, device="cuda")
    grad = torch.full((guard + px4 + guard,), canary, device="cuda")
    torch.cuda.synchronize()
    r.photometricLossDevice(t_rgba.data_ptr(), t_target.data_ptr(), 0.2, None, numbers.data_ptr() + 4 * guard, None)
    r.synchronize()
    out = numbers.cpu().numpy()
    assert np.all(out[:guard] == canary) and np.all(out[guard + 3:] == canary)
    assert np.array_equal(bits(out[guard:guard + 3]), bits(n0))
    assert np.all(grad.cpu().numpy() == canary)
    r.photometricLossDevice(t_rgba.data_ptr(), t_target.data_ptr(), 0.2, None, numbers.data_ptr() + 4 * guard,
                            grad.data_ptr() + 4 * guard)
    r.synchronize()
    out = grad.cpu().numpy()
    assert np.all(out[:guard] == canary) and np.all(out[guard + px4:] == canary)
    assert np.array_equal(bits(out[guard:guard + px4]), bits(g0).reshape(-1))


# ---- 5. the zero-copy path ------------------------------------------------------------------------------------------------

def test_zero_copy_path():
    """small_scene with GS_OUTPUT_RGBA32F enabled: rgba32f == NULL gives the bits of passing gs_output_device's pointer, and
    of the host form fed with gs_read_output -- by the host form and by the device form."""
    pytest.importorskip("torch")
    aos, w, h = small_scene()
    sc = make_scene(aos, w, h)
    r = make_renderer(sc, w, h)
    r.setOutputs(rgba32f=True)
    r.draw(sc)
    _, target = make_inputs("noise", w, h, SEED, None)
    frame = r.readOutput(_lib.GS_OUTPUT_RGBA32F)
    assert frame[..., 3].max() > 0.5
    n_host, g_host = r.photometricLoss(frame, target, 0.2, BG)
    n_null, g_null = r.photometricLoss(None, target, 0.2, BG)
    n_dnull, g_dnull = device_call(r, None, target, 0.2, BG)
    import torch
    t_target, numbers = torch.tensor(target, device="cuda"), torch.zeros(3, device="cuda")
    grad = torch.zeros(h, w, 4, device="cuda")
    torch.cuda.synchronize()
    r.photometricLossDevice(r.outputDevicePtr(_lib.GS_OUTPUT_RGBA32F), t_target.data_ptr(), 0.2, BG, numbers.data_ptr(),
                            grad.data_ptr())
    r.synchronize()
    r.cleanup()
    for n, g in ((n_null, g_null), (n_dnull, g_dnull), (numbers.cpu().numpy(), grad.cpu().numpy())):
        assert np.array_equal(bits(n), bits(n_host)) and np.array_equal(bits(g), bits(g_host))
    assert np.any(g_host[..., 3] != 0)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------

def test_api_refusals(contexts):
    """GS_ERR_INVALID with a message, nothing enqueued (the canary-filled outputs stay as they are), and a valid call
    afterwards still gives the reference's bits of before."""
    w, h = 33, 17
    L = _lib.lib()
    r = contexts(w, h)
    ctx = r._ctx.handle
    rgba, target = make_inputs("noise", w, h, SEED, None)
    n0, g0 = r.photometricLoss(rgba, target, 0.2, None)
    numbers, grad = np.full(3, -7.5, np.float32), np.full((h, w, 4), -7.5, np.float32)
    bgv = np.asarray(BG, np.float32)

    def refused(what, rgba_p, target_p, lam, bg_p, loss_p, grad_p, both=True):
        for fn in (L.gs_photometric_loss, L.gs_photometric_loss_device) if both else (L.gs_photometric_loss,):
            assert fn(ctx, rgba_p, target_p, lam, bg_p, loss_p, grad_p) == _lib.GS_ERR_INVALID, what
            assert what.encode() in L.gs_last_error(ctx), (what, L.gs_last_error(ctx))
        assert np.all(numbers == -7.5) and np.all(grad == -7.5), what

    refused("null target_rgb or loss_out", p(rgba), None, 0.2, None, p(numbers), p(grad))
    refused("null target_rgb or loss_out", p(rgba), p(target), 0.2, None, None, p(grad))
    for lam in (-0.01, 1.01, float("nan"), float("inf")):
        refused("lambda", p(rgba), p(target), lam, None, p(numbers), p(grad))
    for bad in (float("nan"), float("inf")):
        b = bgv.copy()
        b[1] = bad
        refused("bg must be finite", p(rgba), p(target), 0.2, p(b), p(numbers), p(grad))
    refused("must not be the image", p(grad), p(target), 0.2, None, p(numbers), p(grad))
    # the NULL form: the conditions of gs_output_device
    refused("not enabled", None, p(target), 0.2, None, p(numbers), p(grad))
    r.setOutputs(rgba32f=True)
    refused("no frame rendered", None, p(target), 0.2, None, p(numbers), p(grad))
    r.setOutputs()
    with pytest.raises(ValueError):
        r.photometricLoss(rgba[:-1], target)
    with pytest.raises(ValueError):
        r.photometricLoss(rgba, target[:, :-1])
    with pytest.raises(ValueError):
        r.photometricLoss(rgba, target, bg=(1.0, 2.0))
    # a subset of the tile rows
    r.setTileRows(0, 1)
    refused("a subset of the tile rows", p(rgba), p(target), 0.2, None, p(numbers), p(grad))
    r.setTileRows(0, r.sceneInfo().tiles_y)
    n1, g1 = r.photometricLoss(rgba, target, 0.2, None)
    assert np.array_equal(bits(n0), bits(n1)) and np.array_equal(bits(g0), bits(g1))
    # no resolution set: a context with a scene and nothing else
    ctx2 = C.c_void_p()
    assert L.gs_create(None, C.byref(ctx2)) == _lib.GS_OK
    aos = np.ascontiguousarray(gs.makeGaussian((0.0, 0.0, 2.0), (0.1, 0.1, 0.1))[None], dtype=np.float32)
    assert L.gs_upload_gaussians(ctx2, p(aos), 1) == _lib.GS_OK
    for fn in (L.gs_photometric_loss, L.gs_photometric_loss_device):
        assert fn(ctx2, p(rgba), p(target), 0.2, None, p(numbers), p(grad)) == _lib.GS_ERR_INVALID
        assert b"gs_set_resolution not called" in L.gs_last_error(ctx2)
    assert L.gs_destroy(ctx2) == _lib.GS_OK
    assert np.all(numbers == -7.5) and np.all(grad == -7.5)


def test_fast_contexts_are_allowed(contexts):
    """A GS_RENDER_FAST context computes the same bits: the loss does not ask how the image was made."""
    w, h = 33, 17
    rgba, target = make_inputs("noise", w, h, SEED, BG)
    n0, g0 = contexts(w, h).photometricLoss(rgba, target, 0.2, BG)
    n1, g1 = contexts(w, h, mode=gs.GS_RENDER_FAST).photometricLoss(rgba, target, 0.2, BG)
    assert np.array_equal(bits(n0), bits(n1)) and np.array_equal(bits(g0), bits(g1))


def test_sharded_context_is_refused():
    """A context whose rows gs_dist_shard_rows has dealt (world size 1: it owns every row, so this refusal and no other
    answers) is refused by both forms; in a child process, which alone holds the communicator."""
    code = textwrap.dedent("""
        import ctypes as C
        import numpy as np
        from vk3dgaussiansplatting_amd import _lib, makeGaussian
        _lib.preload_rccl()
        L = _lib.lib()
        w, h = 33, 17
        aos = np.ascontiguousarray(makeGaussian((0.0, 0.0, 2.0), (0.1, 0.1, 0.1))[None], dtype=np.float32)
        ctx = C.c_void_p()
        assert L.gs_create(None, C.byref(ctx)) == 0
        assert L.gs_upload_gaussians(ctx, aos.ctypes.data, 1) == 0 and L.gs_set_resolution(ctx, w, h) == 0
        rgba, target = np.zeros((h, w, 4), np.float32), np.full((h, w, 3), 0.5, np.float32)
        numbers, grad = np.full(3, -7.5, np.float32), np.full((h, w, 4), -7.5, np.float32)
        args = (rgba.ctypes.data, target.ctypes.data, 0.2, None, numbers.ctypes.data, grad.ctypes.data)
        assert L.gs_photometric_loss(ctx, *args) == 0 and numbers[1] == 0.5
        numbers[:] = -7.5; grad[:] = -7.5
        ident = C.create_string_buffer(_lib.DIST_UNIQUE_ID_BYTES)
        assert L.gs_dist_unique_id(ident) == 0 and L.gs_dist_init(ctx, ident, 0, 1) == 0, L.gs_last_error(ctx)
        assert L.gs_dist_shard_rows(ctx, _lib.ROWS_CONTIGUOUS) == 0, L.gs_last_error(ctx)
        for fn in (L.gs_photometric_loss, L.gs_photometric_loss_device):
            assert fn(ctx, *args) == _lib.GS_ERR_INVALID and b"sharded context" in L.gs_last_error(ctx)
        assert np.all(numbers == -7.5) and np.all(grad == -7.5)
        assert L.gs_destroy(ctx) == 0
        print("refused-ok")
    """)
    from conftest import ROOT
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "refused-ok" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])


# ---- 7. end to end --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_torch_autograd_end_to_end(sparse):
    """autograd.photometric_loss(autograd.render(records), target).backward() on small_scene: records.grad is bit-identical
    to Renderer.backward(grad) with grad from Renderer.photometricLoss of the same frame; with sparse_grad=True its rows are
    those rows and every other row of the dense gradient is zero."""
    torch = pytest.importorskip("torch")
    from vk3dgaussiansplatting_amd import autograd
    aos, w, h = small_scene()
    cam = make_scene(aos, w, h).getCamera()
    view, proj, pos = cam.getViewMatrix(), cam.getProjectionMatrix(), cam.getPosition()
    _, target = make_inputs("noise", w, h, SEED, None)
    r = autograd.make_renderer(w, h)
    records = torch.tensor(aos, device="cuda", requires_grad=True)
    rgba = autograd.render(records, view, proj, pos, 0, renderer=r, sparse_grad=sparse)
    loss = autograd.photometric_loss(rgba, torch.tensor(target, device="cuda"), 0.2, BG, renderer=r)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    numbers, grad = r.photometricLoss(rgba.detach().cpu().numpy(), target, 0.2, BG)
    assert np.array_equal(bits(numbers[:1]), bits(loss.detach().cpu().numpy().reshape(1)))
    dense = r.backward(grad)
    assert np.any(dense != 0)
    if sparse:
        got = records.grad              # as the library wrote it: coalescing adds the rows to zeros, and -0.0 + 0.0 is +0.0
        ids, rows = got._indices()[0].cpu().numpy(), got._values().cpu().numpy()
        assert got.is_sparse and np.all(np.diff(ids) > 0)
        assert np.array_equal(bits(rows), bits(dense[ids]))
        rest = np.ones(len(dense), bool)
        rest[ids] = False
        assert not bits(dense[rest]).any()
    else:
        assert np.array_equal(bits(records.grad.cpu().numpy()), bits(dense))
    # the upstream scalar multiplies the kernel's gradient
    rgba2 = rgba.detach().clone().requires_grad_(True)
    (3.0 * autograd.photometric_loss(rgba2, torch.tensor(target, device="cuda"), 0.2, BG, renderer=r)).backward()
    assert np.array_equal(rgba2.grad.cpu().numpy(), np.float32(3.0) * grad)
    r.cleanup()
