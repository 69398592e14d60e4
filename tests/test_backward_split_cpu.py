"""The backward's two numerical stages, each with a float64 reference of its own and a scale that belongs to the splat (on
the CPU; tests/test_backward_split_gpu.py runs the kernels against them).

  rows   k_bwd_blend leaves one 10-float row per list element; gs_debug_read(GS_BUF_BACKWARD_ROWS) returns their sum per
         splat (dsx, dsy, dix, diy, diz, dcol[3], dop, dz: the input of bwd_chain).  rows_reference is the tile walk and blend
         of tests/frame64.py (pair_terms) with a zero offset per (list element, pixel) on all ten splat values -- where
         test_absgrad_cpu.abs_screen_gradient has it on the screen position alone -- evaluated on the float32 frame's own
         values (raster32, constants): `signed` is the row sum, `absolute` the same per-pixel terms summed as abs(), the scale
         an error of the blend is measured against.
  chain  bwd_chain takes a splat's row through the per-splat part of the frame.  chain64 is the vector-Jacobian product of
         the ten splat values against given rows, by autograd through frame64.splat_values, the per-splat stage every
         reference shares (here with the camera per splat, any of the five SH modes, the anti-aliasing factor, the number
         format and the branches as arguments); chain_scale is S = sum_j |d value_j / d field| |row_j|, the majorant of the
         rounding of a float32 matrix-vector product, with the sum of the absolute monomials of b_k in place of |b_k| for the
         SH coefficient fields (a basis function that cancels to nearly zero would understate the scale).  camera=True gives
         both the twin for the 35 camera floats, per splat (the tests sum them over the splats), and its scale.

Calibration: both references run once more in torch float32 on the same inputs with the same decisions; the worst
|ref32 - ref64| / scale over the designed scenes is recorded below and each GPU tier is asserted to be at least twice it, so
no tier is fitted to a kernel.  Measured here (test_calibration prints them; the constants are the row maxima, rounded up):

  stage   statistic  ragged   dense    @pose    @garden  extreme  truncated  batch_edges  subpixel  clamp
  rows    median     2.8e-8   1.7e-8   2.9e-8   2.8e-8   3.1e-8   1.5e-8     8.4e-8       2.3e-8    2.8e-8
  rows    max        6.8e-6   4.6e-7   2.4e-6   1.5e-6   5.8e-7   5.2e-7     1.4e-6       1.2e-6    9.4e-7
  chain   median     5.1e-8   5.3e-8   5.6e-8   5.2e-8   5.0e-8   6.1e-8     4.2e-8       4.6e-8    5.1e-8
  chain   99.9th     1.4e-6   3.5e-6   1.5e-6   1.5e-6   1.4e-6   1.3e-6     4.3e-7       9.9e-7    9.8e-7
  chain   max        1.2e-4   9.6e-6   4.2e-5   6.4e-5   2.1e-5   2.8e-6     7.1e-7       3.5e-6    7.1e-6
  chain   share above 8 x CHAIN_REF32_P999
                     1.2e-5   0        6.0e-6   1.2e-5   0        0          0            0         0
  camera  max        1.3e-8   2.6e-7   1.4e-8   1.8e-8   7.5e-8   8.4e-8     2.1e-8       3.5e-8    2.2e-8

The chain under the other SH modes and with the anti-aliasing factor (test_calibration_of_the_chain_variants, rows of the
mode-0 frame): 99.9th percentile 2.2e-6, 4.2e-6, 2.1e-6, 3.0e-6 in modes 1, 2, 4, 5 of `ragged` (max 1.2e-4 in each; the
fewer SH entries a mode has, the more the geometry fields weigh); anti-aliased `ragged`, `ragged@pose`, `subpixel`: 1.5e-6,
1.5e-6, 5.8e-7 (max 6.7e-5, 2.4e-5, 1.6e-6); the largest share above 8 x CHAIN_REF32_P999 is 4.9e-5, in mode 2, a quarter
of the 2e-4 the float32 reference is allowed.  CHAIN_REF32_P999 is mode 2's.

With the monomial scale the chain's tail does not sit in the SH fields, but it does not vanish: what is left (every entry
above 2e-5) is in the scale fields of distant splats a fraction of a pixel wide, where d(ix, iy, iz) / d(scale) cancels
inside the 2-D covariance, below what a sum over the ten values can see.  So the chain keeps two tiers:
every entry within 8 x CHAIN_REF32_MAX, at most 0.1 % of them above 8 x CHAIN_REF32_P999.

Power (test_power): the four wrong-term variants of chain64 -- one term's derivative scaled by 0.9 -- against chain64 on
the same rows: splats with an entry above CHAIN_P999_TIER * S / above CHAIN_TIER * S / splats changed, and the changed
entries today's criterion (2e-2 |ref| + 2e-3 max|ref column|, test_backward_gpu.compare_with_reference) rejects:

  variant        ragged, mode 0                   ragged, mode 1                   dense, mode 0
  sh_direction   2723 / 700 / 2890,  1 of 8670    2240 / 556 / 2539,  3 of 7617    129 / 124 / 129, 15 of 387
  whole_J        2855 / 1638 / 2890, 54 of 7310   2875 / 1653 / 2890, 45 of 7310   129 / 128 / 129, 28 of 290
  J02            2617 / 898 / 2890,  17 of 5107   2611 / 904 / 2890,  17 of 5107   129 / 116 / 129, 12 of 205
  view_depth     2776 / 820 / 2890,  0 of 2890    2798 / 962 / 2890,  0 of 2890    123 / 69 / 129,  1 of 129
"""
import numpy as np
import pytest

from test_outputs_cpu import oracle_params
from test_backward_cpu import batch_edge_scene, frozen_of, truncated_scene
from frame64 import (DECISIONS, FLOOR, WRONG_TERMS, camera_leaves, frame_decisions, frame_values32, live_of, pair_terms,
                     reference_gradient, sh_basis, sh_monomials, sh_range, splat_values, weights)
from test_absgrad_cpu import abs_screen_gradient, splat_values64
from test_antialias_cpu import load_antialias_scene
from test_camera_constants_cpu import clamp_masks, with_constants
from test_backward_camera_cpu import PROJ_CLIP_Z, VIEW_BOTTOM_ROW

torch = pytest.importorskip("torch")

GEOMETRY = [0, 1, 2, 4, 5, 6, 8, 9, 10, 11]

# ---- the calibrated constants (test_calibration re-measures them and fails when one no longer covers its measurement) ------
ROWS_REF32_MAX = 7.0e-6
CHAIN_REF32_MAX = 1.3e-4
CHAIN_REF32_P999 = 4.3e-6
CAMERA_REF32_MAX = 3.0e-7
# what the GPU tests allow: per entry |gpu - reference| <= tier * scale
ROWS_TIER = 16.0 * ROWS_REF32_MAX
CHAIN_TIER = 8.0 * CHAIN_REF32_MAX
CHAIN_P999_TIER = 8.0 * CHAIN_REF32_P999          # ... and at most 0.1 % of the compared entries above this one


def read_fields(sh_mode):
    k_lo, k_hi = sh_range(sh_mode)
    return GEOMETRY + [15] + [12 + 4 * k + c for k in range(k_lo, k_hi) for c in range(3)]


# ---- the chain -----------------------------------------------------------------------------------------------------------------

CAMERA_UNWRITTEN = VIEW_BOTTOM_ROW + PROJ_CLIP_Z          # of the 35 floats (test_backward_camera_cpu.py)


def _pack_camera(gV, gP, gcam):
    """Per-splat [n, 35] from gradients laid out as camera_leaves: view and proj column-major as gs_render takes them, the
    entries gs_camera.hip never writes (the view taken as affine, clip z unread) zeroed."""
    out = torch.cat([gV.transpose(1, 2).reshape(-1, 16), gP.transpose(1, 2).reshape(-1, 16), gcam], 1).numpy().astype(np.float64)
    out[:, CAMERA_UNWRITTEN] = 0.0
    return out


def _listed(rows):
    return np.flatnonzero(np.asarray(rows).any(1))


def _sub(dec, sel):
    return None if dec is None else {k: np.asarray(v)[sel] for k, v in dec.items()}


def chain64(p, aos, ref, rows, dtype=torch.float64, antialias=False, dec=None, wrong=None, camera=False):
    """[N, 84]: the vector-Jacobian product of the ten splat values against rows [N, 10], by autograd through splat_values
    in `dtype`; a splat with an all-zero row is exactly zero (it does not enter).  camera=True: also the per-splat camera
    terms [N, 35] (view[16], proj[16], cam_pos[3] as gs_backward_camera orders them)."""
    sel = _listed(rows)
    n = len(aos)
    out, cam_out = np.zeros((n, 84)), np.zeros((n, 35))
    if len(sel):
        rec = torch.tensor(np.asarray(aos, np.float64)[sel], dtype=dtype, requires_grad=True)
        cams = camera_leaves(p, len(sel), dtype, grad=camera)
        vals, _ = splat_values(p, rec, live_of(ref)[sel], cams, _sub(dec, sel), antialias, wrong)
        (vals * torch.tensor(np.asarray(rows, np.float64)[sel], dtype=dtype)).sum().backward()
        out[sel] = rec.grad.numpy().astype(np.float64)
        if camera:
            cam_out[sel] = _pack_camera(*(t.grad for t in cams))
    return (out, cam_out) if camera else out


def chain_scale(p, aos, ref, rows, antialias=False, dec=None, camera=False):
    """S [N, 84] = sum_j |d value_j / d field| |row_j| in float64 (ten one-hot vector-Jacobian products), with the absolute
    monomials of b_k for the SH coefficient fields; camera=True: also the per-splat camera scale [N, 35]."""
    sel = _listed(rows)
    n = len(aos)
    S, Scam = np.zeros((n, 84)), np.zeros((n, 35))
    if not len(sel):
        return (S, Scam) if camera else S
    rec = torch.tensor(np.asarray(aos, np.float64)[sel], requires_grad=True)
    cams = camera_leaves(p, len(sel), grad=camera)
    vals, aux = splat_values(p, rec, live_of(ref)[sel], cams, _sub(dec, sel), antialias)
    arow = np.abs(np.asarray(rows, np.float64)[sel])
    s, scam = np.zeros((len(sel), 84)), np.zeros((len(sel), 35))
    for j in range(10):
        g = torch.autograd.grad(vals[:, j].sum(), (rec,) + (cams if camera else ()), retain_graph=True, allow_unused=True)
        s += np.abs(g[0].numpy()) * arow[:, j:j + 1]
        if camera:
            z = [torch.zeros_like(t) if gi is None else gi for gi, t in zip(g[1:], cams)]
            scam += np.abs(_pack_camera(*z)) * arow[:, j:j + 1]
    mono = sh_monomials(aux["dirs"]).numpy()
    k_lo, k_hi = sh_range(p.sh_mode)
    for k in range(k_lo, k_hi):
        for c in range(3):
            s[:, 12 + 4 * k + c] = mono[:, k] * arow[:, 5 + c] * aux["colour"][:, c]
    S[sel], Scam[sel] = s, scam
    return (S, Scam) if camera else S


def decisions64(p, aos, ref, antialias=False):
    """The branches splat_values takes in float64, as `dec` for a run in another number format."""
    with torch.no_grad():
        _, aux = splat_values(p, torch.tensor(np.asarray(aos, np.float64)), live_of(ref), antialias=antialias)
    return {k: aux[k] for k in DECISIONS if k in aux}


# ---- the rows ------------------------------------------------------------------------------------------------------------------

def rows_reference(p, aos, ref, flags, w_rgba, w_depth=None, dtype=torch.float64, values=None, leaves=False):
    """(signed [N, 10], absolute [N, 10]) in float64 of L = sum w_rgba * RGBA32F + sum w_depth * depth: frame64.pair_terms
    with the zero offset per (list element, pixel) on all ten splat values, on `values` [N, 10] (default: frame_values32, the
    float32 frame's own, as constants), computed in `dtype`.  leaves=True: a third array, the plain autograd gradient of L
    w.r.t. `values` as one leaf."""
    n = len(aos)
    vals = torch.tensor(frame_values32(p, aos, ref) if values is None else np.asarray(values, np.float64), dtype=dtype,
                        requires_grad=leaves)
    absolute = torch.zeros(n, 10, dtype=torch.float64)
    signed = torch.zeros(n, 10, dtype=torch.float64)
    for g, grad in pair_terms(p, vals, ref, flags, w_rgba, w_depth):
        grad = grad.to(torch.float64)
        absolute.index_add_(0, g, grad.abs().sum(1))
        signed.index_add_(0, g, grad.sum(1))
    out = (signed.numpy(), absolute.numpy())
    return out + (vals.grad.numpy().astype(np.float64),) if leaves else out


# ---- the designed scenes (shared with tests/test_backward_split_gpu.py) ----------------------------------------------------------

CLAMP_CONSTANTS = dict(in_view_limit=0.35)


def clamp_scene():
    """96 x 64, 500 splats of the fog under in_view_limit = 0.35 (the clamp of getCovarianceMatrix at |x / z| > 0.525 and
    |y / z| > 0.35, well inside the frame's +-1.5 and +-1): emitting splats on the x clamp, on the y clamp and on neither."""
    from vk3dgaussiansplatting_amd import synth
    return synth.generate(500, 96, 64, -2.0, seed=57), 96, 64


ALL_SCENES = ("ragged", "dense", "ragged@pose", "ragged@garden", "extreme", "truncated", "batch_edges", "subpixel", "clamp")


def load_split_scene(oracle, name):
    """(aos, w, h, cam, constants) of a designed scene by name."""
    if name == "truncated":
        return truncated_scene() + ({}, {})
    if name == "batch_edges":
        return batch_edge_scene(oracle)[:3] + ({}, {})
    if name == "clamp":
        return clamp_scene() + ({}, CLAMP_CONSTANTS)
    return load_antialias_scene(oracle, name) + ({},)


_FRAMES = {}


def split_frame(oracle, tmp_dir, name, sh_mode=0, seed=1, with_depth=True):
    """dict(aos, w, h, cam, constants, p, ref, flags, wr, wd, signed, absolute) of a designed scene: the oracle's frame, the
    float32 frame's decisions, the loss weights of seed `seed` and rows_reference, computed once.  Shared: do not write."""
    key = (name, sh_mode, seed, with_depth)
    if key not in _FRAMES:
        aos, w, h, cam, constants = load_split_scene(oracle, name)
        p = with_constants(oracle_params(oracle, w, h, sh_mode, **cam), constants)
        ref, flags = frame_decisions(tmp_dir, p, aos)
        wr, wd = weights(h, w, seed)
        wd = wd if with_depth else None
        signed, absolute = rows_reference(p, aos, ref, flags, wr, wd)
        _FRAMES[key] = dict(aos=aos, w=w, h=h, cam=cam, constants=constants, p=p, ref=ref, flags=flags, wr=wr, wd=wd,
                            signed=signed, absolute=absolute)
    return _FRAMES[key]


def emitting_of(ref):
    m = np.zeros(len(ref["stage1"]["cov"]), bool)
    m[np.asarray(ref["id"])[:ref["e"]]] = True
    return m


def ratio_of(err, scale):
    """|err| / scale where scale > 0 (and the assertion that err is exactly zero elsewhere)."""
    assert not err[scale == 0].any()
    return np.abs(err[scale > 0]) / scale[scale > 0]


# ---- tests: composition ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["ragged", "dense"])
def test_composition(oracle_mod, tmp_path, scene):
    """The split reference is the whole one: chain64 of the rows taken at the float64 splat values equals reference_gradient
    to 1e-12 of each column's scale; the widened offsets reproduce the plain autograd rows to 1e-13 of the column's scale;
    columns 0-1 of rows_reference on the frame's own values are abs_screen_gradient's signed and absolute pairs; absolute >=
    |signed| everywhere, and both are exactly zero outside the emitting splats."""
    f = split_frame(oracle_mod, tmp_path, scene)
    p, aos, ref, flags, wr, wd = (f[k] for k in ("p", "aos", "ref", "flags", "wr", "wd"))
    with torch.no_grad():
        sx, sy, ix, iy, iz, col, opac, zview = splat_values64(p, torch.tensor(aos.astype(np.float64)), ref)
        v64 = torch.stack([sx, sy, ix, iy, iz, col[:, 0], col[:, 1], col[:, 2], opac, zview], 1).numpy()
        mine, _ = splat_values(p, torch.tensor(aos.astype(np.float64)), live_of(ref))
    em = emitting_of(ref)
    assert np.all(np.abs(mine.numpy() - v64)[em] <= 1e-12 * np.abs(v64[em]).max(0))        # the restatement is splat_values64
    signed64, absolute64, plain = rows_reference(p, aos, ref, flags, wr, wd, values=mine.numpy(), leaves=True)
    cs = np.abs(plain).max(0)
    assert np.all(np.abs(signed64 - plain) <= 1e-13 * cs), np.abs(signed64 - plain).max(0) / cs
    want = reference_gradient(p, aos, ref, flags, wr.astype(np.float64), wd.astype(np.float64))
    got = chain64(p, aos, ref, signed64)
    scale = np.abs(want).max(0)
    worst = (np.abs(got - want).max(0) / np.maximum(scale, 1e-300)).max()
    print(f"{scene}: chain64(rows64) against reference_gradient, worst column {worst:.1e}; offsets against leaves "
          f"{(np.abs(signed64 - plain).max(0) / cs).max():.1e}")
    assert np.all(np.abs(got - want) <= 1e-12 * scale)
    ab, sg = abs_screen_gradient(p, aos, ref, flags, wr, wd, frozen=np.ones(len(aos), bool))
    for mine2, theirs in ((f["signed"][:, :2], sg), (f["absolute"][:, :2], ab)):      # (a product summed in another order)
        assert np.all(np.abs(mine2 - theirs) <= 1e-13 * np.abs(theirs).max(0)), np.abs(mine2 - theirs).max(0)
    assert np.all(f["absolute"] >= np.abs(f["signed"]))
    assert not f["absolute"][~emitting_of(ref)].any() and np.count_nonzero(f["absolute"].any(1)) > 100


def test_monomial_scale_bounds_the_basis():
    """sh_monomials >= |b_k| on random directions, equal for the single-monomial functions, and at least ten times |b_k|
    somewhere for every function that can cancel (6, 8, 9, 11, 12, 13, 14, 15)."""
    rng = np.random.default_rng(3)
    d = torch.tensor(rng.standard_normal((20000, 3)))
    d = d / torch.sqrt((d * d).sum(1, keepdim=True))
    b, m = sh_basis(d).abs().numpy(), sh_monomials(d).numpy()
    assert np.all(m >= b * (1 - 1e-12))
    single = [0, 1, 2, 3, 4, 5, 7, 10]
    assert np.allclose(m[:, single], b[:, single], rtol=1e-12, atol=0)
    for k in (6, 8, 9, 11, 12, 13, 14, 15):
        assert np.any(m[:, k] > 10 * b[:, k]), k


# ---- tests: calibration ------------------------------------------------------------------------------------------------------

_CALIBRATION = {}


def calibrate(oracle, tmp_dir, scene):
    """The float32 run of each reference against its float64 run on a designed scene: dict(rows, chain, camera) of
    |ref32 - ref64| / scale arrays (rows per entry with absolute > 0; chain per entry with S > 0; camera 35 entries)."""
    if scene not in _CALIBRATION:
        f = split_frame(oracle, tmp_dir, scene)
        p, aos, ref = f["p"], f["aos"], f["ref"]
        s32, _ = rows_reference(p, aos, ref, f["flags"], f["wr"], f["wd"], dtype=torch.float32)
        rows = f["signed"].astype(np.float32).astype(np.float64)       # what a kernel hands on: float32 rows
        keep = ~frozen_of(scene, aos)
        dec = decisions64(p, aos, ref)
        g64, c64 = chain64(p, aos, ref, rows, camera=True)
        g32, c32 = chain64(p, aos, ref, rows, dtype=torch.float32, dec=dec, camera=True)
        S, Scam = chain_scale(p, aos, ref, rows, camera=True)
        _CALIBRATION[scene] = dict(rows=ratio_of(s32 - f["signed"], f["absolute"]),
                                   chain=ratio_of((g32 - g64)[keep], S[keep]),
                                   camera=ratio_of(c32[keep].sum(0) - c64[keep].sum(0), Scam[keep].sum(0)))
    return _CALIBRATION[scene]


@pytest.mark.parametrize("scene", ALL_SCENES)
def test_calibration(oracle_mod, tmp_path, scene):
    """A float32 run of each reference stays under the recorded constants, which are at most half of the GPU tiers (by
    their definition 1/16 and 1/8 of them); the chain's float32 tail above 8 x its 99.9th percentile is under a fifth of the
    0.1 % the GPU test allows."""
    c = calibrate(oracle_mod, tmp_path, scene)
    p999 = float(np.percentile(c["chain"], 99.9))
    tail = float(np.mean(c["chain"] > CHAIN_P999_TIER))
    print(f"{scene}: rows median {np.median(c['rows']):.1e} max {c['rows'].max():.1e} | chain median {np.median(c['chain']):.1e} "
          f"p99.9 {p999:.1e} max {c['chain'].max():.1e} tail {tail:.1e} | camera max {c['camera'].max():.1e}")
    assert c["rows"].max() <= ROWS_REF32_MAX <= 0.5 * ROWS_TIER
    assert c["chain"].max() <= CHAIN_REF32_MAX <= 0.5 * CHAIN_TIER
    assert p999 <= CHAIN_REF32_P999 <= 0.5 * CHAIN_P999_TIER
    assert tail <= 0.2 * 1e-3
    assert c["camera"].max() <= CAMERA_REF32_MAX


CHAIN_VARIANTS = [("ragged", m, False) for m in (1, 2, 4, 5)] + [("ragged", 0, True), ("ragged@pose", 0, True), ("subpixel", 0, True)]


@pytest.mark.parametrize("scene,sh_mode,antialias", CHAIN_VARIANTS,
                         ids=[f"{s}-sh{m}{'-antialias' if a else ''}" for s, m, a in CHAIN_VARIANTS])
def test_calibration_of_the_chain_variants(oracle_mod, tmp_path, scene, sh_mode, antialias):
    """The chain's float32 run under the other SH modes (4 and 5 included, which the oracle cannot draw: the chain takes any
    rows, here those of the mode-0 frame) and with the anti-aliasing factor (the splats within a factor 2 of its floor left
    out, as in the GPU test) stays under the same constants."""
    f = split_frame(oracle_mod, tmp_path, scene)
    aos, ref = f["aos"], f["ref"]
    p = with_constants(oracle_params(oracle_mod, f["w"], f["h"], sh_mode, **f["cam"]), f["constants"])
    rows = f["signed"].astype(np.float32).astype(np.float64)
    dec = decisions64(p, aos, ref, antialias)
    keep = np.ones(len(aos), bool)
    if antialias:
        with torch.no_grad():
            _, aux = splat_values(p, torch.tensor(aos.astype(np.float64)), live_of(ref), antialias=True)
        keep = ~((aux["ratio"] >= FLOOR / 2) & (aux["ratio"] <= 2 * FLOOR))
    g64, c64 = chain64(p, aos, ref, rows, antialias=antialias, camera=True)
    g32, c32 = chain64(p, aos, ref, rows, dtype=torch.float32, antialias=antialias, dec=dec, camera=True)
    S, Scam = chain_scale(p, aos, ref, rows, antialias=antialias, camera=True)
    chain = ratio_of((g32 - g64)[keep], S[keep])
    cam = ratio_of(c32[keep].sum(0) - c64[keep].sum(0), Scam[keep].sum(0))
    p999, tail = float(np.percentile(chain, 99.9)), float(np.mean(chain > CHAIN_P999_TIER))
    print(f"{scene} sh_mode {sh_mode}{' antialias' if antialias else ''}: chain median {np.median(chain):.1e} p99.9 {p999:.1e} "
          f"max {chain.max():.1e} tail {tail:.1e} | camera max {cam.max():.1e}")
    unread = np.setdiff1d(np.arange(84), read_fields(sh_mode))
    assert not S[:, unread].any() and not g64[:, unread].any()
    assert chain.max() <= CHAIN_REF32_MAX and p999 <= CHAIN_REF32_P999 and tail <= 0.2 * 1e-3
    assert cam.max() <= CAMERA_REF32_MAX


# ---- tests: power ------------------------------------------------------------------------------------------------------------

def todays_tolerance(want):
    """test_backward_gpu.compare_with_reference's bound per entry: 2e-2 |want| + 2e-3 max|want column|."""
    return 2e-2 * np.abs(want) + 2e-3 * np.abs(want).max(0)


@pytest.mark.parametrize("scene,sh_mode", [("ragged", 0), ("ragged", 1), ("dense", 0)])
def test_power(oracle_mod, tmp_path, scene, sh_mode):
    """The test of the test.  Each of the four wrong-term variants of chain64 (one term's derivative scaled by 0.9) puts at
    least half of the splats it changes above CHAIN_P999_TIER * S -- the GPU test allows 0.1 % of the entries there -- and
    a quarter of them above CHAIN_TIER * S, where it allows none; on `ragged` today's criterion rejects at most 1 % of the
    entries a variant changes: the gap on record (on `dense`, 129 emitting splats, it is printed).  No kernel is involved."""
    f = split_frame(oracle_mod, tmp_path, scene, sh_mode)
    p, aos, ref = f["p"], f["aos"], f["ref"]
    rows = f["signed"].astype(np.float32).astype(np.float64)
    want = chain64(p, aos, ref, rows)
    S = chain_scale(p, aos, ref, rows)
    for term in WRONG_TERMS:
        got = chain64(p, aos, ref, rows, wrong=(term, 0.9))
        err = np.abs(got - want)
        changed = err > 0
        rejected = (err > CHAIN_P999_TIER * S).any(1)
        hard = (err > CHAIN_TIER * S).any(1)
        today = err[changed] > todays_tolerance(want)[changed]
        print(f"{scene} sh_mode {sh_mode} {term}: {int(rejected.sum())} of {int(changed.any(1).sum())} changed splats above the "
              f"99.9 % tier, {int(hard.sum())} above the hard tier; today's criterion rejects {int(today.sum())} of "
              f"{int(changed.sum())} changed entries")
        assert changed.any(1).sum() >= 100
        assert rejected.sum() >= 0.5 * changed.any(1).sum()
        assert (err > CHAIN_P999_TIER * S)[S > 0].mean() > 1e-3   # ... so the GPU test's 0.1 % allowance is exceeded
        if scene == "ragged":
            assert today.mean() <= 0.01


# ---- tests: the designed scenes are what they claim ----------------------------------------------------------------------------

def test_clamp_scene_reaches_both_clamps(oracle_mod, tmp_path):
    """Among the emitting splats of clamp_scene, by the float32 decisions of bwd_chain (clamp_masks): at least 20 on the x
    clamp, 20 on the y clamp and 20 on neither; float64 takes the same branches; each group has non-zero rows."""
    f = split_frame(oracle_mod, tmp_path, "clamp")
    cx, cy = clamp_masks(f["p"], f["aos"])
    em = emitting_of(f["ref"]) & f["absolute"].any(1)
    counts = int((em & cx).sum()), int((em & cy).sum()), int((em & ~cx & ~cy).sum())
    print("clamp scene: emitting splats with non-zero rows on the x clamp, the y clamp, neither:", counts)
    assert min(counts) >= 20, counts
    dec = decisions64(f["p"], f["aos"], f["ref"])
    assert np.array_equal(dec["clamp_x"][em], cx[em]) and np.array_equal(dec["clamp_y"][em], cy[em])


@pytest.mark.parametrize("scene", ["ragged", "subpixel"])
def test_antialias_branches_are_reached(oracle_mod, scene):
    """The branches of rho the anti-aliased cases reach: `subpixel` has splats on the floor and between, `ragged` between
    only.  The third branch, the cap at 1, cannot be designed: det = (a0 + 0.3)(c0 + 0.3) - b^2 >= det0 = a0 c0 - b^2 in
    exact arithmetic and, rounding being monotone, in float32 too while both are positive, so r = det0 / det > 1 needs a
    determinant that rounding made negative -- a zero_det needle, which no by-value check compares (frozen_of).  Asserted
    here: no visible splat of either scene is on the cap, and the largest splats come within 2e-3 of it."""
    aos, w, h, cam, _ = load_split_scene(oracle_mod, scene)
    p = oracle_params(oracle_mod, w, h, **cam)
    s1 = oracle_mod.init_sort_list(p, aos)
    dec = decisions64(p, aos, dict(stage1=s1), antialias=True)
    with torch.no_grad():
        _, aux = splat_values(p, torch.tensor(aos.astype(np.float64)), live_of(dict(stage1=s1)), antialias=True)
    vis = s1["splats"]["visible"] != 0
    between = vis & ~dec["floored"] & ~dec["capped"]
    print(f"{scene}: floored {int((vis & dec['floored']).sum())}, between {int(between.sum())}, capped "
          f"{int((vis & dec['capped']).sum())}, largest ratio {aux['ratio'][vis].max():.5f}")
    assert between.sum() >= 10 and not (vis & dec["capped"]).any()
    if scene == "subpixel":
        assert (vis & dec["floored"]).sum() >= 3 and aux["ratio"][vis].max() > 0.998
