"""The float64 reference of the EXACT frame, once: the frame restated in torch -- projection, 2-D covariance and its inverse,
SH colour, the blend -- with the discrete decisions of the float32 frame held fixed (which entries each pixel blends and where
it stops: tests/host/blend_trace_ref.c, the loop of blend_outputs_ref.c that reproduces the oracle's frame byte for byte),
differentiated by torch.autograd.  Every gradient test of the library is judged against it.

  decisions    trace_lib, frame_decisions, live_of; raster32 / frame_values32: the float32 values the frame blends
  helpers      sh_basis, sh_range, sh_monomials, camera_leaves, weights, loss_of
  splat_values the per-splat stage: ten values per splat (ROW_NAMES) from its record and its own copy of the camera
  tile_walk    the tiles that blend something, each list cut behind its last blended entry
  blend        a tile's [256, 5] outputs from the values of its entries, per splat or per (list element, pixel)
  pair_terms   the gradient of zero offsets per (list element, pixel): the per-pixel terms of a splat's gradient
  forward64    the three together, and reference_gradient on top of it

The modules of the features (tests/test_*_cpu.py) add their leaves and their sums over this code and hold no copy of it.  It is
trusted by the checks of tests/test_backward_cpu.py: its RGBA32F and depth match the float32 C restatement to 1e-5, and its
gradients match its own central differences."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

ROW_NAMES = ("sx", "sy", "ix", "iy", "iz", "r", "g", "b", "op", "z")          # bwd_chain's row, raster32's keys
FLOOR = float(np.float32(2.5e-5))          # kAntialiasFloor as the kernels hold it

# ---- the decisions and the values of the float32 frame ---------------------------------------------------------------------

_TRACE = {}


def trace_lib(tmp_dir):
    if "lib" not in _TRACE:
        import oracle
        oracle.lib()
        so = os.path.join(str(tmp_dir), "libblend_trace_ref.so")
        odir = os.path.join(ROOT, "oracle")
        build = subprocess.run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", odir, "-o", so,
                                os.path.join(ROOT, "tests", "host", "blend_trace_ref.c"), "-L", odir, "-lgs_oracle",
                                f"-Wl,-rpath,{odir}", "-lm"], capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-2000:]
        R = C.CDLL(so)
        R.gsb_blend_trace.restype = None
        _TRACE["lib"] = R
    return _TRACE["lib"]


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def frame_decisions(tmp_dir, p, aos, ref=None):
    """The oracle's frame and the blend decisions of the float32 frame: flags [E, 256] (entry e adds its colour to tile
    pixel ly * 16 + lx: 1, or 2 where the pixel stops on it, nextT < 1e-4)."""
    import oracle
    aos = np.ascontiguousarray(aos, dtype=np.float32)
    if ref is None:
        ref = oracle.full_pipeline(p, aos)
    e = int(ref["e"])
    flags = np.zeros((max(e, 1), 256), np.uint8)
    trace_lib(tmp_dir).gsb_blend_trace(C.byref(p), ptr(aos), ptr(np.ascontiguousarray(ref["stage1"]["color"])),
                                       ptr(np.ascontiguousarray(ref["stage1"]["cov"])),
                                       ptr(np.ascontiguousarray(ref["id"], dtype=np.uint32)),
                                       ptr(np.ascontiguousarray(ref["ranges"], dtype=np.uint32)), ptr(flags))
    return ref, flags[:e]


def live_of(ref):
    """The det != 0 rule of the float32 frame (RenderGaussians.comp:104) from its stage-1 covariance: a splat with det == 0
    never contributes."""
    cov = np.asarray(ref["stage1"]["cov"], np.float32)
    return (cov[:, 0] * cov[:, 2] - cov[:, 1] * cov[:, 1]) != 0


def raster32(p, aos, ref):
    """Per splat, the float32 values the frame blends (as the C restatement computes them): sx, sy, ix, iy, iz, colour,
    alpha factor, z -- float64 arrays of float32 values."""
    f = np.float32
    a = np.asarray(aos, np.float32)
    view, proj = np.array(p.view, np.float32), np.array(p.proj, np.float32)

    def mul(m, v):
        out = []
        for r in range(4):
            acc = m[r] * v[0]
            for k in range(1, 4):
                acc = acc + m[k * 4 + r] * v[k]
            out.append(acc)
        return out

    one = np.ones(len(a), np.float32)
    pv = mul(view, [a[:, 0], a[:, 1], a[:, 2], one])
    q = mul(proj, pv)
    x, y = q[0] / q[3], -(q[1] / q[3])
    sx, sy = ((x + f(1)) * f(0.5)) * f(p.width), ((y + f(1)) * f(0.5)) * f(p.height)
    cov = np.asarray(ref["stage1"]["cov"], np.float32)
    det = cov[:, 0] * cov[:, 2] - cov[:, 1] * cov[:, 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = np.where(det != 0, f(1) / det, f(0)).astype(np.float32)
    ix, iy, iz = cov[:, 2] * inv, -cov[:, 1] * inv, cov[:, 0] * inv
    col = np.asarray(ref["stage1"]["color"], np.float32)
    op = np.where(det != 0, col[:, 3], f(0))
    return {k: v.astype(np.float64) for k, v in dict(sx=sx, sy=sy, ix=ix, iy=iy, iz=iz, r=col[:, 0], g=col[:, 1], b=col[:, 2],
                                                       op=op, z=-pv[2]).items()}


def stacked(r32):
    """raster32's values as one [N, 10] array in the order of ROW_NAMES."""
    return np.stack([r32[k] for k in ROW_NAMES], 1)


def frame_values32(p, aos, ref):
    """[N, 10] float64 array of the float32 values the frame blends (raster32), in the order of ROW_NAMES."""
    return stacked(raster32(p, aos, ref))


# ---- small helpers ----------------------------------------------------------------------------------------------------------

def sh_basis(d):
    """Common.glsl:94-138 on directions d [M, 3] (torch)."""
    X, Y, Z = -d[:, 0], -d[:, 1], d[:, 2]
    S1, C1 = 2.0 * X * Y, X * X - Y * Y
    S2, C2 = X * S1 + Y * C1, X * C1 - Y * S1
    Z2 = Z * Z
    tc = -2.285228997322329 * Z2 + 0.4570457994644658
    b = [torch.full_like(X, 0.2820947917738781), -0.48860251190292 * Y, 0.4886025119029199 * Z, -0.48860251190292 * X,
         0.5462742152960395 * S1, -1.092548430592079 * Z * Y, 0.9461746957575601 * Z2 - 0.31539156525252,
         -1.092548430592079 * Z * X, 0.5462742152960395 * C1, -0.5900435899266435 * S2, 1.445305721320277 * Z * S1,
         tc * Y, Z * (1.865881662950577 * Z2 - 1.119528997770346), tc * X, 1.445305721320277 * Z * C1,
         -0.5900435899266435 * C2]
    return torch.stack(b, dim=1)


def sh_range(sh_mode):
    """[k_lo, k_hi): the SH coefficients a frame of this GS_SH_* mode evaluates (bwd_chain)."""
    return (1 if sh_mode == 1 else 0), {2: 1, 5: 4, 4: 9}.get(sh_mode, 16)


def sh_monomials(dirs):
    """Per basis function b_k of Common.glsl:94-138 the sum of the absolute values of its monomials in (X, Y, Z) = (-dx, -dy,
    dz), as bwd_chain's sh_basis_grad adds them: [M, 16] >= |b_k|, equal where b_k is a single monomial."""
    X, Y, Z = dirs[:, 0].abs(), dirs[:, 1].abs(), dirs[:, 2].abs()
    X2, Y2, Z2 = X * X, Y * Y, Z * Z
    tc = 2.285228997322329 * Z2 + 0.4570457994644658
    m = [torch.full_like(X, 0.2820947917738781), 0.48860251190292 * Y, 0.4886025119029199 * Z, 0.48860251190292 * X,
         0.5462742152960395 * 2.0 * X * Y, 1.092548430592079 * Z * Y, 0.9461746957575601 * Z2 + 0.31539156525252,
         1.092548430592079 * Z * X, 0.5462742152960395 * (X2 + Y2), 0.5900435899266435 * (3.0 * X2 * Y + Y2 * Y),
         1.445305721320277 * Z * 2.0 * X * Y, tc * Y, Z * (1.865881662950577 * Z2 + 1.119528997770346), tc * X,
         1.445305721320277 * Z * (X2 + Y2), 0.5900435899266435 * (X2 * X + 3.0 * X * Y2)]
    return torch.stack(m, 1)


def camera_leaves(p, n, dtype=torch.float64, grad=False):
    """The frame's camera copied per splat: V [n, 4, 4] with V[g][r][c] = view[c * 4 + r], P likewise, cam [n, 3]."""
    V = torch.tensor(np.array(p.view, np.float64).reshape(4, 4).T, dtype=dtype).expand(n, 4, 4).clone()
    P = torch.tensor(np.array(p.proj, np.float64).reshape(4, 4).T, dtype=dtype).expand(n, 4, 4).clone()
    cam = torch.tensor(np.array(p.cam_pos, np.float64), dtype=dtype).expand(n, 3).clone()
    if grad:
        for t in (V, P, cam):
            t.requires_grad_(True)
    return V, P, cam


def weights(h, w, seed):
    """Loss weights of a frame: dL/dRGBA32F [h, w, 4] standard normal and dL/ddepth [h, w] a tenth of it, float32."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((h, w, 4)).astype(np.float32), (0.1 * rng.standard_normal((h, w))).astype(np.float32)


def loss_of(rgba, dep, w_rgba, w_depth=None):
    """L = sum w_rgba * RGBA32F + sum w_depth * depth."""
    loss = (rgba * torch.tensor(np.asarray(w_rgba, np.float64))).sum()
    if w_depth is not None:
        loss = loss + (dep * torch.tensor(np.asarray(w_depth, np.float64))).sum()
    return loss


def weights_by_tile(p, w_rgba, w_depth=None, dtype=torch.float64):
    """The loss weights as blend lays a tile out: [tiles, 256, 5] (r, g, b, 1 - T, z-blend), zero outside the frame."""
    w, h = p.width, p.height
    gw, gh = (w + 15) // 16, (h + 15) // 16
    wimg = torch.zeros(gh * 16, gw * 16, 5, dtype=dtype)
    wimg[:h, :w, :4] = torch.tensor(np.asarray(w_rgba, np.float64), dtype=dtype)
    if w_depth is not None:
        wimg[:h, :w, 4] = torch.tensor(np.asarray(w_depth, np.float64), dtype=dtype)
    return wimg.reshape(gh, 16, gw, 16, 5).permute(0, 2, 1, 3, 4).reshape(gh * gw, 256, 5)


# ---- the per-splat stage -------------------------------------------------------------------------------------------------------

def _scaled_derivative(x, k):
    """x with its derivative scaled by k (the value is x exactly: x - x.detach() is an exact zero)."""
    return x if k == 1.0 else x.detach() + k * (x - x.detach())


WRONG_TERMS = ("sh_direction", "whole_J", "J02", "view_depth")
DECISIONS = ("clamp_x", "clamp_y", "colour", "floored", "capped")             # the branches of splat_values: its `dec`


def splat_values(p, rec, live, cams=None, dec=None, antialias=False, wrong=None, frozen=None, r32=None, screen_offset=None):
    """(values [N, 10] in the order of ROW_NAMES, aux) of the records rec [N, 84] in rec's number format: screen position,
    inverse 2-D covariance, colour, alpha factor, view depth.  live [N]: the det != 0 rule (live_of).  cams = camera_leaves:
    the camera per splat, so that a camera gradient comes out per splat (default: p's).  All five GS_SH_* modes; opacity * rho
    under antialias (rho of tests/test_antialias_cpu.py with the cap at 1 bwd_chain holds fixed).  The branches are taken as
    `dec` names them (clamp_x, clamp_y [N]; colour [N, 3]: not on max(colour, 0); floored, capped [N]) or, without dec, as the
    values themselves decide.  wrong = (one of WRONG_TERMS, k): that term's derivative scaled by k.  frozen (bool [N]): splats
    that enter with the float32 values of raster32 r32, as constants -- for splats whose float32 2-D covariance is dominated by
    rounding (the needles of the zero_det scene: a float64 restatement of them is another function).  screen_offset [N, 2]:
    added to (sx, sy) after the freeze, frozen splats included.  aux: the decisions taken (NumPy), the unit direction, and of
    the 2-D covariance before its dilation cov0 = (a0, b, c0) and ratio_t = det0 / det (tensors) with ratio, its values."""
    dtype, n = rec.dtype, rec.shape[0]
    w, h = p.width, p.height
    V, P, cam = cams if cams is not None else camera_leaves(p, n, dtype)
    k_of = lambda name: wrong[1] if wrong is not None and wrong[0] == name else 1.0
    live = torch.as_tensor(np.asarray(live, bool))
    pos = rec[:, 0:3]
    ones = torch.ones(n, 1, dtype=dtype)
    vp = torch.einsum("nrc,nc->nr", V, torch.cat([pos, ones], 1))
    q = torch.einsum("nrc,nc->nr", P, vp)
    ndc_x, ndc_y = q[:, 0] / q[:, 3], q[:, 1] / q[:, 3]
    sx, sy = (ndc_x + 1.0) * 0.5 * w, (-ndc_y + 1.0) * 0.5 * h
    # getCovarianceMatrix (Common.glsl:32-78)
    r, x, y, z = rec[:, 8], rec[:, 9], rec[:, 10], rec[:, 11]
    R = torch.stack([torch.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y + 2 * r * z, 2 * x * z - 2 * r * y], 1),
                     torch.stack([2 * x * y - 2 * r * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z + 2 * r * x], 1),
                     torch.stack([2 * x * z + 2 * r * y, 2 * y * z - 2 * r * x, 1 - 2 * x * x - 2 * y * y], 1)], 1)
    M = R * rec[:, None, 4:7]
    Sig = M @ M.transpose(1, 2)
    tan_y = float(np.float32(np.tan(np.float64(np.float32(p.fov_y) * np.float32(0.5)))))
    tan_x = tan_y * w / h
    fx, fy = w / (2.0 * tan_x), h / (2.0 * tan_y)
    lim_x, lim_y = tan_x * p.in_view_limit, tan_y * p.in_view_limit
    tz = vp[:, 2]
    rx, ry = vp[:, 0] / tz, vp[:, 1] / tz
    clamp_x = torch.as_tensor(dec["clamp_x"]) if dec is not None else (rx < -lim_x) | (rx > lim_x)
    clamp_y = torch.as_tensor(dec["clamp_y"]) if dec is not None else (ry < -lim_y) | (ry > lim_y)
    pvx = torch.where(clamp_x, torch.clamp(rx.detach(), -lim_x, lim_x), rx) * tz
    pvy = torch.where(clamp_y, torch.clamp(ry.detach(), -lim_y, lim_y), ry) * tz
    zero = torch.zeros_like(tz)
    J02 = _scaled_derivative(-(fx * pvx) / (tz * tz), k_of("J02"))
    J = torch.stack([torch.stack([fx / tz, zero, J02], 1),
                     torch.stack([zero, fy / tz, -(fy * pvy) / (tz * tz)], 1)], 1)
    J = _scaled_derivative(J, k_of("whole_J"))
    Tm = J @ V[:, :3, :3]
    S2 = Tm @ Sig @ Tm.transpose(1, 2)
    a0, b, c0 = S2[:, 0, 0], S2[:, 1, 0], S2[:, 1, 1]
    a, c = a0 + 0.3, c0 + 0.3
    det = a * c - b * b
    det = torch.where(live, det, torch.ones_like(det))
    ix, iy, iz = c / det, -b / det, a / det
    # colour (Common.glsl:141-170)
    dvec = pos - cam
    dirs = dvec / torch.sqrt((dvec * dvec).sum(1, keepdim=True))
    basis = sh_basis(_scaled_derivative(dirs, k_of("sh_direction")))
    sh = rec[:, 12:76].reshape(-1, 16, 4)[:, :, :3]
    k_lo, k_hi = sh_range(p.sh_mode)
    res = (sh[:, k_lo:k_hi] * basis[:, k_lo:k_hi, None]).sum(1)
    if p.sh_mode == 1:
        res = res - 0.5
    res = res + 0.5
    colour = torch.as_tensor(dec["colour"]) if dec is not None else res >= 0
    col = torch.where(colour, res, torch.zeros_like(res))
    opac = torch.where(live, rec[:, 15], torch.zeros_like(det))
    ratio = (a0 * c0 - b * b) / det
    aux = dict(clamp_x=clamp_x.numpy(), clamp_y=clamp_y.numpy(), colour=colour.numpy(), dirs=dirs.detach(), cov0=(a0, b, c0),
               ratio_t=ratio, ratio=ratio.detach().numpy())
    if antialias:
        floored = torch.as_tensor(dec["floored"]) if dec is not None else ~(ratio > FLOOR)
        capped = torch.as_tensor(dec["capped"]) if dec is not None else ratio > 1.0
        const = torch.where(floored, torch.full_like(ratio, FLOOR), torch.ones_like(ratio))
        opac = opac * torch.sqrt(torch.where(floored | capped, const, ratio))
        aux.update(floored=floored.numpy(), capped=capped.numpy())
    zview = _scaled_derivative(-vp[:, 2], k_of("view_depth"))
    vals = torch.stack([sx, sy, ix, iy, iz, col[:, 0], col[:, 1], col[:, 2], opac, zview], 1)
    if frozen is not None:
        fz = torch.tensor(np.asarray(frozen, bool))
        vals = torch.where(fz[:, None], torch.tensor(stacked(r32), dtype=dtype), vals)
    if screen_offset is not None:
        vals = torch.cat([vals[:, :2] + screen_offset, vals[:, 2:]], 1)
    return vals, aux


# ---- the blend, tile by tile, with the decisions fixed -----------------------------------------------------------------------

def tile_walk(p, ref, flags):
    """Over the tiles that blend something: (tile index t, the slice of the sorted list cut behind the tile's last blended
    entry -- the entries behind every pixel's last one add nothing and get nothing --, the mask m [E, 256] of the (entry,
    pixel) pairs that blend, the splat ids g [E], the pixel coordinates fpx, fpy [1, 256] in float64)."""
    gw, gh = (p.width + 15) // 16, (p.height + 15) // 16
    ids = np.asarray(ref["id"], np.int64)
    ranges = np.asarray(ref["ranges"]).reshape(-1, 2)
    ly, lx = np.divmod(np.arange(256), 16)
    for t in range(gw * gh):
        s, e = int(ranges[t, 0]), int(ranges[t, 1])
        if e <= s:
            continue
        blended = np.flatnonzero(flags[s:e].any(1))
        if not len(blended):
            continue
        cut = slice(s, s + int(blended[-1]) + 1)
        ty, tx = divmod(t, gw)
        yield (t, cut, torch.tensor(flags[cut].astype(bool)), torch.tensor(ids[cut]),
               torch.tensor((tx * 16 + lx).astype(np.float64))[None, :], torch.tensor((ty * 16 + ly).astype(np.float64))[None, :])


def blend(v, m, fpx, fpy):
    """A tile's outputs [256, 5] (r, g, b, 1 - T, z-blend) in v's number format from the values v of its entries in the order
    of ROW_NAMES -- [E, 10], one set per splat, or [E, 256, 10], one per (list element, pixel) -- and the mask m."""
    per_splat = v.dim() == 2
    if per_splat:
        v = v[:, None, :]
    ex = v[:, :, 0] - fpx.to(v.dtype)
    ey = fpy.to(v.dtype) - v[:, :, 1]
    f = -0.5 * (v[:, :, 2] * ex * ex + v[:, :, 4] * ey * ey) - v[:, :, 3] * ex * ey
    f = torch.where(m, f, torch.zeros_like(f))
    alpha = torch.where(m, v[:, :, 8] * torch.exp(f), torch.zeros_like(f))
    Tx = torch.cumprod(torch.cat([torch.ones(1, 256, dtype=v.dtype), 1.0 - alpha[:-1]], 0), 0)
    wgt = Tx * alpha
    chans = torch.cat([v[:, :, 5:8], torch.ones_like(v[:, :, :1]), v[:, :, 9:10]], 2)                 # r, g, b, 1, z
    return wgt.T @ chans[:, 0] if per_splat else (wgt[:, :, None] * chans).sum(0)


def pair_terms(p, vals, ref, flags, w_rgba, w_depth=None, width=10):
    """Per blending tile (splat ids g [E], dL/d(offset) [E, 256, width]) of L = sum w_rgba * RGBA32F + sum w_depth * depth:
    a zero offset per (list element, pixel) is added to the first `width` of the splat values vals [N, 10] of that element at
    that pixel only, so its gradient holds the per-pixel terms of dL/d(value).  A tile's pixels read the offsets of its own
    elements alone, so the gradient is taken tile by tile (the rows of one [E, 256, width] tensor, never held whole); where
    vals is a leaf its own gradient accumulates as well."""
    wtile = weights_by_tile(p, w_rgba, w_depth, vals.dtype)
    for t, _, m, g, fpx, fpy in tile_walk(p, ref, flags):
        off = torch.zeros(len(g), 256, width, dtype=vals.dtype, requires_grad=True)
        v = vals[g][:, None, :] + torch.nn.functional.pad(off, (0, 10 - width))
        (blend(v, m, fpx, fpy) * wtile[t]).sum().backward()
        yield g, off.grad


def forward64(p, rec, ref, flags, frozen=None, r32=None, cams=None, screen_offset=None):
    """The frame of the records rec (torch float64 [N, 84]) with the float32 frame's decisions: rgba32f [H, W, 4] and depth
    [H, W] in float64.  frozen, r32, cams, screen_offset: as splat_values takes them."""
    w, h = p.width, p.height
    vals, _ = splat_values(p, rec, live_of(ref), cams, frozen=frozen, r32=r32, screen_offset=screen_offset)
    drawn, outs = [], []                    # the tiles that blend something and their [256, 5] pixels
    for t, _, m, g, fpx, fpy in tile_walk(p, ref, flags):
        drawn.append(t)
        outs.append(blend(vals[g], m, fpx, fpy))
    # one out-of-place scatter for the whole frame (a slice assignment per tile costs autograd a copy of the frame each:
    # hours on a 65 k-tile grid), then [gh, gw, 16, 16] -> [gh * 16, gw * 16]
    gw, gh = (w + 15) // 16, (h + 15) // 16
    img = torch.zeros(gw * gh, 256, 5, dtype=rec.dtype)
    if drawn:
        img = img.index_copy(0, torch.tensor(drawn, dtype=torch.int64), torch.stack(outs))
    img = img.reshape(gh, gw, 16, 16, 5).permute(0, 2, 1, 3, 4).reshape(gh * 16, gw * 16, 5)[:h, :w]
    return img[..., :4], img[..., 4]


def reference_gradient(p, aos, ref, flags, w_rgba, w_depth=None, frozen=None):
    """dL/d(record) [N, 84] (float64) of L = sum w_rgba * RGBA32F + sum w_depth * depth (zero for frozen splats)."""
    rec = torch.tensor(np.asarray(aos, np.float64), requires_grad=True)
    rgba, dep = forward64(p, rec, ref, flags, frozen, raster32(p, aos, ref) if frozen is not None else None)
    loss_of(rgba, dep, w_rgba, w_depth).backward()
    return rec.grad.numpy()
