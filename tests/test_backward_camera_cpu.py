"""The float64 reference of the frame's camera gradients (include/gsplat.h, gs_backward_camera), on the CPU.

forward64_cam is forward64 of tests/test_backward_cpu.py restated with per-splat camera leaves: every splat gets its own
copy of the view matrix, the projection and the camera position.  The gradient of those leaves is then the per-splat
contribution C[g][35] to dL/dcamera; its column sums are the reference `want`, and S[k] = sum_g |C[g][k]| is the scale
the GPU tests measure against (tests/test_backward_camera_gpu.py).  It is trusted by three checks here: its outputs equal
forward64's, its gradient equals central differences of its own loss, and the translation identity ties it to the
record gradients of reference_gradient.  No frozen splats are used: the zero_det scene is left out (its reference
freezes 600 needles that the GPU differentiates)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from test_outputs_cpu import assert_posed, load_scene, oracle_params
from test_backward_cpu import _sh_basis, forward64, frame_decisions, reference_gradient

torch = pytest.importorskip("torch")

CAMERA_FLOATS = 35
VIEW_BOTTOM_ROW = [3, 7, 11, 15]          # of the 35 floats: the view matrix is taken as affine
PROJ_CLIP_Z = [18, 22, 26, 30]            # ... and no frame reads clip z


def weights(h, w, seed=0):
    """The loss weights of test_backward_gpu.weights (the same numbers for the same seed)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((h, w, 4)).astype(np.float32), (0.1 * rng.standard_normal((h, w))).astype(np.float32)


def camera_leaves(p, n):
    """The frame's camera copied per splat: Vn [n, 4, 4] with Vn[g][r][c] = view[c * 4 + r], Pn likewise, camn [n, 3]."""
    V = torch.tensor(np.array(p.view, np.float64).reshape(4, 4).T)
    P = torch.tensor(np.array(p.proj, np.float64).reshape(4, 4).T)
    cam = torch.tensor(np.array(p.cam_pos, np.float64))
    return V.expand(n, 4, 4).clone(), P.expand(n, 4, 4).clone(), cam.expand(n, 3).clone()


def forward64_cam(p, rec, ref, flags, Vn, Pn, camn):
    """forward64 (tests/test_backward_cpu.py) with the camera of splat g taken from Vn[g], Pn[g], camn[g]: rgba32f
    [H, W, 4] and depth [H, W] in float64, with the float32 frame's decisions."""
    w, h = p.width, p.height
    pos = rec[:, 0:3]
    ones = torch.ones(rec.shape[0], 1, dtype=rec.dtype)
    vp = torch.einsum("nrc,nc->nr", Vn, torch.cat([pos, ones], 1))
    q = torch.einsum("nrc,nc->nr", Pn, vp)
    ndc_x, ndc_y = q[:, 0] / q[:, 3], q[:, 1] / q[:, 3]
    sx, sy = (ndc_x + 1.0) * 0.5 * w, (-ndc_y + 1.0) * 0.5 * h
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
    pvx = torch.clamp(vp[:, 0] / tz, -lim_x, lim_x) * tz
    pvy = torch.clamp(vp[:, 1] / tz, -lim_y, lim_y) * tz
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -(fx * pvx) / (tz * tz)], 1),
                     torch.stack([zero, fy / tz, -(fy * pvy) / (tz * tz)], 1)], 1)
    T = J @ Vn[:, :3, :3]
    S2 = T @ Sig @ T.transpose(1, 2)
    a, b, c = S2[:, 0, 0] + 0.3, S2[:, 1, 0], S2[:, 1, 1] + 0.3
    det = a * c - b * b
    cov32 = ref["stage1"]["cov"]
    live = torch.tensor((cov32[:, 0] * cov32[:, 2] - cov32[:, 1] * cov32[:, 1]) != 0)
    det = torch.where(live, det, torch.ones_like(det))
    ix, iy, iz = c / det, -b / det, a / det
    dvec = pos - camn
    dirs = dvec / torch.sqrt((dvec * dvec).sum(1, keepdim=True))
    basis = _sh_basis(dirs)
    sh = rec[:, 12:76].reshape(-1, 16, 4)[:, :, :3]
    if p.sh_mode == 0:
        col = (sh * basis[:, :, None]).sum(1) + 0.5
    elif p.sh_mode == 1:
        col = (sh[:, 1:] * basis[:, 1:, None]).sum(1) - 0.5 + 0.5
    else:
        col = sh[:, 0] * basis[:, 0:1] + 0.5
    col = torch.clamp(col, min=0.0)
    opac = torch.where(live, rec[:, 15], torch.zeros_like(det))
    zview = -vp[:, 2]
    gw, gh = (w + 15) // 16, (h + 15) // 16
    drawn, outs = [], []
    ids = np.asarray(ref["id"], np.int64)
    ranges = np.asarray(ref["ranges"]).reshape(-1, 2)
    ly, lx = np.divmod(np.arange(256), 16)
    for t in range(gw * gh):
        s, e = int(ranges[t, 0]), int(ranges[t, 1])
        if e <= s:
            continue
        ty, tx = divmod(t, gw)
        blended = np.flatnonzero(flags[s:e].any(1))
        if not len(blended):
            continue
        e = s + int(blended[-1]) + 1
        m = torch.tensor(flags[s:e].astype(bool))
        g = torch.tensor(ids[s:e])
        fpx = torch.tensor((tx * 16 + lx).astype(np.float64))[None, :]
        fpy = torch.tensor((ty * 16 + ly).astype(np.float64))[None, :]
        ex = sx[g][:, None] - fpx
        ey = fpy - sy[g][:, None]
        f = -0.5 * (ix[g][:, None] * ex * ex + iz[g][:, None] * ey * ey) - iy[g][:, None] * ex * ey
        f = torch.where(m, f, torch.zeros_like(f))
        alpha = torch.where(m, opac[g][:, None] * torch.exp(f), torch.zeros_like(f))
        Tx = torch.cumprod(torch.cat([torch.ones(1, 256, dtype=rec.dtype), 1.0 - alpha[:-1]], 0), 0)
        wgt = Tx * alpha
        chans = torch.cat([col[g], torch.ones(len(g), 1, dtype=rec.dtype), zview[g][:, None]], 1)
        drawn.append(t)
        outs.append(wgt.T @ chans)
    img = torch.zeros(gw * gh, 256, 5, dtype=rec.dtype)
    if drawn:
        img = img.index_copy(0, torch.tensor(drawn, dtype=torch.int64), torch.stack(outs))
    img = img.reshape(gh, gw, 16, 16, 5).permute(0, 2, 1, 3, 4).reshape(gh * 16, gw * 16, 5)[:h, :w]
    return img[..., :4], img[..., 4]


def loss_of(rgba, dep, w_rgba, w_depth):
    loss = (rgba * torch.tensor(np.asarray(w_rgba, np.float64))).sum()
    if w_depth is not None:
        loss = loss + (dep * torch.tensor(np.asarray(w_depth, np.float64))).sum()
    return loss


def camera_contributions(p, aos, ref, flags, w_rgba, w_depth=None):
    """C [N, 35] (float64): the contribution of every splat to dL/dview (column-major, as gs_render* takes the matrix),
    dL/dproj and dL/dcam_pos of L = sum w_rgba * RGBA32F + sum w_depth * depth, unmasked."""
    rec = torch.tensor(np.asarray(aos, np.float64))
    Vn, Pn, camn = (t.requires_grad_(True) for t in camera_leaves(p, len(aos)))
    rgba, dep = forward64_cam(p, rec, ref, flags, Vn, Pn, camn)
    loss_of(rgba, dep, w_rgba, w_depth).backward()
    n = len(aos)
    # element c * 4 + r of the float[16] is the matrix's [r][c]
    return np.concatenate([Vn.grad.transpose(1, 2).reshape(n, 16).numpy(), Pn.grad.transpose(1, 2).reshape(n, 16).numpy(),
                           camn.grad.numpy()], 1)


def masked(v):
    """The header's conventions applied to 35 reference numbers: the view's bottom row counts as 0 (the reference
    multiplies by the full matrix and so can have a derivative there; a camera never moves those elements)."""
    v = np.array(v, np.float64, copy=True)
    v[VIEW_BOTTOM_ROW] = 0.0
    return v


_REFERENCE = {}


def camera_reference(key, tmp_dir, p, aos, w_rgba, w_depth):
    """(want [35], S [35], raw column sums [35]) of a frame, computed once per `key` and shared: want = the masked column
    sums of camera_contributions, S[k] = sum_g |C[g][k]|, masked likewise.  The reference's clip-z row is exactly 0."""
    if key not in _REFERENCE:
        ref, flags = frame_decisions(tmp_dir, p, aos)
        Cg = camera_contributions(p, aos, ref, flags, np.asarray(w_rgba, np.float64),
                                  None if w_depth is None else np.asarray(w_depth, np.float64))
        assert np.all(np.isfinite(Cg))
        assert np.all(Cg[:, PROJ_CLIP_Z] == 0)
        _REFERENCE[key] = (masked(Cg.sum(0)), masked(np.abs(Cg).sum(0)), Cg.sum(0))
    return _REFERENCE[key]


# ---- tests ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,sh_mode", [("ragged", 0), ("ragged", 1), ("ragged", 2), ("ragged@pose", 0)])
def test_forward64_cam_equals_forward64(oracle_mod, tmp_path, scene, sh_mode):
    """With every row of the camera leaves a copy of the frame's camera, the outputs are forward64's to 1e-12."""
    aos, w, h, cam = load_scene(scene)
    p = oracle_params(oracle_mod, w, h, sh_mode, **cam)
    ref, flags = frame_decisions(tmp_path, p, aos)
    rec = torch.tensor(aos.astype(np.float64))
    with torch.no_grad():
        a0, d0 = forward64(p, rec, ref, flags)
        a1, d1 = forward64_cam(p, rec, ref, flags, *camera_leaves(p, len(aos)))
    assert float(a0.abs().max()) > 0.1
    assert float((a1 - a0).abs().max()) <= 1e-12 * max(1.0, float(a0.abs().max()))
    assert float((d1 - d0).abs().max()) <= 1e-12 * max(1.0, float(d0.abs().max()))


@pytest.mark.parametrize("sh_mode", [0, 1])
def test_reference_matches_central_differences(oracle_mod, tmp_path, sh_mode):
    """The column sums of the per-splat contributions against float64 central differences of forward64_cam's own loss
    (decisions fixed, so the loss is smooth) on all 12 + 12 + 3 live entries of ragged@pose: relative step 1e-6, bar
    1e-5 of the block's largest |want|.  The clip-z row of the projection is exactly 0 in the reference.  Its view bottom row
    reaches the frame through the projection's last column alone (forward64 multiplies by the full matrix), which a
    perspective projection feeds into clip z only; `masked` sets it to 0 whatever the projection is."""
    aos, w, h, cam = load_scene("ragged@pose")
    p = oracle_params(oracle_mod, w, h, sh_mode, **cam)
    assert_posed(p)
    wr, wd = weights(h, w, 1)
    want, S, raw = camera_reference(("ragged@pose", sh_mode, 1), tmp_path, p, aos, wr, wd)
    assert np.all(raw[PROJ_CLIP_Z] == 0)
    assert np.all(want[VIEW_BOTTOM_ROW] == 0) and np.all(S[VIEW_BOTTOM_ROW] == 0)
    ref, flags = frame_decisions(tmp_path, p, aos)
    rec = torch.tensor(aos.astype(np.float64))
    base = np.concatenate([np.array(p.view, np.float64), np.array(p.proj, np.float64), np.array(p.cam_pos, np.float64)])

    def loss(x):
        V = torch.tensor(x[0:16].reshape(4, 4).T.copy()).expand(len(aos), 4, 4)
        P = torch.tensor(x[16:32].reshape(4, 4).T.copy()).expand(len(aos), 4, 4)
        c = torch.tensor(x[32:35].copy()).expand(len(aos), 3)
        with torch.no_grad():
            a, d = forward64_cam(p, rec, ref, flags, V, P, c)
            return float(loss_of(a, d, wr, wd))

    live = [c * 4 + r for c in range(4) for r in range(3)] + [16 + c * 4 + r for c in range(4) for r in (0, 1, 3)] + [32, 33, 34]
    assert len(live) == 27
    bar = {0: 1e-5 * np.abs(want[0:16]).max(), 1: 1e-5 * np.abs(want[16:32]).max(), 2: 1e-5 * np.abs(want[32:35]).max()}
    assert all(b > 0 for b in bar.values())
    for k in live:
        step = 1e-6 * max(1.0, abs(base[k]))
        xp, xm = base.copy(), base.copy()
        xp[k] += step
        xm[k] -= step
        fd = (loss(xp) - loss(xm)) / (2 * step)
        assert abs(fd - want[k]) <= bar[k // 16], (k, fd, want[k], bar[k // 16])


@pytest.mark.parametrize("scene", ["ragged@pose", "ragged@garden"])
def test_translation_identity(oracle_mod, tmp_path, scene):
    """Moving the camera and the cloud together changes nothing.  For j = 0..2:
    sum_g dL/dpos_g[j] + dcam[j] - sum_{r<3} dview[3 * 4 + r] * view[j * 4 + r] = 0, to 1e-9 of the sum of the absolute
    terms; dL/dpos from reference_gradient, the camera terms from the per-splat contributions."""
    aos, w, h, cam = load_scene(scene)
    p = oracle_params(oracle_mod, w, h, 0, **cam)
    wr, wd = weights(h, w, 1)
    want, S, _ = camera_reference((scene, 0, 1), tmp_path, p, aos, wr, wd)
    ref, flags = frame_decisions(tmp_path, p, aos)
    grad = reference_gradient(p, aos, ref, flags, wr.astype(np.float64), wd.astype(np.float64))
    view = np.array(p.view, np.float64)
    for j in range(3):
        total = grad[:, j].sum() + want[32 + j] - sum(want[12 + r] * view[j * 4 + r] for r in range(3))
        scale = np.abs(grad[:, j]).sum() + S[32 + j] + sum(S[12 + r] * abs(view[j * 4 + r]) for r in range(3))
        assert scale > 0 and abs(total) <= 1e-9 * scale, (j, total, scale)


def test_the_binding_is_present():
    """gs_backward_camera and gs_backward_camera_device are bound; both refuse a NULL context with the code alone, without
    a crash; GS_CAMERA_GRAD_FLOATS is the header's."""
    from vk3dgaussiansplatting_amd import _lib
    assert {"gs_backward_camera", "gs_backward_camera_device"} <= set(_lib.EXPORTS)
    L = _lib.lib()
    out = np.full(CAMERA_FLOATS, -7.0, np.float32)
    assert L.gs_backward_camera(None, out.ctypes.data_as(C.c_void_p)) == _lib.GS_ERR_INVALID
    assert L.gs_backward_camera_device(None, out.ctypes.data_as(C.c_void_p)) == _lib.GS_ERR_INVALID
    assert np.all(out == -7.0)
    hdr = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    assert int(re.search(r"#define GS_CAMERA_GRAD_FLOATS (\d+)u", hdr).group(1)) == _lib.CAMERA_GRAD_FLOATS == CAMERA_FLOATS
