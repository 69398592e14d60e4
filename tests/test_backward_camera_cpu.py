"""The float64 reference of the frame's camera gradients (include/gsplat.h, gs_backward_camera), on the CPU.

forward64_cam is forward64 of tests/frame64.py on per-splat camera leaves (its `cams`): every splat gets its own copy of
the view matrix, the projection and the camera position.  The gradient of those leaves is then the per-splat
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
from frame64 import camera_leaves, forward64, frame_decisions, loss_of, reference_gradient, weights

torch = pytest.importorskip("torch")

CAMERA_FLOATS = 35
VIEW_BOTTOM_ROW = [3, 7, 11, 15]          # of the 35 floats: the view matrix is taken as affine
PROJ_CLIP_Z = [18, 22, 26, 30]            # ... and no frame reads clip z


def forward64_cam(p, rec, ref, flags, Vn, Pn, camn):
    """forward64 with the camera of splat g taken from Vn[g], Pn[g], camn[g] (laid out as camera_leaves)."""
    return forward64(p, rec, ref, flags, cams=(Vn, Pn, camn))


def camera_contributions(p, aos, ref, flags, w_rgba, w_depth=None):
    """C [N, 35] (float64): the contribution of every splat to dL/dview (column-major, as gs_render* takes the matrix),
    dL/dproj and dL/dcam_pos of L = sum w_rgba * RGBA32F + sum w_depth * depth, unmasked."""
    rec = torch.tensor(np.asarray(aos, np.float64))
    Vn, Pn, camn = camera_leaves(p, len(aos), grad=True)
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
