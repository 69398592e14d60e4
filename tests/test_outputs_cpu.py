"""The optional per-pixel outputs of a frame (gs_set_outputs, include/gsplat.h GS_OUTPUT_*) on the CPU: the C restatement
of the blend with alpha and depth (tests/host/blend_outputs_ref.c) is first shown to reproduce the oracle's RGBA8 frame
byte for byte, which is what lets tests/test_outputs_gpu.py trust its alpha and depth; plus the C-ABI's argument checks
without a context.  The helpers here are shared with the GPU tests."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib, synth

_REF = {}


def restatement(tmp_dir):
    """tests/host/blend_outputs_ref.c as a shared library: -O2 -ffp-contract=off, gso_exp from oracle/libgs_oracle.so."""
    if "lib" not in _REF:
        import oracle
        L = oracle.lib()                         # builds oracle/libgs_oracle.so if needed, and maps it
        so = os.path.join(str(tmp_dir), "libblend_outputs_ref.so")
        odir = os.path.join(ROOT, "oracle")
        build = subprocess.run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", odir, "-o", so,
                                os.path.join(ROOT, "tests", "host", "blend_outputs_ref.c"), "-L", odir, "-lgs_oracle",
                                f"-Wl,-rpath,{odir}", "-lm"], capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-2000:]
        R = C.CDLL(so)
        R.gsb_render_outputs.restype = None
        _REF["lib"] = (R, L)
    return _REF["lib"][0]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def reference_outputs(tmp_dir, p, aos, ref=None, base=None):
    """The oracle's frame (oracle.full_pipeline, or `ref` if given) and the restatement's RGBA8 / RGBA32F / depth over its
    intermediates; only the tile rows [p.row_begin, p.row_end) are written (over `base` if given, else zeros)."""
    import oracle
    R = restatement(tmp_dir)
    aos = np.ascontiguousarray(aos, dtype=np.float32)
    if ref is None:
        ref = oracle.full_pipeline(p, aos)
    h, w = p.height, p.width
    rgba = np.zeros((h, w, 4), np.uint8) if base is None else base["rgba"].copy()
    f32 = np.zeros((h, w, 4), np.float32) if base is None else base["rgba32f"].copy()
    dep = np.zeros((h, w), np.float32) if base is None else base["depth"].copy()
    R.gsb_render_outputs(C.byref(p), _ptr(aos), _ptr(np.ascontiguousarray(ref["stage1"]["color"])),
                         _ptr(np.ascontiguousarray(ref["stage1"]["cov"])), _ptr(np.ascontiguousarray(ref["id"], dtype=np.uint32)),
                         _ptr(np.ascontiguousarray(ref["ranges"], dtype=np.uint32)), _ptr(rgba), _ptr(f32), _ptr(dep))
    return dict(ref=ref, rgba=rgba, rgba32f=f32, depth=dep)


def quantise(rgba32f):
    """The UNORM store of RenderGaussians.comp:147-151, floor(clamp(c, 0, 1) * 255 + 0.5), A = 255, in fp32."""
    c = rgba32f[..., :3].astype(np.float32)
    t = np.where(c > np.float32(0), c, np.float32(0))
    t = np.where(t < np.float32(1), t, np.float32(1))
    q = (t * np.float32(255) + np.float32(0.5)).astype(np.uint8)
    return np.concatenate([q, np.full(q.shape[:-1] + (1,), 255, np.uint8)], axis=-1)


# ---- scenes (shared with the GPU tests) ----------------------------------------------------------------------------------

def scene_ragged():
    """333 x 190 (neither side a multiple of 16), 6000 splats of the uniform fog."""
    return synth.generate(6000, 333, 190, -3.0, seed=77), 333, 190


def scene_dense():
    """160 x 96, a dense cloud of large, nearly opaque splats: most pixels end on the early-out (T < 1e-4)."""
    aos = synth.generate(6000, 160, 96, -1.6, seed=5)
    aos[:, 15] = 0.97
    return aos, 160, 96


def scene_zero_det():
    """192 x 112 with needles whose 2x2 covariance has determinant exactly 0 (test_parity_gpu.test_zero_determinant_splats)."""
    aos = synth.generate(3000, 192, 112, -3.0, seed=31)
    k = 600
    aos[:k, 4] = 3.0e4
    aos[:k, 5:7] = 1.0e-6
    aos[:k, 15] = 0.9
    return aos, 192, 112


SCENES = {"ragged": scene_ragged, "dense": scene_dense, "zero_det": scene_zero_det}

# Camera poses (pos, yaw, pitch) for the posed scenes: one generic pose, and GardenScene.cpp's benchmark pose
POSES = {"pose": ((0.7, -0.4, 1.5), 0.6, -0.35), "garden": gs.PlyScene.POSES["garden"]}


def camera(pose, w, h):
    """The renderer's Camera at POSES[pose] (its matrices are those of oracle.camera_matrices, bit for bit)."""
    pos, yaw, pitch = POSES[pose]
    cam = gs.Camera(w / h)
    cam.setPosition(pos)
    cam.setRotation(yaw, pitch)
    cam.recalculate()
    return cam


def in_front_of(aos, w, h, pose):
    """A cloud made for the origin camera (in front of it along +z) moved in front of the camera at POSES[pose], as
    test_parity_gpu.test_reference_benchmark_camera_poses does: the same view-space positions under that camera."""
    view = camera(pose, w, h).getViewMatrix().reshape(4, 4).T.astype(np.float64)      # row-major 4 x 4
    inv = np.linalg.inv(view)
    out = np.array(aos, np.float32, copy=True)
    p = out[:, 0:3].astype(np.float64) * np.array([-1.0, 1.0, -1.0])                # origin camera: view (-x, y, -z)
    out[:, 0:3] = ((inv[:3, :3] @ p.T).T + inv[:3, 3]).astype(np.float32)
    return out


def load_scene(name):
    """A scene of SCENES by name, or 'scene@pose' for that cloud moved in front of the camera at POSES[pose]: (aos, w, h,
    cam) with cam the keyword arguments of oracle_params / make_scene (empty: the origin camera)."""
    scene, _, pose = name.partition("@")
    aos, w, h = SCENES[scene]()
    if not pose:
        return aos, w, h, {}
    pos, yaw, pitch = POSES[pose]
    return in_front_of(aos, w, h, pose), w, h, dict(pos=pos, yaw=yaw, pitch=pitch)


def assert_posed(p):
    """The camera of params p is not the origin camera in disguise: its 3 x 3 view block is not symmetric, it sits away
    from the origin, and the view depth row (view[2], view[6], view[10], view[14]) has more than its z term."""
    W = np.array(p.view, np.float64).reshape(4, 4).T[:3, :3]
    assert np.abs(W - W.T).max() > 0.1, W
    assert np.linalg.norm(np.array(p.cam_pos, np.float64)) > 0.5
    assert any(p.view[k] != 0 for k in (2, 6, 14)), list(p.view)


def known_answer_scene(depths, w=64, h=48, opacity=0.5):
    """Splats of opacity `opacity` on the camera axis at view depths `depths` (origin camera: world (0, 0, z) has view
    depth z exactly), i.e. centred on pixel (w / 2, h / 2), small enough to leave the corner tiles empty."""
    rec = [gs.makeGaussian((0.0, 0.0, float(z)), (0.02 * z, 0.02 * z, 0.02 * z), sh0=(0.4 - 0.3 * k, 0.1, 0.3 * k, opacity))
           for k, z in enumerate(depths)]
    return np.stack(rec).astype(np.float32), w, h


def oracle_params(oracle, w, h, sh_mode=0, pos=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0, **kw):
    pos = np.asarray(pos, np.float32)
    view, proj = oracle.camera_matrices(pos, yaw, pitch, w / h)
    return oracle.make_params(w, h, view, proj, pos, sh_mode=sh_mode, **kw)


def camera_params(oracle, sc, w, h, **kw):
    """Params from a Scene's own camera (its view, projection, position and SH mode), as test_parity_gpu.oracle_run."""
    cam = sc.getCamera()
    return oracle.make_params(w, h, cam.getViewMatrix(), cam.getProjectionMatrix(), cam.getPosition(),
                              sh_mode=int(cam.getShMode()), **kw)


# ---- tests ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,sh_mode", [("ragged", 0), ("ragged", 1), ("ragged", 2), ("dense", 0), ("zero_det", 0),
                                           ("ragged@pose", 0), ("ragged@pose", 1), ("ragged@garden", 0),
                                           ("ragged@garden", 1)])
def test_restatement_reproduces_the_oracle_frame(oracle_mod, tmp_path, scene, sh_mode):
    """Byte for byte the oracle's RGBA8 frame, and the same bytes again from quantising its float colour -- the condition
    under which its alpha and depth are the reference for the GPU's.  Also at posed cameras (a rotated, translated view:
    the depth row and the SH direction's camera position count)."""
    aos, w, h, cam = load_scene(scene)
    p = oracle_params(oracle_mod, w, h, sh_mode, **cam)
    if cam:
        assert_posed(p)
    out = reference_outputs(tmp_path, p, aos)
    assert np.array_equal(out["rgba"], out["ref"]["image"])
    assert np.array_equal(quantise(out["rgba32f"]), out["rgba"])
    a, d = out["rgba32f"][..., 3], out["depth"]
    assert np.all((a >= 0) & (a <= 1)) and np.all(np.isfinite(d)) and np.all(d >= 0)
    empty = a == 0
    assert np.all(out["rgba32f"][empty] == 0) and np.all(d[empty] == 0)
    if scene == "dense":            # the early-out of :136-140 is exercised, and T_end is the entry's nextT there
        assert np.count_nonzero(a > np.float32(1.0 - 1e-4)) > w * h // 4


def test_restatement_known_answer(oracle_mod, tmp_path):
    """One and two splats of opacity 0.5 at view depths 2 and 4 on the centre pixel: a = 0.5 / 0.75, depth = 0.5 z1 /
    0.5 z1 + 0.25 z2, premultiplied colour -- exactly; an empty tile is all zero."""
    for depths in ((2.0,), (2.0, 4.0)):
        aos, w, h = known_answer_scene(depths)
        p = oracle_params(oracle_mod, w, h)
        out = reference_outputs(tmp_path, p, aos)
        col = out["ref"]["stage1"]["color"]
        px = out["rgba32f"][h // 2, w // 2]
        if len(depths) == 1:
            assert px[3] == np.float32(0.5) and out["depth"][h // 2, w // 2] == np.float32(1.0)
            assert np.array_equal(px[:3], np.float32(0.5) * col[0, :3])
        else:
            assert px[3] == np.float32(0.75) and out["depth"][h // 2, w // 2] == np.float32(2.0)
            assert np.array_equal(px[:3], np.float32(0.5) * col[0, :3] + np.float32(0.25) * col[1, :3])
        assert not out["rgba32f"][:16, :16].any() and not out["depth"][:16, :16].any()


def test_output_entry_points_refuse_a_null_context():
    """gs_set_outputs / gs_read_output / gs_output_device: GS_ERR_INVALID on a NULL context, no crash; the binding mirrors
    the header's bits and the version that added them."""
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    dev, size = C.c_void_p(), C.c_size_t()
    assert L.gs_set_outputs(None, 0) == _lib.GS_ERR_INVALID
    assert L.gs_set_outputs(None, _lib.GS_OUTPUT_RGBA32F | _lib.GS_OUTPUT_DEPTH) == _lib.GS_ERR_INVALID
    assert L.gs_read_output(None, _lib.GS_OUTPUT_DEPTH, _ptr(buf), buf.nbytes) == _lib.GS_ERR_INVALID
    assert L.gs_read_output(None, _lib.GS_OUTPUT_RGBA32F, None, 0) == _lib.GS_ERR_INVALID
    assert L.gs_output_device(None, _lib.GS_OUTPUT_RGBA32F, C.byref(dev), C.byref(size)) == _lib.GS_ERR_INVALID
    assert L.gs_output_device(None, _lib.GS_OUTPUT_DEPTH, None, None) == _lib.GS_ERR_INVALID
    assert (gs.GS_OUTPUT_RGBA32F, gs.GS_OUTPUT_DEPTH) == (1, 2) and _lib.API_VERSION >= 6
