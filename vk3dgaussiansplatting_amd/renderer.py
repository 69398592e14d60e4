"""Host-side mirror of the reference's interface for the splat path, over the C-ABI.

Class and method names follow the reference so that tests read like tests of the reference:
  Camera            Engine/Graphics/Camera.{h,cpp}
  ResourceManager   Engine/ResourceManager.{h,cpp}   (gaussian part only)
  Scene + presets   Engine/Application/Scene.h, Scenes/*.cpp
  GpuSort/RadixSort Engine/Graphics/Sort/{GpuSort.h,RadixSort.{h,cpp}}
  Renderer          Engine/Graphics/Renderer.{h,cpp}  (init / initForScene / draw / cleanup + the
                    RECORD_GPU_TIMES running averages)
All compute happens in libgsplat_hip.so; nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
import enum
import math
import os

import numpy as np

from . import _lib
from ._lib import GsAdamParams, GsConfig, GsDensifyParams, GsHostTimings, GsInitParams, GsSceneInfo, GsTimings, default_adam_params  # noqa: F401

FLOATS_PER_GAUSSIAN = 84
GAUSSIAN_DTYPE = np.dtype([
    ("position", "<f4", (4,)), ("scale", "<f4", (4,)), ("rot", "<f4", (4,)),
    ("shCoeffs", "<f4", (16, 4)), ("color", "<f4", (4,)), ("covariance", "<f4", (4,)),
])
assert GAUSSIAN_DTYPE.itemsize == _lib.RECORD_BYTES


class GsplatError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"gsplat error {code}: {message}")
        self.code = code


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _vp(address: int | None):
    """A device address as the library takes it; 0 and None are NULL."""
    return C.c_void_p(address) if address else None


class SphericalHarmonicsMode(enum.IntEnum):  # Camera.h:7-12
    ALL_BANDS = 0
    SKIP_FIRST_BAND = 1
    ONLY_FIRST_BAND = 2
    # no reference counterpart (GS_SH_DEGREE_1 / _2 of include/gsplat.h): the sum cut at 4 and at 9 coefficients
    DEGREE_2 = 4
    DEGREE_1 = 5


class Camera:
    """Camera.cpp:7-105.  The window's aspect ratio is passed explicitly (there is no window)."""

    NEAR_PLANE = 0.1
    FAR_PLANE = 100.0

    def __init__(self, aspect_ratio: float = 1280.0 / 720.0):
        self.position = np.array([0.0, 0.0, 2.0], dtype=np.float32)   # Camera.cpp:61
        self.yaw = SMATH_PI                                           # Camera.cpp:66
        self.pitch = 0.0
        self.shMode = SphericalHarmonicsMode.ALL_BANDS
        self.aspectRatio = float(aspect_ratio)
        self.viewMatrix = np.eye(4, dtype=np.float32).reshape(16)
        self.projectionMatrix = np.eye(4, dtype=np.float32).reshape(16)
        self.recalculate()

    def setPosition(self, newPos):
        self.position = np.asarray(newPos, dtype=np.float32).reshape(3)

    def setRotation(self, yaw: float, pitch: float):
        self.yaw, self.pitch = float(np.float32(yaw)), float(np.float32(pitch))

    def setShMode(self, mode):
        self.shMode = SphericalHarmonicsMode(int(mode))

    def setAspectRatio(self, aspect: float):
        self.aspectRatio = float(aspect)

    def recalculate(self):  # Camera.cpp:50-54
        view = np.zeros(16, dtype=np.float32)
        proj = np.zeros(16, dtype=np.float32)
        rc = _lib.lib().gs_camera_matrices(_p(self.position), self.yaw, self.pitch,
                                           float(np.float32(self.aspectRatio)), self.NEAR_PLANE,
                                           self.FAR_PLANE, _p(view), _p(proj))
        if rc != 0:
            raise GsplatError(rc, "gs_camera_matrices")
        self.viewMatrix, self.projectionMatrix = view, proj

    def update(self):  # Camera.cpp:82-131 without the keyboard/mouse part
        self.recalculate()

    def getViewMatrix(self):
        return self.viewMatrix

    def getProjectionMatrix(self):
        return self.projectionMatrix

    def getPosition(self):
        return self.position

    def getYaw(self):                      # Camera.h:52-53
        return self.yaw

    def getPitch(self):
        return self.pitch

    def getShMode(self):
        return self.shMode


class ResourceManager:
    """Gaussian part of Engine/ResourceManager.cpp: addGaussian (:158), loadGaussians (:167-300)."""

    def __init__(self):
        self.gaussians = np.zeros((0, FLOATS_PER_GAUSSIAN), dtype=np.float32)

    def clearAllGaussians(self):
        self.gaussians = np.zeros((0, FLOATS_PER_GAUSSIAN), dtype=np.float32)

    def addGaussian(self, gaussianData) -> int:
        rec = np.asarray(gaussianData, dtype=np.float32).reshape(1, FLOATS_PER_GAUSSIAN)
        gid = self.gaussians.shape[0]
        self.gaussians = np.concatenate([self.gaussians, rec], axis=0)
        return gid

    def setGaussians(self, aos: np.ndarray):
        self.gaussians = np.ascontiguousarray(aos, dtype=np.float32).reshape(-1, FLOATS_PER_GAUSSIAN)

    def loadGaussians(self, filePath: str):
        """ResourceManager.cpp:167-300.  A missing file is reported and the call returns with the
        list unchanged, like the reference's Log::error + return (:169-173)."""
        n = C.c_uint32(0)
        L = _lib.lib()
        rc = L.gs_convert_ply(os.fsencode(filePath), None, 0, C.byref(n))
        if rc == _lib.GS_ERR_IO:
            print("[Log Error]: " + L.gs_ply_last_error().decode())
            return
        if rc != 0:
            raise GsplatError(rc, L.gs_ply_last_error().decode())
        out = np.zeros((n.value, FLOATS_PER_GAUSSIAN), dtype=np.float32)
        rc = L.gs_convert_ply(os.fsencode(filePath), _p(out), n.value, C.byref(n))
        if rc != 0:
            raise GsplatError(rc, L.gs_ply_last_error().decode())
        self.gaussians = out
        print(f"[Log]: Number of gaussians: {n.value}")

    def getGaussians(self) -> np.ndarray:
        return self.gaussians


def makeGaussian(position, scale, rot=(0.0, 0.0, 0.0, 1.0), sh0=(0.0, 0.0, 0.0, 1.0)) -> np.ndarray:
    """GaussianData{} with the defaults of ShaderStructs.h:59-70 (rot = (0,0,0,1), shCoeffs[0] = (0,0,0,1))."""
    g = np.zeros(FLOATS_PER_GAUSSIAN, dtype=np.float32)
    g[0:3] = position
    sc = np.asarray(scale, dtype=np.float32).reshape(-1)
    g[4:4 + sc.size] = sc
    g[8:12] = rot
    g[12:16] = sh0
    return g


class Scene:
    """Engine/Application/Scene.h:36-39."""

    def __init__(self, resourceManager: ResourceManager | None = None, aspect_ratio: float = 1280.0 / 720.0):
        self.resourceManager = resourceManager or ResourceManager()
        self.camera = Camera(aspect_ratio)

    def init(self):
        pass

    def update(self):
        self.camera.update()

    def getCamera(self) -> Camera:
        return self.camera

    def getResourceManager(self) -> ResourceManager:
        return self.resourceManager


SMATH_PI = float(np.float32(3.141592))     # SMath.cpp:4 -- not the float nearest to pi


def _msvc_rand(seed=1):
    state = seed
    while True:
        state = (state * 214013 + 2531011) & 0xFFFFFFFF
        yield (state >> 16) & 0x7FFF


def _rand_colour(rnd):
    """glm::vec4((rand() % 10000) / 10000.0f, ..., ..., 1.0f): the order in which the three arguments are evaluated is
    unspecified in C++; g++ (the cross-check of tests/golden/ref_glm_smath.json) and MSVC x64 go right to left, so the
    first draw lands in blue."""
    b, g, r = (np.float32((next(rnd) % 10000) / np.float32(10000.0)) for _ in range(3))
    return (r, g, b, 1.0)


class TestSortScene(Scene):
    """Scenes/TestSortScene.cpp:6-34 (colours: MSVC rand() with the default seed 1)."""

    __test__ = False

    def init(self):
        self.camera.setPosition((0.0, 0.0, 0.0))
        self.camera.setRotation(0.0, 0.0)
        self.camera.recalculate()
        rnd = _msvc_rand()
        near, far = np.float32(Camera.NEAR_PLANE), np.float32(Camera.FAR_PLANE)
        for i in range(64 * 3):
            keyDepth = np.uint32((i + 1) * 1024)
            zOffset = (np.float32(keyDepth) / np.float32(4294967295)) * (far - near) + near
            pos = (np.float32((np.float32(-8.0) + np.float32(i)) * np.float32(0.01)), 0.0, zOffset)
            self.resourceManager.addGaussian(makeGaussian(pos, (0.02, 0.02, 0.02, 0.02), sh0=_rand_colour(rnd)))


class SimpleTestGaussiansScene(Scene):
    """Scenes/SimpleTestGaussiansScene.cpp:6-29."""

    def init(self):
        self.camera.setPosition((0.0, 0.0, 2.0))
        self.camera.setRotation(SMATH_PI, 0.0)
        self.camera.recalculate()
        rnd = _msvc_rand()
        for i in range(16):
            self.resourceManager.addGaussian(
                makeGaussian((-8.0 + float(i), 0.0, -1.0), (0.1, 0.2, 0.5, 0.0), sh0=_rand_colour(rnd)))


class PlyScene(Scene):
    """GardenScene / TrainScene / BicycleScene (Scenes/*.cpp): benchmark camera pose + a .ply path."""

    POSES = {
        "garden": ((-0.620010, 0.189628, 2.271181), 2.971590, -1.074159),   # GardenScene.cpp:11-12
        "train": ((-2.857887, 0.188856, 1.048745), 1.361593, 0.005841),     # TrainScene.cpp:11-12
        "bicycle": ((0.945927, -0.294418, -0.181088), -1.108407, -0.324159), # BicycleScene.cpp:11-12
    }

    def __init__(self, name: str, plyPath: str, **kw):
        super().__init__(**kw)
        self.name, self.plyPath = name, plyPath

    def init(self):
        pos, yaw, pitch = self.POSES[self.name]
        self.camera.setPosition(pos)
        self.camera.setRotation(yaw, pitch)
        self.camera.recalculate()
        self.resourceManager.loadGaussians(self.plyPath)


def savePpm(path: str, rgba: np.ndarray):
    """Frame sink replacing the swapchain present (Subrenderer.cpp:292-345): binary PPM, RGB only."""
    img = np.ascontiguousarray(rgba[..., :3], dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def saveImage(path: str, rgba: np.ndarray):
    """The library's own sink (gs_write_image): .ppm or .png by extension; raises GsplatError on failure."""
    img = np.ascontiguousarray(rgba, dtype=np.uint8)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("saveImage wants an [H, W, 4] uint8 frame")
    rc = _lib.lib().gs_write_image(os.fsencode(path), _p(img), img.shape[1], img.shape[0])
    if rc != 0:
        raise GsplatError(rc, f"gs_write_image({path!r}) failed")


def write_ply(path: str, rows: np.ndarray, space: str = "records"):
    """gs_write_ply: rows (float32 (n, 84), host) as a binary .ply in the INRIA layout that ResourceManager.loadGaussians
    reads.  space="records": rows as the frame reads them (log and logit are taken here); space="raw": rows in the raw
    space of gs_adam_rows_raw_device, written as they are -- a lossless checkpoint.  Raises GsplatError on failure."""
    if space not in ("records", "raw"):
        raise ValueError(f"space must be 'records' or 'raw', not {space!r}")
    a = np.ascontiguousarray(rows, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != FLOATS_PER_GAUSSIAN:
        raise ValueError(f"rows must be (n, {FLOATS_PER_GAUSSIAN}), not {a.shape}")
    L = _lib.lib()
    rc = L.gs_write_ply(os.fsencode(path), _p(a), a.shape[0], _lib.GS_PLY_FROM_RAW if space == "raw" else _lib.GS_PLY_FROM_RECORDS)
    if rc != 0:
        raise GsplatError(rc, L.gs_ply_last_error().decode() if rc == _lib.GS_ERR_IO else f"gs_write_ply({path!r}): invalid argument")


CAMERA_CONSTANTS = ("near_plane", "far_plane", "ndc_cull", "in_view_limit", "fov_y")   # the five floats of gs_config


def _config(device: int = 0, render_mode: int = _lib.GS_RENDER_EXACT, record_timings=True,
            sort_algorithm: int = _lib.GS_SORT_RADIX4, render_kernel: int = _lib.GS_RENDER_KERNEL_AUTO,
            tile_order: int = _lib.GS_TILE_ORDER_LONGEST_FIRST, count_launches: int = _lib.GS_COUNT_AUTO,
            near_plane=None, far_plane=None, ndc_cull=None, in_view_limit=None, fov_y=None) -> GsConfig:
    """gs_default_config with these fields written over it.  near_plane .. fov_y: the camera constants of gs_config
    (include/gsplat.h); None keeps what gs_default_config wrote."""
    cfg = GsConfig()
    _lib.lib().gs_default_config(C.byref(cfg))
    cfg.device_ordinal = device
    cfg.render_mode = render_mode
    cfg.sort_algorithm = sort_algorithm     # GPU_SORT_ALGORITHM, Renderer.h:33
    cfg.render_kernel = render_kernel
    cfg.tile_order = tile_order
    cfg.count_launches = count_launches     # GS_COUNT_*: a Count launch per radix pass, or per sort (short lists)
    cfg.record_timings = int(record_timings)   # 0 off, 1 buckets, 2 buckets + per-Scatter events
    for name, value in zip(CAMERA_CONSTANTS, (near_plane, far_plane, ndc_cull, in_view_limit, fov_y)):
        if value is not None:
            setattr(cfg, name, float(value))
    return cfg


_CONFIG_OPTIONS = _config.__code__.co_varnames[:_config.__code__.co_argcount]     # the names of _config's parameters


class _Context:
    """Owns one gs_ctx, made from a finished gs_config (_config)."""

    def __init__(self, cfg: GsConfig):
        L = _lib.lib()
        self.cfg = cfg
        self.handle = C.c_void_p()
        rc = L.gs_create(C.byref(cfg), C.byref(self.handle))
        if rc != 0:
            raise GsplatError(rc, L.gs_last_error(None).decode())

    def check(self, rc: int, allow_warn: bool = True) -> int:
        if rc < 0 or (rc > 0 and not allow_warn):
            raise GsplatError(rc, _lib.lib().gs_last_error(self.handle).decode())
        return rc

    def close(self):
        if self.handle:
            handle, self.handle = self.handle, C.c_void_p()   # gs_destroy always frees the context: never touch it again
            _lib.lib().gs_destroy(handle)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GpuSort:
    """Sort/GpuSort.h:8-22."""

    def initForScene(self, maxNumSortElements: int, numTiles: int):
        raise NotImplementedError

    def computeSort(self, tile, depth, ident):
        raise NotImplementedError

    def gpuClearBuffers(self):
        pass

    def cleanup(self):
        pass


class RadixSort(GpuSort):
    """Sort/RadixSort.{h,cpp} used stand-alone on caller arrays (gs_sort_host)."""

    RS_BITS_PER_PASS = 4
    RS_BIN_COUNT = 16
    SORT_ALGORITHM = _lib.GS_SORT_RADIX4

    def __init__(self, device: int = 0, count_launches: int = _lib.GS_COUNT_AUTO):
        self._ctx = _Context(_config(device, sort_algorithm=self.SORT_ALGORITHM, count_launches=count_launches))
        self.maxNumSortElements = 0
        self.radixSortNumSortBits = 0

    @staticmethod
    def getMinNumBits(x: int) -> int:  # RadixSort.cpp:7-16
        return int(x).bit_length()

    def initForScene(self, maxNumSortElements: int, numTiles: int):  # RadixSort.cpp:144-205
        self.maxNumSortElements = int(maxNumSortElements)
        sortBits = 32 + self.getMinNumBits(numTiles - 1)
        self.radixSortNumSortBits = ((sortBits + 3) // 4) * 4

    def computeSort(self, tile, depth, ident):
        """Returns sorted copies (tile, depth, id); stable, by the low radixSortNumSortBits bits."""
        t = np.ascontiguousarray(tile, dtype=np.uint32).copy()
        d = np.ascontiguousarray(depth, dtype=np.uint32).copy()
        i = np.ascontiguousarray(ident, dtype=np.uint32).copy()
        if not (t.size == d.size == i.size):
            raise ValueError("tile/depth/id must have equal length")
        if t.size > self.maxNumSortElements:
            raise ValueError("more elements than initForScene allowed")
        self._ctx.check(_lib.lib().gs_sort_host(self._ctx.handle, _p(t), _p(d), _p(i), t.size,
                                                self.radixSortNumSortBits))
        return t, d, i

    def bench(self, n: int, numTiles: int, iters: int = 5, seed: int = 1):
        ms, ok = C.c_float(0), C.c_uint32(0)
        self._ctx.check(_lib.lib().gs_sort_bench(self._ctx.handle, n, numTiles, iters, seed,
                                                 C.byref(ms), C.byref(ok)))
        return float(ms.value), bool(ok.value)

    def cleanup(self):
        self._ctx.close()


class RadixSort8(RadixSort):
    """The A/B variant behind the same seam: 8-bit digits, half the passes, same result (GS_SORT_RADIX8)."""

    RS_BITS_PER_PASS = 8
    RS_BIN_COUNT = 256
    SORT_ALGORITHM = _lib.GS_SORT_RADIX8


class Renderer:
    """Renderer.{h,cpp}: init / initForScene / draw / cleanup and the GPU timing averages."""

    WAIT_ELAPSED_WARMUP_FRAMES_FOR_AVG = 1000   # Renderer.h:142
    WAIT_ELAPSED_FRAMES_FOR_AVG = 1000          # Renderer.h:143
    TILE_SIZE = 16                              # Renderer.h:146

    def __init__(self, width: int = 1280, height: int = 720, device: int = 0,
                 render_mode: int = _lib.GS_RENDER_EXACT, record_timings: bool = True,
                 warmup_frames: int | None = None, sort_algorithm: int = _lib.GS_SORT_RADIX4,
                 render_kernel: int = _lib.GS_RENDER_KERNEL_AUTO,
                 tile_order: int = _lib.GS_TILE_ORDER_LONGEST_FIRST, count_launches: int = _lib.GS_COUNT_AUTO,
                 near_plane: float | None = None, far_plane: float | None = None, ndc_cull: float | None = None,
                 in_view_limit: float | None = None, fov_y: float | None = None, antialias: bool = False):
        """antialias: setAntialias for the context init() creates.  near_plane, far_plane, ndc_cull, in_view_limit, fov_y: the camera constants of gs_config, fixed for the life of
        the context (None: gs_default_config's, the reference's).  proj drives the screen position, fov_y the covariance's
        focal lengths: INTEGRATION.md, "Real cameras".  self.cfg is the gs_config init() hands to gs_create."""
        given = locals()                                     # _config's options are arguments here under their own names
        self.cfg = _config(**{name: given[name] for name in _CONFIG_OPTIONS})
        self.width, self.height = int(width), int(height)   # swapchain extent (Engine.cpp:35)
        self._ctx: _Context | None = None
        self.resourceManager: ResourceManager | None = None
        self.numGaussians = 0
        self.numSortElements = 0
        self.frameSerial = 0        # counts the calls that launched a sort list: what was drawn before the last is gone
        self._outputs_mask = None   # the GS_OUTPUT_* mask setOutputs set last
        self.antialias = bool(antialias)
        self.warmupFrames = self.WAIT_ELAPSED_WARMUP_FRAMES_FOR_AVG if warmup_frames is None else warmup_frames
        self._reset_avgs()

    def _reset_avgs(self):
        self.elapsedFrames = 0
        self.avgInitSortListMs = self.avgSortMs = self.avgFindRangesMs = 0.0
        self.avgRenderGaussiansMs = self.avgTotalGpuTimeMs = 0.0

    # -- Renderer.cpp:688-694
    def init(self, resourceManager: ResourceManager):
        self.resourceManager = resourceManager
        self._ctx = _Context(self.cfg)
        if self.antialias:
            self.setAntialias(True)

    # -- Renderer.cpp:696-710
    def getNumTiles(self) -> int:
        return ((self.width + 15) // 16) * ((self.height + 15) // 16)

    @staticmethod
    def getCeilPowTwo(x: int) -> int:
        num = 1
        while num < x:
            num *= 2
        return num

    # -- Renderer.cpp:712-756
    def initForScene(self, scene: Scene | None = None, share_with: "Renderer | None" = None):
        """share_with: another Renderer whose uploaded gaussians this one renders too (gs_share_scene) -- the way
        to keep several frames in flight (GfxSettings::FRAMES_IN_FLIGHT, GfxSettings.h:15) without uploading the
        scene once per frame slot.  The arrays are reference-counted: clean the renderers up in any order."""
        assert self._ctx is not None, "Renderer.init() first"
        L = _lib.lib()
        if share_with is not None:
            assert share_with._ctx is not None
            self._ctx.check(L.gs_share_scene(self._ctx.handle, share_with._ctx.handle))
        else:
            g = self.resourceManager.getGaussians()
            if g.shape[0] == 0:
                raise GsplatError(_lib.GS_ERR_NO_SCENE, "no gaussians in the resource manager")
            g = np.ascontiguousarray(g, dtype=np.float32)
            self._ctx.check(L.gs_upload_gaussians(self._ctx.handle, _p(g), g.shape[0]))
        self._ctx.check(L.gs_set_resolution(self._ctx.handle, self.width, self.height))
        info = self.sceneInfo()
        self.numGaussians = info.num_gaussians
        self.numSortElements = info.capacity
        self._reset_avgs()

    def sceneInfo(self) -> GsSceneInfo:
        info = GsSceneInfo()
        self._ctx.check(_lib.lib().gs_get_scene_info(self._ctx.handle, C.byref(info)))
        return info

    def setTileRows(self, row_begin: int, row_end: int):
        self._ctx.check(_lib.lib().gs_set_tile_rows(self._ctx.handle, row_begin, row_end))

    def setTileRowsInterleaved(self, phase: int, stride: int, compact_output: bool = True):
        """Rank `phase` of `stride`: tile rows phase, phase + stride, ...; with compact_output drawDevice writes the
        rank's strip (owned rows packed) instead of addressing the whole frame."""
        self._ctx.check(_lib.lib().gs_set_tile_rows_interleaved(self._ctx.handle, phase, stride, int(compact_output)))

    def setBandGradients(self, enable: bool = True):
        """gs_set_band_gradients: with it on, a renderer that owns a band of tile rows (setTileRows*) serves backward*,
        visibleCount, backwardCamera* and contribDevice with the terms of its own pixels -- partial sums over the frame's tile
        rows, which the caller adds up over the bands (rowsAccumulateDevice / rowsCollectDevice).  Off (the default): refused."""
        self._ctx.check(_lib.lib().gs_set_band_gradients(self._ctx.handle, 1 if enable else 0))

    def setAntialias(self, enable: bool = True):
        """gs_set_antialias: the frames drawn from now on blend every splat at opacity * sqrt(det S / det(S + 0.3 I)), S its
        2-D covariance before the dilation (floored; include/gsplat.h) -- the opacity compensation of anti-aliased training.
        A host flag of this renderer's context; the last frame and its gradients stay those of the frame as drawn."""
        self._ctx.check(_lib.lib().gs_set_antialias(self._ctx.handle, 1 if enable else 0))
        self.antialias = bool(enable)

    def setAbsGradients(self, enable: bool = True):
        """gs_set_abs_gradients: with it on, every backward* also leaves, per list element, the sums over its tile's pixels
        of |dL_p/dsx| and |dL_p/dsy| (the AbsGS statistic) in the context's scratch, 8 bytes per list element of capacity;
        absScreenGradientDevice and densifyStatsAbsDevice read them.  What backward* returns does not change by a bit."""
        self._ctx.check(_lib.lib().gs_set_abs_gradients(self._ctx.handle, 1 if enable else 0))

    @staticmethod
    def _camera_args(cam: Camera):
        """view, proj, pos and sh_mode of a Camera, as _launch takes them."""
        return cam.getViewMatrix(), cam.getProjectionMatrix(), cam.getPosition(), int(cam.getShMode())

    def _launch(self, fn, view, proj, cam_pos, sh_mode, *tail) -> int:
        """fn = gs_render* or gs_debug_init_sort_list under the camera (view, proj: 16 floats, column-major; cam_pos: 3) with
        the arguments behind sh_mode in tail; returns the checked status."""
        v = np.ascontiguousarray(view, dtype=np.float32).reshape(16)
        p = np.ascontiguousarray(proj, dtype=np.float32).reshape(16)
        c = np.ascontiguousarray(cam_pos, dtype=np.float32).reshape(3)
        self.frameSerial += 1
        return self._ctx.check(fn(self._ctx.handle, _p(v), _p(p), _p(c), int(sh_mode), *tail))

    def drawCamera(self, view, proj, cam_pos, sh_mode: int, device_ptr: int | None = None, sync: bool = True) -> int:
        """drawDevice under a camera given by its matrices instead of a Scene; returns the status (also lastStatus)."""
        fn = _lib.lib().gs_render_device if sync else _lib.lib().gs_render_device_async
        self.lastStatus = self._launch(fn, view, proj, cam_pos, sh_mode, _vp(device_ptr))
        return self.lastStatus

    # -- Renderer.cpp:297-515
    def draw(self, scene: Scene, out: np.ndarray | None = None) -> np.ndarray:
        if out is None:
            out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self.lastStatus = self._launch(_lib.lib().gs_render, *self._camera_args(scene.getCamera()), _p(out))
        self._accumulate()
        return out

    def drawDevice(self, scene: Scene, device_ptr: int | None = None, sync: bool = True, compact_rows: bool = False):
        """Same frame with the image left in HBM (device_ptr = e.g. torch tensor .data_ptr()).  compact_rows only
        documents the call site: whether rows are packed is a property of the context (setTileRowsInterleaved)."""
        self.drawCamera(*self._camera_args(scene.getCamera()), device_ptr, sync)
        if sync:
            self._accumulate()

    def synchronize(self):
        self._ctx.check(_lib.lib().gs_synchronize(self._ctx.handle))

    def setStream(self, hip_stream: int | None):
        self._ctx.check(_lib.lib().gs_set_stream(self._ctx.handle, C.c_void_p(hip_stream or 0)))

    def timings(self) -> GsTimings:
        t = GsTimings()
        self._ctx.check(_lib.lib().gs_get_timings(self._ctx.handle, C.byref(t)))
        return t

    def hostTimings(self) -> dict:
        """RECORD_CPU_TIMES of the last draw (Renderer.cpp:399-456): waitForFence, recordCommandBuffer, present, CPU frame."""
        t = GsHostTimings()
        self._ctx.check(_lib.lib().gs_get_host_timings(self._ctx.handle, C.byref(t)))
        return {"wait_for_gpu": round(t.wait_ms, 4), "record_commands": round(t.record_ms, 4),
                "present": round(t.present_ms, 4), "cpu_frame": round(t.cpu_frame_ms, 4)}

    def _accumulate(self):  # Renderer.cpp:477-488
        t = self.timings()
        if self.elapsedFrames >= self.warmupFrames:
            w = 1.0 / (self.elapsedFrames - self.warmupFrames + 1.0)
            avg = lambda a, v: (1.0 - w) * a + w * v   # getNewAvgTime, Renderer.h:134
            self.avgInitSortListMs = avg(self.avgInitSortListMs, t.init_sort_list_ms)
            self.avgSortMs = avg(self.avgSortMs, t.radix_sort_ms)
            self.avgFindRangesMs = avg(self.avgFindRangesMs, t.find_ranges_ms)
            self.avgRenderGaussiansMs = avg(self.avgRenderGaussiansMs, t.render_ms)
            self.avgTotalGpuTimeMs = avg(self.avgTotalGpuTimeMs, t.total_ms)
        self.elapsedFrames += 1

    # -- stage-level read-back (no reference counterpart)
    def debugInitSortList(self, scene: Scene) -> int:
        return self._launch(_lib.lib().gs_debug_init_sort_list, *self._camera_args(scene.getCamera()))

    def debugRead(self, which: int) -> np.ndarray:
        info = self.sceneInfo()
        L = _lib.lib()
        if which == _lib.BUF_COUNT:
            a = np.zeros(1, dtype=np.uint64)
        elif which in (_lib.BUF_COLOR, _lib.BUF_COV):
            a = np.zeros((info.num_gaussians, 4), dtype=np.float32)
        elif which == _lib.BUF_RASTER_OPACITY:
            a = np.zeros(info.num_gaussians, dtype=np.float32)
        elif which == _lib.BUF_RANGES:
            a = np.zeros((info.tiles_x * info.tiles_y, 2), dtype=np.uint32)
        elif which == _lib.BUF_WAVE_WROTE:
            a = np.zeros((info.num_gaussians + 63) // 64, dtype=np.uint8)
        elif which == _lib.BUF_TILE_ORDER:
            a = np.zeros(info.rows_owned * info.tiles_x, dtype=np.uint32)
        elif which == _lib.BUF_PASS0_OFFSETS:    # the rows of the blocks, then the sixteen digit bases
            a = np.zeros(((info.num_gaussians + 255) // 256 + 1, 16), dtype=np.uint32)
        elif which == _lib.BUF_BACKWARD_ROWS:    # dsx, dsy, dix, diy, diz, dcol[3], dop, dz per splat (bwd_chain's row)
            a = np.zeros((info.num_gaussians, 10), dtype=np.float32)
        elif which == _lib.BUF_BAND_BLOCKS:      # word 0 is the count: read it, then the records behind it
            cnt = np.zeros(1, dtype=np.uint32)
            self._ctx.check(L.gs_debug_read(self._ctx.handle, which, _p(cnt), 4))
            a = np.zeros(1 + int(cnt[0]), dtype=np.uint32)
            self._ctx.check(L.gs_debug_read(self._ctx.handle, which, _p(a), a.nbytes))
            return a[1:]
        elif which == _lib.BUF_IMAGE:
            a = np.zeros((info.height, info.width, 4), dtype=np.uint8)
        else:
            cnt = np.zeros(1, dtype=np.uint64)
            self._ctx.check(L.gs_debug_read(self._ctx.handle, _lib.BUF_COUNT, _p(cnt), 8))
            e = int(min(int(cnt[0]), info.capacity))
            a = np.zeros(e, dtype=np.uint32)
        if a.nbytes:
            self._ctx.check(L.gs_debug_read(self._ctx.handle, which, _p(a), a.nbytes))
        return a

    # -- optional per-pixel outputs (no reference counterpart; include/gsplat.h, GS_OUTPUT_*)
    def setOutputs(self, rgba32f: bool = False, depth: bool = False):
        """What every later frame leaves beside the RGBA8 image: rgba32f = premultiplied colour before the clamp + alpha
        (1 - final transmittance), depth = the blend of the splats' view depths with the colour's weights (expected depth =
        depth / alpha).  Both off (the default) = the RGBA8 frame alone."""
        mask = (_lib.GS_OUTPUT_RGBA32F if rgba32f else 0) | (_lib.GS_OUTPUT_DEPTH if depth else 0)
        self._ctx.check(_lib.lib().gs_set_outputs(self._ctx.handle, mask))
        self._outputs_mask = mask

    def ensureOutputs(self, mask: int):
        """setOutputs for the GS_OUTPUT_* mask, unless it is the mask setOutputs set last (the call waits for the stream)."""
        if mask != self._outputs_mask:
            self.setOutputs(rgba32f=bool(mask & _lib.GS_OUTPUT_RGBA32F), depth=bool(mask & _lib.GS_OUTPUT_DEPTH))

    def readOutput(self, which: int) -> np.ndarray:
        """The last frame's GS_OUTPUT_RGBA32F (float32 (H, W, 4)) or GS_OUTPUT_DEPTH (float32 (H, W)) buffer."""
        info = self.sceneInfo()
        shape = (info.height, info.width, 4) if which == _lib.GS_OUTPUT_RGBA32F else (info.height, info.width)
        a = np.zeros(shape, dtype=np.float32)
        self._ctx.check(_lib.lib().gs_read_output(self._ctx.handle, int(which), _p(a), a.nbytes))
        return a

    def outputDevicePtr(self, which: int) -> int:
        """Device address of that buffer (same layout as readOutput); valid until the next setOutputs, resolution or
        tile-row change.  Its contents are the last enqueued frame's once synchronize() has returned."""
        dev, size = C.c_void_p(), C.c_size_t()
        self._ctx.check(_lib.lib().gs_output_device(self._ctx.handle, int(which), C.byref(dev), C.byref(size)))
        return int(dev.value)

    # -- gradients of a frame (no reference counterpart; include/gsplat.h, gs_backward*)
    def _grad_args(self, grad_rgba32f, grad_depth):
        """dL/dRGBA32F (H, W, 4) and dL/dDEPTH (H, W) or None as contiguous float32 of the frame's shape."""
        info = self.sceneInfo()
        g = np.ascontiguousarray(grad_rgba32f, dtype=np.float32)
        if g.shape != (info.height, info.width, 4):
            raise ValueError(f"grad_rgba32f must have shape {(info.height, info.width, 4)}, not {g.shape}")
        d = None
        if grad_depth is not None:
            d = np.ascontiguousarray(grad_depth, dtype=np.float32)
            if d.shape != (info.height, info.width):
                raise ValueError(f"grad_depth must have shape {(info.height, info.width)}, not {d.shape}")
        return g, d

    def backward(self, grad_rgba32f: np.ndarray, grad_depth: np.ndarray | None = None) -> np.ndarray:
        """dL/d(record), float32 (N, 84) in the record layout of setGaussians, of the last frame drawn (GS_RENDER_EXACT, whole
        frame) from dL/dRGBA32F (float32 (H, W, 4)) and optionally dL/dDEPTH (float32 (H, W)): the quantities of
        setOutputs(rgba32f=True, depth=True), whether or not they are enabled."""
        g, d = self._grad_args(grad_rgba32f, grad_depth)
        out = np.zeros((self.sceneInfo().num_gaussians, FLOATS_PER_GAUSSIAN), dtype=np.float32)
        self._ctx.check(_lib.lib().gs_backward(self._ctx.handle, _p(g), None if d is None else _p(d), _p(out)))
        return out

    def backwardDevice(self, grad_rgba32f_ptr: int, grad_depth_ptr: int | None, grad_records_ptr: int):
        """The same with device addresses (float32 (H, W, 4), (H, W) or None, (N, 84)); enqueued on the context's stream
        without waiting (synchronize() waits)."""
        self._ctx.check(_lib.lib().gs_backward_device(self._ctx.handle, C.c_void_p(grad_rgba32f_ptr),
                                                      _vp(grad_depth_ptr),
                                                      C.c_void_p(grad_records_ptr)))

    def visibleCount(self) -> int:
        """|V|: how many splats the last frame rasterised (tiles_touched != 0); waits for the context's stream."""
        count = C.c_uint32()
        self._ctx.check(_lib.lib().gs_visible_count(self._ctx.handle, C.byref(count)))
        return int(count.value)

    def backwardVisible(self, grad_rgba32f: np.ndarray, grad_depth: np.ndarray | None = None, max_rows: int | None = None):
        """backward() for the splats the frame rasterised alone: (ids uint32 (k,), rows float32 (k, 84), count) with ids
        ascending, rows[i] = backward()[ids[i]] bit for bit, count = |V| and k = min(count, max_rows).  max_rows=None sizes
        with visibleCount().  lastStatus is GS_WARN_OVERFLOW when count > max_rows."""
        g, d = self._grad_args(grad_rgba32f, grad_depth)
        if max_rows is None:
            max_rows = self.visibleCount()
        max_rows = int(max_rows)
        ids = np.zeros(max_rows, dtype=np.uint32)
        rows = np.zeros((max_rows, FLOATS_PER_GAUSSIAN), dtype=np.float32)
        count = C.c_uint32()
        self.lastStatus = self._ctx.check(_lib.lib().gs_backward_visible(
            self._ctx.handle, _p(g), None if d is None else _p(d), _p(ids) if max_rows else None,
            _p(rows) if max_rows else None, max_rows, C.byref(count)))
        k = min(int(count.value), max_rows)
        return ids[:k], rows[:k], int(count.value)

    def backwardVisibleDevice(self, grad_rgba32f_ptr: int, grad_depth_ptr: int | None, ids_ptr: int | None,
                              rows_ptr: int | None, max_rows: int, count_ptr: int):
        """The same with device addresses (ids: uint32 (max_rows,), rows: float32 (max_rows, 84), count: one uint32);
        enqueued on the context's stream without waiting.  The caller compares the count with max_rows after
        synchronize()."""
        self._ctx.check(_lib.lib().gs_backward_visible_device(
            self._ctx.handle, C.c_void_p(grad_rgba32f_ptr), _vp(grad_depth_ptr),
            _vp(ids_ptr), _vp(rows_ptr), int(max_rows),
            _vp(count_ptr)))

    def backwardCamera(self) -> np.ndarray:
        """The camera's gradients of the last frame, float32 (35,): [0:16] dL/dview, [16:32] dL/dproj (both column-major, as
        drawCamera takes the matrices), [32:35] dL/dcam_pos -- with the dL/d(outputs) the last backward*() on this frame was
        given (gs_backward_camera; a backward form that computed rows must have run on the frame).  The view's bottom row and
        the projection's clip-z row are exactly 0 (include/gsplat.h)."""
        out = np.zeros(_lib.CAMERA_GRAD_FLOATS, dtype=np.float32)
        self._ctx.check(_lib.lib().gs_backward_camera(self._ctx.handle, _p(out)))
        return out

    def backwardCameraDevice(self, grad_camera_ptr: int):
        """The same into 35 float32 at a device address; enqueued on the context's stream without waiting."""
        self._ctx.check(_lib.lib().gs_backward_camera_device(self._ctx.handle, _vp(grad_camera_ptr)))

    # -- photometric loss of a frame (no reference counterpart; include/gsplat.h, gs_photometric_loss*)
    @staticmethod
    def _bg_arg(bg):
        """bg as three contiguous float32 (kept alive by the caller for the call) or None."""
        if bg is None:
            return None
        b = np.ascontiguousarray(bg, dtype=np.float32)
        if b.shape != (3,):
            raise ValueError(f"bg must have 3 components, not shape {b.shape}")
        return b

    def photometricLoss(self, rgba: np.ndarray | None, target: np.ndarray, lam: float = 0.2, bg=None, want_grad: bool = True):
        """(1 - lam) * L1 + lam * (1 - SSIM) of rgba (float32 (H, W, 4): the quantities of setOutputs(rgba32f=True); None =
        the context's own buffer of the last frame) over the background bg (3 floats, None = black) against target (float32
        (H, W, 3)).  Returns (numbers, grad): numbers = float32 (3,) {loss, L1, DSSIM}; grad = dloss/d(rgba) float32 (H, W, 4)
        as backward() takes it, or None with want_grad=False."""
        info = self.sceneInfo()
        a = None
        if rgba is not None:
            a = np.ascontiguousarray(rgba, dtype=np.float32)
            if a.shape != (info.height, info.width, 4):
                raise ValueError(f"rgba must have shape {(info.height, info.width, 4)}, not {a.shape}")
        t = np.ascontiguousarray(target, dtype=np.float32)
        if t.shape != (info.height, info.width, 3):
            raise ValueError(f"target must have shape {(info.height, info.width, 3)}, not {t.shape}")
        b = self._bg_arg(bg)
        numbers = np.zeros(3, dtype=np.float32)
        grad = np.zeros((info.height, info.width, 4), dtype=np.float32) if want_grad else None
        self._ctx.check(_lib.lib().gs_photometric_loss(self._ctx.handle, None if a is None else _p(a), _p(t), float(lam),
                                                       None if b is None else _p(b), _p(numbers),
                                                       None if grad is None else _p(grad)))
        return numbers, grad

    def photometricLossDevice(self, rgba_ptr: int | None, target_ptr: int, lam: float, bg, loss_ptr: int, grad_ptr: int | None):
        """The same with device addresses (rgba: float32 (H, W, 4) or None for the context's own buffer, target: (H, W, 3),
        loss: 3 floats, grad: (H, W, 4) or None); bg stays a host value.  Enqueued on the context's stream without waiting."""
        b = self._bg_arg(bg)
        self._ctx.check(_lib.lib().gs_photometric_loss_device(
            self._ctx.handle, _vp(rgba_ptr), _vp(target_ptr),
            float(lam), None if b is None else _p(b), _vp(loss_ptr),
            _vp(grad_ptr)))

    def uploadDevice(self, ptr: int, n: int):
        """Gaussian records (float32 (n, 84)) from device memory.  With the scene's n: rewritten in place on the context's
        stream, resolution kept; with another n: a new scene, and the resolution is set again here."""
        same = self.sceneInfo().num_gaussians == int(n)
        self._ctx.check(_lib.lib().gs_upload_gaussians_device(self._ctx.handle, C.c_void_p(int(ptr)), int(n)))
        if not same:
            self._ctx.check(_lib.lib().gs_set_resolution(self._ctx.handle, self.width, self.height))
            info = self.sceneInfo()
            self.numGaussians, self.numSortElements = info.num_gaussians, info.capacity

    # -- one optimiser step on the listed rows (no reference counterpart; include/gsplat.h, gs_adam_rows_device)
    def adamRowsDevice(self, records_ptr: int, m_ptr: int, v_ptr: int, n: int, ids_ptr: int, rows_ptr: int, count_ptr: int,
                       max_rows: int, params: GsAdamParams):
        """Adam on rows ids[i], i < min(count, max_rows), of the caller's records, m and v (device addresses, float32 (n, 84))
        with the gradient rows (max_rows, 84); ids, rows and count as backwardVisibleDevice left them.  params:
        default_adam_params(), with `step` = the number of this step, counted from 1.  Enqueued on the context's stream
        without waiting."""
        self._ctx.check(_lib.lib().gs_adam_rows_device(self._ctx.handle, _vp(records_ptr), _vp(m_ptr), _vp(v_ptr), int(n), _vp(ids_ptr),
                                                       _vp(rows_ptr), _vp(count_ptr), int(max_rows), C.byref(params)))

    def uploadRowsDevice(self, ptr: int, n: int, ids_ptr: int, count_ptr: int, max_rows: int):
        """uploadDevice for the listed rows alone: the planes of splats ids[i], i < min(count, max_rows), rewritten in place from
        the records at ptr (float32 (n, 84), n = the scene's).  Enqueued on the context's stream without waiting."""
        self._ctx.check(_lib.lib().gs_upload_rows_device(self._ctx.handle, _vp(ptr), int(n), _vp(ids_ptr), _vp(count_ptr), int(max_rows)))

    # -- the raw parameter space (no reference counterpart; include/gsplat.h, gs_adam_rows_raw_device and the calls around it)
    def adamRowsRawDevice(self, raw_ptr: int, records_ptr: int, m_ptr: int, v_ptr: int, n: int, ids_ptr: int, rows_ptr: int,
                          count_ptr: int, max_rows: int, params: GsAdamParams):
        """adamRowsDevice in raw space: the gradient rows (with respect to the records, as backwardVisibleDevice left them)
        are chained to log-scale, logit-opacity and the rotation before normalisation, Adam moves raw, m and v (the
        clamps of params apply to the raw values), and the listed rows of records are rewritten as act(raw).  params:
        default_adam_params(space="raw").  Enqueued on the context's stream without waiting."""
        self._ctx.check(_lib.lib().gs_adam_rows_raw_device(
            self._ctx.handle, _vp(raw_ptr), _vp(records_ptr), _vp(m_ptr), _vp(v_ptr), int(n), _vp(ids_ptr), _vp(rows_ptr), _vp(count_ptr),
            int(max_rows), C.byref(params)))

    def recordsFromRawDevice(self, raw_ptr: int, records_ptr: int, n: int):
        """records = act(raw) on the 59 fields of all n rows (exp of the log-scales, sigmoid of the logit, the rotation
        normalised).  Device addresses, float32 (n, 84).  Enqueued on the context's stream without waiting."""
        self._ctx.check(_lib.lib().gs_records_from_raw_device(self._ctx.handle, _vp(raw_ptr), _vp(records_ptr), int(n)))

    def rawFromRecordsDevice(self, records_ptr: int, raw_ptr: int, n: int):
        """The inverse: raw = (log of the scales, logit of the opacity clamped to [2^-24, 1 - 2^-24], everything else the
        same bits).  Enqueued on the context's stream without waiting."""
        self._ctx.check(_lib.lib().gs_raw_from_records_device(self._ctx.handle, _vp(records_ptr), _vp(raw_ptr), int(n)))

    def resetOpacityRawDevice(self, raw_ptr: int, records_ptr: int, m_ptr: int | None, v_ptr: int | None, n: int,
                              max_opacity: float = 0.01):
        """The INRIA opacity reset: every opacity above max_opacity becomes sigmoid(logit(max_opacity)) in records and its
        logit in raw; float 15 of every row of m and v (both given or both None) becomes 0.  Follow it with a full upload.
        Enqueued on the context's stream without waiting."""
        self._ctx.check(_lib.lib().gs_reset_opacity_raw_device(self._ctx.handle, _vp(raw_ptr), _vp(records_ptr), _vp(m_ptr), _vp(v_ptr),
                                                               int(n), float(max_opacity)))

    # -- adaptive density control (no reference counterpart; include/gsplat.h, gs_densify_stats_device / gs_densify_device)
    def densifyStatsDevice(self, ids_ptr: int, count_ptr: int, max_rows: int, n: int, grad_accum_ptr: int, seen_ptr: int,
                           max_radius_ptr: int):
        """The statistics of the step just differentiated, into the caller's device arrays (float32, uint32, float32 of n):
        for ids[i], i < min(count, max_rows), as backwardVisibleDevice left them for this frame, grad_accum += the norm of
        the screen-position gradient in NDC units, seen += 1, max_radius = max(itself, the screen radius in pixels).
        Enqueued on the context's stream without waiting."""
        self._ctx.check(_lib.lib().gs_densify_stats_device(self._ctx.handle, _vp(ids_ptr), _vp(count_ptr), int(max_rows), int(n),
                                                           _vp(grad_accum_ptr), _vp(seen_ptr), _vp(max_radius_ptr)))

    def absScreenGradientDevice(self, ids_ptr: int, count_ptr: int, max_rows: int, abs_out_ptr: int):
        """abs_out[i] (float32 (max_rows, 2) on the device) = the sums of |dL_p/dsx| and |dL_p/dsy| over the pixels that blend
        splat ids[i], i < min(count, max_rows), in pixel units, from the last backward* run with setAbsGradients on; (0, 0)
        for an id >= n.  A band renderer with setBandGradients on gives the partial sums of its pixels, which add up over
        bands.  Enqueued on the context's stream without waiting."""
        self._ctx.check(_lib.lib().gs_abs_screen_gradient_device(self._ctx.handle, _vp(ids_ptr), _vp(count_ptr), int(max_rows),
                                                                 _vp(abs_out_ptr)))

    def densifyStatsAbsDevice(self, ids_ptr: int, count_ptr: int, max_rows: int, n: int, grad_accum_abs_ptr: int):
        """grad_accum_abs (float32 of n, the caller's) += the norm of the absolute pair in NDC units, for the ids
        densifyStatsDevice takes and beside it (seen and max_radius stay with that call).  Enqueued on the context's stream
        without waiting."""
        self._ctx.check(_lib.lib().gs_densify_stats_abs_device(self._ctx.handle, _vp(ids_ptr), _vp(count_ptr), int(max_rows), int(n),
                                                               _vp(grad_accum_abs_ptr)))

    def densifyDevice(self, records_ptr: int, m_ptr: int | None, v_ptr: int | None, n: int, grad_accum_ptr: int, seen_ptr: int,
                      max_radius_ptr: int, params: GsDensifyParams, records_out_ptr: int, m_out_ptr: int | None,
                      v_out_ptr: int | None, max_out: int, counts_ptr: int):
        """The new cloud (clone, split, prune: gs_densify_device) from records / m / v (n, 84) and the statistics into
        records_out / m_out / v_out (max_out, 84), the children beside their parents; counts (4 uint32 on the device) =
        outputs (not truncated), cloned, split, pruned.  m, v, m_out and v_out: all given or all None.  params:
        default_densify_params().  Enqueued on the context's stream without waiting; needs no scene."""
        self._ctx.check(_lib.lib().gs_densify_device(
            self._ctx.handle, _vp(records_ptr), _vp(m_ptr), _vp(v_ptr), int(n), _vp(grad_accum_ptr), _vp(seen_ptr), _vp(max_radius_ptr),
            C.byref(params), _vp(records_out_ptr), _vp(m_out_ptr), _vp(v_out_ptr), int(max_out), _vp(counts_ptr)))

    # -- pruning by contribution (no reference counterpart; include/gsplat.h, gs_contrib_device / gs_prune_below_device)
    def contribDevice(self, n: int, wmax_ptr: int, wsum_ptr: int | None = None, pixels_ptr: int | None = None):
        """The blend weights w = T * alpha of the last frame, per splat, accumulated into the caller's device arrays of n
        (zeros before the first frame): wmax (float32) = max(itself, the largest w), wsum (float32, or None) += the sum in
        the header's fixed order, pixels (uint32, or None) += the number of (pixel, entry) pairs, saturating.  A splat that
        adds colour to no pixel is not touched.  Enqueued on the context's stream without waiting."""
        self._ctx.check(_lib.lib().gs_contrib_device(self._ctx.handle, int(n), _vp(wmax_ptr), _vp(wsum_ptr), _vp(pixels_ptr)))

    def pruneBelowDevice(self, score_ptr: int, threshold: float, n: int, records_ptr: int, raw_ptr: int | None, m_ptr: int | None,
                         v_ptr: int | None, records_out_ptr: int | None, raw_out_ptr: int | None, m_out_ptr: int | None,
                         v_out_ptr: int | None, max_out: int, counts_ptr: int):
        """The rows g with score[g] >= threshold (score: float32 (n,); a NaN is dropped) of records / raw / m / v (n, 84)
        copied bit for bit, in order, to the first rows of records_out / raw_out / m_out / v_out (max_out, 84); counts (2
        uint32 on the device) = kept (not truncated), dropped.  raw, m and v: each None together with its output.  Enqueued
        on the context's stream without waiting; needs no scene."""
        self._ctx.check(_lib.lib().gs_prune_below_device(
            self._ctx.handle, _vp(score_ptr), float(threshold), int(n), _vp(records_ptr), _vp(raw_ptr), _vp(m_ptr), _vp(v_ptr),
            _vp(records_out_ptr), _vp(raw_out_ptr), _vp(m_out_ptr), _vp(v_out_ptr), int(max_out), _vp(counts_ptr)))

    # -- MCMC (no reference counterpart; include/gsplat.h, gs_relocate_device / gs_grow_device / gs_position_noise_device)
    def relocateDevice(self, records_ptr: int, raw_ptr: int | None, m_ptr: int | None, v_ptr: int | None, n: int,
                       min_opacity: float, seed: int, ids_out_ptr: int | None, max_rows: int, counts_ptr: int):
        """3DGS-MCMC relocation in place on records / raw / m / v (n, 84; raw None, m and v None together): every splat with
        opacity <= min_opacity receives the row of a live one drawn in proportion to its opacity, the opacity and scales of
        every copy corrected so that the picture stays.  ids_out (max_rows uint32) = the changed rows, ascending; counts (3
        uint32 on the device) = changed (not truncated), dead, sources -- what uploadRowsDevice takes.  Enqueued on the
        context's stream without waiting; needs no scene."""
        self._ctx.check(_lib.lib().gs_relocate_device(
            self._ctx.handle, _vp(records_ptr), _vp(raw_ptr), _vp(m_ptr), _vp(v_ptr), int(n), float(min_opacity),
            int(seed) & 0xFFFFFFFFFFFFFFFF, _vp(ids_out_ptr), int(max_rows), _vp(counts_ptr)))

    def growDevice(self, records_ptr: int, raw_ptr: int | None, m_ptr: int | None, v_ptr: int | None, n: int, min_opacity: float,
                   seed: int, n_add: int, records_out_ptr: int | None, raw_out_ptr: int | None, m_out_ptr: int | None,
                   v_out_ptr: int | None, max_out: int, counts_ptr: int):
        """The cloud grown by n_add rows (gs_grow_device): n_add live splats drawn in proportion to their opacity, every
        drawn splat's copies beside it in records_out / raw_out / m_out / v_out (max_out, 84) with the relocation values and
        zero moments, every other row copied bit for bit; counts (2 uint32 on the device) = outputs, sources.  raw, m and v:
        each None together with its output.  Enqueued on the context's stream without waiting; needs no scene."""
        self._ctx.check(_lib.lib().gs_grow_device(
            self._ctx.handle, _vp(records_ptr), _vp(raw_ptr), _vp(m_ptr), _vp(v_ptr), int(n), float(min_opacity),
            int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_add), _vp(records_out_ptr), _vp(raw_out_ptr), _vp(m_out_ptr), _vp(v_out_ptr),
            int(max_out), _vp(counts_ptr)))

    def positionNoiseDevice(self, records_ptr: int, raw_ptr: int | None, n: int, ids_ptr: int | None, count_ptr: int | None,
                            max_rows: int, scale: float, gate_k: float = 100.0, gate_x0: float = 0.995, seed: int = 0):
        """3DGS-MCMC exploration noise on the positions of rows ids[i], i < min(count, max_rows) -- every row with ids None --
        of records and (the same bits) raw: Sigma z of the splat's own covariance, gated by its opacity, times scale (the
        caller's noise_lr * lr[GS_ADAM_POSITION]).  Enqueued on the context's stream without waiting; needs no scene."""
        self._ctx.check(_lib.lib().gs_position_noise_device(
            self._ctx.handle, _vp(records_ptr), _vp(raw_ptr), int(n), _vp(ids_ptr), _vp(count_ptr), int(max_rows), float(scale),
            float(gate_k), float(gate_x0), int(seed) & 0xFFFFFFFFFFFFFFFF))

    # -- several views per optimiser step (no reference counterpart; include/gsplat.h, gs_rows_accumulate_device / gs_rows_collect_device)
    def rowsAccumulateDevice(self, acc_ptr: int, mark_ptr: int, n: int, ids_ptr: int, rows_ptr: int, count_ptr: int, max_rows: int,
                             weight: float = 1.0):
        """The listed rows of one frame (ids, rows, count as backwardVisibleDevice left them) times weight, summed into the
        caller's accumulator acc (float32 (n, 84)) on the 59 fields: a store where mark (uint32 (n,), zeros before the first
        frame of a batch) is 0, an add elsewhere; then mark += 1 on the listed splats.  Device addresses.  Enqueued on the
        context's stream without waiting; needs no scene."""
        self._ctx.check(_lib.lib().gs_rows_accumulate_device(self._ctx.handle, _vp(acc_ptr), _vp(mark_ptr), int(n), _vp(ids_ptr),
                                                             _vp(rows_ptr), _vp(count_ptr), int(max_rows), float(weight)))

    def rowsCollectDevice(self, acc_ptr: int, mark_ptr: int, n: int, ids_out_ptr: int | None, rows_out_ptr: int | None, max_rows: int,
                          count_out_ptr: int):
        """The splats with a non-zero mark, ascending, as one list: ids_out (uint32 (max_rows,)), rows_out (float32 (max_rows, 84):
        the fields of acc, +0 elsewhere) and count_out (their number, not clamped) -- what adamRowsDevice and uploadRowsDevice
        take; mark is zero afterwards, and the sums of rows beyond max_rows are dropped.  max_rows == 0 with ids_out and
        rows_out None only counts (and clears).  Enqueued on the context's stream without waiting; needs no scene."""
        self._ctx.check(_lib.lib().gs_rows_collect_device(self._ctx.handle, _vp(acc_ptr), _vp(mark_ptr), int(n), _vp(ids_out_ptr),
                                                          _vp(rows_out_ptr), int(max_rows), _vp(count_out_ptr)))

    # -- a cloud from points (no reference counterpart; include/gsplat.h, gs_knn_mean_dist2_device / gs_records_from_points_device)
    def knnMeanDist2Device(self, points_ptr: int, n: int, dist2_out_ptr: int):
        """dist2_out[i] = the mean of the three smallest squared distances from point i to the other points, exact, in input
        order.  Device addresses: float32 (n, 3) and (n,).  Enqueued on the context's stream without waiting; needs no scene."""
        self._ctx.check(_lib.lib().gs_knn_mean_dist2_device(self._ctx.handle, _vp(points_ptr), int(n), _vp(dist2_out_ptr)))

    def recordsFromPointsDevice(self, points_ptr: int, colors_ptr: int | None, n: int, params: GsInitParams, records_out_ptr: int,
                                order_out_ptr: int | None = None):
        """The first records of a training run from points in the .ply's frame (and colours in [0, 1], or None): scale from
        the three nearest neighbours, params.opacity, identity rotation, SH DC from the colour, rows in the loader's
        Morton order; order_out (uint32 (n,), or None) = the input index of every output row.  Device addresses; params:
        default_init_params().  Enqueued on the context's stream without waiting; needs no scene."""
        self._ctx.check(_lib.lib().gs_records_from_points_device(
            self._ctx.handle, _vp(points_ptr), _vp(colors_ptr), int(n), C.byref(params), _vp(records_out_ptr), _vp(order_out_ptr)))

    # -- Renderer.cpp:230-270
    def cleanup(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None
