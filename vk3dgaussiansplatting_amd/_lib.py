"""ctypes loader for the in-tree libgsplat_hip.so (C-ABI in include/gsplat.h).

The product path has no CPU fallback: if the HIP library is missing or cannot be loaded this
module raises; it never imports anything from oracle/.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("GS_LIB_OVERRIDE") or os.path.join(CSRC, "libgsplat_hip.so")   # override: tuning builds only

GS_OK = 0
GS_WARN_OVERFLOW = 1
GS_ERR_INVALID = -1
GS_ERR_HIP = -2
GS_ERR_NO_SCENE = -3
GS_ERR_IO = -4
GS_ERR_FORMAT = -5
GS_ERR_NO_DEVICE = -6

GS_RENDER_EXACT = 0
GS_RENDER_FAST = 1
GS_RENDER_KERNEL_AUTO, GS_RENDER_KERNEL_WAVE_1PX, GS_RENDER_KERNEL_WAVE_2PX = 0, 1, 2
GS_RENDER_KERNEL_WAVE_4PX, GS_RENDER_KERNEL_WORKGROUP, GS_RENDER_KERNEL_WORKGROUP_8X8 = 4, 16, 17
GS_TILE_ORDER_LONGEST_FIRST, GS_TILE_ORDER_RASTER = 0, 1
GS_COUNT_AUTO, GS_COUNT_PER_PASS, GS_COUNT_FED = 0, 1, 2
GS_SORT_RADIX4 = 0
GS_SORT_TILE_BUCKET = 1
GS_SORT_RADIX4_SPLAT_FIRST = 2
GS_SORT_RADIX8 = 3
GS_SORT_RADIX8_SPLAT_FIRST = 4
GS_OUTPUT_RGBA32F, GS_OUTPUT_DEPTH = 1, 2   # gs_set_outputs mask bits / gs_read_output `which`

(BUF_SORTED_TILE, BUF_SORTED_DEPTH, BUF_SORTED_ID, BUF_RANGES, BUF_COLOR, BUF_COV, BUF_COUNT,
 BUF_UNSORTED_TILE, BUF_UNSORTED_DEPTH, BUF_UNSORTED_ID, BUF_IMAGE) = range(11)
BUF_RASTER_OPACITY = 11
BUF_WAVE_WROTE, BUF_BAND_BLOCKS, BUF_TILE_ORDER = 12, 13, 14   # the work the last frame skipped (include/gsplat.h)
BUF_PASS0_OFFSETS = 15      # the scanned digit rows of a frame whose k_emit did pass 0 of the depth sort
BUF_BACKWARD_ROWS = 16      # float[N][10]: the summed rows the per-splat chain of the last gs_backward* consumed

RECORD_BYTES = 336

# field groups of gs_adam_params (GS_ADAM_*): the 59 floats of the 84-float record gs_backward gives gradients to
GS_ADAM_POSITION, GS_ADAM_SCALE, GS_ADAM_ROTATION, GS_ADAM_SH_DC, GS_ADAM_OPACITY, GS_ADAM_SH_REST = range(6)
GS_ADAM_GROUPS = 6
GS_PLY_FROM_RECORDS, GS_PLY_FROM_RAW = 0, 1   # gs_write_ply `space`: rows as the frame reads them / in the raw space
# group of every float of a record; -1: one of the 25 floats gs_adam_rows_device and gs_upload_rows_device never touch
ADAM_GROUP_OF_FLOAT = tuple(
    [GS_ADAM_POSITION] * 3 + [-1] + [GS_ADAM_SCALE] * 3 + [-1] + [GS_ADAM_ROTATION] * 4 + [GS_ADAM_SH_DC] * 3 + [GS_ADAM_OPACITY]
    + ([GS_ADAM_SH_REST] * 3 + [-1]) * 15 + [-1] * 8)


class GsConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device_ordinal", C.c_int32),
        ("tile_size", C.c_uint32),
        ("near_plane", C.c_float),
        ("far_plane", C.c_float),
        ("ndc_cull", C.c_float),
        ("in_view_limit", C.c_float),
        ("fov_y", C.c_float),
        ("sort_algorithm", C.c_uint32),
        ("render_mode", C.c_uint32),
        ("record_timings", C.c_uint32),
        ("render_kernel", C.c_uint32),
        ("tile_order", C.c_uint32),
        ("count_launches", C.c_uint32),
    ]


class GsTimings(C.Structure):
    _fields_ = [
        ("init_sort_list_ms", C.c_float),
        ("radix_sort_ms", C.c_float),
        ("find_ranges_ms", C.c_float),
        ("render_ms", C.c_float),
        ("total_ms", C.c_float),
        ("num_sort_elements", C.c_uint32),
        ("overflowed", C.c_uint32),
        ("emitted_elements", C.c_uint64),
        ("scatter_ms_avg", C.c_float),
        ("scatter_launches", C.c_uint32),
        ("scatter_tile_ms_avg", C.c_float),
        ("scatter_tile_launches", C.c_uint32),
        ("scatter_bytes_per_elem", C.c_float),
        ("scatter_tile_bytes_per_elem", C.c_float),
    ]


class GsSceneInfo(C.Structure):
    _fields_ = [
        ("num_gaussians", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("tiles_x", C.c_uint32),
        ("tiles_y", C.c_uint32),
        ("capacity", C.c_uint32),
        ("num_sort_bits", C.c_uint32),
        ("row_begin", C.c_uint32),
        ("row_end", C.c_uint32),
        ("tile_word_bytes", C.c_uint32),
        ("row_stride", C.c_uint32),
        ("first_row", C.c_uint32),
        ("rows_owned", C.c_uint32),
    ]


class GsAdamParams(C.Structure):
    """gs_adam_params: one Adam step of gs_adam_rows_device (filled by gs_default_adam_params)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("step", C.c_uint32),
        ("beta1", C.c_float),
        ("beta2", C.c_float),
        ("eps", C.c_float),
        ("lr", C.c_float * GS_ADAM_GROUPS),
        ("lo", C.c_float * GS_ADAM_GROUPS),
        ("hi", C.c_float * GS_ADAM_GROUPS),
    ]


class GsDensifyParams(C.Structure):
    """gs_densify_params: the thresholds of gs_densify_device (filled by gs_default_densify_params)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("grad_threshold", C.c_float),
        ("split_scale", C.c_float),
        ("prune_opacity", C.c_float),
        ("prune_scale", C.c_float),
        ("prune_radius", C.c_float),
        ("split_shrink", C.c_float),
        ("seed", C.c_uint64),
    ]


class GsInitParams(C.Structure):
    """gs_init_params: what gs_records_from_points_device gives every new record (filled by gs_default_init_params)."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("opacity", C.c_float),
        ("min_dist2", C.c_float),
        ("max_scale", C.c_float),
    ]


class GsHostTimings(C.Structure):
    """gs_host_timings: the RECORD_CPU_TIMES figures (Renderer.cpp:399-456)."""
    _fields_ = [
        ("wait_ms", C.c_float),
        ("record_ms", C.c_float),
        ("present_ms", C.c_float),
        ("cpu_frame_ms", C.c_float),
    ]


# every symbol include/gsplat.h declares (tests check the .so exports exactly these)
EXPORTS = [
    "gs_default_config", "gs_create", "gs_destroy", "gs_last_error", "gs_upload_gaussians",
    "gs_load_ply", "gs_convert_ply", "gs_ply_last_error", "gs_set_resolution", "gs_set_tile_rows",
    "gs_get_scene_info", "gs_render", "gs_render_device", "gs_render_device_async",
    "gs_synchronize", "gs_get_timings", "gs_debug_read", "gs_debug_init_sort_list",
    "gs_set_stream", "gs_camera_matrices", "gs_sort_host", "gs_sort_bench", "gs_membench", "gs_write_image", "gs_share_scene",
    "gs_get_host_timings", "gs_set_tile_rows_interleaved", "gs_api_version", "gs_runtime_versions",
    "gs_dist_unique_id", "gs_dist_init", "gs_gather_strips", "gs_dist_destroy", "gs_dist_shard_rows", "gs_render_sharded",
    "gs_render_sharded_async", "gs_sharded_frame", "gs_sharded_read", "gs_dist_rebalance", "gs_dist_bands", "gs_balance_rows",
    "gs_set_outputs", "gs_read_output", "gs_output_device",
    "gs_backward", "gs_backward_device", "gs_upload_gaussians_device",
    "gs_visible_count", "gs_backward_visible", "gs_backward_visible_device",
    "gs_photometric_loss", "gs_photometric_loss_device",
    "gs_default_adam_params", "gs_adam_rows_device", "gs_upload_rows_device",
    "gs_densify_stats_device", "gs_default_densify_params", "gs_densify_device",
    "gs_default_adam_params_raw", "gs_adam_rows_raw_device", "gs_records_from_raw_device", "gs_raw_from_records_device",
    "gs_reset_opacity_raw_device", "gs_write_ply",
    "gs_backward_camera", "gs_backward_camera_device",
    "gs_default_init_params", "gs_knn_mean_dist2_device", "gs_records_from_points_device",
    "gs_rows_accumulate_device", "gs_rows_collect_device",
    "gs_sh_mode_of_degree",
    "gs_contrib_device", "gs_prune_below_device",
    "gs_relocate_device", "gs_grow_device", "gs_position_noise_device",
    "gs_set_band_gradients",
    "gs_set_antialias",
    "gs_set_abs_gradients", "gs_abs_screen_gradient_device", "gs_densify_stats_abs_device",
]
# GS_SH_*: the sh_mode of a frame (0, 1, 2 = the reference's Camera.h modes; 5 and 4 = SH degree 1 and 2; 3 names none)
GS_SH_ALL_BANDS, GS_SH_SKIP_FIRST_BAND, GS_SH_ONLY_FIRST_BAND, GS_SH_DEGREE_2, GS_SH_DEGREE_1 = 0, 1, 2, 4, 5
CAMERA_GRAD_FLOATS = 35    # GS_CAMERA_GRAD_FLOATS: [0..15] dL/dview, [16..31] dL/dproj, [32..34] dL/dcam_pos
ROWS_CONTIGUOUS, ROWS_INTERLEAVED, ROWS_BALANCED = 0, 1, 2   # GS_ROWS_*
API_VERSION = 7            # GS_API_VERSION of include/gsplat.h this binding was written against
DIST_UNIQUE_ID_BYTES = 128


class GsplatLibraryMissing(RuntimeError):
    pass


def build(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 build of the library, in-tree (make -C csrc)."""
    args = ["make", "-C", CSRC, "-j8"]
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(args, check=True, stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def _preload_torch_bundled(soname: str, why: str) -> None:
    """Maps <torch>/lib/<soname> with RTLD_GLOBAL when torch is installed but not imported yet -- no `import torch`, just the
    one shared object -- so that a library requested later under the same SONAME resolves to the copy torch will use."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("GS_HIP_RUNTIME") == "system":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    bundled = os.path.join(list(spec.submodule_search_locations)[0], "lib", soname)
    if os.path.exists(bundled):
        try:
            C.CDLL(bundled, mode=C.RTLD_GLOBAL)
        except OSError as ex:   # a broken wheel must not take the library down with it
            import warnings
            warnings.warn(f"could not pre-load {bundled} ({ex}); {why}")


def _one_hip_runtime() -> None:
    """A process must hold ONE HIP runtime.  PyTorch-ROCm wheels bundle their own libamdhip64.so (+ HSA runtime) with
    the same SONAME as the /opt/rocm copy this library links, and the dynamic loader hands every later request for that
    SONAME the copy that came first: torch first -> this library runs on torch's runtime (the configuration every GPU
    test runs in); this library first -> torch later finds the system libamdhip64 beside its own HSA runtime and
    reports "No HIP GPUs are available".  So, when torch is installed but not imported yet, its libamdhip64 is mapped
    before ours, and a later `import torch` (dist.ShardedFrame on a cuda device, bench.py) works in either order.
    GS_HIP_RUNTIME=system keeps the /opt/rocm runtime for processes that will never import torch."""
    _preload_torch_bundled("libamdhip64.so", "importing torch after this point may fail to see the GPU")


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GsplatLibraryMissing(
            f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)")
    _one_hip_runtime()
    L = C.CDLL(LIB_PATH)
    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    # the structs above are this file's copy of the header: refuse a library of another API version instead of handing
    # it structs it reads differently
    if not hasattr(L, "gs_api_version"):
        raise GsplatLibraryMissing(f"{LIB_PATH} predates gs_api_version(): rebuild it (make -C {CSRC})")
    L.gs_api_version.argtypes = []
    L.gs_api_version.restype = u32
    if L.gs_api_version() != API_VERSION:
        raise GsplatLibraryMissing(f"{LIB_PATH} has API version {L.gs_api_version()}, this binding expects {API_VERSION}: rebuild it")
    ctxp = C.c_void_p
    L.gs_default_config.argtypes = [C.POINTER(GsConfig)]
    L.gs_default_config.restype = None
    L.gs_create.argtypes = [C.POINTER(GsConfig), C.POINTER(ctxp)]
    L.gs_destroy.argtypes = [ctxp]
    L.gs_last_error.argtypes = [ctxp]
    L.gs_last_error.restype = C.c_char_p
    L.gs_upload_gaussians.argtypes = [ctxp, vp, u32]
    L.gs_load_ply.argtypes = [ctxp, C.c_char_p]
    L.gs_convert_ply.argtypes = [C.c_char_p, vp, u32, C.POINTER(u32)]
    L.gs_ply_last_error.argtypes = []
    L.gs_ply_last_error.restype = C.c_char_p
    L.gs_set_resolution.argtypes = [ctxp, u32, u32]
    L.gs_set_tile_rows.argtypes = [ctxp, u32, u32]
    L.gs_get_scene_info.argtypes = [ctxp, C.POINTER(GsSceneInfo)]
    L.gs_render.argtypes = [ctxp, vp, vp, vp, u32, vp]
    L.gs_render_device.argtypes = [ctxp, vp, vp, vp, u32, vp]
    L.gs_render_device_async.argtypes = [ctxp, vp, vp, vp, u32, vp]
    L.gs_synchronize.argtypes = [ctxp]
    L.gs_get_timings.argtypes = [ctxp, C.POINTER(GsTimings)]
    L.gs_debug_read.argtypes = [ctxp, C.c_int, vp, C.c_size_t]
    L.gs_debug_init_sort_list.argtypes = [ctxp, vp, vp, vp, u32]
    L.gs_set_stream.argtypes = [ctxp, vp]
    L.gs_camera_matrices.argtypes = [vp, f32, f32, f32, f32, f32, vp, vp]
    L.gs_sort_host.argtypes = [ctxp, vp, vp, vp, u32, u32]
    L.gs_sort_bench.argtypes = [ctxp, u32, u32, u32, C.c_uint64, C.POINTER(f32), C.POINTER(u32)]
    L.gs_membench.argtypes = [ctxp, C.c_int, C.c_size_t, u32, u32, C.POINTER(f32), C.POINTER(f32)]
    L.gs_write_image.argtypes = [C.c_char_p, vp, u32, u32]
    L.gs_share_scene.argtypes = [ctxp, ctxp]
    L.gs_get_host_timings.argtypes = [ctxp, C.POINTER(GsHostTimings)]
    L.gs_set_tile_rows_interleaved.argtypes = [ctxp, u32, u32, u32]
    L.gs_runtime_versions.argtypes = [C.POINTER(C.c_int)] * 3
    L.gs_dist_unique_id.argtypes = [vp]
    L.gs_dist_init.argtypes = [ctxp, vp, C.c_int, C.c_int]
    L.gs_gather_strips.argtypes = [ctxp, vp, vp, C.c_size_t, C.c_int]
    L.gs_dist_destroy.argtypes = [ctxp]
    L.gs_dist_shard_rows.argtypes = [ctxp, u32]
    L.gs_render_sharded.argtypes = [ctxp, vp, vp, vp, u32, vp]
    L.gs_render_sharded_async.argtypes = [ctxp, vp, vp, vp, u32]
    L.gs_sharded_frame.argtypes = [ctxp, u32, C.POINTER(vp)]
    L.gs_sharded_read.argtypes = [ctxp, u32, vp]
    L.gs_dist_rebalance.argtypes = [ctxp, C.POINTER(u32)]
    L.gs_dist_bands.argtypes = [ctxp, C.POINTER(u32), u32]
    L.gs_balance_rows.argtypes = [C.POINTER(C.c_double), u32, u32, C.POINTER(u32)]
    L.gs_set_outputs.argtypes = [ctxp, u32]
    L.gs_read_output.argtypes = [ctxp, u32, vp, C.c_size_t]
    L.gs_output_device.argtypes = [ctxp, u32, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.gs_backward.argtypes = [ctxp, vp, vp, vp]
    L.gs_backward_device.argtypes = [ctxp, vp, vp, vp]
    L.gs_upload_gaussians_device.argtypes = [ctxp, vp, u32]
    L.gs_visible_count.argtypes = [ctxp, vp]
    L.gs_backward_visible.argtypes = [ctxp, vp, vp, vp, vp, u32, vp]
    L.gs_backward_visible_device.argtypes = [ctxp, vp, vp, vp, vp, u32, vp]
    L.gs_photometric_loss.argtypes = [ctxp, vp, vp, f32, vp, vp, vp]
    L.gs_photometric_loss_device.argtypes = [ctxp, vp, vp, f32, vp, vp, vp]
    L.gs_default_adam_params.argtypes = [C.POINTER(GsAdamParams)]
    L.gs_default_adam_params.restype = None
    L.gs_adam_rows_device.argtypes = [ctxp, vp, vp, vp, u32, vp, vp, vp, u32, C.POINTER(GsAdamParams)]
    L.gs_upload_rows_device.argtypes = [ctxp, vp, u32, vp, vp, u32]
    L.gs_densify_stats_device.argtypes = [ctxp, vp, vp, u32, u32, vp, vp, vp]
    L.gs_default_densify_params.argtypes = [C.POINTER(GsDensifyParams)]
    L.gs_default_densify_params.restype = None
    L.gs_densify_device.argtypes = [ctxp, vp, vp, vp, u32, vp, vp, vp, C.POINTER(GsDensifyParams), vp, vp, vp, u32, vp]
    L.gs_default_adam_params_raw.argtypes = [C.POINTER(GsAdamParams)]
    L.gs_default_adam_params_raw.restype = None
    L.gs_adam_rows_raw_device.argtypes = [ctxp, vp, vp, vp, vp, u32, vp, vp, vp, u32, C.POINTER(GsAdamParams)]
    L.gs_records_from_raw_device.argtypes = [ctxp, vp, vp, u32]
    L.gs_raw_from_records_device.argtypes = [ctxp, vp, vp, u32]
    L.gs_reset_opacity_raw_device.argtypes = [ctxp, vp, vp, vp, vp, u32, f32]
    L.gs_write_ply.argtypes = [C.c_char_p, vp, u32, u32]
    L.gs_backward_camera.argtypes = [ctxp, vp]
    L.gs_backward_camera_device.argtypes = [ctxp, vp]
    L.gs_default_init_params.argtypes = [C.POINTER(GsInitParams)]
    L.gs_default_init_params.restype = None
    L.gs_knn_mean_dist2_device.argtypes = [ctxp, vp, u32, vp]
    L.gs_records_from_points_device.argtypes = [ctxp, vp, vp, u32, C.POINTER(GsInitParams), vp, vp]
    L.gs_rows_accumulate_device.argtypes = [ctxp, vp, vp, u32, vp, vp, vp, u32, f32]
    L.gs_rows_collect_device.argtypes = [ctxp, vp, vp, u32, vp, vp, u32, vp]
    L.gs_sh_mode_of_degree.argtypes = [u32, C.POINTER(u32)]
    L.gs_contrib_device.argtypes = [ctxp, u32, vp, vp, vp]
    L.gs_prune_below_device.argtypes = [ctxp, vp, f32, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp]
    L.gs_relocate_device.argtypes = [ctxp, vp, vp, vp, vp, u32, f32, C.c_uint64, vp, u32, vp]
    L.gs_grow_device.argtypes = [ctxp, vp, vp, vp, vp, u32, f32, C.c_uint64, u32, vp, vp, vp, vp, u32, vp]
    L.gs_position_noise_device.argtypes = [ctxp, vp, vp, u32, vp, vp, u32, f32, f32, f32, C.c_uint64]
    L.gs_set_band_gradients.argtypes = [ctxp, u32]
    L.gs_set_antialias.argtypes = [ctxp, u32]
    L.gs_set_abs_gradients.argtypes = [ctxp, u32]
    L.gs_abs_screen_gradient_device.argtypes = [ctxp, vp, vp, u32, vp]
    L.gs_densify_stats_abs_device.argtypes = [ctxp, vp, vp, u32, u32, vp]
    _lib = L
    _check_hip_runtime(L)
    return L


def sh_mode_of_degree(degree: int) -> int:
    """gs_sh_mode_of_degree: the frame mode (GS_SH_*) of an active SH degree 0..3 -> 2, 5, 4, 0.  No context, no GPU."""
    mode = C.c_uint32()
    if not 0 <= int(degree) <= 0xFFFFFFFF or lib().gs_sh_mode_of_degree(int(degree), C.byref(mode)) != GS_OK:
        raise ValueError(f"sh_mode_of_degree: degree must be 0..3, got {degree!r}")
    return int(mode.value)


def _default_params(who: str, struct, fill, overrides: dict):
    """A parameter struct as `fill` (its gs_default_*_params) writes it, with keyword overrides by field name: an integer field takes
    int(value), a float field float(value), an array of floats a sequence of its length or {index: value} for some of its
    elements.  struct_size, or a name the struct does not have: TypeError."""
    p = struct()
    fill(C.byref(p))
    kinds = {name: kind for name, kind in struct._fields_ if name != "struct_size"}
    for name, value in overrides.items():
        kind = kinds.get(name)
        if kind is None:
            raise TypeError(f"{who}: unknown parameter {name!r}")
        if issubclass(kind, C.Array):
            if not isinstance(value, dict) and len(value) != kind._length_:
                raise ValueError(f"{name} needs {kind._length_} values or a dict of groups")
            arr = getattr(p, name)
            for g, x in (value.items() if isinstance(value, dict) else enumerate(value)):
                arr[int(g)] = float(x)
        else:
            setattr(p, name, float(value) if kind is C.c_float else int(value))
    return p


def default_adam_params(space: str = "records", **overrides) -> GsAdamParams:
    """gs_default_adam_params: step 1, beta1 0.9, beta2 0.999, eps 1e-15, the INRIA learning rates per GS_ADAM_* group
    (acting on record-space values here) and the clamps scale >= 1e-7, opacity in [0, 1].  space="raw":
    gs_default_adam_params_raw, the same without any clamp (for adamRowsRawDevice, where the rates act on log-scales and
    logit-opacities).  overrides: beta1, beta2, eps, step as numbers; lr, lo, hi as a sequence of six or as {GS_ADAM_*
    group: value} for some of them."""
    if space not in ("records", "raw"):
        raise ValueError(f"space must be 'records' or 'raw', not {space!r}")
    fill = lib().gs_default_adam_params_raw if space == "raw" else lib().gs_default_adam_params
    return _default_params("default_adam_params", GsAdamParams, fill, overrides)


def default_densify_params(**overrides) -> GsDensifyParams:
    """gs_default_densify_params: grad_threshold 2e-4, split_scale 0.01, prune_opacity 0.005, prune_scale and prune_radius
    +inf (none), split_shrink 1.6, seed 0.  overrides: any of those fields by name."""
    return _default_params("default_densify_params", GsDensifyParams, lib().gs_default_densify_params, overrides)


def default_init_params(**overrides) -> GsInitParams:
    """gs_default_init_params: opacity 0.1, min_dist2 1e-7, max_scale +inf (none).  overrides: any of those fields by name."""
    return _default_params("default_init_params", GsInitParams, lib().gs_default_init_params, overrides)


def hip_runtime_path() -> str | None:
    """The libamdhip64 this process really bound (from /proc/self/maps)."""
    try:
        for line in open("/proc/self/maps"):
            if "libamdhip64" in line:
                return line.split()[-1]
    except OSError:
        pass
    return None


def runtime_info() -> dict:
    """HIP version the library was built against, the runtime / driver versions the process bound, and that runtime's path."""
    b, r, d = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = lib().gs_runtime_versions(C.byref(b), C.byref(r), C.byref(d))
    return {"rc": rc, "hip_build": b.value, "hip_runtime": r.value, "hip_driver": d.value, "runtime_path": hip_runtime_path()}


def _check_hip_runtime(L) -> None:
    """libgsplat_hip.so is compiled against /opt/rocm's headers and may run on the libamdhip64 a PyTorch wheel bundles
    (_one_hip_runtime): a different MAJOR version is reported -- loudly, once -- because nothing else would."""
    b, r = C.c_int(0), C.c_int(0)
    if L.gs_runtime_versions(C.byref(b), C.byref(r), None) != GS_OK or not b.value or not r.value:
        return                                     # no usable runtime here (CPU-only container): nothing to compare
    if b.value // 10_000_000 != r.value // 10_000_000:
        import warnings
        warnings.warn(f"libgsplat_hip.so was built against HIP {b.value} but the process bound HIP runtime {r.value} "
                      f"({hip_runtime_path()}); set GS_HIP_RUNTIME=system to keep /opt/rocm's runtime in processes that never import torch")


def preload_rccl() -> None:
    """gs_dist_init binds RCCL by SONAME (librccl.so.1).  In a process that will import torch later, map the copy the
    PyTorch wheel bundles first, so that both sides end up on ONE RCCL over ONE HIP runtime."""
    _preload_torch_bundled("librccl.so", "gs_dist_init will bind the system RCCL")
