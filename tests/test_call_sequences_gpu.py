"""What the host layer answers, call by call: one table of short sequences of raw C-ABI calls on a scene of 64 gaussians at
32 x 32 (2 x 2 tiles, max_rows 64), and after every call (return code, gs_last_error text) against the committed list
tests/golden/call_sequences.json.  The table holds every refusal of the training calls (Adam, the raw space, gs_backward*,
gs_visible_count, gs_photometric_loss*, density control): each null pointer, n == 0, each bad parameter field, each aliasing
pair, each wrong state -- and the sequences that decide what a frame leaves behind (uploads, tile rows, gs_debug_init_sort_list,
gs_set_outputs, gs_set_resolution).  No row provokes a HIP error.

The committed list was recorded from the library of the commit before the host layer was split into gs_api.cpp, gs_train.cpp
and gs_debug.cpp: GS_LIB_OVERRIDE=<that libgsplat_hip.so> GS_CALL_SEQUENCES_RECORD=1 pytest tests/test_call_sequences_gpu.py
writes it (record_golden below) instead of comparing."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from vk3dgaussiansplatting_amd import _lib, synth
from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "call_sequences.json")
N, W, H, MAX_OUT = 64, 32, 32, 128
NAN, INF = math.nan, math.inf
RGBA, DEPTH = _lib.GS_OUTPUT_RGBA32F, _lib.GS_OUTPUT_DEPTH

# ---- the pieces rows are made of.  A step is (function, arguments...); "@name" is a buffer or value of `buffers`,
# ("adam" | "adam_raw" | "densify", {field: value | (index, value)}) a parameter struct with those fields changed.
UPLOAD = ("gs_upload_gaussians", "@h_aos", N)
RES = ("gs_set_resolution", W, H)
FRAME = ("gs_render_device", "@view", "@proj", "@pos", 0, None)
SCENE = [UPLOAD, RES]
DRAWN = SCENE + [FRAME]
LIST = ("gs_debug_init_sort_list", "@view", "@proj", "@pos", 0)
BWD = ("gs_backward_device", "@grad", None, "@rows_n")
VIS = ("gs_backward_visible_device", "@grad", None, "@ids", "@rows", N, "@count")
STATS = ("gs_densify_stats_device", "@ids", "@count", N, N, "@gacc", "@seen", "@maxr")
READ_SORTED = ("gs_debug_read", _lib.BUF_SORTED_ID, "@h_word", 4)
READ_UNSORTED = ("gs_debug_read", _lib.BUF_UNSORTED_ID, "@h_word", 4)
READ_OUT = ("gs_read_output", RGBA, "@h_rgba", W * H * 16)
OUT_DEV = ("gs_output_device", RGBA, "@out_dev", "@out_size")
LOSS_OWN = ("gs_photometric_loss_device", None, "@target", 0.2, None, "@loss", "@grad")
ADAM_ARGS = ["@rec", "@m", "@v", N, "@ids", "@rows", "@count", N, ("adam", {})]
RAW_ARGS = ["@raw", "@rec2", "@m", "@v", N, "@ids", "@rows", "@count", N, ("adam_raw", {})]
RESET_ARGS = ["@raw", "@rec2", "@m", "@v", N, 0.01]
LOSS_ARGS = ["@rgba", "@target", 0.2, "@bg", "@loss", "@grad"]
LOSS_HOST_ARGS = ["@h_rgba", "@h_target", 0.2, "@bg", "@h_loss", "@h_grad"]
VIS_ARGS = list(VIS[1:])
VIS_HOST_ARGS = ["@h_grad", None, "@h_ids", "@h_rows", N, "@h_count"]
STATS_ARGS = list(STATS[1:])
DENSIFY_ARGS = ["@rec", "@m", "@v", N, "@gacc", "@seen", "@maxr", ("densify", {}), "@rec_out", "@m_out", "@v_out", MAX_OUT, "@counts"]
BAD_ADAM = [{"struct_size": 4}, {"step": 0}, {"beta1": 1.0}, {"beta1": -0.5}, {"beta1": NAN}, {"beta2": 1.0}, {"beta2": NAN},
            {"eps": -1.0}, {"eps": INF}, {"eps": NAN}, {"lr": (2, -1.0)}, {"lr": (5, INF)}, {"lr": (0, NAN)},
            {"lo": (1, 1.0), "hi": (1, 0.0)}, {"lo": (3, NAN)}, {"hi": (4, NAN)}, {"beta1": 0.999999, "lr": (0, 3e38)}]
BAD_DENSIFY = [{"struct_size": 8}, {"grad_threshold": NAN}, {"split_shrink": 0.0}, {"split_shrink": -1.0}, {"split_shrink": NAN}]


def swapped(args, changes):
    """args with the positions of `changes` replaced."""
    out = list(args)
    for k, v in changes.items():
        out[k] = v
    return out


def variants(name, fn, args, before, changes_list):
    """One row per entry of changes_list: `before`, then fn with those arguments changed."""
    return [(f"{name}[{i}]", list(before) + [(fn, *swapped(args, ch))]) for i, ch in enumerate(changes_list)]


def nulls(positions):
    return [{k: None} for k in positions]


def table():
    rows = []
    # -- Adam in record space and in raw space
    rows += variants("adam_null", "gs_adam_rows_device", ADAM_ARGS, [], nulls([0, 1, 2, 4, 5, 6, 8]) + [{3: 0}])
    rows += variants("adam_no_rows", "gs_adam_rows_device", ADAM_ARGS, [],
                     [{0: None, 1: None, 2: None, 4: None, 5: None, 6: None, 7: 0}, {7: 0, 3: 0}, {}])
    rows += variants("adam_bad", "gs_adam_rows_device", ADAM_ARGS, [], [{8: ("adam", bad)} for bad in BAD_ADAM])
    rows += variants("raw_null", "gs_adam_rows_raw_device", RAW_ARGS, [], nulls([0, 1, 2, 3, 5, 6, 7, 9]) + [{4: 0}])
    rows += variants("raw_bad", "gs_adam_rows_raw_device", RAW_ARGS, [], [{9: ("adam_raw", bad)} for bad in BAD_ADAM])
    rows += variants("raw_alias", "gs_adam_rows_raw_device", RAW_ARGS, [],
                     [{0: "@rec2"}, {2: "@rec2"}, {3: "@rec2"}, {0: "@rec2_tail"}, {0: "@rec2", 8: 0}, {8: 0}, {}])
    for fn in ("gs_records_from_raw_device", "gs_raw_from_records_device"):
        rows += variants(fn, fn, ["@raw", "@rec2", N], [], nulls([0, 1]) + [{2: 0}, {0: "@rec2"}, {0: "@rec2_tail"}, {}])
    rows += variants("reset", "gs_reset_opacity_raw_device", RESET_ARGS, [],
                     nulls([0, 1, 2, 3]) + [{4: 0}, {5: 0.0}, {5: 1.0}, {5: -1.0}, {5: NAN}, {2: None, 3: None}, {}])
    # -- gs_backward*, gs_visible_count
    for fn, args in (("gs_backward_device", ["@grad", "@depth", "@rows_n"]), ("gs_backward", ["@h_grad", "@h_depth", "@h_rows_n"])):
        rows += variants(fn, fn, args, DRAWN, nulls([0, 2]) + [{1: None}, {}])
        rows += [(f"{fn}[no scene]", [(fn, *args)]), (f"{fn}[no resolution]", [UPLOAD, (fn, *args)]),
                 (f"{fn}[no frame]", SCENE + [(fn, *args)]), (f"{fn}[fast]", ["fast"] + DRAWN + [(fn, *args)]),
                 (f"{fn}[band]", SCENE + [("gs_set_tile_rows", 0, 1), FRAME, (fn, *args)])]
    rows += [("visible_count", DRAWN + [("gs_visible_count", None), ("gs_visible_count", "@h_count")]),
             ("visible_count[no frame]", SCENE + [("gs_visible_count", "@h_count")])]
    for fn, args in (("gs_backward_visible_device", VIS_ARGS), ("gs_backward_visible", VIS_HOST_ARGS)):
        rows += variants(fn, fn, args, DRAWN, nulls([0, 5, 2, 3]) + [{2: None, 3: None, 4: 0}, {4: 1}, {}])
        rows += [(f"{fn}[no frame]", SCENE + [(fn, *args)]), (f"{fn}[fast]", ["fast"] + DRAWN + [(fn, *args)])]
    # -- gs_photometric_loss*
    for fn, args in (("gs_photometric_loss_device", LOSS_ARGS), ("gs_photometric_loss", LOSS_HOST_ARGS)):
        rows += variants(fn, fn, args, DRAWN, nulls([1, 4]) + [{2: -0.1}, {2: 1.1}, {2: NAN}, {3: "@bg_nan"}, {3: "@bg_inf"},
                                                                {3: None}, {5: None}, {5: args[0]}, {0: None}, {}])
        rows += [(f"{fn}[no resolution]", [UPLOAD, (fn, *args)]),
                 (f"{fn}[band]", SCENE + [("gs_set_tile_rows", 1, 2), (fn, *args)]),
                 (f"{fn}[own, no frame]", SCENE + [("gs_set_outputs", RGBA), (fn, *swapped(args, {0: None}))]),
                 (f"{fn}[own, depth only]", SCENE + [("gs_set_outputs", DEPTH), FRAME, (fn, *swapped(args, {0: None}))]),
                 (f"{fn}[own]", SCENE + [("gs_set_outputs", RGBA), FRAME, (fn, *swapped(args, {0: None}))])]
    rows += [("loss_device[own, grad is the image]",
              SCENE + [("gs_set_outputs", RGBA), FRAME, OUT_DEV, ("gs_photometric_loss_device", None, "@target", 0.2, None, "@loss", "@out_dev_value")])]
    # -- density control
    rows += variants("stats_null", "gs_densify_stats_device", STATS_ARGS, DRAWN + [VIS], nulls([0, 1, 4, 5, 6]) + [{3: N + 1}, {2: 0}, {}])
    rows += [("stats[no frame]", SCENE + [STATS]), ("stats[no backward]", DRAWN + [STATS]),
             ("stats[count only is no backward]", DRAWN + [("gs_backward_visible_device", "@grad", None, None, None, 0, "@count"), STATS]),
             ("stats[dense backward]", DRAWN + [BWD, STATS])]
    rows += variants("densify_null", "gs_densify_device", DENSIFY_ARGS, [],
                     nulls([0, 4, 5, 6, 12, 8, 7]) + [{3: 0}, {3: 0x80000000}, {8: None, 9: None, 10: None, 11: 0}, {}])
    rows += variants("densify_bad", "gs_densify_device", DENSIFY_ARGS, [], [{7: ("densify", bad)} for bad in BAD_DENSIFY])
    rows += variants("densify_moments", "gs_densify_device", DENSIFY_ARGS, [],
                     [{1: None}, {2: None}, {9: None}, {10: None}, {1: None, 2: None}, {9: None, 10: None},
                      {1: None, 2: None, 9: None, 10: None}, {9: None, 10: None, 11: 0, 8: None}])
    ins, outs = ["@rec", "@m", "@v", "@gacc", "@seen", "@maxr"], [8, 9, 10, 12]
    rows += variants("densify_alias_in", "gs_densify_device", DENSIFY_ARGS, [], [{o: i} for o in outs for i in ins])
    rows += variants("densify_alias_out", "gs_densify_device", DENSIFY_ARGS, [],
                     [{b: DENSIFY_ARGS[a]} for k, a in enumerate(outs) for b in outs[k + 1:]] + [{12: "@rec_out_tail"}])
    # -- what a frame leaves behind
    rows += [
        ("frame, backward", DRAWN + [BWD]),
        ("frame, in-place upload, backward", DRAWN + [("gs_upload_gaussians_device", "@rec", N), BWD, FRAME, BWD]),
        ("frame, rows upload, backward", DRAWN + [("gs_upload_rows_device", "@rec", N, "@ids", "@count", N), BWD, VIS, FRAME, VIS]),
        ("frame, tile rows, backward", DRAWN + [("gs_set_tile_rows", 0, 2), BWD, ("gs_visible_count", "@h_count"), FRAME, BWD]),
        ("frame, interleaved rows, backward", DRAWN + [("gs_set_tile_rows_interleaved", 0, 1, 0), BWD, FRAME, BWD]),
        ("frame, list, frame", DRAWN + [LIST, BWD, VIS, READ_UNSORTED, FRAME, READ_SORTED, READ_UNSORTED, BWD]),
        ("list alone", SCENE + [READ_SORTED, LIST, READ_UNSORTED, BWD, STATS]),
        ("frame, visible backward, stats", DRAWN + [VIS, STATS]),
        ("frame, visible backward, frame, stats", DRAWN + [VIS, FRAME, STATS, VIS, STATS]),
        ("frame, outputs, read", DRAWN + [("gs_set_outputs", RGBA), READ_OUT, OUT_DEV, LOSS_OWN]),
        ("frame, outputs, frame, read", DRAWN + [("gs_set_outputs", RGBA), FRAME, READ_OUT, OUT_DEV, LOSS_OWN, BWD]),
        ("frame, resolution", SCENE + [("gs_set_outputs", RGBA), FRAME, VIS, RES, BWD, ("gs_visible_count", "@h_count"), VIS, STATS,
                                       READ_SORTED, READ_UNSORTED, READ_OUT, OUT_DEV, LOSS_OWN]),
        ("frame, new scene", DRAWN + [("gs_upload_gaussians_device", "@rec_out", MAX_OUT), BWD, READ_SORTED, RES, BWD]),
    ]
    return rows


@pytest.fixture(scope="module")
def buffers():
    import torch
    dev = torch.device("cuda:0")
    aos = np.ascontiguousarray(synth.generate(N, W, H, -3.0, seed=11), dtype=np.float32)
    view, proj = np.zeros(16, np.float32), np.zeros(16, np.float32)
    pos = np.zeros(3, np.float32)
    assert _lib.lib().gs_camera_matrices(pos.ctypes.data, 0.0, 0.0, W / H, 0.1, 100.0, view.ctypes.data, proj.ctypes.data) == 0
    f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
    # rec2: what the raw-space calls rewrite (rec stays the scene)
    t = {"rec": torch.tensor(aos, device=dev), "rec2": torch.tensor(aos, device=dev), "m": f32(N, 84), "v": f32(N, 84), "raw": f32(N, 84), "rows": f32(N, 84),
         "rows_n": f32(N, 84), "ids": i32(N), "count": i32(1), "grad": f32(H, W, 4), "depth": f32(H, W), "rgba": f32(H, W, 4),
         "target": f32(H, W, 3), "loss": f32(4), "gacc": f32(N), "seen": i32(N), "maxr": f32(N),
         "rec_out": torch.tensor(np.concatenate([aos, aos]), device=dev), "m_out": f32(MAX_OUT, 84), "v_out": f32(MAX_OUT, 84),
         "counts": i32(4)}
    h = {"h_aos": aos, "view": view, "proj": proj, "pos": pos, "h_word": np.zeros(1, np.uint32),
         "h_rgba": np.zeros((H, W, 4), np.float32), "h_grad": np.zeros((H, W, 4), np.float32), "h_depth": np.zeros((H, W), np.float32),
         "h_target": np.zeros((H, W, 3), np.float32), "h_loss": np.zeros(3, np.float32), "h_rows_n": np.zeros((N, 84), np.float32),
         "h_ids": np.zeros(N, np.uint32), "h_rows": np.zeros((N, 84), np.float32), "h_count": np.zeros(1, np.uint32),
         "bg": np.array([0.1, 0.2, 0.3], np.float32), "bg_nan": np.array([0.0, NAN, 0.0], np.float32),
         "bg_inf": np.array([0.0, 0.0, INF], np.float32)}
    b = {k: x.data_ptr() for k, x in t.items()}
    b.update({k: x.ctypes.data for k, x in h.items()})
    b["rec2_tail"] = b["rec2"] + (N - 1) * 336          # shares its first record with the last of rec2
    b["rec_out_tail"] = b["rec_out"] + MAX_OUT * 336 - 8
    b["_keep"] = (t, h)
    b["_count"] = t["count"]
    torch.cuda.synchronize()
    return b


def make_params(kind, changes):
    L = _lib.lib()
    p = _lib.GsDensifyParams() if kind == "densify" else _lib.GsAdamParams()
    {"adam": L.gs_default_adam_params, "adam_raw": L.gs_default_adam_params_raw, "densify": L.gs_default_densify_params}[kind](C.byref(p))
    for field, value in changes.items():
        if isinstance(value, tuple):
            getattr(p, field)[value[0]] = value[1]
        else:
            setattr(p, field, value)
    return p


def run_row(steps, b):
    """The (return code, gs_last_error text) of every call of one row, on a context of its own."""
    import torch
    L = _lib.lib()
    L.gs_last_error.restype = C.c_char_p
    cfg = _lib.GsConfig()
    L.gs_default_config(C.byref(cfg))
    if steps[0] == "fast":
        cfg.render_mode, steps = _lib.GS_RENDER_FAST, steps[1:]
    ctx = C.c_void_p()
    assert L.gs_create(C.byref(cfg), C.byref(ctx)) == 0
    b["_count"].zero_()
    torch.cuda.synchronize()
    out_dev, out_size, keep, answers = C.c_void_p(), C.c_size_t(), [], []
    try:
        for fn, *args in steps:
            call = []
            for a in args:
                if isinstance(a, tuple):
                    keep.append(make_params(*a))
                    a = C.byref(keep[-1])
                elif a == "@out_dev":
                    a = C.byref(out_dev)
                elif a == "@out_size":
                    a = C.byref(out_size)
                elif a == "@out_dev_value":
                    a = out_dev.value
                elif isinstance(a, str):
                    a = b[a[1:]]
                call.append(a)
            rc = getattr(L, fn)(ctx, *call)
            answers.append([int(rc), L.gs_last_error(ctx).decode()])
            assert rc != _lib.GS_ERR_HIP, (fn, answers[-1])      # no row may provoke a HIP error
        assert L.gs_synchronize(ctx) == 0
    finally:
        L.gs_destroy(ctx)
    return answers


def record_golden(answers):
    """GS_CALL_SEQUENCES_RECORD=1 (with GS_LIB_OVERRIDE naming the library to record): writes the committed list."""
    with open(GOLDEN, "w") as f:
        json.dump(answers, f, indent=0, sort_keys=True)
        f.write("\n")


def test_every_call_answers_as_recorded(buffers):
    rows = table()
    assert len({name for name, _ in rows}) == len(rows)
    answers = {name: run_row(steps, buffers) for name, steps in rows}
    if os.environ.get("GS_CALL_SEQUENCES_RECORD"):
        record_golden(answers)
        return
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(answers)
    for name, steps in rows:
        calls = [step[0] for step in steps if step != "fast"]
        assert len(answers[name]) == len(golden[name]) == len(calls), name
        for call, got, want in zip(calls, answers[name], golden[name]):
            assert got == want, (name, call, got, want)
