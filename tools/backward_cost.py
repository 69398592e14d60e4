"""What a backward pass (gs_backward_device, include/gsplat.h) costs against the forward frame: the forward's total_ms
(gs_get_timings, hipEvents) and the backward's host-measured time (enqueue + gs_synchronize), medians of --iters runs after
3 warm-up runs; then the same backward again under `rocprofv3 --kernel-trace --stats` (a child process) for its split into
the blend backward (k_bwd_blend, with the three small kernels of the per-splat scan before it) and the row sum + chain
(k_bwd_rowsum_chain).  The visible form (gs_backward_visible_device with max_rows = |V|) is timed in the same window, dense
and visible iterations alternating in one process so that both see the same neighbours; it runs the <true> instantiations
of the same kernels, which the trace tells from the dense <false> ones by the template argument in the kernel name
(k_splat_offsets<gs::BwdSource<true>>; k_bwd_blend is one kernel for both).  A trace in which a part of the split matches
no kernel is an error, not a zero.  camera_ms is gs_backward_camera_device + gs_synchronize behind the visible backward
of the same iteration (it re-reads that backward's rows), in the same alternating loop; the trace splits it into
k_bwd_camera_blocks and k_bwd_camera_reduce.  One JSON line per config.

    python tools/backward_cost.py [C Chard ...] [--iters 20]"""
import argparse, csv, glob, json, os, re, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("configs", nargs="*", default=["C", "Chard"])
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--child", action="store_true", help="run the backward only (under rocprofv3)")
a = ap.parse_args()

import numpy as np
import torch
import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import synth


def setup(name):
    aos, cfg = synth.generate_config(name)
    w, h = cfg["width"], cfg["height"]
    rm = gs.ResourceManager(); rm.setGaussians(aos)
    sc = gs.Scene(rm, aspect_ratio=w / h)
    cam = sc.getCamera(); cam.setPosition((0, 0, 0)); cam.setRotation(0.0, 0.0); cam.recalculate()
    r = gs.Renderer(w, h, record_timings=1, warmup_frames=0)
    r.init(rm); r.initForScene(sc)
    rng = np.random.default_rng(0)
    gr = torch.tensor(rng.standard_normal((h, w, 4)).astype(np.float32), device="cuda")
    gd = torch.tensor(rng.standard_normal((h, w)).astype(np.float32), device="cuda")
    out = torch.empty(len(aos), 84, device="cuda")
    torch.cuda.synchronize()
    return r, sc, gr, gd, out, len(aos), w, h


def backward_ms(r, gr, gd, out):
    t0 = time.perf_counter()
    r.backwardDevice(gr.data_ptr(), gd.data_ptr(), out.data_ptr())
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3


def visible_buffers(r, sc):
    """|V| of the frame and device buffers of exactly that size: ids, rows, the count word."""
    r.drawDevice(sc, None, sync=True)
    v = r.visibleCount()
    ids = torch.empty(max(v, 1), dtype=torch.int32, device="cuda")
    rows = torch.empty(max(v, 1), 84, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return v, ids, rows, count


def visible_ms(r, gr, gd, vis):
    v, ids, rows, count = vis
    t0 = time.perf_counter()
    r.backwardVisibleDevice(gr.data_ptr(), gd.data_ptr(), ids.data_ptr(), rows.data_ptr(), v, count.data_ptr())
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3


def camera_ms(r, cam):
    t0 = time.perf_counter()
    r.backwardCameraDevice(cam.data_ptr())
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3


if a.child:
    for name in a.configs:
        r, sc, gr, gd, out, n, w, h = setup(name)
        vis = visible_buffers(r, sc)
        cam = torch.zeros(35, device="cuda")
        for _ in range(a.iters):
            backward_ms(r, gr, gd, out)
            visible_ms(r, gr, gd, vis)
            camera_ms(r, cam)
        r.cleanup()
    sys.exit(0)

for name in a.configs:
    r, sc, gr, gd, out, n, w, h = setup(name)
    vis = visible_buffers(r, sc)
    fwd, bwd, bvis, bcam = [], [], [], []
    cam = torch.zeros(35, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        r.drawDevice(sc, None, sync=True)
        backward_ms(r, gr, gd, out)
        visible_ms(r, gr, gd, vis)
        camera_ms(r, cam)
    for _ in range(a.iters):
        r.drawDevice(sc, None, sync=True)
        fwd.append(r.timings().total_ms)
        bwd.append(backward_ms(r, gr, gd, out))
        bvis.append(visible_ms(r, gr, gd, vis))
        bcam.append(camera_ms(r, cam))
    assert int(vis[3].item()) == vis[0]
    assert bool(torch.isfinite(cam).all()) and int((cam != 0).sum()) >= 20
    elems = r.timings().num_sort_elements
    r.cleanup()
    split = {}
    if shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="bwd_cost_")
        rc = subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
                             "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), name, "--child",
                             "--iters", str(a.iters)], capture_output=True, text=True).returncode
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if rc == 0 and files:
            us = {}
            for row in csv.DictReader(open(files[0])):
                us[row["Name"]] = float(row["AverageNs"]) / 1e3
            # "void gs::k_splat_offsets<gs::BwdSource<true> >(gs::BwdSource<true>, ...)" -> "k_splat_offsets<gs::BwdSource<true>>":
            # the template argument tells the dense instantiation from the visible one
            kname = lambda k: re.sub(r"^(void )?(gs::)?", "", k).split("(")[0].replace(" ", "")

            def ms(key):
                hits = [v for k, v in us.items() if kname(k) == key]
                if not hits:
                    raise SystemExit(f"backward_cost: no kernel named {key} in the trace; it has {sorted(map(kname, us))}")
                return sum(hits) / 1e3
            scan = lambda vis: sum(ms(f"{k}<gs::BwdSource<{vis}>>") for k in ("k_splat_block_sums", "k_splat_scan_blocks", "k_splat_offsets"))
            split = {"blend_backward_ms": round(ms("k_bwd_blend") + scan("false"), 4),
                     "rowsum_chain_ms": round(ms("k_bwd_rowsum_chain<false>"), 4),
                     "slot_offsets_ms": round(scan("false"), 4), "visible_scan_ms": round(scan("true"), 4),
                     "visible_rowsum_chain_ms": round(ms("k_bwd_rowsum_chain<true>"), 4),
                     "camera_blocks_ms": round(ms("k_bwd_camera_blocks"), 4), "camera_reduce_ms": round(ms("k_bwd_camera_reduce"), 4)}
        shutil.rmtree(d, ignore_errors=True)
    fm, bm, vm = float(np.median(fwd)), float(np.median(bwd)), float(np.median(bvis))
    print(json.dumps({"config": name, "width": w, "height": h, "gaussians": n, "elements": int(elems), "iters": a.iters,
                      "visible": vis[0], "forward_total_ms_median": round(fm, 4), "backward_ms_median": round(bm, 4),
                      "backward_vs_forward": round(bm / fm, 3), "backward_visible_ms_median": round(vm, 4),
                      "camera_ms": round(float(np.median(bcam)), 4), **split}), flush=True)
