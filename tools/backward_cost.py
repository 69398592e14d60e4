"""What a backward pass (gs_backward_device, include/gsplat.h) costs against the forward frame: the forward's total_ms
(gs_get_timings, hipEvents) and the backward's host-measured time (enqueue + gs_synchronize), medians of --iters runs after
3 warm-up runs; then the same backward again under `rocprofv3 --kernel-trace --stats` (a child process) for its split into
the blend backward (k_bwd_blend, with the three small slot-offset kernels before it), the row sum (k_bwd_rowsum) and the
chain (k_bwd_chain).  One JSON line per config.

    python tools/backward_cost.py [C Chard ...] [--iters 20]"""
import argparse, csv, glob, json, os, shutil, subprocess, sys, tempfile, time
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


if a.child:
    for name in a.configs:
        r, sc, gr, gd, out, n, w, h = setup(name)
        r.drawDevice(sc, None, sync=True)
        for _ in range(a.iters):
            backward_ms(r, gr, gd, out)
        r.cleanup()
    sys.exit(0)

for name in a.configs:
    r, sc, gr, gd, out, n, w, h = setup(name)
    fwd, bwd = [], []
    for _ in range(3):
        r.drawDevice(sc, None, sync=True)
        backward_ms(r, gr, gd, out)
    for _ in range(a.iters):
        r.drawDevice(sc, None, sync=True)
        fwd.append(r.timings().total_ms)
        bwd.append(backward_ms(r, gr, gd, out))
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
            pick = lambda key: sum(v for k, v in us.items() if key in k)
            split = {"blend_backward_ms": round((pick("k_bwd_blend") + pick("k_bwd_block_sums") + pick("k_bwd_scan_blocks") +
                                                 pick("k_bwd_offsets")) / 1e3, 4),
                     "row_sum_ms": round(pick("k_bwd_rowsum") / 1e3, 4), "chain_ms": round(pick("k_bwd_chain") / 1e3, 4),
                     "slot_offsets_ms": round((pick("k_bwd_block_sums") + pick("k_bwd_scan_blocks") + pick("k_bwd_offsets")) / 1e3, 4)}
        shutil.rmtree(d, ignore_errors=True)
    fm, bm = float(np.median(fwd)), float(np.median(bwd))
    print(json.dumps({"config": name, "width": w, "height": h, "gaussians": n, "elements": int(elems), "iters": a.iters,
                      "forward_total_ms_median": round(fm, 4), "backward_ms_median": round(bm, 4),
                      "backward_vs_forward": round(bm / fm, 3), **split}), flush=True)
