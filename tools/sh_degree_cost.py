"""What a frame and its visible backward cost per SH mode (include/gsplat.h, GS_SH_*): degree 0, 1, 2, 3 = modes 2, 5, 4, 0.

In one process, the modes alternating frame by frame so that all see the same neighbours: the InitSortList bucket and the
frame total of gs_get_timings (hipEvents) and gs_backward_visible_device + gs_synchronize on the host clock (max_rows = |V|),
medians of --iters rounds after 3 warm-up rounds.  Then, per mode, a child process under `rocprofv3 --kernel-trace --stats`
that draws and differentiates in that mode alone: the mean launch of k_project (whichever instantiation the mode runs) and of
k_bwd_rowsum_chain<true>.  A trace without one of the two is an error, not a zero.  bytes_per_emitting_splat is what
k_project must read for a splat that emits, from shapes: 44 + 12 K with K = 1, 4, 9, 16 coefficients (position 12, scale
12, rotation 16, opacity 4; three planes per coefficient).  One JSON line per config.

    python tools/sh_degree_cost.py [C Chard ...] [--iters 10] [--modes 2 5 4 0] [--root TREE]

--root TREE imports the package (and its library) from another checkout of this repository, e.g. the parent commit with
--modes 0, to measure it with the same tool in the same visit."""
import argparse, csv, glob, json, os, re, shutil, subprocess, sys, tempfile, time

ap = argparse.ArgumentParser()
ap.add_argument("configs", nargs="*", default=["C", "Chard"])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--modes", type=int, nargs="+", default=[2, 5, 4, 0])
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--child", type=int, default=None, metavar="MODE", help="draw + visible backward in MODE only (under rocprofv3)")
a = ap.parse_args()
ROOT = os.path.abspath(a.root)
sys.path.insert(0, ROOT)

import numpy as np
import torch
import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import synth

COEFFICIENTS = {2: 1, 5: 4, 4: 9, 0: 16, 1: 15}


def setup(name, mode):
    """Context, scene and buffers; the first frame (which sizes the visible list) is drawn in `mode`, so that a traced child
    launches the kernels of its own mode alone."""
    aos, cfg = synth.generate_config(name)
    w, h = cfg["width"], cfg["height"]
    rm = gs.ResourceManager(); rm.setGaussians(aos)
    sc = gs.Scene(rm, aspect_ratio=w / h)
    cam = sc.getCamera(); cam.setPosition((0, 0, 0)); cam.setRotation(0.0, 0.0); cam.setShMode(mode); cam.recalculate()
    r = gs.Renderer(w, h, record_timings=1, warmup_frames=0)
    r.init(rm); r.initForScene(sc)
    gr = torch.tensor(np.random.default_rng(0).standard_normal((h, w, 4)).astype(np.float32), device="cuda")
    r.drawDevice(sc, None, sync=True)
    v = r.visibleCount()
    ids = torch.empty(max(v, 1), dtype=torch.int32, device="cuda")
    rows = torch.empty(max(v, 1), 84, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return r, sc, gr, (v, ids, rows, count), len(aos), w, h


def frame_and_backward(r, sc, gr, vis, mode):
    """-> (init_sort_list_ms, total_ms, visible backward ms)"""
    v, ids, rows, count = vis
    sc.getCamera().setShMode(mode)
    r.drawDevice(sc, None, sync=True)
    t = r.timings()
    t0 = time.perf_counter()
    r.backwardVisibleDevice(gr.data_ptr(), None, ids.data_ptr(), rows.data_ptr(), v, count.data_ptr())
    r.synchronize()
    return t.init_sort_list_ms, t.total_ms, (time.perf_counter() - t0) * 1e3


if a.child is not None:
    for name in a.configs:
        r, sc, gr, vis, n, w, h = setup(name, a.child)
        for _ in range(a.iters):
            frame_and_backward(r, sc, gr, vis, a.child)
        r.cleanup()
    sys.exit(0)


def traced(name, mode):
    """Mean launch (us) of k_project and k_bwd_rowsum_chain<true> in a child that runs `mode` alone."""
    d = tempfile.mkdtemp(prefix="sh_cost_")
    try:
        rc = subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
                             "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), name, "--child", str(mode),
                             "--iters", str(a.iters), "--root", ROOT], capture_output=True, text=True)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if rc.returncode != 0 or not files:
            raise SystemExit(f"sh_degree_cost: the traced run of {name} mode {mode} failed (exit {rc.returncode})\n{rc.stderr[-2000:]}")
        found = {}
        for row in csv.DictReader(open(files[0])):
            k = re.sub(r"^(void )?(gs::)?", "", row["Name"]).split("(")[0].replace(" ", "")
            if k.startswith("k_project<") or k == "k_bwd_rowsum_chain<true>":
                found[k] = (float(row["AverageNs"]) / 1e3, int(row["Calls"]))
        proj = [k for k in found if k.startswith("k_project<")]
        if len(proj) != 1 or "k_bwd_rowsum_chain<true>" not in found:
            raise SystemExit(f"sh_degree_cost: expected one k_project instantiation and k_bwd_rowsum_chain<true>, the trace has {sorted(found)}")
        return {"k_project": proj[0], "k_project_us": round(found[proj[0]][0], 2),
                "k_bwd_rowsum_chain_true_us": round(found["k_bwd_rowsum_chain<true>"][0], 2)}
    finally:
        shutil.rmtree(d, ignore_errors=True)


for name in a.configs:
    r, sc, gr, vis, n, w, h = setup(name, a.modes[0])
    seen ={m: ([], [], []) for m in a.modes}
    for it in range(3 + a.iters):
        for m in a.modes:
            got = frame_and_backward(r, sc, gr, vis, m)
            if it >= 3:
                for k in range(3):
                    seen[m][k].append(got[k])
    assert int(vis[3].item()) == vis[0]
    elems = r.timings().num_sort_elements
    r.cleanup()
    per_mode = {}
    for m in a.modes:
        per_mode[str(m)] = {"coefficients": COEFFICIENTS[m], "bytes_per_emitting_splat": 44 + 12 * COEFFICIENTS[m],
                            "init_sort_list_ms": round(float(np.median(seen[m][0])), 4), "total_ms": round(float(np.median(seen[m][1])), 4),
                            "backward_visible_ms": round(float(np.median(seen[m][2])), 4)}
        if shutil.which("rocprofv3"):
            per_mode[str(m)].update(traced(name, m))
    print(json.dumps({"config": name, "width": w, "height": h, "gaussians": n, "elements": int(elems), "visible": vis[0],
                      "iters": a.iters, "modes": per_mode}), flush=True)
