"""What anti-aliased frames (include/gsplat.h, gs_set_antialias) cost: a frame and its visible backward with the flag off and on.

In one process, the flags alternating frame by frame so that both see the same neighbours: the InitSortList bucket and the
frame total of gs_get_timings (hipEvents) and gs_backward_visible_device + gs_synchronize on the host clock (max_rows = |V|),
medians of --iters rounds after 3 warm-up rounds, the whole measurement --repeats times over (the spread between the repeats
is what a difference between two builds has to be read against).  Then, per flag, a child process under `rocprofv3
--kernel-trace --stats` that draws and differentiates with that flag alone: the mean launch of k_project (whichever
instantiation the flag runs) and of k_bwd_rowsum_chain<true>.  A trace without one of the two is an error, not a zero.  One JSON
line per config.

    python tools/antialias_cost.py [C ...] [--iters 10] [--repeats 3] [--flags 0 1] [--root TREE] [--no-trace]

--root TREE imports the package (and its library) from another checkout of this repository, e.g. the parent commit with
--flags 0 (it has no switch), to measure it with the same tool in the same visit.  --registers prints instead, without a GPU,
the registers and scratch of every k_project instantiation of --root from the compiler's resource-usage remarks.  The cloud
of a config is kept in --cache (if given) between the processes of a visit."""
import argparse, csv, glob, json, os, re, shutil, subprocess, sys, tempfile, time

ap = argparse.ArgumentParser()
ap.add_argument("configs", nargs="*", default=["C"])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--flags", type=int, nargs="+", default=[0, 1])
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--cache", default=None, metavar="DIR", help="keep the generated clouds here (e.g. a tmpfs)")
ap.add_argument("--no-trace", action="store_true")
ap.add_argument("--registers", action="store_true")
ap.add_argument("--child", type=int, default=None, metavar="FLAG", help="draw + visible backward with FLAG only (under rocprofv3)")
a = ap.parse_args()
ROOT = os.path.abspath(a.root)

if a.registers:
    csrc = os.path.join(ROOT, "vk3dgaussiansplatting_amd", "csrc")
    flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
             "-fhip-fp32-correctly-rounded-divide-sqrt"]                       # the Makefile's
    with tempfile.TemporaryDirectory() as d:
        rc = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                             os.path.join(csrc, "gs_project.hip"), "-o", os.path.join(d, "p.o")], capture_output=True, text=True)
    if rc.returncode != 0:
        raise SystemExit(rc.stderr[-2000:])
    rows, cur = [], None
    for ln in rc.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            cur = {"name": re.sub(r"^void gs::|\(.*$", "", name)}
            rows.append(cur)
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    for r in rows:
        if r["name"].startswith("k_project<"):
            print(f"#   {r['name']:<34} VGPRs {r['VGPRs']:3d}  SGPRs {r['TotalSGPRs']:3d}  SGPR spill {r['SGPRs Spill']:2d}  VGPR spill {r['VGPRs Spill']:2d}"
                  f"  scratch {r['ScratchSize [bytes/lane]']:2d} B/lane  occupancy {r['Occupancy [waves/SIMD]']} waves/SIMD")
    sys.exit(0)

sys.path.insert(0, ROOT)

import numpy as np
import torch
import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import synth


def cloud(name):
    cfg = dict(synth.CONFIGS[name])
    path = os.path.join(a.cache, f"antialias_cost_{name}.npy") if a.cache else None
    if path and os.path.exists(path):
        return np.load(path), cfg
    aos, cfg = synth.generate_config(name)
    if path:
        np.save(path, aos)
    return aos, cfg


def set_flag(r, flag):
    if hasattr(r, "setAntialias"):
        r.setAntialias(bool(flag))
    elif flag:
        raise SystemExit(f"antialias_cost: the package under {ROOT} has no Renderer.setAntialias")


def setup(name, flag):
    """Context, scene and buffers; the first frame (which sizes the visible list) is drawn with `flag`, so that a traced child
    launches the kernels of its own flag alone."""
    aos, cfg = cloud(name)
    w, h = cfg["width"], cfg["height"]
    rm = gs.ResourceManager(); rm.setGaussians(aos)
    sc = gs.Scene(rm, aspect_ratio=w / h)
    cam = sc.getCamera(); cam.setPosition((0, 0, 0)); cam.setRotation(0.0, 0.0); cam.recalculate()
    r = gs.Renderer(w, h, record_timings=1, warmup_frames=0)
    r.init(rm); r.initForScene(sc)
    set_flag(r, flag)
    gr = torch.tensor(np.random.default_rng(0).standard_normal((h, w, 4)).astype(np.float32), device="cuda")
    r.drawDevice(sc, None, sync=True)
    v = r.visibleCount()
    ids = torch.empty(max(v, 1), dtype=torch.int32, device="cuda")
    rows = torch.empty(max(v, 1), 84, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return r, sc, gr, (v, ids, rows, count), len(aos), w, h


def frame_and_backward(r, sc, gr, vis, flag):
    """-> (init_sort_list_ms, total_ms, visible backward ms)"""
    v, ids, rows, count = vis
    set_flag(r, flag)
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


def traced(name, flag):
    """Mean launch (us) of k_project and k_bwd_rowsum_chain<true> in a child that runs `flag` alone."""
    d = tempfile.mkdtemp(prefix="aa_cost_")
    try:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "p", "--",
               sys.executable, os.path.abspath(__file__), name, "--child", str(flag), "--iters", str(a.iters), "--root", ROOT]
        if a.cache:
            cmd += ["--cache", a.cache]
        rc = subprocess.run(cmd, capture_output=True, text=True)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if rc.returncode != 0 or not files:
            raise SystemExit(f"antialias_cost: the traced run of {name} flag {flag} failed (exit {rc.returncode})\n{rc.stderr[-2000:]}")
        found = {}
        for row in csv.DictReader(open(files[0])):
            k = re.sub(r"^(void )?(gs::)?", "", row["Name"]).split("(")[0].replace(" ", "")
            if k.startswith("k_project<") or k == "k_bwd_rowsum_chain<true>":
                found[k] = (float(row["AverageNs"]) / 1e3, int(row["Calls"]))
        proj = [k for k in found if k.startswith("k_project<")]
        if len(proj) != 1 or "k_bwd_rowsum_chain<true>" not in found:
            raise SystemExit(f"antialias_cost: expected one k_project instantiation and k_bwd_rowsum_chain<true>, the trace has {sorted(found)}")
        return {"k_project": proj[0], "k_project_us": round(found[proj[0]][0], 2),
                "k_bwd_rowsum_chain_true_us": round(found["k_bwd_rowsum_chain<true>"][0], 2)}
    finally:
        shutil.rmtree(d, ignore_errors=True)


for name in a.configs:
    r, sc, gr, vis, n, w, h = setup(name, a.flags[0])
    per_flag = {str(f): {"init_sort_list_ms": [], "total_ms": [], "backward_visible_ms": []} for f in a.flags}
    for rep in range(a.repeats):
        seen = {f: ([], [], []) for f in a.flags}
        for it in range(3 + a.iters):
            for f in a.flags:
                got = frame_and_backward(r, sc, gr, vis, f)
                if it >= 3:
                    for k in range(3):
                        seen[f][k].append(got[k])
        for f in a.flags:
            for k, key in enumerate(("init_sort_list_ms", "total_ms", "backward_visible_ms")):
                per_flag[str(f)][key].append(round(float(np.median(seen[f][k])), 4))     # one median per repeat
    assert int(vis[3].item()) == vis[0]
    elems = r.timings().num_sort_elements
    r.cleanup()
    if not a.no_trace and shutil.which("rocprofv3"):
        for f in a.flags:
            per_flag[str(f)].update(traced(name, f))
    print(json.dumps({"config": name, "root": os.path.relpath(ROOT), "width": w, "height": h, "gaussians": n, "elements": int(elems),
                      "visible": vis[0], "iters": a.iters, "repeats": a.repeats, "flags": per_flag}), flush=True)
