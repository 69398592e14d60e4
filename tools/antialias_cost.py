"""What anti-aliased frames (include/gsplat.h, gs_set_antialias) cost: a frame and its visible backward with the flag off and on.

In one process, the flags alternating frame by frame so that both see the same neighbours: the InitSortList bucket and the
frame total of gs_get_timings (hipEvents) and gs_backward_visible_device + gs_synchronize on the host clock (max_rows = |V|),
medians of --iters rounds after 3 warm-up rounds, the whole measurement --repeats times over (the spread between the repeats
is what a difference between two builds has to be read against).  Then, per flag, a child process under `rocprofv3
--kernel-trace --stats` that draws and differentiates with that flag alone: the mean launch of k_project (whichever
instantiation the flag runs) and of k_bwd_rowsum_chain<true>.  A trace without one of the two is an error, not a zero.  One JSON
line per config.  The loop, the child and the trace are costlib's variant_* routines, shared with sh_degree_cost.py.

    python tools/antialias_cost.py [C ...] [--iters 10] [--repeats 3] [--flags 0 1] [--root TREE] [--no-trace]

--root TREE imports the package (and its library) from another checkout of this repository, e.g. the parent commit with
--flags 0 (it has no switch), to measure it with the same tool in the same visit.  --registers prints instead, without a GPU,
the registers and scratch of every k_project instantiation of --root from the compiler's resource-usage remarks.  The cloud
of a config is kept in --cache (if given) between the processes of a visit."""
import argparse, json, os, re, shutil, subprocess, sys, tempfile
import costlib

ap = argparse.ArgumentParser()
ap.add_argument("configs", nargs="*", default=["C"])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--flags", type=int, nargs="+", default=[0, 1])
ap.add_argument("--root", default=costlib.ROOT)
costlib.add_cache_argument(ap)
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

costlib.use_root(ROOT)


def set_flag(r, sc, flag):
    if hasattr(r, "setAntialias"):
        r.setAntialias(bool(flag))
    elif flag:
        raise SystemExit(f"antialias_cost: the package under {ROOT} has no Renderer.setAntialias")


if a.child is not None:
    costlib.variant_child(a.configs, set_flag, a.child, a.iters, a.cache)
    sys.exit(0)

for name in a.configs:
    medians, s, elems, visible = costlib.variant_rounds(name, set_flag, a.flags, a.iters, a.repeats, a.cache)
    per_flag = {str(f): medians[f] for f in a.flags}                         # one median per repeat
    if not a.no_trace and shutil.which("rocprofv3"):
        for f in a.flags:
            per_flag[str(f)].update(costlib.variant_trace(
                [os.path.abspath(__file__), name, "--child", str(f), "--iters", str(a.iters), "--root", ROOT],
                f"antialias_cost ({name}, flag {f})", a.cache))
    print(json.dumps({"config": name, "root": os.path.relpath(ROOT), "width": s.w, "height": s.h, "gaussians": s.n, "elements": elems,
                      "visible": visible, "iters": a.iters, "repeats": a.repeats, "flags": per_flag}), flush=True)
