"""What gs_set_abs_gradients (include/gsplat.h) costs gs_backward_visible_device, in three builds measured in one visit: the
parent commit (--root names its checkout, built), this commit with the switch off, and this commit with the switch on.  Every
measurement is a fresh child process under `rocprofv3 --kernel-trace --stats` that imports the package of its own checkout and
runs --iters visible backwards per config after 3 warm-up runs; the builds alternate (parent, off, on), --repeats times, so
that each build's repeated runs show the spread a build has against itself in this visit.  Per config the profile holds the mean
launch of k_bwd_blend (and of k_bwd_rowsum_chain<true> and the three scan kernels) per run, both spreads, the verdict "the
switch-off median lies inside the parent's own [min, max]", the on / off ratio, the bytes the switch adds (8 per list element
of capacity, 2 KiB of LDS per workgroup), and the registers, LDS and scratch of the kernel's instantiations in both checkouts
(k_bwd_blend.usage beside the sources where a build left it, else one device-only compile).

    python tools/absgrad_cost.py [C Chard ...] --root ../parent [--iters 20] [--repeats 5] [--cache DIR] [--out profiles/absgrad_cost.txt]
    python tools/absgrad_cost.py --resources-only [--root ../parent]      # no GPU: the resource tables alone"""
import argparse, json, os, re, subprocess, sys, tempfile
import costlib

ap = argparse.ArgumentParser()
ap.add_argument("configs", nargs="*", default=["C", "Chard"])
ap.add_argument("--root", default=None, help="the parent commit's checkout, built")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(costlib.ROOT, "profiles", "absgrad_cost.txt"))
ap.add_argument("--resources-only", action="store_true")
costlib.add_cache_argument(ap)
ap.add_argument("--child", choices=["parent", "off", "on"], help="run the backwards of one build only (under rocprofv3)")
a = ap.parse_args()

SCAN = ("k_splat_block_sums<gs::BwdSource<true>>", "k_splat_scan_blocks<gs::BwdSource<true>>", "k_splat_offsets<gs::BwdSource<true>>")
USAGE = re.compile(r"(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)")


def resource_usage(root):
    """{instantiation: {SGPRs, VGPRs, scratch, occupancy, LDS}} of k_bwd_blend in the checkout at root."""
    csrc = os.path.join(root, "vk3dgaussiansplatting_amd", "csrc")
    kept = os.path.join(csrc, "k_bwd_blend.usage")
    if os.path.exists(kept):
        text = open(kept).read()
    else:
        flags = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt"
        rc = subprocess.run(["hipcc", *flags.split(), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "gs_backward.hip",
                             "-o", os.devnull], cwd=csrc, capture_output=True, text=True)
        if rc.returncode != 0:
            raise SystemExit(f"absgrad_cost: gs_backward.hip of {root} does not compile\n{rc.stderr[-2000:]}")
        text = re.sub(r" *\[-Rpass[^\]]*\]", "", rc.stderr)
    table, name = {}, None
    for key, value in USAGE.findall(text):
        if key == "Function Name":
            name = "k_bwd_blend" + ("<true>" if "ILb1E" in value else "<false>" if "ILb0E" in value else "") if "k_bwd_blend" in value else None
        elif name:
            table.setdefault(name, {})[key.split(" [")[0]] = int(value)
    if not table:
        raise SystemExit(f"absgrad_cost: no k_bwd_blend in the resource usage of {root}")
    return table


def child():
    gs, _ = costlib.use_root(a.root if a.child == "parent" else None)
    for name in a.configs:
        s = costlib.config_scene(name, record_timings=1, cache=a.cache)
        if a.child != "parent":
            s.r.setAbsGradients(a.child == "on")
        gr, gd = costlib.image_grads(s.h, s.w, depth=True)
        v, ids, rows, count = costlib.visible_list(s.r, s.sc)
        for _ in range(3 + a.iters):
            s.r.backwardVisibleDevice(gr.data_ptr(), gd.data_ptr(), ids.data_ptr(), rows.data_ptr(), v, count.data_ptr())
            s.r.synchronize()
        assert int(count.item()) == v
        s.r.cleanup()


if a.child:
    child()
    sys.exit(0)

here, parent = resource_usage(costlib.ROOT), resource_usage(a.root) if a.root else None
same = parent is not None and here["k_bwd_blend<false>"] == next(iter(parent.values()))
lines = [{"resource_usage": "this commit", **here}]
if parent is not None:
    lines += [{"resource_usage": "parent commit", **parent}, {"k_bwd_blend<false>_equals_the_parent's_kernel_in_every_figure": same}]
if a.resources_only:
    for line in lines:
        print(json.dumps(line))
    sys.exit(0)
if not a.root:
    raise SystemExit("absgrad_cost: --root must name the parent commit's checkout")

gs, synth = costlib.use_root(torch=False)
cache = a.cache or tempfile.mkdtemp(prefix="absgrad_cost_")
for name in a.configs:
    runs = {b: [] for b in ("parent", "off", "on")}
    for _ in range(a.repeats):
        for build in runs:
            argv = [os.path.abspath(__file__), name, "--child", build, "--iters", str(a.iters)] + (["--root", a.root] if a.root else [])
            stats = costlib.traced_child(argv, 400, "absgrad_cost", cache=cache)
            blend = costlib.find_kernels(stats, ("k_bwd_blend",), "absgrad_cost")
            want = {"parent": "k_bwd_blend", "off": "k_bwd_blend<false>", "on": "k_bwd_blend<true>"}[build]
            if blend != [want]:
                raise SystemExit(f"absgrad_cost: build {build} launched {blend}, not {want}")
            runs[build].append({"k_bwd_blend_us": round(stats[want].average_us, 2), "calls": stats[want].calls,
                                "k_bwd_rowsum_chain_true_us": round(costlib.kernel_us(stats, "k_bwd_rowsum_chain<true>", "absgrad_cost"), 2),
                                "scan_us": round(sum(costlib.kernel_us(stats, k, "absgrad_cost") for k in SCAN), 2)})
    us = {b: [run["k_bwd_blend_us"] for run in runs[b]] for b in runs}
    cfg = synth.CONFIGS[name]
    tiles = ((cfg["width"] + 15) // 16) * ((cfg["height"] + 15) // 16)
    capacity = 1
    while capacity < cfg["n"] + 1024 * tiles:
        capacity *= 2
    med = {b: costlib.median(us[b]) for b in us}
    lines.append({"config": name, "iters": a.iters, "repeats": a.repeats, "runs": runs,
                  "k_bwd_blend_us_median": med, "k_bwd_blend_us_min_max": {b: [min(us[b]), max(us[b])] for b in us},
                  "parent_spread_us": round(max(us["parent"]) - min(us["parent"]), 2), "off_spread_us": round(max(us["off"]) - min(us["off"]), 2),
                  "off_median_inside_parent_min_max": min(us["parent"]) <= med["off"] <= max(us["parent"]),
                  "off_over_parent": round(med["off"] / med["parent"], 4), "on_over_off": round(med["on"] / med["off"], 4),
                  "abs_rows_bytes": 8 * capacity, "rows_bytes": 40 * capacity, "lds_bytes_added_per_workgroup": 4 * 64 * 2 * 4})
header = ("# tools/absgrad_cost.py: gs_backward_visible_device in three builds alternating in one visit (parent commit, this commit with\n"
          "# gs_set_abs_gradients off, and on); mean launch of k_bwd_blend per traced child run (rocprofv3 --kernel-trace --stats), microseconds.\n"
          "# The switch off must cost nothing: its median against the parent's own [min, max].  The switch on is reported, not bounded.\n")
costlib.write_lines(a.out, header, lines)
for line in lines:
    print(json.dumps(line), flush=True)
