"""What a cloud from points costs on the GPU (include/gsplat.h, gs_records_from_points_device and gs_knn_mean_dist2_device):
a uniform cube and the clustered cloud of synth.py's config Chard, at n = 100 000, 1 000 000 and the count of config C.

The whole calls are timed on the product library: HIP events around every call on one stream, means (and min, max) over
--iters repetitions after --warmup.  The six launches of a call -- bounds, codes, sort, gather + boxes, search, rows -- and
the two counts of the search are taken from a tuning build of the library (-DGS_INIT_PROBE: events between the launches, and
a search kernel that counts, per wave, the boxes that survive the coarse box-against-box test and those that survive the
per-lane point-against-box test), in a child process, since a process holds one build of the library:

    tools/build_variants.sh init_probe:-DGS_INIT_PROBE
    python tools/init_cost.py [--iters 5] [--warmup 2] [--out profiles/init_cost.txt]

Without build_variants/lib_init_probe.so the per-launch columns and the counts are left out and the file says so."""
import argparse, ctypes as C, json, os, subprocess, sys
import costlib
from costlib import ROOT
PROBE_LIB = os.path.join(ROOT, "build_variants", "lib_init_probe.so")
LAUNCHES = ("bounds", "codes", "sort", "gather_boxes", "search", "rows")

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sizes", default="100000,1000000,C")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_cost.txt"))
ap.add_argument("--probe-child", action="store_true", help=argparse.SUPPRESS)
a = ap.parse_args()

gs, synth = costlib.use_root()
import numpy as np
import torch
from vk3dgaussiansplatting_amd import _lib

sizes = [synth.CONFIGS["C"]["n"] if s == "C" else int(s) for s in a.sizes.split(",")]


def points_of(kind, n):
    """float32 [n, 3] in the .ply's frame and colours: a uniform cube, or the positions of the Chard generator (clustered)."""
    rng = np.random.default_rng(n)
    if kind == "uniform":
        p = rng.random((n, 3), dtype=np.float32) * np.float32(2) - np.float32(1)
    else:
        aos, _ = synth.generate_config("Chard", n=n)
        p = np.ascontiguousarray(aos[:, 0:3] * np.array([-1, -1, 1], np.float32))
    return p, rng.random((n, 3), dtype=np.float32)


dev = torch.device("cuda:0")
r = gs.Renderer(64, 64, record_timings=False)
r.init(gs.ResourceManager())
stream = torch.cuda.Stream(device=dev)
r.setStream(stream.cuda_stream)


timed = lambda call: costlib.event_ms(stream, [call])[0]
mean_of = lambda x: costlib.summary(x)[0]
spread = lambda x: costlib.summary(x)[2]
rows = []
for kind in ("uniform", "clustered"):
    for n in sizes:
        p_host, c_host = points_of(kind, n)
        p, c = torch.tensor(p_host, device=dev), torch.tensor(c_host, device=dev)
        rec = torch.empty(n, 84, device=dev)
        order = torch.empty(n, dtype=torch.int32, device=dev)
        d2 = torch.empty(n, device=dev)
        params = gs.default_init_params()
        torch.cuda.synchronize()
        records = lambda: r.recordsFromPointsDevice(p.data_ptr(), c.data_ptr(), n, params, rec.data_ptr(), order.data_ptr())
        knn = lambda: r.knnMeanDist2Device(p.data_ptr(), n, d2.data_ptr())
        row = {"cloud": kind, "n": n, "boxes": (n + 63) // 64}
        with torch.cuda.stream(stream):
            if a.probe_child:
                L = _lib.lib()
                records()
                coarse, lane, ms = C.c_uint64(), C.c_uint64(), (C.c_float * 6)()
                per = []
                for k in range(a.warmup + a.iters):
                    records()
                    rc = L.gs_init_probe_read(r._ctx.handle, C.c_uint32(n), C.byref(coarse), C.byref(lane), ms)
                    assert rc == 0, rc
                    if k >= a.warmup:
                        per.append(list(ms))
                row["launch_ms_mean"] = {name: mean_of([x[i] for x in per]) for i, name in enumerate(LAUNCHES)}
                waves = row["boxes"]
                row["coarse_survivors_per_wave"] = round(coarse.value / waves, 2)
                row["lane_survivors_per_wave"] = round(lane.value / waves, 2)
                row["coarse_tests_per_wave"] = waves - 1
            else:
                t_rec = [timed(records) for _ in range(a.warmup + a.iters)][a.warmup:]
                t_knn = [timed(knn) for _ in range(a.warmup + a.iters)][a.warmup:]
                row.update(records_ms_mean=mean_of(t_rec), records_ms_min_max=spread(t_rec), knn_ms_mean=mean_of(t_knn),
                           knn_ms_min_max=spread(t_knn))
        torch.cuda.synchronize()
        rows.append(row)
        print(json.dumps(row), flush=True)
        del p, c, rec, order, d2
r.setStream(None)
r.cleanup()
if a.probe_child:
    sys.exit(0)

# the per-launch times and the counts: the same clouds through the tuning build, in a fresh process
probe = {}
if os.path.exists(PROBE_LIB):
    env = dict(os.environ, GS_LIB_OVERRIDE=PROBE_LIB)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--probe-child", "--iters", str(a.iters), "--warmup", str(a.warmup),
                          "--sizes", a.sizes], env=env, check=True, stdout=subprocess.PIPE, text=True).stdout
    for ln in out.splitlines():
        if ln.startswith("{"):
            d = json.loads(ln)
            probe[(d["cloud"], d["n"])] = d
for row in rows:
    row.update({k: v for k, v in probe.get((row["cloud"], row["n"]), {}).items() if k not in row})

header = ("# tools/init_cost.py on one MI355X: gs_records_from_points_device (bounds, codes, sort, gather + boxes, search, rows) and\n"
          "# gs_knn_mean_dist2_device (the same without the rows) on a uniform cube and on the clustered cloud of config Chard; HIP\n"
          "# events around every call on one stream, means (and min, max) over `iters` repetitions after `warmup`.\n"
          "# launch_ms_mean and the survivor counts come from the -DGS_INIT_PROBE build (events between the launches, a counting\n"
          "# search): per wave of 64 query points, coarse_tests = the boxes tested against the wave's box (all others, 64 per\n"
          "# round), coarse_survivors = those the box-against-box bound kept, lane_survivors = those some lane's own\n"
          "# point-against-box bound kept, whose 64 points were then staged and tried.  Recorded numbers, not a bound.\n")
if not probe:
    header += "# build_variants/lib_init_probe.so was not there: no per-launch times and no counts in this run.\n"
lines = list(rows)
# Do the n^2 / 4096 coarse tests dominate at the largest count?  Everything else in the search is linear in n (the
# survivors per wave hardly move), so search_ms = a n + b n^2 through the two largest sizes separates the two.
top = sorted(sizes)[-2:]
for kind in ("uniform", "clustered"):
    two = [row for n in top for row in rows if row["cloud"] == kind and row["n"] == n and "launch_ms_mean" in row]
    if len(two) != 2 or top[0] == top[1]:
        continue
    (n1, t1), (n2, t2) = ((row["n"] / 1e6, row["launch_ms_mean"]["search"]) for row in two)
    b = (t2 - t1 * n2 / n1) / (n2 * n2 - n1 * n2)
    a_lin = t1 / n1 - b * n1
    big, ms = two[1], two[1]["launch_ms_mean"]
    quad = b * n2 * n2
    verdict = ("the coarse tests DOMINATE here: the next step is a second box level (a box per 64 boxes, tested first), not built"
               if quad > 0.5 * t2 else
               "the coarse tests do not dominate here; they would equal the linear part near n = "
               f"{a_lin / b:.0f} M, where the next step would be a second box level (a box per 64 boxes, tested first), not built"
               if b > 0 else "no quadratic part is measurable here; a second box level (a box per 64 boxes), the next step if it ever is, is not built")
    lines.append(f"# {kind} at n = {big['n']}: the search is {100 * ms['search'] / sum(ms.values()):.0f} % of the call; a wave makes "
            f"{big['coarse_tests_per_wave']} coarse tests (n^2 / 4096 in all) for {big['coarse_survivors_per_wave']} coarse and "
            f"{big['lane_survivors_per_wave']} per-lane survivors.  search_ms = {a_lin:.3f} n + {b:.4f} n^2 (n in millions, through the two "
            f"largest sizes): the quadratic part is {quad:.2f} of {t2:.2f} ms -- {verdict}.")
costlib.write_lines(a.out, header, lines)
