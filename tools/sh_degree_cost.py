"""What a frame and its visible backward cost per SH mode (include/gsplat.h, GS_SH_*): degree 0, 1, 2, 3 = modes 2, 5, 4, 0.

In one process, the modes alternating frame by frame so that all see the same neighbours: the InitSortList bucket and the
frame total of gs_get_timings (hipEvents) and gs_backward_visible_device + gs_synchronize on the host clock (max_rows = |V|),
medians of --iters rounds after 3 warm-up rounds.  Then, per mode, a child process under `rocprofv3 --kernel-trace --stats`
that draws and differentiates in that mode alone: the mean launch of k_project (whichever instantiation the mode runs) and of
k_bwd_rowsum_chain<true>.  A trace without one of the two is an error, not a zero.  bytes_per_emitting_splat is what
k_project must read for a splat that emits, from shapes: 44 + 12 K with K = 1, 4, 9, 16 coefficients (position 12, scale
12, rotation 16, opacity 4; three planes per coefficient).  One JSON line per config.  The loop, the child and the trace are
costlib's variant_* routines, shared with antialias_cost.py.

    python tools/sh_degree_cost.py [C Chard ...] [--iters 10] [--modes 2 5 4 0] [--root TREE] [--cache DIR]

--root TREE imports the package (and its library) from another checkout of this repository, e.g. the parent commit with
--modes 0, to measure it with the same tool in the same visit."""
import argparse, json, os, shutil, sys
import costlib

ap = argparse.ArgumentParser()
ap.add_argument("configs", nargs="*", default=["C", "Chard"])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--modes", type=int, nargs="+", default=[2, 5, 4, 0])
ap.add_argument("--root", default=costlib.ROOT)
costlib.add_cache_argument(ap)
ap.add_argument("--child", type=int, default=None, metavar="MODE", help="draw + visible backward in MODE only (under rocprofv3)")
a = ap.parse_args()
ROOT = os.path.abspath(a.root)
costlib.use_root(ROOT)

COEFFICIENTS = {2: 1, 5: 4, 4: 9, 0: 16, 1: 15}
set_mode = lambda r, sc, mode: sc.getCamera().setShMode(mode)

if a.child is not None:
    costlib.variant_child(a.configs, set_mode, a.child, a.iters, a.cache)
    sys.exit(0)

for name in a.configs:
    medians, s, elems, visible = costlib.variant_rounds(name, set_mode, a.modes, a.iters, 1, a.cache)
    per_mode = {}
    for m in a.modes:
        per_mode[str(m)] = {"coefficients": COEFFICIENTS[m], "bytes_per_emitting_splat": 44 + 12 * COEFFICIENTS[m],
                            **{key: one[0] for key, one in medians[m].items()}}
        if shutil.which("rocprofv3"):
            per_mode[str(m)].update(costlib.variant_trace(
                [os.path.abspath(__file__), name, "--child", str(m), "--iters", str(a.iters), "--root", ROOT],
                f"sh_degree_cost ({name}, mode {m})", a.cache))
    print(json.dumps({"config": name, "width": s.w, "height": s.h, "gaussians": s.n, "elements": elems, "visible": visible,
                      "iters": a.iters, "modes": per_mode}), flush=True)
