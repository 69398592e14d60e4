"""What a backward pass (gs_backward_device, include/gsplat.h) costs against the forward frame: the forward's total_ms
(gs_get_timings, hipEvents) and the backward's host-measured time (enqueue + gs_synchronize), medians of --iters runs after
3 warm-up runs; then the same backward again under `rocprofv3 --kernel-trace --stats` (a child process) for its split into
the blend backward (k_bwd_blend, with the three small kernels of the per-splat scan before it) and the row sum + chain
(k_bwd_rowsum_chain).  The visible form (gs_backward_visible_device with max_rows = |V|) is timed in the same window, dense
and visible iterations alternating in one process so that both see the same neighbours; it runs the <true> instantiations
of the same kernels, which the trace tells from the dense <false> ones by the template argument in the kernel name
(k_splat_offsets<gs::BwdSource<true>>; k_bwd_blend<false> is one kernel for both; <true> adds the absolute columns, tools/absgrad_cost.py).  A traced child that fails, or a trace in which a
part of the split matches no kernel, is an error, not a zero.  camera_ms is gs_backward_camera_device + gs_synchronize behind
the visible backward of the same iteration (it re-reads that backward's rows), in the same alternating loop; the trace splits
it into k_bwd_camera_blocks and k_bwd_camera_reduce.  One JSON line per config.

    python tools/backward_cost.py [C Chard ...] [--iters 20] [--cache DIR]"""
import argparse, json, os, shutil, sys
import costlib

ap = argparse.ArgumentParser()
ap.add_argument("configs", nargs="*", default=["C", "Chard"])
ap.add_argument("--iters", type=int, default=20)
costlib.add_cache_argument(ap)
ap.add_argument("--child", action="store_true", help="run the backward only (under rocprofv3)")
a = ap.parse_args()

costlib.use_root()
import numpy as np
import torch


def setup(name):
    s = costlib.config_scene(name, record_timings=1, cache=a.cache)
    gr, gd = costlib.image_grads(s.h, s.w, depth=True)
    out = torch.empty(s.n, 84, device="cuda")
    v, ids, rows, count = vis = costlib.visible_list(s.r, s.sc)
    cam = torch.zeros(35, device="cuda")
    torch.cuda.synchronize()
    r = s.r
    backward_ms = lambda: costlib.host_ms(r, lambda: r.backwardDevice(gr.data_ptr(), gd.data_ptr(), out.data_ptr()))
    visible_ms = lambda: costlib.host_ms(r, lambda: r.backwardVisibleDevice(gr.data_ptr(), gd.data_ptr(), ids.data_ptr(), rows.data_ptr(), v, count.data_ptr()))
    camera_ms = lambda: costlib.host_ms(r, lambda: r.backwardCameraDevice(cam.data_ptr()))
    return s, vis, cam, (backward_ms, visible_ms, camera_ms)


if a.child:
    for name in a.configs:
        s, vis, cam, timers = setup(name)
        for _ in range(a.iters):
            for ms in timers:
                ms()
        s.r.cleanup()
    sys.exit(0)

for name in a.configs:
    s, vis, cam, timers = setup(name)
    r = s.r
    fwd, bwd, bvis, bcam = [], [], [], []
    for it in range(3 + a.iters):
        r.drawDevice(s.sc, None, sync=True)
        total = r.timings().total_ms
        got = [ms() for ms in timers]
        if it >= 3:
            fwd.append(total); bwd.append(got[0]); bvis.append(got[1]); bcam.append(got[2])
    assert int(vis[3].item()) == vis[0]
    assert bool(torch.isfinite(cam).all()) and int((cam != 0).sum()) >= 20
    elems = r.timings().num_sort_elements
    r.cleanup()
    split = {}
    if shutil.which("rocprofv3"):
        stats = costlib.traced_child([os.path.abspath(__file__), name, "--child", "--iters", str(a.iters)], 300, "backward_cost", cache=a.cache)
        # the template argument tells the dense instantiation from the visible one
        ms = lambda key: costlib.kernel_us(stats, key, "backward_cost") / 1e3
        scan = lambda vis: sum(ms(f"{k}<gs::BwdSource<{vis}>>") for k in ("k_splat_block_sums", "k_splat_scan_blocks", "k_splat_offsets"))
        split = {"blend_backward_ms": round(ms("k_bwd_blend<false>") + scan("false"), 4),
                 "rowsum_chain_ms": round(ms("k_bwd_rowsum_chain<false>"), 4),
                 "slot_offsets_ms": round(scan("false"), 4), "visible_scan_ms": round(scan("true"), 4),
                 "visible_rowsum_chain_ms": round(ms("k_bwd_rowsum_chain<true>"), 4),
                 "camera_blocks_ms": round(ms("k_bwd_camera_blocks"), 4), "camera_reduce_ms": round(ms("k_bwd_camera_reduce"), 4)}
    print(json.dumps({"config": name, "width": s.w, "height": s.h, "gaussians": s.n, "elements": int(elems), "iters": a.iters,
                      "visible": vis[0], "forward_total_ms_median": costlib.median(fwd), "backward_ms_median": costlib.median(bwd),
                      "backward_vs_forward": round(float(np.median(bwd) / np.median(fwd)), 3), "backward_visible_ms_median": costlib.median(bvis),
                      "camera_ms": costlib.median(bcam), **split}), flush=True)
