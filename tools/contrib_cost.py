"""What pruning by contribution costs on the GPU (include/gsplat.h): gs_contrib_device on a frame, and gs_prune_below_device
on the whole cloud, next to the forward frame and gs_backward_visible_device of the same visit.  Per config (C and Chard
under their own cameras): one torch stream handed to gs_set_stream, every call bracketed by HIP events, the four calls
alternating in one loop so that all see the same neighbours; mean, median and min / max over --iters repetitions after
--warmup.  The prune copies records, m and v with a score that drops half the cloud (every second splat): it reads
4 bytes of score per splat three times (twice in the scan, once in the writer) and 3 x 336 bytes per kept splat, and writes
3 x 336 per kept splat; prune_bytes counts the score once.  With --trace the same loop runs again under
`rocprofv3 --kernel-trace --stats` (a child process) for the split of gs_contrib_device into its slot-offset scan,
k_contrib_blend and k_contrib_rowsum, next to k_bwd_blend of the same trace.

    python tools/contrib_cost.py [C Chard ...] [--iters 20] [--warmup 3] [--trace] [--out profiles/contrib_cost.txt] [--cache DIR]"""
import argparse, json, os, shutil, sys
import costlib
from costlib import ROOT

ap = argparse.ArgumentParser()
ap.add_argument("configs", nargs="*", default=["C", "Chard"])
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--trace", action="store_true", help="also split the calls into kernels with rocprofv3 (a second run)")
ap.add_argument("--child", action="store_true", help="run the loop only (under rocprofv3)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrib_cost.txt"))
costlib.add_cache_argument(ap)
a = ap.parse_args()

gs, _ = costlib.use_root()
import numpy as np
import torch

dev = torch.device("cuda:0")


def measure(name):
    aos, n, w, h, rm, sc, r = costlib.config_scene(name, record_timings=False, cache=a.cache)
    grad_image = costlib.image_grads(h, w)
    visible, ids, rows, count = costlib.visible_list(r, sc)
    elems = int(r.debugRead(gs.BUF_COUNT)[0])
    wmax, wsum = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pixels = torch.zeros(n, dtype=torch.int32, device=dev)
    records = torch.tensor(aos, device=dev)
    m, v = torch.rand_like(records), torch.rand_like(records)
    score = (torch.arange(n, device=dev) % 2).float()            # every second splat goes
    out = [torch.empty((n + 1) // 2, 84, device=dev) for _ in range(3)]
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    r.setStream(stream.cuda_stream)
    args = gs.Renderer._camera_args(sc.getCamera())
    calls = {
        "forward": lambda: r.drawCamera(*args, None, sync=False),
        "backward_visible": lambda: r.backwardVisibleDevice(grad_image.data_ptr(), None, ids.data_ptr(), rows.data_ptr(), visible,
                                                            count.data_ptr()),
        "contrib": lambda: r.contribDevice(n, wmax.data_ptr(), wsum.data_ptr(), pixels.data_ptr()),
        "contrib_wmax_only": lambda: r.contribDevice(n, wmax.data_ptr(), None, None),
        "prune": lambda: r.pruneBelowDevice(score.data_ptr(), 0.5, n, records.data_ptr(), None, m.data_ptr(), v.data_ptr(),
                                            out[0].data_ptr(), None, out[1].data_ptr(), out[2].data_ptr(), len(out[0]),
                                            counts.data_ptr()),
    }
    ms = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for it in range(a.warmup + a.iters):
            for k, call in calls.items():
                t = costlib.event_ms(stream, [call])[0]
                if it >= a.warmup:
                    ms[k].append(t)
    torch.cuda.synchronize()
    kept, dropped = (int(x) for x in counts.cpu().numpy().view(np.uint32))
    assert int(count.item()) == visible and kept == n // 2 and kept + dropped == n
    blended = int((wmax > 0).sum())
    assert 0 < blended <= visible
    r.setStream(None)
    r.cleanup()
    line = {"config": name, "width": w, "height": h, "gaussians": n, "elements": elems, "visible": visible, "blended": blended,
            "iters": a.iters, "warmup": a.warmup}
    for k, x in ms.items():
        line[k + "_ms_mean"], line[k + "_ms_median"], line[k + "_ms_min_max"] = costlib.summary(x)
    prune_bytes = 2 * 3 * 336 * kept + 4 * n
    line.update(contrib_vs_backward_visible=round(line["contrib_ms_median"] / line["backward_visible_ms_median"], 3),
                prune_kept=kept, prune_bytes=prune_bytes,
                prune_achieved_tbytes_per_s=round(prune_bytes / (line["prune_ms_median"] * 1e-3) / 1e12, 3))
    return line


if a.child:
    for name in a.configs:
        measure(name)
    sys.exit(0)


def trace(line):
    """The averages per launch of the kernels behind the calls, from a second run of the loop under rocprofv3."""
    stats = costlib.traced_child([os.path.abspath(__file__), line["config"], "--child", "--iters", str(a.iters), "--warmup", str(a.warmup)],
                                 400, "contrib_cost", cache=a.cache)
    ms = lambda *words: costlib.kernel_us(stats, words, "contrib_cost") / 1e3       # the kernels whose name holds every word
    scan = lambda src: sum(ms(k + "<", src) for k in ("k_splat_block_sums", "k_splat_scan_blocks", "k_splat_offsets"))
    line.update(k_contrib_blend_ms=round(ms("k_contrib_blend"), 4), k_contrib_rowsum_ms=round(ms("k_contrib_rowsum"), 4),
                slot_offsets_ms=round(scan("BwdSource<false>"), 4), k_bwd_blend_ms=round(ms("k_bwd_blend"), 4),
                k_bwd_rowsum_chain_ms=round(ms("k_bwd_rowsum_chain<true>"), 4),
                prune_scan_ms=round(scan("PruneSource"), 4), k_prune_write_ms=round(ms("k_prune_write"), 4))


HEADER = ("# tools/contrib_cost.py on one MI355X: gs_contrib_device (slot-offset scan + k_contrib_blend + k_contrib_rowsum; with wsum and pixels, and\n"
          "# with wmax alone) and gs_prune_below_device (scan + k_prune_write; records, m and v, every second splat dropped) next to the forward frame\n"
          "# (gs_render_device_async) and gs_backward_visible_device (max_rows = visible) of the same visit; configs under their own cameras; HIP events\n"
          "# around every call on one stream, the calls alternating in one loop; mean, median and [min, max] over `iters` repetitions after `warmup`.\n"
          "# prune_bytes = 2 x 3 x 336 x kept + 4 x n (rows read and written, the score once).  k_*_ms: rocprofv3 kernel stats of a second, traced\n"
          "# run of the same loop (averages per launch; slot_offsets_ms and prune_scan_ms = the three kernels of the per-splat scan).\n"
          "# Recorded numbers, not a bound.\n")
lines = [measure(name) for name in a.configs]
for line in lines:
    print(json.dumps(line), flush=True)
costlib.write_lines(a.out, HEADER, lines)                     # the event timings are on disk before the traced runs start
if a.trace:
    if not shutil.which("rocprofv3"):
        raise SystemExit("contrib_cost: --trace needs rocprofv3")
    for line in lines:
        trace(line)
        print(json.dumps(line), flush=True)
    costlib.write_lines(a.out, HEADER, lines)
