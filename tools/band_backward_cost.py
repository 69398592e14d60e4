"""What the visible backward of a tile-row band (gs_set_band_gradients + gs_backward_visible_device, include/gsplat.h) costs
beside the whole frame's, on one GPU, one band after another: config C dealt into R = 2, 4, 8 contiguous bands (equal tile
rows) and R = 8 interleaved.  Per band: the sort elements of its frame, |V_band|, the host-timed call (enqueue +
gs_synchronize, median of --iters after one warm-up), and -- from one `rocprofv3 --kernel-trace` of a child process that runs
the same sequence -- the milliseconds of the scan (the three kernels of gs_splat_scan.h over BwdSource<true>), the blend
(k_bwd_blend) and the row sum + chain (k_bwd_rowsum_chain<true>): the child's launches are told apart by their order, five
per call.  The first entry is the whole grid on the same build; each dealing ends with its slowest band beside it.  Recorded,
not gated.  One JSON line per band and per dealing.

    python tools/band_backward_cost.py [--iters 5] [--out profiles/band_backward_cost.txt] [--cache DIR]"""
import argparse, json, os, shutil, sys
import costlib
from costlib import ROOT

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C")
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_backward_cost.txt"))
costlib.add_cache_argument(ap)
ap.add_argument("--child", action="store_true", help="run the sequence only (under rocprofv3)")
a = ap.parse_args()

costlib.use_root()
import numpy as np
import torch

CALL = ("k_splat_block_sums<gs::BwdSource<true>>", "k_splat_scan_blocks<gs::BwdSource<true>>",
        "k_splat_offsets<gs::BwdSource<true>>", "k_bwd_blend<false>", "k_bwd_rowsum_chain<true>")   # the launches of one call, in order


def sequence(gh):
    """[(dealing, band index, spec)]: spec None = the whole grid, ("rows", b, e) or ("il", phase, stride)."""
    seq = [("whole", 0, None)]
    for R in (2, 4, 8):
        edges = [round(k * gh / R) for k in range(R + 1)]
        seq += [(f"contiguous R={R}", k, ("rows", edges[k], edges[k + 1])) for k in range(R)]
    return seq + [("interleaved R=8", k, ("il", k, 8)) for k in range(8)]


def run(record):
    s = costlib.config_scene(a.config, record_timings=1, cache=a.cache)
    n, w, h, sc, r = s.n, s.w, s.h, s.sc, s.r
    r.setBandGradients(True)
    gr, gd = costlib.image_grads(h, w, depth=True)
    ids, rows = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, 84, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gh = (h + 15) // 16
    for dealing, k, spec in sequence(gh):
        if spec is None:
            r.setTileRows(0, gh)
        elif spec[0] == "rows":
            r.setTileRows(spec[1], spec[2])
        else:
            r.setTileRowsInterleaved(spec[1], spec[2], False)
        r.drawDevice(sc, None, sync=True)
        ms = [costlib.host_ms(r, lambda: r.backwardVisibleDevice(gr.data_ptr(), gd.data_ptr(), ids.data_ptr(), rows.data_ptr(), n, count.data_ptr()))
              for _ in range(a.iters + 1)]                      # the first is the warm-up
        record(dict(dealing=dealing, band=k, rows=None if spec is None else list(spec[1:]), elements=int(r.timings().num_sort_elements),
                    visible=int(count.item()), visible_backward_ms_median=costlib.median(ms[1:])))
    r.cleanup()
    return dict(config=a.config, width=w, height=h, gaussians=n, tiles_y=gh, iters=a.iters)


if a.child:
    run(lambda rec: None)
    sys.exit(0)

bands = []
head = run(bands.append)

# the split: one traced child, its launches in start order, five per call, iters + 1 calls per band
if shutil.which("rocprofv3"):
    seq = costlib.traced_child([os.path.abspath(__file__), "--child", "--config", a.config, "--iters", str(a.iters)], 500,
                               "band_backward_cost", stats=False, cache=a.cache)
    seq = [(k, ms) for k, ms in seq if k in CALL]
    calls = len(bands) * (a.iters + 1)
    if len(seq) != calls * len(CALL) or any(seq[i][0] != CALL[i % len(CALL)] for i in range(len(seq))):
        raise SystemExit(f"band_backward_cost: {len(seq)} launches of the backward in the trace, expected {calls} x {CALL}")
    per_call = np.array([ms for _, ms in seq]).reshape(len(bands), a.iters + 1, len(CALL))[:, 1:, :]
    med = np.median(per_call, axis=1)
    for b, m in zip(bands, med):
        b.update(scan_ms=round(float(m[0] + m[1] + m[2]), 4), blend_ms=round(float(m[3]), 4), rowsum_chain_ms=round(float(m[4]), 4))

lines = [json.dumps({**head, **b}) for b in bands]
whole = bands[0]
for dealing in dict.fromkeys(b["dealing"] for b in bands[1:]):
    mine = [b for b in bands if b["dealing"] == dealing]
    slow = max(mine, key=lambda b: b["visible_backward_ms_median"])
    lines.append(json.dumps(dict(dealing=dealing, slowest_band=slow["band"], slowest_visible_backward_ms=slow["visible_backward_ms_median"],
                                 whole_frame_visible_backward_ms=whole["visible_backward_ms_median"],
                                 slowest_vs_whole=round(slow["visible_backward_ms_median"] / whole["visible_backward_ms_median"], 3),
                                 sum_of_bands_ms=round(sum(b["visible_backward_ms_median"] for b in mine), 4),
                                 elements_sum=sum(b["elements"] for b in mine), visible_sum=sum(b["visible"] for b in mine))))
header = ("# tools/band_backward_cost.py on one MI355X: gs_backward_visible_device (max_rows = N) of a context that owns a band of tile rows, gs_set_band_gradients on,\n"
          "# one band after another on one context; host-timed call (enqueue + gs_synchronize), median; scan / blend / rowsum_chain from one rocprofv3 kernel trace of the same\n"
          "# sequence in a child process (medians over the same iterations).  The first line is the whole grid on the same build.  Recorded, not gated.\n")
costlib.write_lines(a.out, header, lines)
print("\n".join(lines), flush=True)
