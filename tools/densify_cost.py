"""What adaptive density control costs on the GPU (include/gsplat.h): gs_densify_stats_device behind a step's
gs_backward_visible_device, and gs_densify_device on the whole cloud.  Config C under its own camera: one frame, a random
image gradient, the visible-row backward; the statistics of --steps such steps; then the new cloud with a threshold at the
median mean gradient of the seen splats and the split scale at the median largest scale, so that clones and splits both
occur.  Everything runs on one torch stream handed to gs_set_stream; every repetition is bracketed by HIP events, and the
means are over --iters repetitions after --warmup.  Bytes: the statistics read 8 bytes per slot of a listed splat (two of
its row's ten floats, in 40-byte rows) + 12 of its raster record and read and write 12 bytes of the three arrays; the new
cloud reads 3 x 336 bytes per input splat (records, m, v; the rule's few floats three times more, out of the caches) + 12
of statistics and writes 3 x 336 per output.

    python tools/densify_cost.py [--config C] [--iters 20] [--warmup 3] [--steps 4] [--out profiles/densify_cost.txt] [--cache DIR]"""
import argparse, json, os
import costlib
from costlib import ROOT

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densify_cost.txt"))
costlib.add_cache_argument(ap)
a = ap.parse_args()

gs, _ = costlib.use_root()
import numpy as np
import torch

aos, n, w, h, rm, sc, r = costlib.config_scene(a.config, record_timings=False, cache=a.cache)
dev = torch.device("cuda:0")
rows_listed, ids, rows, count = costlib.visible_list(r, sc, costlib.image_grads(h, w))
accum, seen, radius = torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, device=dev)
records = torch.tensor(aos, device=dev)
m, v = torch.rand_like(records), torch.rand_like(records)
out = [torch.empty(2 * n, 84, device=dev) for _ in range(3)]
counts = torch.zeros(4, dtype=torch.int32, device=dev)
stream = torch.cuda.Stream(device=dev)
torch.cuda.synchronize()
r.setStream(stream.cuda_stream)
timed = lambda call: costlib.event_ms(stream, [call])[0]
stats = lambda: r.densifyStatsDevice(ids.data_ptr(), count.data_ptr(), rows_listed, n, accum.data_ptr(), seen.data_ptr(), radius.data_ptr())
stats_ms, densify_ms = [], []
with torch.cuda.stream(stream):
    for k in range(a.warmup + a.iters):
        t = timed(stats)
        if k >= a.warmup:
            stats_ms.append(t)
    # the statistics of --steps steps, from zero
    for t_ in (accum, seen, radius):
        t_.zero_()
    for _ in range(a.steps):
        stats()
    stream.synchronize()
    was_seen = seen > 0
    mean = (accum[was_seen] / seen[was_seen].float())
    p = gs.default_densify_params(grad_threshold=float(mean.median()), split_scale=float(records[:, 4:7].max(1).values.median()), seed=1)
    densify = lambda: r.densifyDevice(records.data_ptr(), m.data_ptr(), v.data_ptr(), n, accum.data_ptr(), seen.data_ptr(), radius.data_ptr(),
                                      p, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), 2 * n, counts.data_ptr())
    for k in range(a.warmup + a.iters):
        t = timed(densify)
        if k >= a.warmup:
            densify_ms.append(t)
torch.cuda.synchronize()
n_out, cloned, split, pruned = (int(x) for x in counts.cpu().numpy().view(np.uint32))
r.setStream(None)
r.cleanup()

(s_ms, _, s_spread), (d_ms, _, d_spread) = costlib.summary(stats_ms), costlib.summary(densify_ms)
densify_bytes = 3 * 336 * (n + n_out) + 12 * n
line = {"config": a.config, "width": w, "height": h, "gaussians": n, "rows": rows_listed, "iters": a.iters, "warmup": a.warmup,
        "stats_ms_mean": s_ms, "stats_ms_min_max": s_spread,
        "stats_steps_accumulated": a.steps, "grad_threshold": p.grad_threshold, "split_scale": p.split_scale,
        "outputs": n_out, "cloned": cloned, "split": split, "pruned": pruned,
        "densify_ms_mean": d_ms, "densify_ms_min_max": d_spread, "densify_bytes": densify_bytes,
        "densify_achieved_tbytes_per_s": round(densify_bytes / (d_ms * 1e-3) / 1e12, 3)}
print(json.dumps(line), flush=True)
costlib.write_lines(
    a.out, ("# tools/densify_cost.py on one MI355X: gs_densify_stats_device on the rows of one gs_backward_visible_device, and\n"
            "# gs_densify_device (three scan launches + the write) on the whole cloud with records, m and v; config C under its own\n"
            "# camera; HIP events around every call on one stream, means (and min, max) over `iters` repetitions after `warmup`.\n"
            "# densify_bytes = 3 x 336 x (inputs + outputs) + 12 per input.  Recorded numbers, not a bound.\n"), [line])
