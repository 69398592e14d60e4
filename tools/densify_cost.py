"""What adaptive density control costs on the GPU (include/gsplat.h): gs_densify_stats_device behind a step's
gs_backward_visible_device, and gs_densify_device on the whole cloud.  Config C under its own camera: one frame, a random
image gradient, the visible-row backward; the statistics of --steps such steps; then the new cloud with a threshold at the
median mean gradient of the seen splats and the split scale at the median largest scale, so that clones and splits both
occur.  Everything runs on one torch stream handed to gs_set_stream; every repetition is bracketed by HIP events, and the
means are over --iters repetitions after --warmup.  Bytes: the statistics read 8 bytes per slot of a listed splat (two of
its row's ten floats, in 40-byte rows) + 12 of its raster record and read and write 12 bytes of the three arrays; the new
cloud reads 3 x 336 bytes per input splat (records, m, v; the rule's few floats three times more, out of the caches) + 12
of statistics and writes 3 x 336 per output.

    python tools/densify_cost.py [--config C] [--iters 20] [--warmup 3] [--steps 4] [--out profiles/densify_cost.txt]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densify_cost.txt"))
a = ap.parse_args()

import numpy as np
import torch
import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import synth

aos, cfg = synth.generate_config(a.config)
aos = np.ascontiguousarray(aos, dtype=np.float32)
n, w, h = len(aos), cfg["width"], cfg["height"]
rm = gs.ResourceManager(); rm.setGaussians(aos)
sc = gs.Scene(rm, aspect_ratio=w / h)
cam = sc.getCamera(); cam.setPosition((0, 0, 0)); cam.setRotation(0.0, 0.0); cam.recalculate()
r = gs.Renderer(w, h, record_timings=False, warmup_frames=0)
r.init(rm); r.initForScene(sc)

dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
grad_image = torch.tensor(rng.standard_normal((h, w, 4)).astype(np.float32), device=dev)
r.drawDevice(sc, None, sync=True)
rows_listed = r.visibleCount()
ids = torch.zeros(rows_listed, dtype=torch.int32, device=dev)
rows = torch.zeros(rows_listed, 84, device=dev)
count = torch.zeros(1, dtype=torch.int32, device=dev)
accum, seen, radius = torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, device=dev)
records = torch.tensor(aos, device=dev)
m, v = torch.rand_like(records), torch.rand_like(records)
out = [torch.empty(2 * n, 84, device=dev) for _ in range(3)]
counts = torch.zeros(4, dtype=torch.int32, device=dev)
stream = torch.cuda.Stream(device=dev)
torch.cuda.synchronize()
r.backwardVisibleDevice(grad_image.data_ptr(), None, ids.data_ptr(), rows.data_ptr(), rows_listed, count.data_ptr())
r.synchronize()
assert int(count.item()) == rows_listed
r.setStream(stream.cuda_stream)


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


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

mean_of = lambda x: round(float(np.mean(x)), 4)
spread = lambda x: [round(float(np.min(x)), 4), round(float(np.max(x)), 4)]
d_ms = mean_of(densify_ms)
densify_bytes = 3 * 336 * (n + n_out) + 12 * n
line = {"config": a.config, "width": w, "height": h, "gaussians": n, "rows": rows_listed, "iters": a.iters, "warmup": a.warmup,
        "stats_ms_mean": mean_of(stats_ms), "stats_ms_min_max": spread(stats_ms),
        "stats_steps_accumulated": a.steps, "grad_threshold": p.grad_threshold, "split_scale": p.split_scale,
        "outputs": n_out, "cloned": cloned, "split": split, "pruned": pruned,
        "densify_ms_mean": d_ms, "densify_ms_min_max": spread(densify_ms), "densify_bytes": densify_bytes,
        "densify_achieved_tbytes_per_s": round(densify_bytes / (d_ms * 1e-3) / 1e12, 3)}
print(json.dumps(line), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("# tools/densify_cost.py on one MI355X: gs_densify_stats_device on the rows of one gs_backward_visible_device, and\n"
            "# gs_densify_device (three scan launches + the write) on the whole cloud with records, m and v; config C under its own\n"
            "# camera; HIP events around every call on one stream, means (and min, max) over `iters` repetitions after `warmup`.\n"
            "# densify_bytes = 3 x 336 x (inputs + outputs) + 12 per input.  Recorded numbers, not a bound.\n")
    f.write(json.dumps(line) + "\n")
