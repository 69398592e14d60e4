"""What the optimiser step on the visible rows costs on the GPU (include/gsplat.h): gs_adam_rows_device +
gs_upload_rows_device against the route INTEGRATION.md documented before them, torch.optim.SparseAdam.step() on the same
sparse gradient + the full in-place gs_upload_gaussians_device.  Config C under its own camera: one frame, then
gs_backward_visible_device with a random image gradient lists the rows.  Everything runs on one torch stream handed to
gs_set_stream; every repetition is bracketed by HIP events (one pair per call, so the two halves of a route are also known
alone), the two routes alternate repetition by repetition so that both see the same neighbours, and the means are over
--iters repetitions after --warmup.  Bytes per row are what the Adam kernel has to move: the gradient's 59 fields read, and
the 59 fields of records, m and v read and written (7 x 236); the upload reads a record (336) and writes 60 plane values
(240), and both uploads then read 16 bytes per splat of the scene for the block bounds.  The raw-space step,
gs_adam_rows_raw_device, runs beside the record-space one on the same rows in the same repetitions (--out-raw): it also
writes the record's fields and reads its scale, rotation and opacity again (8 x 236 + 32 bytes per row).

    python tools/adam_cost.py [--config C] [--iters 20] [--warmup 3] [--out profiles/adam_cost.txt] [--out-raw profiles/adam_raw_cost.txt] [--cache DIR]"""
import argparse, json, os
import costlib
from costlib import ROOT, event_ms

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_cost.txt"))
ap.add_argument("--out-raw", default=os.path.join(ROOT, "profiles", "adam_raw_cost.txt"))
costlib.add_cache_argument(ap)
a = ap.parse_args()

gs, _ = costlib.use_root()
import numpy as np
import torch

ADAM_BYTES_PER_ROW = 7 * 59 * 4
ADAM_RAW_BYTES_PER_ROW = 8 * 59 * 4 + (3 + 4 + 1) * 4      # + the record's fields written, its scale, rotation and opacity read
UPLOAD_BYTES_PER_ROW = 336 + 60 * 4

aos, n, w, h, rm, sc, r = costlib.config_scene(a.config, record_timings=False, cache=a.cache)
dev = torch.device("cuda:0")
rows_listed, ids, rows, count = costlib.visible_list(r, sc, costlib.image_grads(h, w))

records = torch.tensor(aos, device=dev)
m, v = torch.zeros_like(records), torch.zeros_like(records)
# the documented route: one [N, 84] leaf, a sparse COO gradient over the listed rows, SparseAdam, then every record uploaded
leaf = torch.nn.Parameter(torch.tensor(aos, device=dev))
opt = torch.optim.SparseAdam([leaf], lr=1e-3)
leaf.grad = torch.sparse_coo_tensor(ids.long()[None], rows, size=(n, 84)).coalesce()
stream = torch.cuda.Stream(device=dev)
torch.cuda.synchronize()
r.setStream(stream.cuda_stream)
step = [0]


def adam():
    step[0] += 1
    r.adamRowsDevice(records.data_ptr(), m.data_ptr(), v.data_ptr(), n, ids.data_ptr(), rows.data_ptr(), count.data_ptr(),
                     rows_listed, gs.default_adam_params(step=step[0]))


# the raw route (gs_adam_rows_raw_device) on the same rows: its own raw / records / m / v, records == act(raw) from the start
raw, raw_records = torch.zeros_like(records), torch.tensor(aos, device=dev)
raw_m, raw_v = torch.zeros_like(records), torch.zeros_like(records)
torch.cuda.synchronize()
r.rawFromRecordsDevice(raw_records.data_ptr(), raw.data_ptr(), n)
r.recordsFromRawDevice(raw.data_ptr(), raw_records.data_ptr(), n)
r.synchronize()
raw_step = [0]


def adam_raw():
    raw_step[0] += 1
    r.adamRowsRawDevice(raw.data_ptr(), raw_records.data_ptr(), raw_m.data_ptr(), raw_v.data_ptr(), n, ids.data_ptr(), rows.data_ptr(),
                        count.data_ptr(), rows_listed, gs.default_adam_params(space="raw", step=raw_step[0]))


new_route = [adam, lambda: r.uploadRowsDevice(records.data_ptr(), n, ids.data_ptr(), count.data_ptr(), rows_listed)]
old_route = [opt.step, lambda: r.uploadDevice(leaf.data_ptr(), n)]
new_ms, old_ms, raw_ms = [], [], []
with torch.cuda.stream(stream):
    for k in range(a.warmup + a.iters):
        t_new, t_raw, t_old = event_ms(stream, new_route), event_ms(stream, [adam_raw]), event_ms(stream, old_route)
        if k >= a.warmup:
            new_ms.append(t_new)
            old_ms.append(t_old)
            raw_ms.append(t_raw)
torch.cuda.synchronize()
r.setStream(None)
r.cleanup()

new_ms, old_ms = np.array(new_ms), np.array(old_ms)
mean = lambda x: costlib.summary(x)[0]
spread = lambda x: costlib.summary(x)[2]
adam_ms, upload_rows_ms = mean(new_ms[:, 0]), mean(new_ms[:, 1])
new_total, old_total = mean(new_ms.sum(1)), mean(old_ms.sum(1))
line = {"config": a.config, "width": w, "height": h, "gaussians": n, "rows": rows_listed, "iters": a.iters, "warmup": a.warmup,
        "adam_rows_ms_mean": adam_ms, "adam_rows_ms_min_max": spread(new_ms[:, 0]),
        "adam_bytes_per_row": ADAM_BYTES_PER_ROW,
        "adam_achieved_tbytes_per_s": round(rows_listed * ADAM_BYTES_PER_ROW / (adam_ms * 1e-3) / 1e12, 3),
        "upload_rows_ms_mean": upload_rows_ms, "upload_rows_ms_min_max": spread(new_ms[:, 1]),
        "upload_rows_bytes_per_row": UPLOAD_BYTES_PER_ROW, "block_bounds_bytes_per_gaussian": 16,
        "upload_rows_achieved_tbytes_per_s": round((rows_listed * UPLOAD_BYTES_PER_ROW + 16 * n) / (upload_rows_ms * 1e-3) / 1e12, 3),
        "adam_rows_plus_upload_rows_ms_mean": new_total, "adam_rows_plus_upload_rows_ms_min_max": spread(new_ms.sum(1)),
        "sparse_adam_step_ms_mean": mean(old_ms[:, 0]), "sparse_adam_step_ms_min_max": spread(old_ms[:, 0]),
        "full_upload_ms_mean": mean(old_ms[:, 1]), "full_upload_ms_min_max": spread(old_ms[:, 1]),
        "sparse_adam_plus_full_upload_ms_mean": old_total, "sparse_adam_plus_full_upload_ms_min_max": spread(old_ms.sum(1)),
        "documented_route_over_new_route": round(old_total / new_total, 2),
        "new_route_is_faster": bool(new_total < old_total)}
print(json.dumps(line), flush=True)
costlib.write_lines(
    a.out, "# tools/adam_cost.py on one MI355X: gs_adam_rows_device + gs_upload_rows_device against torch.optim.SparseAdam.step() on the\n"
            "# same sparse gradient + the full in-place gs_upload_gaussians_device; config C under its own camera, the rows of one\n"
            "# gs_backward_visible_device; HIP events around every call on one stream, the routes alternating, means (and min, max) over\n"
            "# `iters` repetitions after `warmup`.  GPU times; the host-side wait for the count that the documented route also needs\n"
            "# (gs_visible_count, to size the COO tensor) is not in them.  Recorded numbers, not a bound.\n", [line])

# the raw step beside the record step, the same rows in the same run
raw_ms = np.array(raw_ms)
raw_mean = mean(raw_ms[:, 0])
raw_line = {"config": a.config, "width": w, "height": h, "gaussians": n, "rows": rows_listed, "iters": a.iters, "warmup": a.warmup,
            "adam_rows_raw_ms_mean": raw_mean, "adam_rows_raw_ms_min_max": spread(raw_ms[:, 0]),
            "adam_raw_bytes_per_row": ADAM_RAW_BYTES_PER_ROW,
            "adam_raw_achieved_tbytes_per_s": round(rows_listed * ADAM_RAW_BYTES_PER_ROW / (raw_mean * 1e-3) / 1e12, 3),
            "adam_rows_ms_mean": adam_ms, "adam_rows_ms_min_max": spread(new_ms[:, 0]), "adam_bytes_per_row": ADAM_BYTES_PER_ROW,
            "adam_achieved_tbytes_per_s": line["adam_achieved_tbytes_per_s"],
            "raw_over_records_ms": round(raw_mean / adam_ms, 3),
            "raw_over_records_bytes": round(ADAM_RAW_BYTES_PER_ROW / ADAM_BYTES_PER_ROW, 3)}
# the finding, from the two ratios: a kernel that moves its bytes at (nearly) its neighbour's rate is bound by them as that one is
rate_ratio = raw_line["adam_raw_achieved_tbytes_per_s"] / raw_line["adam_achieved_tbytes_per_s"]
raw_line["raw_rate_over_records_rate"] = round(rate_ratio, 3)
raw_line["raw_is_bandwidth_bound_like_records"] = bool(rate_ratio >= 0.9)
finding = (f"# Finding of this run: the times are in the ratio {raw_line['raw_over_records_ms']}, the bytes in the ratio "
           f"{raw_line['raw_over_records_bytes']}; the raw kernel moves {raw_line['adam_raw_achieved_tbytes_per_s']} TB/s, "
           f"{round(100 * rate_ratio, 1)} % of the record kernel's {raw_line['adam_achieved_tbytes_per_s']} TB/s in the same run: ")
finding += ("the exps, the division and the square root did not make it VALU-bound.\n" if rate_ratio >= 0.9 else
            "well below what the bytes say -- the arithmetic (four exps, a division and a square root per row) shows; "
            "look at its VALU busy before trusting the byte count.\n")
print(json.dumps(raw_line), flush=True)
costlib.write_lines(
    a.out_raw, "# tools/adam_cost.py on one MI355X: gs_adam_rows_raw_device beside gs_adam_rows_device, the same listed rows in the same run,\n"
            "# the calls alternating; HIP events around every call, means (and min, max) over `iters` repetitions after `warmup`.\n"
            "# Bytes per row: the raw kernel reads the gradient's 59 fields, reads and writes the 59 fields of raw, m and v, writes the\n"
            "# record's 59 fields (8 x 236) and reads the record's scale, rotation and opacity again (32); the record kernel moves 7 x 236.\n"
            "# It also evaluates four pinned exps per row.  Recorded numbers, not a bound; both kernels' times and the\n"
            "# ratios are of this one run.\n" + finding, [raw_line])
