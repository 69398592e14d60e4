"""What summing the visible rows of several views costs on the GPU (include/gsplat.h): gs_rows_accumulate_device per view and one
gs_rows_collect_device, against the route a torch trainer has without them -- index_add_ of every view's rows into a dense
[N, 84] gradient, the touched rows found with nonzero (which waits on the host for their number) and gathered -- and next to
gs_membench's device-to-device copy rate on the same device in the same run.  Config C under two cameras (its own and a nearby
pose): one frame and one gs_backward_visible_device with a random image gradient per camera list the rows.  Everything runs on
one torch stream handed to gs_set_stream; every call is bracketed by HIP events, the two routes alternate repetition by
repetition, and the means are over --iters repetitions after --warmup.  Bytes are what the kernels have to move, computed
from the counts of this run:
  accumulate, per listed row: the row's 59 fields read and acc's written (2 x 236), acc's read as well unless the touch is the
             splat's first (+ 236), the id read twice and the mark read twice and written once (20);
  collect:   mark read twice and the scan's offset written per splat (12 n); per member of the union its mark cleared and its id
             written and read again (12), its 59 fields read and a whole row written (236 + 336).
Then, as an observation only, the per-view losses of 20 VisibleAdam.step_batch steps on the dense test scene under the tests' two
cameras.

    python tools/batch_cost.py [--config C] [--iters 20] [--warmup 3] [--out profiles/batch_cost.txt] [--cache DIR]"""
import argparse, ctypes as C, json, os, sys
import costlib
from costlib import ROOT, event_ms
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_cost.txt"))
costlib.add_cache_argument(ap)
a = ap.parse_args()

gs, _ = costlib.use_root()
import numpy as np
import torch
from vk3dgaussiansplatting_amd import _lib

POSES = (dict(pos=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0), dict(pos=(0.2, 0.1, -0.5), yaw=0.1, pitch=-0.05))
WEIGHTS = (0.5, 0.5)
FIELD_BYTES, ROW_BYTES = 59 * 4, 336

aos, n, w, h, rm, sc, r = costlib.config_scene(a.config, record_timings=False, cache=a.cache)
dev = torch.device("cuda:0")
grad_image = costlib.image_grads(h, w)
views = []
for pose in POSES:
    cam = sc.getCamera(); cam.setPosition(pose["pos"]); cam.setRotation(pose["yaw"], pose["pitch"]); cam.recalculate()
    listed, ids, rows, count = costlib.visible_list(r, sc, grad_image)
    views.append((ids, rows, count, listed))

acc = torch.empty(n, 84, device=dev)
mark = torch.zeros(n, dtype=torch.int32, device=dev)
ids_out = torch.zeros(n, dtype=torch.int32, device=dev)
rows_out = torch.zeros(n, 84, device=dev)
count_out = torch.zeros(1, dtype=torch.int32, device=dev)
# the torch route's buffers: the dense gradient and the touched flags, and the views' ids as the int64 torch indexes with
dense = torch.zeros(n, 84, device=dev)
flags = torch.zeros(n, dtype=torch.bool, device=dev)
ids64 = [v[0].long() for v in views]
stream = torch.cuda.Stream(device=dev)
torch.cuda.synchronize()
r.setStream(stream.cuda_stream)


def accumulate(b):
    ids, rows, count, listed = views[b]
    return lambda: r.rowsAccumulateDevice(acc.data_ptr(), mark.data_ptr(), n, ids.data_ptr(), rows.data_ptr(), count.data_ptr(), listed, WEIGHTS[b])


def collect():
    r.rowsCollectDevice(acc.data_ptr(), mark.data_ptr(), n, ids_out.data_ptr(), rows_out.data_ptr(), n, count_out.data_ptr())


torch_out = {}


def torch_clear():
    dense.zero_()
    flags.zero_()


def torch_add(b):
    def call():
        dense.index_add_(0, ids64[b], views[b][1], alpha=WEIGHTS[b])
        flags[ids64[b]] = True
    return call


def torch_list():
    idx = flags.nonzero().squeeze(1)              # waits on the host for the number of touched rows
    torch_out["ids"], torch_out["rows"] = idx, dense.index_select(0, idx)


new_route = [accumulate(0), accumulate(1), collect]
old_route = [torch_clear, torch_add(0), torch_add(1), torch_list]
new_ms, old_ms = [], []
with torch.cuda.stream(stream):
    for k in range(a.warmup + a.iters):
        t_new, t_old = event_ms(stream, new_route), event_ms(stream, old_route)
        if k >= a.warmup:
            new_ms.append(t_new)
            old_ms.append(t_old)
torch.cuda.synchronize()
union = int(count_out.cpu().numpy().view(np.uint32)[0])
# the two routes list the same splats, and sum the same values up to the last bits (index_add_ multiplies and adds in one)
assert union == len(torch_out["ids"]) and bool((torch_out["ids"] == ids_out[:union].long()).all())
worst = float((torch_out["rows"] - rows_out[:union]).abs().max())
scale = float(rows_out[:union].abs().max())
r.setStream(None)

# the copy rate of the same device in the same run: 1 GiB buffers, 16-byte accesses, plain and with four loads in flight
L, hctx = _lib.lib(), r._ctx.handle
copy = {}
for kind, name in ((1, "copy16"), (10, "copy16_x4")):
    g_, ms_ = C.c_float(), C.c_float()
    assert L.gs_membench(hctx, kind, 1 << 30, 0, 20, C.byref(g_), C.byref(ms_)) == 0
    copy[name] = round(g_.value / 1e3, 3)
r.cleanup()

new_ms, old_ms = np.array(new_ms), np.array(old_ms)
mean = lambda x: costlib.summary(x)[0]
spread = lambda x: costlib.summary(x)[2]
listed = [v[3] for v in views]
common = listed[0] + listed[1] - union
acc_bytes = [listed[0] * (2 * FIELD_BYTES + 20), listed[1] * (2 * FIELD_BYTES + 20) + common * FIELD_BYTES]
col_bytes = 12 * n + union * (12 + FIELD_BYTES + ROW_BYTES)
rate = lambda b, ms: round(b / (ms * 1e-3) / 1e12, 3)
best_copy = max(copy.values())
line = {"config": a.config, "width": w, "height": h, "gaussians": n, "rows_view0": listed[0], "rows_view1": listed[1],
        "rows_in_both": common, "rows_union": union, "weights": list(WEIGHTS), "iters": a.iters, "warmup": a.warmup,
        "accumulate_view0_ms_mean": mean(new_ms[:, 0]), "accumulate_view0_ms_min_max": spread(new_ms[:, 0]),
        "accumulate_view0_bytes": acc_bytes[0], "accumulate_view0_tbytes_per_s": rate(acc_bytes[0], mean(new_ms[:, 0])),
        "accumulate_view1_ms_mean": mean(new_ms[:, 1]), "accumulate_view1_ms_min_max": spread(new_ms[:, 1]),
        "accumulate_view1_bytes": acc_bytes[1], "accumulate_view1_tbytes_per_s": rate(acc_bytes[1], mean(new_ms[:, 1])),
        "collect_ms_mean": mean(new_ms[:, 2]), "collect_ms_min_max": spread(new_ms[:, 2]),
        "collect_bytes": col_bytes, "collect_tbytes_per_s": rate(col_bytes, mean(new_ms[:, 2])),
        "membench_copy_tbytes_per_s": copy,
        "accumulate_view0_over_copy": round(rate(acc_bytes[0], mean(new_ms[:, 0])) / best_copy, 3),
        "accumulate_view1_over_copy": round(rate(acc_bytes[1], mean(new_ms[:, 1])) / best_copy, 3),
        "collect_over_copy": round(rate(col_bytes, mean(new_ms[:, 2])) / best_copy, 3),
        "two_accumulates_plus_collect_ms_mean": mean(new_ms.sum(1)), "two_accumulates_plus_collect_ms_min_max": spread(new_ms.sum(1)),
        "torch_zero_ms_mean": mean(old_ms[:, 0]), "torch_index_add_view0_ms_mean": mean(old_ms[:, 1]),
        "torch_index_add_view1_ms_mean": mean(old_ms[:, 2]), "torch_nonzero_gather_ms_mean": mean(old_ms[:, 3]),
        "torch_route_ms_mean": mean(old_ms.sum(1)), "torch_route_ms_min_max": spread(old_ms.sum(1)),
        "torch_route_over_new_route": round(mean(old_ms.sum(1)) / mean(new_ms.sum(1)), 2),
        "routes_list_the_same_splats": True, "largest_difference_of_a_sum": worst, "largest_sum": scale}
print(json.dumps(line), flush=True)

# ---- the observation: 20 step_batch steps on the dense test scene under the tests' two cameras
from vk3dgaussiansplatting_amd.autograd import VisibleAdam
from test_outputs_cpu import SCENES

STEPS = 20
d_aos, dw, dh = SCENES["dense"]()
d_aos = np.ascontiguousarray(d_aos, dtype=np.float32)
truth = d_aos.copy()
truth[:, 12:15] += 0.3 * np.random.default_rng(3).standard_normal((len(d_aos), 3)).astype(np.float32)


def dense_scene(records, pose):
    m = gs.ResourceManager(); m.setGaussians(records)
    s = gs.Scene(m, aspect_ratio=dw / dh)
    c = s.getCamera(); c.setPosition(pose["pos"]); c.setRotation(pose["yaw"], pose["pitch"]); c.recalculate()
    return s


cameras, targets = [], []
for pose in POSES:
    s = dense_scene(truth, pose)
    rt = gs.Renderer(dw, dh, record_timings=False, warmup_frames=0)
    rt.init(s.getResourceManager()); rt.initForScene(s); rt.setOutputs(rgba32f=True)
    rt.draw(s)
    targets.append(torch.tensor(np.ascontiguousarray(rt.readOutput(gs.GS_OUTPUT_RGBA32F)[..., :3]), device=dev))
    rt.cleanup()
    cameras.append(gs.Renderer._camera_args(s.getCamera())[:3])
s0 = dense_scene(d_aos, POSES[0])
rd = gs.Renderer(dw, dh, record_timings=False, warmup_frames=0)
rd.init(s0.getResourceManager()); rd.initForScene(s0); rd.setOutputs(rgba32f=True)
records = torch.tensor(d_aos, device=dev)
torch.cuda.synchronize()
opt = VisibleAdam(records, renderer=rd)
numbers = [opt.step_batch(cameras, targets, 0) for _ in range(STEPS)]
opt.stream.synchronize()
losses = [[round(float(x), 6) for x in t.cpu().numpy()[:, 0]] for t in numbers]
rd.setStream(None)
rd.cleanup()
train = {"scene": "dense (6000 splats, 160 x 96)", "views": 2, "steps": STEPS, "target": "frames of the cloud with its SH constant term moved by noise of 0.3",
         "loss_per_step_per_view": losses, "mean_loss_first_step": round(float(np.mean(losses[0])), 6),
         "mean_loss_last_step": round(float(np.mean(losses[-1])), 6)}
print(json.dumps(train), flush=True)

costlib.write_lines(
    a.out, ("# tools/batch_cost.py on one MI355X: gs_rows_accumulate_device for each of two views and one gs_rows_collect_device against the\n"
            "# torch route (zero a dense [N, 84] gradient and the touched flags, index_add_ per view, nonzero + index_select), and gs_membench's\n"
            "# device-to-device copy rate (1 GiB buffers) on the same device in the same run.  Config C under its own camera and a nearby\n"
            "# pose, the rows of one gs_backward_visible_device per view; HIP events around every call on one stream, the routes\n"
            "# alternating, means (and min, max) over `iters` repetitions after `warmup`.  Bytes: what each call has to move, from this\n"
            "# run's counts (the tool's docstring has the formulas); rates = those bytes over the GPU time; *_over_copy = that rate over the\n"
            "# better of the two copy rates.  GPU times: the host wait inside nonzero is not in them.  Recorded numbers, not a bound.\n"),
    [line, "# Observation only: the per-view losses of 20 VisibleAdam.step_batch steps (default rates, weights 1/2) on the dense test scene.", train])
