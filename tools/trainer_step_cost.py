"""What the host pays to enqueue a training step: VisibleAdam.step and VisibleAdam.step_batch with two views on the dense test scene
(6000 splats at 160 x 96, the scene and the two poses of tools/batch_cost.py), where the GPU work is short enough for the host to
show.  Per method, after --warmup steps: the median host time of a call over --steps calls with no wait in between, and the wall
time of those calls up to one final stream.synchronize(), per call.  One JSON line; the package comes from PYTHONPATH when it is
set there (that is how two commits are compared on one built library, with GS_LIB_OVERRIDE naming it).

    python tools/trainer_step_cost.py [--steps 200] [--warmup 20]
    python tools/trainer_step_cost.py --verdict runs.jsonl      # the lines of parent (P) and this tree (T) runs -> the bounds

--verdict: P = the lines whose package is not this tree's.  Per number, no T run may lie above P's slowest run by more than P's own
max - min."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)                        # behind PYTHONPATH
sys.path.append(os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--verdict")
a = ap.parse_args()

if a.verdict:
    runs = [json.loads(ln) for ln in open(a.verdict)]
    own = lambda run: run["package"] == "vk3dgaussiansplatting_amd"
    for run in runs:
        print("T" if own(run) else "P", json.dumps(run))
    over = []
    for key in ("step_host_us_median", "step_wall_us", "step_batch2_host_us_median", "step_batch2_wall_us"):
        p, t = [run[key] for run in runs if not own(run)], [run[key] for run in runs if own(run)]
        bound = max(p) + (max(p) - min(p))
        over += [key] * (max(t) > bound)
        print(f"{key}: P min {min(p)} max {max(p)} -> bound {bound:.2f}; T {t} -> {'OVER' if max(t) > bound else 'within'}")
    print("verdict:", "over in " + ", ".join(over) if over else "every T run within the bound, for all four numbers")
    sys.exit(0)

import numpy as np
import torch
import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd.autograd import VisibleAdam, make_renderer
from test_outputs_cpu import SCENES

POSES = (dict(pos=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0), dict(pos=(0.2, 0.1, -0.5), yaw=0.1, pitch=-0.05))
aos, w, h = SCENES["dense"]()
aos = np.ascontiguousarray(aos, dtype=np.float32)
cameras = []
for pose in POSES:
    cam = gs.Camera(w / h)
    cam.setPosition(pose["pos"]); cam.setRotation(pose["yaw"], pose["pitch"]); cam.recalculate()
    cameras.append(gs.Renderer._camera_args(cam)[:3])
rng = np.random.default_rng(3)
targets = [torch.tensor(rng.random((h, w, 3), dtype=np.float32), device="cuda:0") for _ in POSES]


def measure(call):
    """(median host microseconds of a call, wall microseconds per call up to the final synchronize) of `call` on a fresh optimiser."""
    r = make_renderer(w, h)
    opt = VisibleAdam(torch.tensor(aos, device="cuda:0"), renderer=r)
    for _ in range(a.warmup):
        call(opt)
    opt.stream.synchronize()
    host = []
    begin = time.perf_counter()
    for _ in range(a.steps):
        t0 = time.perf_counter()
        call(opt)
        host.append(time.perf_counter() - t0)
    opt.stream.synchronize()
    wall = time.perf_counter() - begin
    r.setStream(None)
    r.cleanup()
    return round(statistics.median(host) * 1e6, 2), round(wall / a.steps * 1e6, 2)


step = measure(lambda opt: opt.step(*cameras[0], 0, targets[0]))
batch = measure(lambda opt: opt.step_batch(cameras, targets, 0))
print(json.dumps({"package": os.path.relpath(os.path.dirname(os.path.abspath(gs.__file__)), ROOT), "steps": a.steps, "warmup": a.warmup,
                  "step_host_us_median": step[0], "step_wall_us": step[1],
                  "step_batch2_host_us_median": batch[0], "step_batch2_wall_us": batch[1]}), flush=True)
