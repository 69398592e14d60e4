"""What the photometric loss (gs_photometric_loss_device, include/gsplat.h: loss + gradient, three kernels) costs on the GPU
at 1920 x 1080 and 3840 x 2160, from HIP events on the stream the library is given (gs_set_stream): blocks of --reps calls
between two events, --iters blocks after 3 warm-up blocks, the median per call.  In the same window, alternating block by
block so that both see the same neighbours, the same loss written with torch conv2d (11 x 11 window, groups = 3, padding = 5)
+ autograd on the same GPU.  Then the context's dense backward at config C (gs_backward_device + gs_synchronize, host-timed
like tools/backward_cost.py, profiles/backward_cost.txt) as the yardstick of a training step, the kernels' own times from a
child run under `rocprofv3 --kernel-trace --stats`, and the accuracy figures of tests/test_loss_gpu.py: the kernels' and
float32 torch's worst error against the float64 reference over the test's shapes, kinds, lambdas and backgrounds.

    python tools/loss_cost.py [--iters 20] [--reps 50] [--out profiles/loss_cost.txt] [--no-backward] [--cache DIR]"""
import argparse, json, os, shutil, sys
import costlib
from costlib import ROOT
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_cost.txt"))
ap.add_argument("--no-backward", action="store_true", help="skip the config C backward (40 s of cloud generation)")
ap.add_argument("--child", nargs=2, type=int, metavar=("W", "H"), help="run the loss at W x H only (under rocprofv3)")
costlib.add_cache_argument(ap)
a = ap.parse_args()

gs, _ = costlib.use_root()
import numpy as np
import torch
import torch.nn.functional as F

SIZES = ((1920, 1080), (3840, 2160))
LAM, BG = 0.2, (0.2, 0.5, 0.9)
# HBM bytes per pixel the kernels need: forward reads rgba 16 + target 12 and writes three maps 36; backward reads the maps 36,
# rgba 16, target 12 and writes the gradient 16 (halo texels come from the caches)
BYTES_PER_PIXEL = 16 + 12 + 36 + 36 + 16 + 12 + 16


def context(w, h, stream):
    aos = gs.makeGaussian((0.0, 0.0, 2.0), (0.1, 0.1, 0.1), sh0=(0.5, 0.5, 0.5, 0.8))[None].astype(np.float32)
    rm = gs.ResourceManager(); rm.setGaussians(aos)
    r = gs.Renderer(w, h, record_timings=False, warmup_frames=0)
    r.init(rm); r.initForScene(gs.Scene(rm, aspect_ratio=w / h))
    r.setStream(stream.cuda_stream)
    return r


def images(w, h):
    rng = np.random.default_rng(0)
    target = torch.tensor(rng.uniform(0, 1, (h, w, 3)).astype(np.float32), device="cuda")
    rgba = torch.tensor(rng.uniform(0, 1, (h, w, 4)).astype(np.float32), device="cuda")
    return rgba, target


def torch_loss_and_grad(rgba, target, window, bg):
    x = rgba.detach().requires_grad_(True)
    img = (x[..., :3] + (1.0 - x[..., 3:4]) * bg).permute(2, 0, 1)[None]
    g = target.permute(2, 0, 1)[None]
    conv = lambda t: F.conv2d(t, window, padding=5, groups=3)
    mu1, mu2 = conv(img), conv(g)
    s1, s2, s12 = conv(img * img) - mu1 * mu1, conv(g * g) - mu2 * mu2, conv(img * g) - mu1 * mu2
    ssim = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s1 + s2 + 9e-4))
    loss = (1.0 - LAM) * (img - g).abs().mean() + LAM * (1.0 - ssim.mean())
    loss.backward()
    return loss.detach(), x.grad


def block_ms(stream, reps, call):
    return costlib.event_ms(stream, [lambda: [call() for _ in range(reps)]])[0] / reps


def measure(w, h, iters, reps):
    from test_loss_cpu import window as window64
    stream = torch.cuda.Stream()
    r = context(w, h, stream)
    rgba, target = images(w, h)
    numbers, grad = torch.zeros(3, device="cuda"), torch.zeros(h, w, 4, device="cuda")
    w1 = torch.tensor(window64(), dtype=torch.float32, device="cuda")
    win = (w1[:, None] * w1[None, :]).reshape(1, 1, 11, 11).repeat(3, 1, 1, 1)
    bg = torch.tensor(BG, device="cuda")
    torch.cuda.synchronize()
    ours = lambda: r.photometricLossDevice(rgba.data_ptr(), target.data_ptr(), LAM, BG, numbers.data_ptr(), grad.data_ptr())
    ours_loss_only = lambda: r.photometricLossDevice(rgba.data_ptr(), target.data_ptr(), LAM, BG, numbers.data_ptr(), None)
    with torch.cuda.stream(stream):
        theirs = lambda: torch_loss_and_grad(rgba, target, win, bg)
        t_loss, t_grad = theirs()
        ours()
        stream.synchronize()
        agree = {"loss_rel_diff": abs(float(numbers[0]) - float(t_loss)) / abs(float(t_loss)),
                 "grad_max_diff_over_scale": float((grad - t_grad).abs().max() / t_grad.abs().max())}
        if a.child:
            for _ in range(iters):
                ours()
            stream.synchronize()
            r.cleanup()
            return None
        for _ in range(3):
            block_ms(stream, reps, ours); block_ms(stream, reps, ours_loss_only); block_ms(stream, max(reps // 10, 1), theirs)
        t_ours, t_only, t_torch = [], [], []
        for _ in range(iters):
            t_ours.append(block_ms(stream, reps, ours))
            t_only.append(block_ms(stream, reps, ours_loss_only))
            t_torch.append(block_ms(stream, max(reps // 10, 1), theirs))
    r.cleanup()
    med = lambda v: float(np.median(v))
    ms = med(t_ours)
    return {"width": w, "height": h, "iters": iters, "reps": reps, "loss_and_gradient_ms_median": round(ms, 4),
            "loss_and_gradient_ms_min_max": [round(min(t_ours), 4), round(max(t_ours), 4)],
            "loss_only_ms_median": round(med(t_only), 4), "torch_conv2d_autograd_ms_median": round(med(t_torch), 4),
            "torch_over_ours": round(med(t_torch) / ms, 1), "bytes_per_pixel_needed": BYTES_PER_PIXEL,
            "achieved_gbytes_per_s_over_needed_bytes": round(BYTES_PER_PIXEL * w * h / (ms * 1e-3) / 1e9, 1),
            "agreement_with_torch_float32": agree}


def backward_config_c(iters):
    aos, n, w, h, rm, sc, r = costlib.config_scene("C", record_timings=1, cache=a.cache)
    gr = costlib.image_grads(h, w)
    out = torch.empty(n, 84, device="cuda")
    torch.cuda.synchronize()
    fwd, bwd = [], []
    for k in range(3 + iters):
        r.drawDevice(sc, None, sync=True)
        ms = costlib.host_ms(r, lambda: r.backwardDevice(gr.data_ptr(), None, out.data_ptr()))
        if k >= 3:
            fwd.append(r.timings().total_ms)
            bwd.append(ms)
    r.cleanup()
    return {"config": "C", "width": w, "height": h, "iters": iters, "forward_total_ms_median": costlib.median(fwd),
            "backward_ms_median": costlib.median(bwd)}


def kernel_split(w, h, iters):
    if not shutil.which("rocprofv3"):
        return {}
    stats = costlib.traced_child([os.path.abspath(__file__), "--child", str(w), str(h), "--iters", str(iters)], 300, "loss_cost")
    return {name: {"calls": k.calls, "average_us": round(k.average_us, 2), "min_us": round(k.min_us, 2), "max_us": round(k.max_us, 2)}
            for name, k in stats.items() if name.startswith("k_loss_")}


def accuracy():
    """The worst figures of tests/test_loss_gpu.py::test_by_value, for the kernels and for float32 torch on the CPU."""
    from test_loss_cpu import BGS, LAMBDAS, SEED, SHAPES, TOL, loss_float32, loss_reference, make_inputs
    out = []
    for kind, tol in TOL.items():
        worst = {"kind": kind, "tol": tol, "gpu_gradient_over_plane_scale": 0.0, "gpu_numbers_relative": 0.0,
                 "gpu_dssim_absolute": 0.0, "torch_float32_gradient_over_scale_lambda_0.2_no_bg": 0.0,
                 "torch_float32_loss_relative_lambda_0.2_no_bg": 0.0}
        for w, h in SHAPES:
            stream = torch.cuda.Stream()
            r = context(w, h, stream)
            for lam in LAMBDAS:
                for bg in BGS:
                    rgba, target = make_inputs(kind, w, h, SEED, bg)
                    ref_n, ref_g = loss_reference(rgba, target, lam, bg)
                    n, g = r.photometricLoss(rgba, target, lam, bg)
                    err = np.abs(g.astype(np.float64) - ref_g).reshape(-1, 4).max(0)
                    scale = np.abs(ref_g).reshape(-1, 4).max(0)
                    worst["gpu_gradient_over_plane_scale"] = max(worst["gpu_gradient_over_plane_scale"],
                                                                 float((err / np.where(scale > 0, scale, 1.0)).max()))
                    nerr = np.abs(n.astype(np.float64) - ref_n)
                    rel = nerr / np.abs(ref_n)
                    small = ref_n[2] < 1e-3
                    worst["gpu_numbers_relative"] = max(worst["gpu_numbers_relative"], float(rel[1]),
                                                        float(rel[0]) if not (small and lam == 1.0) else 0.0,
                                                        float(rel[2]) if not small else 0.0)
                    worst["gpu_dssim_absolute"] = max(worst["gpu_dssim_absolute"], float(nerr[2]))
                    if lam == 0.2 and bg is None:
                        for separable in (True, False):
                            tn, tg = loss_float32(rgba, target, lam, bg, separable)
                            worst["torch_float32_gradient_over_scale_lambda_0.2_no_bg"] = max(
                                worst["torch_float32_gradient_over_scale_lambda_0.2_no_bg"],
                                float(np.abs(tg - ref_g).max() / np.abs(ref_g).max()))
                            worst["torch_float32_loss_relative_lambda_0.2_no_bg"] = max(
                                worst["torch_float32_loss_relative_lambda_0.2_no_bg"], abs(float(tn[0]) - ref_n[0]) / abs(ref_n[0]))
            r.cleanup()
        out.append({k: (float(f"{v:.3e}") if isinstance(v, float) else v) for k, v in worst.items()})
    return out


if a.child:
    measure(a.child[0], a.child[1], a.iters, a.reps)
    sys.exit(0)

lines = []
for w, h in SIZES:
    lines.append(measure(w, h, a.iters, a.reps))
    print(json.dumps(lines[-1]), flush=True)
for w, h in SIZES:
    lines.append({"width": w, "height": h, "kernels_rocprofv3": kernel_split(w, h, a.iters)})
    print(json.dumps(lines[-1]), flush=True)
if not a.no_backward:
    lines.append(backward_config_c(10))
    lines[-1]["loss_and_gradient_over_backward"] = round(lines[0]["loss_and_gradient_ms_median"] / lines[-1]["backward_ms_median"], 4)
    print(json.dumps(lines[-1]), flush=True)
for row in accuracy():
    lines.append({"accuracy": row})
    print(json.dumps(lines[-1]), flush=True)
costlib.write_lines(
    a.out, ("# tools/loss_cost.py on one MI355X: gs_photometric_loss_device (loss + gradient; loss only) and the same loss by torch conv2d + autograd,\n"
            "# HIP events around blocks of `reps` calls on one stream, alternating, medians of `iters` blocks after 3 warm-up blocks; the kernels' own\n"
            "# times from a rocprofv3 --kernel-trace --stats child per size; the dense backward of config C (host-timed, as\n"
            "# profiles/backward_cost.txt); the accuracy figures of tests/test_loss_gpu.py against the float64 reference.\n"), lines)
