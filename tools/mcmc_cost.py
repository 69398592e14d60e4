"""What the MCMC calls cost on the GPU (include/gsplat.h): gs_relocate_device with 1 %, 10 % and 50 % of the splats dead,
gs_grow_device by 5 %, gs_position_noise_device on every row, each beside gs_densify_device on the same cloud (zero
statistics: every row kept, a plain copy of records, m and v -- the call of the parent commit that moves the same arrays)
and beside gs_membench's device-to-device copy rate in the same run.  Config C's cloud in raw space with moments, no scene
and no resolution.  Relocation runs in place, so every repetition starts from a fresh copy of the cloud (the copy is outside
the events).  Everything runs on one torch stream handed to gs_set_stream; every repetition is bracketed by HIP events, and
the means are over --iters repetitions after --warmup.

    python tools/mcmc_cost.py [--config C] [--iters 10] [--warmup 2] [--out profiles/mcmc_cost.txt] [--cache DIR]"""
import argparse, ctypes as C, json, os
import costlib
from costlib import ROOT

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcmc_cost.txt"))
costlib.add_cache_argument(ap)
a = ap.parse_args()

gs, _ = costlib.use_root()
import numpy as np
import torch
from vk3dgaussiansplatting_amd import _lib

aos, _ = costlib.cloud(a.config, a.cache)
n = len(aos)
r = gs.Renderer(64, 64, record_timings=False, warmup_frames=0)
r.init(gs.ResourceManager())

dev = torch.device("cuda:0")
MIN_OPACITY, SEED, ROW = 0.005, 12345, 336
records0 = torch.tensor(aos, device=dev)
del aos
raw0 = torch.empty_like(records0)
m, v = torch.rand_like(records0), torch.rand_like(records0)
records, raw = torch.empty_like(records0), torch.empty_like(records0)
ids = torch.zeros(n, dtype=torch.int32, device=dev)
counts = torch.zeros(4, dtype=torch.int32, device=dev)
stream = torch.cuda.Stream(device=dev)
torch.cuda.synchronize()
r.rawFromRecordsDevice(records0.data_ptr(), raw0.data_ptr(), n)
r.recordsFromRawDevice(raw0.data_ptr(), records0.data_ptr(), n)
r.synchronize()
alive0 = int((records0[:, 15] > MIN_OPACITY).sum())
r.setStream(stream.cuda_stream)


def timed(call, before=None):
    mean, _, spread = costlib.summary([costlib.event_ms(stream, [call], before)[0] for _ in range(a.warmup + a.iters)][a.warmup:])
    return {"ms_mean": mean, "ms_min_max": spread}


line = {"config": a.config, "gaussians": n, "alive_in_the_config": alive0, "iters": a.iters, "warmup": a.warmup, "relocate": []}
with torch.cuda.stream(stream):
    rng = torch.Generator(device=dev)
    rng.manual_seed(1)
    for dead_fraction in (0.01, 0.10, 0.50):
        kill = torch.rand(n, device=dev, generator=rng) < dead_fraction
        work_rec, work_raw = records0.clone(), raw0.clone()
        work_rec[kill, 15] = 3.4e-4
        work_raw[kill, 15] = -8.0

        def fresh():
            records.copy_(work_rec)
            raw.copy_(work_raw)

        res = timed(lambda: r.relocateDevice(records.data_ptr(), raw.data_ptr(), m.data_ptr(), v.data_ptr(), n, MIN_OPACITY, SEED,
                                             ids.data_ptr(), n, counts.data_ptr()), before=fresh)
        stream.synchronize()
        changed, dead, sources = (int(x) for x in counts.cpu().numpy().view(np.uint32)[:3])
        # a source: its record and raw rows read, 16 bytes of each written, two moment rows zeroed; a dead splat: two rows read, four
        # written; every splat: its opacity twice, 16 bytes of scratch written and read, 4 of ids
        moved = sources * (2 * ROW + 32 + 2 * ROW) + dead * 6 * ROW + n * (8 + 32 + 4)
        res.update(dead_fraction=dead_fraction, changed=changed, dead=dead, sources=sources, bytes=moved,
                   achieved_tbytes_per_s=round(moved / (res["ms_mean"] * 1e-3) / 1e12, 3))
        line["relocate"].append(res)
        del work_rec, work_raw, kill
    # growth by 5 %: every array travels
    n_add = int(1.05 * n) - n
    out = [torch.empty(n + n_add, 84, device=dev) for _ in range(4)]
    res = timed(lambda: r.growDevice(records0.data_ptr(), raw0.data_ptr(), m.data_ptr(), v.data_ptr(), n, MIN_OPACITY, SEED, n_add,
                                     out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), n + n_add,
                                     counts.data_ptr()))
    stream.synchronize()
    outputs, sources = (int(x) for x in counts.cpu().numpy().view(np.uint32)[:2])
    moved = 4 * ROW * (n + outputs)
    res.update(n_add=n_add, outputs=outputs, sources=sources, bytes=moved, achieved_tbytes_per_s=round(moved / (res["ms_mean"] * 1e-3) / 1e12, 3))
    line["grow"] = res
    # noise on every row: position, scale, rotation and opacity read, the position written twice
    records.copy_(records0)
    raw.copy_(raw0)
    res = timed(lambda: r.positionNoiseDevice(records.data_ptr(), raw.data_ptr(), n, None, None, 0, 1e-3, 100.0, 0.995, SEED))
    moved = n * (12 + 12 + 16 + 4 + 24)
    res.update(bytes=moved, achieved_tbytes_per_s=round(moved / (res["ms_mean"] * 1e-3) / 1e12, 3))
    line["position_noise_all_rows"] = res
    # gs_densify_device on the same cloud, zero statistics: every row kept, records, m and v copied
    accum, seen, radius = torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, device=dev)
    p = gs.default_densify_params(prune_opacity=0.0)
    res = timed(lambda: r.densifyDevice(records0.data_ptr(), m.data_ptr(), v.data_ptr(), n, accum.data_ptr(), seen.data_ptr(),
                                        radius.data_ptr(), p, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), n + n_add,
                                        counts.data_ptr()))
    stream.synchronize()
    kept = int(counts.cpu().numpy().view(np.uint32)[0])
    moved = 3 * ROW * (n + kept) + 12 * n
    res.update(outputs=kept, bytes=moved, achieved_tbytes_per_s=round(moved / (res["ms_mean"] * 1e-3) / 1e12, 3))
    line["densify_all_kept"] = res
torch.cuda.synchronize()
r.setStream(None)

# the copy rate of the same device in the same run: 1 GiB buffers, 16-byte accesses, plain and with four loads in flight
L, hctx = _lib.lib(), r._ctx.handle
copy = {}
for kind, name in ((1, "copy16"), (10, "copy16_x4")):
    g_, ms_ = C.c_float(), C.c_float()
    assert L.gs_membench(hctx, kind, 1 << 30, 0, 20, C.byref(g_), C.byref(ms_)) == 0
    copy[name] = round(g_.value / 1e3, 3)
line["membench_copy_tbytes_per_s"] = copy
r.cleanup()

print(json.dumps(line), flush=True)
costlib.write_lines(
    a.out, ("# tools/mcmc_cost.py on one MI355X: gs_relocate_device (raw space, with moments, ids listed) with 1 %, 10 % and 50 % of\n"
            "# config C's splats dead, gs_grow_device by 5 % (records, raw, m, v), gs_position_noise_device on every row,\n"
            "# gs_densify_device on the same cloud with every row kept (records, m, v) and gs_membench's copy rate, in one run; HIP events\n"
            "# around every call on one stream, means (and min, max) over `iters` repetitions after `warmup`.  bytes: the rows read and\n"
            "# written as the tool's text counts them.  Recorded numbers, not a bound.\n"), [line])
