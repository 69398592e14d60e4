"""What the optional outputs of gs_set_outputs cost: the RenderGaussians bucket (gs_get_timings().render_ms, hipEvents,
record_timings = 1) and the InitSortList bucket (k_project stores the view depths with GS_OUTPUT_DEPTH) with mask 0 / 1 / 2
/ 3, median of --frames synchronous frames after 5 warm-up frames, the masks taken in turn over --rounds rounds (so that
clock drift spreads over all of them).  One JSON line per (config, mask).

    python tools/outputs_cost.py [C Chard ...] [--frames 25] [--rounds 3] [--cache DIR]"""
import argparse, json
import costlib

ap = argparse.ArgumentParser()
ap.add_argument("configs", nargs="*", default=["C", "Chard"])
ap.add_argument("--frames", type=int, default=25)
ap.add_argument("--rounds", type=int, default=3)
costlib.add_cache_argument(ap)
a = ap.parse_args()

gs, _ = costlib.use_root(torch=False)
import numpy as np

MASKS = (0, gs.GS_OUTPUT_RGBA32F, gs.GS_OUTPUT_DEPTH, gs.GS_OUTPUT_RGBA32F | gs.GS_OUTPUT_DEPTH)
for name in a.configs:
    aos, n, w, h, rm, sc, r = costlib.config_scene(name, record_timings=1, cache=a.cache)
    render = {m: [] for m in MASKS}
    init = {m: [] for m in MASKS}
    frame = None
    for _ in range(a.rounds):
        for m in MASKS:
            r.setOutputs(rgba32f=bool(m & gs.GS_OUTPUT_RGBA32F), depth=bool(m & gs.GS_OUTPUT_DEPTH))
            for _ in range(5):
                r.drawDevice(sc, None, sync=True)
            for _ in range(a.frames):
                r.drawDevice(sc, None, sync=True)
                t = r.timings()
                render[m].append(t.render_ms)
                init[m].append(t.init_sort_list_ms)
            img = r.debugRead(gs.BUF_IMAGE)
            frame = img if frame is None else frame
            assert np.array_equal(img, frame), "the RGBA8 frame must not depend on the mask"
    base = float(np.median(render[0]))
    for m in MASKS:
        med = float(np.median(render[m]))
        print(json.dumps({"config": name, "width": w, "height": h, "mask": m, "frames": len(render[m]),
                          "render_ms_median": costlib.median(render[m]), "render_vs_mask0": round(med / base - 1.0, 4),
                          "init_sort_list_ms_median": costlib.median(init[m])}), flush=True)
    r.cleanup()
