"""What the optional outputs of gs_set_outputs cost: the RenderGaussians bucket (gs_get_timings().render_ms, hipEvents,
record_timings = 1) and the InitSortList bucket (k_project stores the view depths with GS_OUTPUT_DEPTH) with mask 0 / 1 / 2
/ 3, median of --frames synchronous frames after 5 warm-up frames, the masks taken in turn over --rounds rounds (so that
clock drift spreads over all of them).  One JSON line per (config, mask).

    python tools/outputs_cost.py [C Chard ...] [--frames 25] [--rounds 3]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("configs", nargs="*", default=["C", "Chard"])
ap.add_argument("--frames", type=int, default=25)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
MASKS = (0, gs.GS_OUTPUT_RGBA32F, gs.GS_OUTPUT_DEPTH, gs.GS_OUTPUT_RGBA32F | gs.GS_OUTPUT_DEPTH)
for name in a.configs:
    aos, cfg = synth.generate_config(name)
    w, h = cfg["width"], cfg["height"]
    rm = gs.ResourceManager(); rm.setGaussians(aos)
    sc = gs.Scene(rm, aspect_ratio=w / h)
    cam = sc.getCamera(); cam.setPosition((0, 0, 0)); cam.setRotation(0.0, 0.0); cam.recalculate()
    r = gs.Renderer(w, h, record_timings=1, warmup_frames=0)
    r.init(rm); r.initForScene(sc)
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
                          "render_ms_median": round(med, 4), "render_vs_mask0": round(med / base - 1.0, 4),
                          "init_sort_list_ms_median": round(float(np.median(init[m])), 4)}), flush=True)
    r.cleanup()
