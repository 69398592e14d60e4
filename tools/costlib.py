"""What the tools/*_cost.py scripts share: how a config's scene is set up, how a call is timed, how a rocprofv3 child run is
started and its CSV read, how a profile file is written.  Helpers, not a framework: a tool keeps its own arguments, byte counts,
header text, ratios and asserts, and parses its arguments before it calls anything here that touches the GPU.  Importing this
module imports neither torch nor the package; use_root() is the one place that does, so that a tool's --root can name the
checkout whose package (and library) is measured while the tool and this module come from their own."""
import collections, csv, glob, json, os, re, shutil, subprocess, sys, tempfile, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_package = None


def use_root(root=None, torch=True):
    """(gs, synth) of the checkout at `root` (default: this one).  The first call decides; later calls return the same pair.
    torch is imported here too, first: behind a live HIP context its import takes seconds longer, more under rocprofv3.
    torch=False is for a tool that never touches it."""
    global _package
    if _package is None:
        if torch:
            import torch
        sys.path.insert(0, os.path.abspath(root or ROOT))
        import vk3dgaussiansplatting_amd as gs
        from vk3dgaussiansplatting_amd import synth
        _package = (gs, synth)
    return _package


def add_cache_argument(ap):
    ap.add_argument("--cache", default=None, metavar="DIR", help="keep the generated clouds here (e.g. a tmpfs) between the processes of a visit")


def cloud(name, cache=None):
    """(aos, cfg) of a config: contiguous float32 records, generated, or loaded from / saved to `cache`."""
    gs, synth = use_root()
    path = os.path.join(cache, f"cost_cloud_{name}.npy") if cache else None
    if path and os.path.exists(path):
        return np.load(path), dict(synth.CONFIGS[name])
    aos, cfg = synth.generate_config(name)
    aos = np.ascontiguousarray(aos, dtype=np.float32)
    if path:
        os.makedirs(cache, exist_ok=True)
        np.save(path, aos)
    return aos, cfg


ConfigScene = collections.namedtuple("ConfigScene", "aos n w h rm sc r")


def config_scene(name, *, record_timings, cache=None):
    """A config under its own camera (the origin, yaw and pitch 0) and a renderer initialised for it."""
    gs, _ = use_root()
    aos, cfg = cloud(name, cache)
    w, h = cfg["width"], cfg["height"]
    rm = gs.ResourceManager(); rm.setGaussians(aos)
    sc = gs.Scene(rm, aspect_ratio=w / h)
    cam = sc.getCamera(); cam.setPosition((0, 0, 0)); cam.setRotation(0.0, 0.0); cam.recalculate()
    r = gs.Renderer(w, h, record_timings=record_timings, warmup_frames=0)
    r.init(rm); r.initForScene(sc)
    return ConfigScene(aos, len(aos), w, h, rm, sc, r)


def image_grads(h, w, depth=False):
    """The random dL/d(image) every tool feeds, [h, w, 4] on the device; with depth, (that, dL/d(depth) [h, w]) from the same generator."""
    import torch
    rng = np.random.default_rng(0)
    gr = torch.tensor(rng.standard_normal((h, w, 4)).astype(np.float32), device="cuda")
    return (gr, torch.tensor(rng.standard_normal((h, w)).astype(np.float32), device="cuda")) if depth else gr


def visible_list(r, sc, grad=None):
    """Draws the scene; -> (|V|, ids, rows, count) with device buffers of max(|V|, 1) rows.  With `grad` (an image gradient),
    gs_backward_visible_device fills them once and the count that came back is checked."""
    import torch
    r.drawDevice(sc, None, sync=True)
    v = r.visibleCount()
    ids = torch.zeros(max(v, 1), dtype=torch.int32, device="cuda")
    rows = torch.zeros(max(v, 1), 84, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if grad is not None:
        r.backwardVisibleDevice(grad.data_ptr(), None, ids.data_ptr(), rows.data_ptr(), v, count.data_ptr())
        r.synchronize()
        assert int(count.item()) == v and bool(torch.isfinite(rows).all())
    return v, ids, rows, count


def event_ms(stream, calls, before=None):
    """The calls back to back on the stream, an event before each and one behind the last: milliseconds per call.  `before` runs
    first, outside the events."""
    import torch
    if before is not None:
        before()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
    for e, call in zip(ev, calls):
        e.record(stream)
        call()
    ev[-1].record(stream)
    ev[-1].synchronize()
    return [ev[k].elapsed_time(ev[k + 1]) for k in range(len(calls))]


def host_ms(r, call):
    """Host clock around the call and gs_synchronize: milliseconds."""
    t0 = time.perf_counter()
    call()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(samples):
    return round(float(np.median(samples)), 4)


def summary(samples):
    """(mean, median, [min, max]), rounded to four places."""
    return round(float(np.mean(samples)), 4), median(samples), [round(float(np.min(samples)), 4), round(float(np.max(samples)), 4)]


def write_lines(path, header, lines):
    """The header as it is, then one line each: a str as it is, anything else as JSON."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(header)
        for line in lines:
            f.write((line if isinstance(line, str) else json.dumps(line)) + "\n")


# ---- a child process under rocprofv3 and what it leaves

def kernel_name(raw):
    """"void gs::k_splat_offsets<gs::BwdSource<true> >(gs::BwdSource<true>, ...)" -> "k_splat_offsets<gs::BwdSource<true>>": the
    template arguments stay, they tell the instantiations apart.  The cut is at the first "(" outside the template arguments: a
    type of an unnamed namespace is spelt gs::(anonymous namespace)::PruneSource there."""
    name, depth = re.sub(r"^(void )?(gs::)?", "", raw), 0
    for i, c in enumerate(name):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            return name[:i].replace(" ", "")
    return name.replace(" ", "")


KernelStat = collections.namedtuple("KernelStat", "average_us calls min_us max_us")


def _csv_files(d, suffix):
    return glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True)          # rocprofv3 nests its output under host and pid


def _csv_rows(d, suffix):
    files = _csv_files(d, suffix)
    if not files:
        raise SystemExit(f"no *{suffix} under {d}")
    with open(files[0], newline="") as f:
        return list(csv.DictReader(f))


def read_kernel_stats(d):
    """{name: KernelStat} of the *kernel_stats.csv under d; kernels that share a normalised name are taken as one (times added)."""
    stats = {}
    for row in _csv_rows(d, "kernel_stats.csv"):
        k, new = kernel_name(row["Name"]), [float(row["AverageNs"]) / 1e3, int(row["Calls"]), float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3]
        stats[k] = KernelStat(*(x + y for x, y in zip(stats.get(k, (0, 0, 0, 0)), new)))
    return stats


def read_kernel_trace(d):
    """[(name, ms)] of the *kernel_trace.csv under d, in start order."""
    rows = sorted(_csv_rows(d, "kernel_trace.csv"), key=lambda row: int(row["Start_Timestamp"]))
    return [(kernel_name(row["Kernel_Name"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6) for row in rows]


def find_kernels(stats, key, who):
    """The names in stats that equal `key` (a str) or hold every word of it (a tuple); none is an error, not a zero."""
    hits = [k for k in stats if (k == key if isinstance(key, str) else all(word in k for word in key))]
    if not hits:
        raise SystemExit(f"{who}: no kernel {key!r} in the trace; it has {sorted(stats)}")
    return hits


def kernel_us(stats, key, who):
    """Mean launch in microseconds, added over the kernels find_kernels() gives."""
    return sum(stats[k].average_us for k in find_kernels(stats, key, who))


def traced_child(argv, limit_s, who, stats=True, cache=None):
    """Runs `python argv...` in a fresh process under rocprofv3 --kernel-trace within limit_s seconds; -> read_kernel_stats of what it
    left (stats=False: read_kernel_trace).  A child that fails or leaves no CSV stops the tool."""
    d = tempfile.mkdtemp(prefix="costlib_")
    try:
        rc = subprocess.run(["timeout", "-k", "10", str(limit_s), "rocprofv3", "--kernel-trace", *(["--stats"] if stats else []),
                             "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable, *argv, *(["--cache", cache] if cache else [])],
                            capture_output=True, text=True)
        suffix = "kernel_stats.csv" if stats else "kernel_trace.csv"
        if rc.returncode != 0 or not _csv_files(d, suffix):
            raise SystemExit(f"{who}: the traced child failed (exit {rc.returncode}, {len(_csv_files(d, suffix))} *{suffix})\n{rc.stderr[-2000:]}")
        return read_kernel_stats(d) if stats else read_kernel_trace(d)
    finally:
        shutil.rmtree(d, ignore_errors=True)


# ---- sh_degree_cost.py and antialias_cost.py: a frame + visible backward per variant (an SH mode, the anti-alias flag)

FRAME_KEYS = ("init_sort_list_ms", "total_ms", "backward_visible_ms")


def variant_setup(name, set_variant, variant, cache):
    """Scene, gradient and visible list; the first frame (which sizes the list) is drawn with `variant`, so that a traced child
    launches the kernels of its own variant alone."""
    s = config_scene(name, record_timings=1, cache=cache)
    set_variant(s.r, s.sc, variant)
    return s, image_grads(s.h, s.w), visible_list(s.r, s.sc)


def variant_frame(s, gr, vis, set_variant, variant):
    """-> (init_sort_list_ms, total_ms, visible backward ms on the host clock)"""
    v, ids, rows, count = vis
    set_variant(s.r, s.sc, variant)
    s.r.drawDevice(s.sc, None, sync=True)
    t = s.r.timings()
    return t.init_sort_list_ms, t.total_ms, host_ms(s.r, lambda: s.r.backwardVisibleDevice(gr.data_ptr(), None, ids.data_ptr(), rows.data_ptr(), v, count.data_ptr()))


def variant_child(configs, set_variant, variant, iters, cache):
    """What a traced child runs: `iters` frames + backwards of one variant per config."""
    for name in configs:
        s, gr, vis = variant_setup(name, set_variant, variant, cache)
        for _ in range(iters):
            variant_frame(s, gr, vis, set_variant, variant)
        s.r.cleanup()


def variant_rounds(name, set_variant, variants, iters, repeats, cache):
    """The variants alternating frame by frame, `repeats` times 3 warm-up + `iters` rounds.
    -> ({variant: {key of FRAME_KEYS: [one median per repeat]}}, scene, sort elements, |V|)"""
    s, gr, vis = variant_setup(name, set_variant, variants[0], cache)
    medians = {x: {key: [] for key in FRAME_KEYS} for x in variants}
    for _ in range(repeats):
        seen = {x: [] for x in variants}
        for it in range(3 + iters):
            for x in variants:
                got = variant_frame(s, gr, vis, set_variant, x)
                if it >= 3:
                    seen[x].append(got)
        for x in variants:
            for key, samples in zip(FRAME_KEYS, zip(*seen[x])):
                medians[x][key].append(median(samples))
    assert int(vis[3].item()) == vis[0]
    elems = int(s.r.timings().num_sort_elements)
    s.r.cleanup()
    return medians, s, elems, vis[0]


def variant_trace(argv, who, cache):
    """Mean launch (us) of k_project (whichever one instantiation ran) and k_bwd_rowsum_chain<true> in a traced child."""
    stats = traced_child(argv, 300, who, cache=cache)
    proj = find_kernels(stats, ("k_project<",), who)
    if len(proj) != 1:
        raise SystemExit(f"{who}: expected one k_project instantiation, the trace has {proj}")
    return {"k_project": proj[0], "k_project_us": round(stats[proj[0]].average_us, 2),
            "k_bwd_rowsum_chain_true_us": round(kernel_us(stats, "k_bwd_rowsum_chain<true>", who), 2)}
