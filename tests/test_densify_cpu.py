"""Adaptive density control (include/gsplat.h, gs_densify_stats_device / gs_densify_device), on the CPU: the NumPy restatement
of the rule and of the counter-based normals, a designed statistics array in which every comparison of the rule decides
alone, and the float64 reference of dL/d(screen position) -- the gradient of forward64's (tests/frame64.py) screen_offset, a
zero tensor added to (sx, sy).  tests/test_densify_gpu.py compares the GPU with them.  Helpers are shared with that file."""
import ctypes as C

import numpy as np
import pytest

from test_outputs_cpu import load_scene, oracle_params
from test_backward_cpu import frozen_of
from frame64 import forward64, frame_decisions, loss_of, raster32, reference_gradient

torch = pytest.importorskip("torch")

F = np.float32
INF = float("inf")
DEFAULTS = dict(grad_threshold=2e-4, split_scale=0.01, prune_opacity=0.005, prune_scale=INF, prune_radius=INF,
                split_shrink=1.6, seed=0)
# the parameters of the designed array: every prune test is on
DESIGN_PARAMS = dict(DEFAULTS, prune_scale=0.5, prune_radius=40.0, seed=0x1234567_89ABCDEF)
FLIPS = ("opacity", "scale", "radius", "threshold", "split", "seen", "nan_max", "pruned_wins")


# ---- the normals ----------------------------------------------------------------------------------------------------------

def mix(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d); x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b); x ^= x >> np.uint32(16)
    return x


def normal_words(seed, g):
    """w(c, a, j) of the header for splats g (uint32 array): uint32 [len(g), 2, 3, 2]."""
    g = np.asarray(g, np.uint32)
    seed = int(seed)
    with np.errstate(over="ignore"):
        h = mix(mix(g ^ np.uint32(seed & 0xFFFFFFFF)) + np.uint32(seed >> 32))
        k = (np.arange(12, dtype=np.uint32) + np.uint32(1)) * np.uint32(0x9E3779B9)      # c * 6 + a * 2 + j + 1
        return mix(h[:, None] + k[None, :]).reshape(-1, 2, 3, 2)


def normals(seed, g):
    """z of (seed, g, child, axis) in float64: [len(g), 2, 3]."""
    w = normal_words(seed, g)
    u1 = ((w[..., 0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[..., 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(np.float64(F(6.2831855)) * u2)


# ---- the rule -------------------------------------------------------------------------------------------------------------

def rot_matrix(q):
    """getRotMat of the record's rot [.., 4] (r, x, y, z), R[.., row, col], in q's dtype."""
    r, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y + 2 * r * z, 2 * x * z - 2 * r * y], -1),
                     np.stack([2 * x * y - 2 * r * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z + 2 * r * x], -1),
                     np.stack([2 * x * z + 2 * r * y, 2 * y * z - 2 * r * x, 1 - 2 * x * x - 2 * y * y], -1)], -2)


def densify_kinds(records, stats, params, flip=None):
    """Per input splat 0 pruned, 1 kept, 2 clone, 3 split: the rule of the header in float32, every comparison as written.
    flip: one of FLIPS, that comparison replaced by its neighbour (for the check that the designed array is decisive)."""
    rec = np.asarray(records, F)
    accum, seen, radius = (np.asarray(stats[k]) for k in ("grad_accum", "seen", "max_radius"))
    p = {k: F(v) for k, v in params.items() if k != "seed"}
    with np.errstate(invalid="ignore", divide="ignore"):
        mx = (lambda a, b: np.fmax(a, b)) if flip == "nan_max" else (lambda a, b: np.where(a > b, a, b))
        smax = mx(mx(rec[:, 4], rec[:, 5]), rec[:, 6])
        op = rec[:, 15]
        pruned = ((op <= p["prune_opacity"]) if flip == "opacity" else (op < p["prune_opacity"])) | \
                 ((smax >= p["prune_scale"]) if flip == "scale" else (smax > p["prune_scale"])) | \
                 ((radius >= p["prune_radius"]) if flip == "radius" else (radius > p["prune_radius"]))
        count = np.maximum(seen, 1) if flip == "seen" else seen
        mean = np.where(count != 0, accum.astype(F) / np.maximum(count, 1).astype(F), F(0)).astype(F)
        grow = (mean > p["grad_threshold"]) if flip == "threshold" else (mean >= p["grad_threshold"])
        if flip != "pruned_wins":
            grow = grow & ~pruned
        split = grow & ((smax >= p["split_scale"]) if flip == "split" else (smax > p["split_scale"]))
    kind = np.where(grow, np.where(split, 3, 2), np.where(pruned, 0, 1))
    return kind.astype(np.int64)


def densify_ref(records, m, v, stats, params, flip=None):
    """gs_densify_device restated: dict(records, m, v: the outputs [n_out, 84] float32; counts (n_out, cloned, split, pruned);
    kind [n]; offset [n] = o(g); child [n_out] = 0 / 1 for the two children of a split, -1 elsewhere; parent [n_out]; pos64
    [n_out, 3] = the float64 positions of the children (nan elsewhere); bound [n_out, 3] = sum_k |R[i][k] s[k]| of theirs).
    Everything but the children's positions is exact float32; those are float64 from the float64 normals."""
    rec = np.ascontiguousarray(records, F)
    n = len(rec)
    kind = densify_kinds(rec, stats, params, flip)
    k = np.array([0, 1, 2, 2])[kind]
    offset = np.concatenate([[0], np.cumsum(k)[:-1]]).astype(np.int64)
    n_out = int(k.sum())
    parent = np.repeat(np.arange(n), k)
    second = np.arange(n_out) - offset[parent]                       # 0 / 1: which output of its parent
    out = rec[parent].copy()
    zero_moments = (kind[parent] == 3) | ((kind[parent] == 2) & (second == 1))
    outs = {"records": out}
    for name, a in (("m", m), ("v", v)):
        if a is not None:
            o = np.ascontiguousarray(a, F)[parent].copy()
            o[zero_moments] = 0
            outs[name] = o
    child = np.where(kind[parent] == 3, second, -1)
    is_child = child >= 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        out[is_child, 4:7] = rec[parent[is_child], 4:7] / F(params["split_shrink"])
        pos64 = np.full((n_out, 3), np.nan)
        bound = np.full((n_out, 3), np.nan)
        if is_child.any():
            g = parent[is_child]
            z = normals(params["seed"], g)[np.arange(len(g)), child[is_child]]              # [children, 3]
            M = rot_matrix(rec[g, 8:12].astype(np.float64)) * rec[g, None, 4:7].astype(np.float64)
            pos64[is_child] = rec[g, 0:3].astype(np.float64) + np.einsum("cik,ck->ci", M, z)
            bound[is_child] = np.abs(M).sum(-1)
            out[is_child, 0:3] = pos64[is_child].astype(F)
    counts = (n_out, int((kind == 2).sum()), int((kind == 3).sum()), int((kind == 0).sum()))
    return dict(outs, counts=counts, kind=kind, offset=offset, child=child, parent=parent, pos64=pos64, bound=bound)


# ---- the designed array ---------------------------------------------------------------------------------------------------

SENTINEL = 0xFFC54321                    # a NaN with a payload in the floats nothing reads: a copy that is not bitwise shows
UNUSED = [3, 7] + list(range(19, 76, 4)) + list(range(76, 84))

# name -> (changes of the base row, expected kind).  Base: scales (0.005, 0.004, 0.003), opacity 0.5, accum 0, seen 1,
# radius 5: kept.  "GROW" stands for an accumulator of 1.0 (mean 1 >= 2e-4).
T, S = F(DESIGN_PARAMS["grad_threshold"]), F(DESIGN_PARAMS["split_scale"])
DESIGN = [
    ("base", {}, 1),
    ("pruned_by_opacity", dict(op=0.004), 0),
    ("pruned_by_scale", dict(s=(0.003, 0.6, 0.002)), 0),
    ("pruned_by_radius", dict(radius=41.0), 0),
    ("mean_equals_threshold", dict(accum=T), 2),
    ("mean_below_threshold", dict(accum=np.nextafter(T, F(0))), 1),
    ("unseen_with_accumulator", dict(accum=1.0, seen=0), 1),
    ("smax_equals_split_scale", dict(accum=1.0, s=(0.002, S, 0.003)), 2),
    ("smax_above_split_scale", dict(accum=1.0, s=(0.002, 0.003, np.nextafter(S, F(1)))), 3),
    ("nan_first_scale", dict(accum=1.0, s=(np.nan, 0.02, 0.003)), 3),          # max(NaN, b) = b: the others decide
    ("nan_last_scale", dict(accum=1.0, s=(0.02, 0.6, np.nan)), 2),             # max(a, NaN) = NaN: neither pruned nor split
    ("nan_accumulator", dict(accum=np.nan), 1),
    ("nan_radius", dict(accum=1.0, radius=np.nan), 2),
    ("pruned_would_grow", dict(accum=1.0, op=0.001, s=(0.02, 0.03, 0.04)), 0),
    ("opacity_equals_bound", dict(op=F(DESIGN_PARAMS["prune_opacity"])), 1),
    ("scale_equals_bound", dict(s=(0.003, F(DESIGN_PARAMS["prune_scale"]), 0.002)), 1),
    ("radius_equals_bound", dict(radius=F(DESIGN_PARAMS["prune_radius"])), 1),
    ("split", dict(accum=5e-3, seen=7, s=(0.05, 0.02, 0.08), rot=(0.3, -0.2, 0.5, 0.8)), 3),
    ("mean_of_three", dict(accum=1e-3, seen=3), 2),                            # 3.3e-4
    ("mean_of_seven", dict(accum=1e-3, seen=7), 1),                            # 1.4e-4
]
D = len(DESIGN)


def designed(n=D, seed=5):
    """(records, m, v [n, 84], stats) with the designed rows tiled over n: everything the rule does not read is random
    (rotations not unit, moments not zero), the unused floats carry SENTINEL."""
    rng = np.random.default_rng(seed)
    rec = rng.uniform(-1.0, 1.0, (n, 84)).astype(F)
    m, v = rng.standard_normal((n, 84)).astype(F), rng.uniform(0.0, 1.0, (n, 84)).astype(F)
    for a in (rec, m, v):
        a.view(np.uint32)[:, UNUSED] = SENTINEL
    accum, seen, radius = np.zeros(n, F), np.ones(n, np.uint32), np.full(n, 5.0, F)
    rec[:, 4:7], rec[:, 15] = (0.005, 0.004, 0.003), 0.5
    for i in range(n):
        ch = DESIGN[i % D][1]
        if "s" in ch:
            rec[i, 4:7] = ch["s"]
        if "rot" in ch:
            rec[i, 8:12] = ch["rot"]
        rec[i, 15] = ch.get("op", 0.5)
        accum[i], seen[i], radius[i] = ch.get("accum", 0.0), ch.get("seen", 1), ch.get("radius", 5.0)
    return rec, m, v, dict(grad_accum=accum, seen=seen, max_radius=radius)


VARIANTS = {
    "designed": DESIGN_PARAMS,
    "all_kept": dict(DEFAULTS, prune_opacity=0.0, grad_threshold=INF, seed=3),
    "all_pruned": dict(DEFAULTS, prune_opacity=INF, seed=3),
    "all_split": dict(DEFAULTS, prune_opacity=0.0, grad_threshold=-INF, split_scale=-INF, seed=3),
}


def variant_inputs(name, n):
    """The designed array of n rows for a variant; all_split has its NaNs replaced (a NaN mean or scale does not split)."""
    rec, m, v, st = designed(n)
    if name == "all_split":
        rec[:, 4:7] = np.nan_to_num(rec[:, 4:7], nan=0.01)
        st["grad_accum"] = np.nan_to_num(st["grad_accum"], nan=1.0)
    return rec, m, v, st


def test_the_designed_array_takes_every_branch():
    rec, m, v, st = designed()
    ref = densify_ref(rec, m, v, st, DESIGN_PARAMS)
    for i, (name, _, want) in enumerate(DESIGN):
        assert ref["kind"][i] == want, (name, ref["kind"][i])
    cloned, split, pruned = (sum(1 for d in DESIGN if d[2] == k) for k in (2, 3, 0))
    assert ref["counts"] == (D + cloned + split - pruned, cloned, split, pruned) and min(cloned, split, pruned) >= 3
    # the outputs: stable order, copies bit for bit, zero moments where the header says so
    b = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.all(np.diff(ref["parent"]) >= 0)
    for o, g in enumerate(ref["parent"]):
        kind, second = ref["kind"][g], o - ref["offset"][g]
        if kind == 3:
            assert np.array_equal(b(ref["records"][o])[7:], b(rec[g])[7:]) and b(ref["records"][o])[3] == b(rec[g])[3]
            assert not ref["m"][o].any() and not ref["v"][o].any()
            assert np.array_equal(ref["records"][o, 4:7], rec[g, 4:7] / F(1.6)) or np.isnan(rec[g, 4:7]).any()
        else:
            assert np.array_equal(b(ref["records"][o]), b(rec[g]))
            if kind == 2 and second == 1:
                assert not b(ref["m"][o]).any() and not b(ref["v"][o]).any()
            else:
                assert np.array_equal(b(ref["m"][o]), b(m[g])) and np.array_equal(b(ref["v"][o]), b(v[g]))
    # the two children of a split differ, and sit within 6 sigma
    for g in np.flatnonzero(ref["kind"] == 3):
        o = ref["offset"][g]
        assert not np.array_equal(ref["pos64"][o], ref["pos64"][o + 1])
        if not np.isnan(ref["bound"][o]).any():
            assert np.all(np.abs(ref["pos64"][o:o + 2] - rec[g, 0:3]) <= 5.77 * ref["bound"][o:o + 2] + 1e-12)
    for name, params in VARIANTS.items():
        r = densify_ref(*variant_inputs(name, D), params)
        want = {"all_kept": (D, 0, 0, 0), "all_pruned": (0, 0, 0, D), "all_split": (2 * D, 0, D, 0)}.get(name)
        assert want is None or r["counts"] == want, (name, r["counts"])


@pytest.mark.parametrize("flip", FLIPS)
def test_the_design_is_decisive(flip):
    """Every comparison of the restatement, replaced by its neighbour (< by <=, > by >=, >= by >, seen ignored, a maximum
    that drops a NaN, growth that ignores the prune), changes the kinds of the designed array -- and only in the row made
    for it."""
    rec, m, v, st = designed()
    a, b = densify_kinds(rec, st, DESIGN_PARAMS), densify_kinds(rec, st, DESIGN_PARAMS, flip)
    changed = [DESIGN[i][0] for i in np.flatnonzero(a != b)]
    want = {"opacity": ["opacity_equals_bound"], "scale": ["scale_equals_bound"], "radius": ["radius_equals_bound"],
            "threshold": ["mean_equals_threshold"], "split": ["smax_equals_split_scale"], "seen": ["unseen_with_accumulator"],
            "nan_max": ["nan_last_scale"], "pruned_wins": ["pruned_would_grow"]}[flip]
    assert changed == want, (flip, changed)
    assert densify_ref(rec, m, v, st, DESIGN_PARAMS, flip)["counts"] != densify_ref(rec, m, v, st, DESIGN_PARAMS)["counts"]


def test_the_normals_are_standard_normal():
    """10^5 draws of the restated normals (50 000 splats, child 0 and child 1, axis 0): |mean| < 4 / sqrt(N),
    |var - 1| < 4 sqrt(2 / N); the children differ, the axes differ, another seed gives other draws, the same seed the same;
    u1 is never 0 (no infinite draw) and |z| <= 5.77."""
    g = np.arange(50_000, dtype=np.uint32)
    z = normals(DESIGN_PARAMS["seed"], g)
    for sample in (z[:, :, 0].ravel(), z[:, 0, :2].ravel(), z[:, 1, 1:].ravel()):
        n = len(sample)
        assert n == 100_000
        assert abs(sample.mean()) < 4 / np.sqrt(n), sample.mean()
        assert abs(sample.var() - 1.0) < 4 * np.sqrt(2 / n), sample.var()
    assert np.all(np.isfinite(z)) and np.abs(z).max() <= 5.77
    assert not np.any(z[:, 0] == z[:, 1]) and not np.any(z[:, :, 0] == z[:, :, 1])
    assert abs(np.corrcoef(z[:, 0, 0], z[:, 1, 0])[0, 1]) < 4 / np.sqrt(len(g))
    assert np.array_equal(z, normals(DESIGN_PARAMS["seed"], g))
    for other in (DESIGN_PARAMS["seed"] ^ 1, DESIGN_PARAMS["seed"] ^ (1 << 32)):        # each half of the seed counts
        assert not np.any(normals(other, g) == z)
    # the integer part against plain Python integers
    for x0 in (0, 1, 0x9E3779B9, 0xFFFFFFFF, 123456789):
        x = x0
        x ^= x >> 16; x = x * 0x7feb352d & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846ca68b & 0xFFFFFFFF; x ^= x >> 16
        assert int(mix(np.array([x0], np.uint32))[0]) == x
    seed, g0 = DESIGN_PARAMS["seed"], 4321
    h = int(mix(np.array([(int(mix(np.array([g0 ^ (seed & 0xFFFFFFFF)], np.uint32))[0]) + (seed >> 32)) & 0xFFFFFFFF], np.uint32))[0])
    want = [int(mix(np.array([(h + (k + 1) * 0x9E3779B9) & 0xFFFFFFFF], np.uint32))[0]) for k in range(12)]
    assert normal_words(seed, [g0]).ravel().tolist() == want         # k = c * 6 + a * 2 + j


# ---- the float64 reference of dL/d(sx, sy) ----------------------------------------------------------------------------------

def forward64_screen(p, rec, off, ref, flags, frozen=None, r32=None):
    """forward64 with `off` (torch float64 [N, 2]) added to the screen position (sx, sy) of every splat, frozen ones
    included (its `screen_offset`): with off == 0 the images are those of forward64 exactly."""
    return forward64(p, rec, ref, flags, frozen, r32, screen_offset=off)


def screen_gradient(p, aos, ref, flags, w_rgba, w_depth=None, frozen=None):
    """(dL/d(sx, sy) [N, 2], dL/d(record) [N, 84]) in float64 of L = sum w_rgba * RGBA32F + sum w_depth * depth."""
    rec = torch.tensor(np.asarray(aos, np.float64), requires_grad=True)
    off = torch.zeros(len(aos), 2, dtype=torch.float64, requires_grad=True)
    rgba, dep = forward64_screen(p, rec, off, ref, flags, frozen, raster32(p, aos, ref) if frozen is not None else None)
    loss_of(rgba, dep, w_rgba, w_depth).backward()
    return off.grad.numpy(), rec.grad.numpy()


def screen_norm(dscreen, w, h):
    """What gs_densify_stats_device accumulates, from dL/d(sx, sy): the norm of the NDC-unit gradient."""
    return np.hypot(dscreen[:, 0] * 0.5 * w, dscreen[:, 1] * 0.5 * h)


@pytest.mark.parametrize("scene", ["ragged", "zero_det", "ragged@pose"])
def test_screen_reference_is_forward64_with_one_zero_added(oracle_mod, tmp_path, scene):
    """With the offset at zero forward64_screen's images equal forward64's exactly, and its record gradient equals
    reference_gradient; the screen gradient itself is not trivial, and through the projection it gives the part of the
    position gradient that the screen position carries (for a splat far from the clamp: checked by one central difference
    of the offset)."""
    aos, w, h, cam = load_scene(scene)
    p = oracle_params(oracle_mod, w, h, **cam)
    ref, flags = frame_decisions(tmp_path, p, aos)
    fz = frozen_of(scene, aos)
    frozen = fz if fz.any() else None
    r32 = raster32(p, aos, ref) if frozen is not None else None
    rec = torch.tensor(aos.astype(np.float64))
    with torch.no_grad():
        a0, d0 = forward64(p, rec, ref, flags, frozen, r32)
        a1, d1 = forward64_screen(p, rec, torch.zeros(len(aos), 2, dtype=torch.float64), ref, flags, frozen, r32)
    assert torch.equal(a0, a1) and torch.equal(d0, d1)
    rng = np.random.default_rng(2)
    wr, wd = rng.standard_normal((h, w, 4)), 0.1 * rng.standard_normal((h, w))
    ds, drec = screen_gradient(p, aos, ref, flags, wr, wd, frozen)
    assert np.array_equal(drec, reference_gradient(p, aos, ref, flags, wr, wd, frozen))
    emitting = np.unique(np.asarray(ref["id"])[:ref["e"]])
    assert np.count_nonzero(ds.any(1)) > 20 and not ds[np.setdiff1d(np.arange(len(aos)), emitting)].any()
    g = int(emitting[np.argmax(np.abs(ds[emitting, 0]))])
    step = 1e-6

    def loss(dx):
        off = torch.zeros(len(aos), 2, dtype=torch.float64)
        off[g, 0] = dx
        with torch.no_grad():
            a, d = forward64_screen(p, rec, off, ref, flags, frozen, r32)
        return float((a.numpy() * wr).sum() + (d.numpy() * wd).sum())

    fd = (loss(step) - loss(-step)) / (2 * step)
    assert abs(fd - ds[g, 0]) <= 1e-5 + 1e-4 * abs(fd), (fd, ds[g, 0])


def test_densify_entry_points_refuse_a_null_context():
    """gs_densify_stats_device / gs_densify_device: GS_ERR_INVALID on a NULL context, no crash; the defaults are the header's,
    the struct is 40 bytes, and the API version is unchanged."""
    from vk3dgaussiansplatting_amd import _lib
    import vk3dgaussiansplatting_amd as gs
    L = _lib.lib()
    buf = np.zeros(84, F)
    ptr = buf.ctypes.data_as(C.c_void_p)
    p = gs.default_densify_params()
    assert L.gs_densify_stats_device(None, ptr, ptr, 1, 1, ptr, ptr, ptr) == _lib.GS_ERR_INVALID
    assert L.gs_densify_device(None, ptr, None, None, 1, ptr, ptr, ptr, C.byref(p), ptr, None, None, 1, ptr) == _lib.GS_ERR_INVALID
    L.gs_default_densify_params(None)
    assert p.struct_size == C.sizeof(_lib.GsDensifyParams) == 40
    got = {k: getattr(p, k) for k in DEFAULTS}
    assert got == {k: (F(v) if k != "seed" else v) for k, v in DEFAULTS.items()}, got
    q = gs.default_densify_params(grad_threshold=1e-3, seed=2**40 + 5, prune_radius=20)
    assert (q.grad_threshold, q.seed, q.prune_radius, q.split_shrink) == (F(1e-3), 2**40 + 5, 20.0, F(1.6))
    with pytest.raises(TypeError):
        gs.default_densify_params(struct_size=4)
    with pytest.raises(TypeError):
        gs.default_densify_params(threshold=1.0)
    assert _lib.API_VERSION == 7 and L.gs_api_version() == 7
