"""A cloud from points (include/gsplat.h, gs_knn_mean_dist2_device / gs_records_from_points_device) without a GPU: the NumPy
float32 restatements tests/test_init_gpu.py compares the kernels with -- the brute-force mean squared distance to the three
nearest other points, the loader's Morton order, the records -- and the designed clouds.  The order rule and the rotation
bits are pinned to the loader itself (gs_write_ply, then gs_convert_ply); the pruning bound of the search is checked to be
conservative in float32."""
import functools

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_raw_cpu import convert_ply

F = np.float32
FLT_MAX, FLT_TINY = F(np.finfo(np.float32).max), F(np.finfo(np.float32).tiny)
SH_C0 = F(0.28209479177387814)
DEFAULTS = dict(opacity=F(0.1), min_dist2=F(1e-7), max_scale=F(np.inf))


# ---- the restatements ---------------------------------------------------------------------------------------------------------

def knn_mean_dist2_ref(points, chunk=256):
    """dist2[i] = ((a + b) + c) / 3.0f, a <= b <= c the three smallest d2(i, j) = (dx * dx + dy * dy) + dz * dz over j != i,
    dx = x_j - x_i: float32 throughout, brute force, `chunk` rows at a time."""
    p = np.ascontiguousarray(points, F)
    n = len(p)
    assert n >= 4
    out = np.empty(n, F)
    with np.errstate(all="ignore"):
        for i0 in range(0, n, chunk):
            q = p[i0:i0 + chunk]
            dx, dy, dz = (p[None, :, a] - q[:, None, a] for a in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F
            d2[np.arange(len(q)), np.arange(i0, i0 + len(q))] = np.inf        # the index itself, never a duplicate of it
            best = np.sort(np.partition(d2, 2, axis=1)[:, :3], axis=1)
            out[i0:i0 + chunk] = ((best[:, 0] + best[:, 1]) + best[:, 2]) / F(3.0)
    return out


def flipped(points):
    """The record's position of a .ply point (ResourceManager.cpp:231-236)."""
    return np.ascontiguousarray(points, F) * np.array([-1.0, -1.0, 1.0], F)


def part_by2(x):
    x = x & np.uint32(0x000003ff)
    x = (x ^ (x << np.uint32(16))) & np.uint32(0xff0000ff)
    x = (x ^ (x << np.uint32(8))) & np.uint32(0x0300f00f)
    x = (x ^ (x << np.uint32(4))) & np.uint32(0x030c30c3)
    x = (x ^ (x << np.uint32(2))) & np.uint32(0x09249249)
    return x


def morton_codes_ref(points):
    """The loader's codes (gs_ply.cpp, sweep 1) of the flipped positions: bounds from FLT_MAX and the smallest positive
    normal float, q = f2u((pos - min) / delta * 1023.0f), NaN and values <= 0 to 0, saturating."""
    pos = flipped(points)
    lo = np.minimum(FLT_MAX, pos.min(0)).astype(F)
    hi = np.maximum(FLT_TINY, pos.max(0)).astype(F)
    with np.errstate(all="ignore"):
        t = (pos - lo) / (hi - lo) * F(1023.0)
    assert t.dtype == F
    q = np.zeros(t.shape, np.uint32)
    inside = (t > 0) & (t < F(4294967296.0))                   # a NaN compares false
    q[inside] = t[inside].astype(np.uint32)
    q[t >= F(4294967296.0)] = 0xFFFFFFFF
    return (part_by2(q[:, 2]) << np.uint32(2)) + (part_by2(q[:, 1]) << np.uint32(1)) + part_by2(q[:, 0])


def morton_order_ref(points):
    """order[k] = the input index of output row k: a stable sort by all 32 bits of the code."""
    return np.argsort(morton_codes_ref(points), kind="stable").astype(np.uint32)


def records_from_points_ref(points, colors=None, dist2=None, **params):
    """(records [n, 84], order [n]) as gs_records_from_points_device defines them."""
    p = dict(DEFAULTS, **{k: F(v) for k, v in params.items()})
    points = np.ascontiguousarray(points, F)
    dist2 = knn_mean_dist2_ref(points) if dist2 is None else dist2
    order = morton_order_ref(points)
    rec = np.zeros((len(points), 84), F)
    rec[:, 0:3] = flipped(points)[order]
    d = np.where(dist2 < p["min_dist2"], p["min_dist2"], dist2).astype(F)
    s = np.sqrt(d)
    s = np.where(s > p["max_scale"], p["max_scale"], s).astype(F)
    rec[:, 4:7] = s[order, None]
    rec[:, 8:12] = np.array([-0.0, -0.0, 1.0, -0.0], F)       # the loader's record of rot_0..3 = (1, 0, 0, 0): pinned below
    if colors is not None:
        rec[:, 12:15] = ((np.ascontiguousarray(colors, F) - F(0.5)) / SH_C0)[order]
    rec[:, 15] = p["opacity"]
    assert rec.dtype == F
    return rec, order


# ---- the designed clouds ------------------------------------------------------------------------------------------------------

KINDS = ["uniform", "lattice", "duplicates", "identical", "planar", "seam", "outliers", "shifted"]
SIZES = [4, 5, 63, 64, 65, 255, 256, 257, 4097]
LARGE = 20_000                     # 313 boxes: five rounds of the 64-wide box test
LARGE_KINDS = KINDS                # its brute force is 4e8 pairs: about a second on the host


@functools.lru_cache(maxsize=None)
def cloud(kind, n):
    """(points [n, 3], colors [n, 3]) of a designed cloud, read-only.  The colours are distinct per point, so a row names
    its input even where positions repeat."""
    rng = np.random.default_rng([KINDS.index(kind), n])
    u = lambda *shape: rng.random(shape, dtype=F)
    if kind == "uniform":                                     # (a)
        p = u(n, 3) * F(2) - F(1)
    elif kind == "shifted":                                   # (g): (a) moved by 1e4 on every axis
        p = cloud("uniform", n)[0] + F(1e4)
    elif kind == "lattice":                                   # (b): distinct integer points, many exactly equal distances
        side = int(np.ceil(n ** (1 / 3))) + 1
        cells = rng.permutation(side ** 3)[:n]
        p = np.stack([cells % side, cells // side % side, cells // side ** 2], 1).astype(F)
    elif kind == "duplicates":                                # (c): 8 locations, whole boxes of zero extent, d2 = 0 ties
        p = (u(8, 3) * F(4) - F(2))[rng.integers(0, 8, n)]
    elif kind == "identical":                                 # (c): every delta 0, every row at the min_dist2 floor
        p = np.tile(np.array([[0.25, -1.5, 3.0]], F), (n, 1))
    elif kind == "planar":                                    # (d): one flat axis, the NaN-to-0 code path
        p = u(n, 3) * F(2) - F(1)
        p[:, 2] = F(0.25)
    elif kind == "seam":                                      # (e): two thin slabs either side of the box's middle plane
        p = u(n, 3) * F(2) - F(1)
        # the plane where the top bit of the order's x turns, q = 512 of 1023: flipped x = 1 / 1023 in the box [-1, 1]
        p[:, 0] = -(F(1 / 1023) + (u(n) * F(4e-4) + F(1e-4)) * np.where(np.arange(n) % 2 == 0, F(1), F(-1)))
        p[0], p[1] = F(-1), F(1)                              # the corners of that box
    elif kind == "outliers":                                  # (f): a tight cluster, five outliers far from it and each other
        p = (u(n, 3) - F(0.5)) * F(1e-3)
        k = min(5, n - 3)
        p[:k] = np.array([[100, 0, 0], [0, -150, 0], [0, 0, 220], [-300, 300, 0], [170, 170, -170]], F)[:k]
    else:
        raise KeyError(kind)
    p = np.ascontiguousarray(rng.permutation(p), F)
    c = np.ascontiguousarray(u(n, 3))
    p.setflags(write=False); c.setflags(write=False)
    return p, c


@functools.lru_cache(maxsize=None)
def reference(kind, n):
    """(dist2 [n], records with colours [n, 84], order [n]) of a designed cloud under the defaults, computed once."""
    p, c = cloud(kind, n)
    dist2 = knn_mean_dist2_ref(p)
    rec, order = records_from_points_ref(p, c, dist2)
    for a in (dist2, rec, order):
        a.setflags(write=False)
    return dist2, rec, order


# ---- tests --------------------------------------------------------------------------------------------------------------------

def test_brute_force_on_known_clouds():
    """The restatement on clouds whose answer is known: a unit lattice line, duplicates that count, the index that does not."""
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [10, 0, 0]], F)
    want = [(1 + 4 + 9) / 3, (1 + 1 + 4) / 3, (1 + 1 + 4) / 3, (1 + 4 + 9) / 3, (49 + 64 + 81) / 3]
    assert np.array_equal(knn_mean_dist2_ref(line), np.array(want, F))
    dup = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [2, 0, 0]], F)
    assert np.array_equal(knn_mean_dist2_ref(dup), np.array([4 / 3, 4 / 3, 4 / 3, 4], F))
    assert not reference("identical", 65)[0].any()
    rec = reference("identical", 65)[1]
    assert np.all(rec[:, 4:7] == np.sqrt(F(1e-7)))
    for kind in KINDS:                                        # chunking does not change a bit
        p = cloud(kind, 257)[0]
        assert np.array_equal(knn_mean_dist2_ref(p, chunk=7), reference(kind, 257)[0]), kind


def test_clouds_are_what_they_claim():
    p = cloud("seam", 4097)[0]
    order = reference("seam", 4097)[2]
    above = -p[:, 0] > F(1 / 1023)
    assert p[:, 0].max() == 1 and p[:, 0].min() == -1 and np.sum(above) > 2000 and np.sum(~above) > 2000
    assert np.sum(np.abs(-p[:, 0] - F(1 / 1023)) < 6e-4) == len(p) - 2        # all but the two corners
    # neighbours in space, far apart in the order: the nearest point across the plane is hundreds of rows away for most
    rank = np.empty(len(p), np.int64); rank[order] = np.arange(len(p))
    far = 0
    for i in range(0, 4097, 64):
        other = np.flatnonzero(above != above[i])
        j = other[np.argmin(((p[other] - p[i]) ** 2).sum(1))]
        far += abs(rank[i] - rank[j]) > 512
    assert far > 40
    assert len(np.unique(cloud("duplicates", 4097)[0], axis=0)) == 8
    assert len(np.unique(cloud("lattice", 4097)[0], axis=0)) == 4097
    codes = morton_codes_ref(cloud("planar", 257)[0])
    assert not (codes & np.uint32(0x24924924)).any()          # the flat axis: 0 / 0 = NaN, then 0
    d = reference("outliers", 257)[0]
    assert np.sum(d > 1e3) == 5                               # the outliers' neighbours are all far away
    assert reference("shifted", 257)[0].max() < 1.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [5, 257, 4097])
def test_loader_round_trip(tmp_path, kind, n):
    """records_from_points_ref written with gs_write_ply(GS_PLY_FROM_RECORDS) and read with gs_convert_ply: the rows come
    back in the same order, and positions, rotation and the 48 SH floats bit for bit -- the restated order rule and the
    rotation bits are the loader's.  Scale and opacity pass a host log and the loader's exp: the bounds of the writer's own
    round trip (tests/test_raw_cpu.py, test_ply_round_trip)."""
    rec = reference(kind, n)[1]
    path = str(tmp_path / "cloud.ply")
    gs.write_ply(path, rec, "records")
    back = convert_ply(path)
    assert back.shape == rec.shape
    exact = [c for c in range(84) if not (4 <= c < 7 or c == 15)]
    assert np.array_equal(back[:, exact].view(np.uint32), rec[:, exact].view(np.uint32))      # the colours are distinct: same order
    assert np.array_equal(back[:, 8:12].view(np.uint32), np.tile(np.array([-0.0, -0.0, 1.0, -0.0], F).view(np.uint32), (n, 1)))
    s = rec[:, 4:7].astype(np.float64)
    assert np.all(np.abs(back[:, 4:7].astype(np.float64) - s) <= s * 2.0 ** -23 * (np.abs(np.log(s)) + 2))
    assert np.all(np.abs(back[:, 15].astype(np.float64) - rec[:, 15]) <= 2.0 ** -22)


def test_loader_round_trip_without_colours_and_negative_octant(tmp_path):
    """A cloud whose flipped positions are all negative: the loader's max starts at the smallest POSITIVE float, so the
    bounds are not the cloud's own; and colours NULL: SH DC +0."""
    p = np.abs(cloud("uniform", 257)[0]) + F(0.5)
    p[:, 2] *= F(-1)                                          # flipped: (-x, -y, z) all below zero
    assert flipped(p).max() < 0
    rec, order = records_from_points_ref(p)
    assert not rec[:, 12:15].view(np.uint32).any()
    own = np.argsort(morton_codes_ref(p), kind="stable")
    naive_lo, naive_hi = flipped(p).min(0), flipped(p).max(0)
    t = ((flipped(p) - naive_lo) / (naive_hi - naive_lo) * F(1023.0)).astype(np.uint32)
    naive = np.argsort((part_by2(t[:, 2]) << np.uint32(2)) + (part_by2(t[:, 1]) << np.uint32(1)) + part_by2(t[:, 0]), kind="stable")
    assert not np.array_equal(own, naive)                     # the start value matters here
    path = str(tmp_path / "neg.ply")
    gs.write_ply(path, rec, "records")
    back = convert_ply(path)
    assert np.array_equal(back[:, 0:3].view(np.uint32), rec[:, 0:3].view(np.uint32))
    assert np.array_equal(rec[:, 0:3], flipped(p)[order])


def test_pruning_bound_is_conservative_in_float32():
    """The search drops a box when (ex * ex + ey * ey) + ez * ez > third best, e = max(lo - p, p - hi, 0) per axis (or box
    against box).  Subtraction, multiplication and addition are monotone under round-to-nearest, so the bound never exceeds
    the computed d2 of a member: checked over random boxes and points, coordinates offset by 1e4 included, and at the
    gaps of one ulp where a bound computed in another shape would err."""
    rng = np.random.default_rng(5)
    worst = -np.inf
    for offset in (0.0, 1e4, -1e4, 3e6):
        for scale in (1.0, 1e-3, 1e-6 * max(abs(offset), 1.0)):
            members = (rng.standard_normal((400, 64, 3)) * scale + offset).astype(F)
            lo, hi = members.min(1), members.max(1)
            for spread in (1.0, 3.0, 30.0):
                q = (rng.standard_normal((400, 16, 3)) * scale * spread + offset).astype(F)
                e = np.maximum(np.maximum(lo[:, None] - q, q - hi[:, None]), F(0))
                bound = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                d = members[:, None, :, :] - q[:, :, None, :]
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                assert bound.dtype == F and d2.dtype == F
                assert np.all(bound[:, :, None] <= d2)
                worst = max(worst, float((bound[:, :, None] - d2).max()))
                # box against box: the query points' own box against the members' box
                qlo, qhi = q.min(1), q.max(1)
                eb = np.maximum(np.maximum(lo - qhi, qlo - hi), F(0))
                bb = (eb[:, 0] * eb[:, 0] + eb[:, 1] * eb[:, 1]) + eb[:, 2] * eb[:, 2]
                assert np.all(bb[:, None, None] <= d2)
    assert worst <= 0.0


def test_defaults_and_struct():
    p = gs.default_init_params()
    assert p.struct_size == 16 and p.opacity == F(0.1) and p.min_dist2 == F(1e-7) and p.max_scale == np.inf
    q = gs.default_init_params(opacity=0.5, max_scale=2.0)
    assert q.opacity == 0.5 and q.max_scale == 2.0 and q.min_dist2 == F(1e-7)
    with pytest.raises(TypeError):
        gs.default_init_params(struct_size=3)
    with pytest.raises(TypeError):
        gs.default_init_params(scale=1.0)
    L = _lib.lib()
    assert L.gs_knn_mean_dist2_device(None, None, 10, None) == _lib.GS_ERR_INVALID            # a NULL context: the code alone
    assert L.gs_records_from_points_device(None, None, None, 10, None, None, None) == _lib.GS_ERR_INVALID
    L.gs_default_init_params(None)
