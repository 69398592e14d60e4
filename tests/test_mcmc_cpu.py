"""The MCMC calls of include/gsplat.h restated in NumPy (mcmc_ref, imported by tests/test_mcmc_gpu.py): the sampler with
Python integers for the 128-bit product, the relocation values in float32 in the header's order and in float64, the noise
in float64, the layouts of gs_relocate_device and gs_grow_device.  The checks here need no GPU: the float32 recurrence on
the grid the header quotes, the sampler's invariants, a designed cloud in which every comparison decides alone, and the
NULL-context refusals.  The other refusals need a context: tests/test_mcmc_gpu.py."""
import math
import types

import numpy as np
import pytest

from vk3dgaussiansplatting_amd import _lib
from test_densify_cpu import mix, normals, rot_matrix
from test_raw_cpu import E, FLT_MIN, OPACITY_HI

F = np.float32
RMAX = 51
HI = OPACITY_HI                                   # 0x1.fffffep-1f
B = np.array([[math.comb(a, b) for b in range(RMAX)] for a in range(RMAX)], dtype=np.float64).astype(F)   # exact below 2^53
Q = np.array([1.0 / math.sqrt(k + 1) for k in range(RMAX)], dtype=np.float64).astype(F)
ALIVE, DEAD_NO_DRAW = -1, -2                      # src_of of a row that is no copy


# ---- the sampler ----------------------------------------------------------------------------------------------------------

def weights(records, min_opacity, flip=False):
    """w(g) of the header, uint64 [n].  flip: aliveness with >= instead of > (for the check that the design is decisive)."""
    o = np.asarray(records, F)[:, 15]
    with np.errstate(invalid="ignore"):
        alive = (o >= F(min_opacity)) if flip else (o > F(min_opacity))
        w = np.where(alive, np.minimum(o, F(1)) * F(16777216.0), F(0))
    return np.where(alive, w, 0).astype(np.uint64)                     # the conversion truncates; the values are exact


def draw_words(i, seed):
    """r64 of draws i (uint32 array) as Python integers."""
    i = np.asarray(i, np.uint32)
    seed = int(seed)
    with np.errstate(over="ignore"):
        h = mix(mix(i ^ np.uint32(seed & 0xFFFFFFFF)) + np.uint32(seed >> 32))
        hi, lo = mix(h + np.uint32(0x9E3779B9)), mix(h + np.uint32(2) * np.uint32(0x9E3779B9))
    return [(int(a) << 32) | int(b) for a, b in zip(hi, lo)]


def point_of(r64, total):
    return (r64 * total) >> 64


def sources(i, seed, w):
    """The source of every draw i: the one g with P(g) <= t < P(g) + w(g).  total > 0."""
    inclusive = np.cumsum(w.astype(np.uint64))
    total = int(inclusive[-1])
    t = np.array([point_of(r, total) for r in draw_words(i, seed)], dtype=np.uint64)
    return np.searchsorted(inclusive, t, side="right").astype(np.int64)


# ---- the values -----------------------------------------------------------------------------------------------------------

def ratio(cnt):
    return np.minimum(np.asarray(cnt, np.int64) + 1, RMAX)


def denominator32(op, r):
    """D of the header for stored opacities op (float32 [k]) and ratios r (int [k]): float32, in its nesting."""
    op = np.asarray(op, F)
    r = np.asarray(r, np.int64)
    D = np.zeros(len(op), F)
    for i in range(1, int(r.max(initial=0)) + 1):
        on = r >= i
        p, sg = op.copy(), F(1)
        for k in range(i):
            D = np.where(on, D + B[i - 1, k] * ((sg * Q[k]) * p), D)
            p = p * op
            sg = -sg
    assert D.dtype == F
    return D


def denominator64(op, r):
    op = np.asarray(op, np.float64)
    return np.array([sum(math.comb(i - 1, k) * (-1) ** k / math.sqrt(k + 1) * float(o) ** (k + 1) for i in range(1, int(n) + 1) for k in range(i))
                     for o, n in zip(op, r)])


def opacity64(o, r, min_opacity):
    """oc of the header in float64: 1 - (1 - min(o, hi))^(1 / r), clamped to [min_opacity, hi]."""
    o = np.minimum(np.asarray(o, np.float64), float(HI))
    o1 = -np.expm1(np.log1p(-o) / np.asarray(r, np.float64))
    return np.clip(o1, float(F(min_opacity)), float(HI))


def scales32(o_old, s_old, o_stored, r):
    """s'_k = c * s_k, c = o / D(o', r), from the opacity bits that were stored: float32, no transcendental."""
    with np.errstate(all="ignore"):
        c = np.asarray(o_old, F) / denominator32(o_stored, r)
        return c[:, None] * np.asarray(s_old, F), c


def values32(o, s, cnt, min_opacity, raw):
    """The relocation values in float32 with NumPy's log1p / expm1 / log standing for the device's: dict(o, s, raw_o, raw_s).
    The layouts use it; where the device's own transcendentals matter, tests/test_mcmc_gpu.py compares under an allowance."""
    o, s, r = np.asarray(o, F), np.asarray(s, F), ratio(cnt)
    with np.errstate(all="ignore"):
        o1 = -np.expm1(np.log1p(-np.minimum(o, HI)) / r.astype(F)).astype(F)
        oc = np.where(o1 < F(min_opacity), F(min_opacity), np.where(o1 > HI, HI, o1)).astype(F)
        out = dict(o=oc, raw_o=None, raw_s=None)
        if raw:
            out["raw_o"] = np.log(oc / (F(1) - oc)).astype(F)
            out["o"] = (F(1) / (F(1) + E(-out["raw_o"], np.float32))).astype(F)
        out["s"], _ = scales32(o, s, out["o"], r)
        if raw:
            out["raw_s"] = np.log(np.where(out["s"] < FLT_MIN, FLT_MIN, out["s"])).astype(F)
            out["s"] = E(out["raw_s"], np.float32).astype(F)
    return out


# ---- the layouts ----------------------------------------------------------------------------------------------------------

def relocate_ref(records, min_opacity, seed, flip=False):
    """gs_relocate_device's decisions: dead [n] bool, src_of [n] (the source of a dead d that drew, ALIVE, DEAD_NO_DRAW), cnt [n],
    ids (the changed rows, ascending), counts (changed, dead, sources)."""
    w = weights(records, min_opacity, flip)
    n = len(w)
    dead = w == 0
    src_of = np.where(dead, DEAD_NO_DRAW, ALIVE).astype(np.int64)
    cnt = np.zeros(n, np.int64)
    if int(w.sum()) > 0 and dead.any():
        d = np.flatnonzero(dead)
        src_of[d] = sources(d, seed, w)
        cnt = np.bincount(src_of[d], minlength=n)
    changed = (src_of >= 0) | (cnt > 0)
    return types.SimpleNamespace(w=w, dead=dead, src_of=src_of, cnt=cnt, ids=np.flatnonzero(changed),
                                 counts=(int(changed.sum()), int(dead.sum()), int((cnt > 0).sum())))


def grow_ref(records, min_opacity, seed, n_add):
    """gs_grow_device's decisions: cnt [n], offset [n] = o(g), parent [n_out], counts (outputs, sources)."""
    w = weights(records, min_opacity)
    n = len(w)
    cnt = np.zeros(n, np.int64)
    if int(w.sum()) > 0 and n_add:
        cnt = np.bincount(sources(np.arange(n_add), seed, w), minlength=n)
    k = 1 + cnt
    offset = np.concatenate([[0], np.cumsum(k)[:-1]]).astype(np.int64)
    return types.SimpleNamespace(w=w, cnt=cnt, offset=offset, parent=np.repeat(np.arange(n), k),
                                 counts=(int(k.sum()), int((cnt > 0).sum())))


# ---- the noise ------------------------------------------------------------------------------------------------------------

def noise_ref(records, g, scale, gate_k, gate_x0, seed):
    """pos64 [len(g), 3] = the float64 positions after the noise, and bound [len(g), 3] = gate * scale * sum_k |R[i][k]| s_k^2
    sum_j |R[j][k]|, the size the allowance of a unit normal's error is carried through."""
    rec = np.asarray(records, F)[g].astype(np.float64)
    z = normals(seed, g)[:, 0, :]
    R, s, o = rot_matrix(rec[:, 8:12]), rec[:, 4:7], rec[:, 15]
    gate = 1.0 / (1.0 + np.exp(-(float(F(gate_k)) * ((1.0 - o) - float(F(gate_x0))))))
    a = s * np.einsum("gjk,gj->gk", R, z)
    off = np.einsum("gik,gk->gi", R * s[:, None, :], a)
    bound = gate[:, None] * float(F(scale)) * np.einsum("gik,gk->gi", np.abs(R), s * s * np.abs(R).sum(1))
    return rec[:, 0:3] + off * gate[:, None] * float(F(scale)), bound


mcmc_ref = types.SimpleNamespace(weights=weights, draw_words=draw_words, point_of=point_of, sources=sources, ratio=ratio,
                                 denominator32=denominator32, denominator64=denominator64, opacity64=opacity64,
                                 scales32=scales32, values32=values32, relocate_ref=relocate_ref, grow_ref=grow_ref,
                                 noise_ref=noise_ref)


# ---- checks ---------------------------------------------------------------------------------------------------------------

GRID = [0.0051, 0.01, 0.05, 0.1, 0.3, 0.5, 0.8, 0.95, 0.99, 0.999, 0.99999, 1 - 2 ** -24]


def test_the_float32_recurrence_on_the_grid():
    """Opacities from 0.0051 to 1 - 2^-24, every r in 1..51, with the clamps: D > 0, 0 < c <= 1, and D within 6e-4 relative of
    its float64 value."""
    o = np.repeat(np.array(GRID, dtype=np.float64).astype(F), RMAX)
    r = np.tile(np.arange(1, RMAX + 1), len(GRID))
    op = opacity64(o, r, 0.005).astype(F)
    op = np.where(op < F(0.005), F(0.005), np.where(op > HI, HI, op))
    D = denominator32(op, r)
    c = o / D
    D64 = denominator64(op, r)
    worst = float(np.max(np.abs(D.astype(np.float64) - D64) / np.abs(D64)))
    print("float32 D against float64: worst relative error", worst, "c in", float(c.min()), float(c.max()))
    assert np.all(D > 0) and np.all(np.isfinite(c)) and np.all(c > 0) and np.all(c <= 1)
    assert worst <= 6e-4
    # r = 1: the splat itself, unchanged up to rounding
    assert np.allclose(c[r == 1], 1.0, rtol=2e-7)


def test_the_point_lies_below_the_total_at_both_ends():
    for total in (1, 2, 3, 2 ** 24, 2 ** 24 + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 55 - 1, 2 ** 55):
        assert point_of(0, total) == 0
        assert point_of(2 ** 64 - 1, total) == total - 1 < total


def test_a_source_never_has_weight_zero():
    rng = np.random.default_rng(5)
    for n, p_dead in ((1, 0.0), (7, 0.5), (300, 0.9), (300, 0.1), (1000, 0.99)):
        rec = np.zeros((n, 84), F)
        rec[:, 15] = rng.uniform(0.006, 1.2, n)
        rec[rng.random(n) < p_dead, 15] = rng.choice(F([0.0, 0.005, 0.001, np.nan, -1.0]))
        rec[rng.integers(n), 15] = 0.7                                  # at least one alive
        w = weights(rec, 0.005)
        i = np.arange(4000)
        src = sources(i, 0xABCDEF0123456789, w)
        assert np.all(w[src] > 0)
        inclusive = np.cumsum(w)
        t = np.array([point_of(r, int(inclusive[-1])) for r in draw_words(i, 0xABCDEF0123456789)], dtype=np.uint64)
        assert np.all(inclusive[src] - w[src] <= t) and np.all(t < inclusive[src])
        if n >= 300:                                                     # in proportion to the weights, roughly
            assert len(np.unique(src)) > 1


def designed_cloud():
    """Six splats in which every comparison decides alone: opacity == min_opacity (dead under >, alive under >=), a NaN (dead),
    just above the threshold (alive, a small weight), above 1 (alive, weight 2^24 exactly), 0 and an ordinary one."""
    rec = np.zeros((6, 84), F)
    rec[:, 15] = [0.005, np.nan, np.nextafter(F(0.005), F(1)), 1.5, 0.0, 0.5]
    rec[:, 4:7] = 0.1
    return rec


def test_the_designed_cloud_is_decisive():
    rec = designed_cloud()
    w = weights(rec, 0.005)
    assert list(w) == [0, 0, int(float(np.nextafter(F(0.005), F(1))) * 2 ** 24), 2 ** 24, 0, 2 ** 23]
    a = relocate_ref(rec, 0.005, 7)
    assert a.counts[1] == 3 and list(np.flatnonzero(a.dead)) == [0, 1, 4] and np.all(a.w[a.src_of[a.dead]] > 0)
    assert a.counts[0] == 3 + a.counts[2] and list(a.ids) == sorted(set(np.flatnonzero(a.dead)) | set(np.flatnonzero(a.cnt)))
    b = relocate_ref(rec, 0.005, 7, flip=True)
    assert b.counts[1] == 2 and not b.dead[0] and (a.counts != b.counts)
    # the values of a source: the stored pair is consistent in both spaces
    for raw in (False, True):
        v = values32(rec[[5, 3], 15], rec[[5, 3], 4:7], [1, 60], 0.005, raw)
        assert np.all(v["o"] > 0) and np.all(v["o"] < rec[[5, 3], 15]) and np.all(v["s"] < F(0.1)) and np.all(v["s"] > 0)
        want = opacity64(rec[[5, 3], 15], ratio([1, 60]), 0.005)
        assert np.allclose(v["o"], want, rtol=1e-5)
    assert list(ratio([0, 1, 49, 50, 51, 10 ** 6])) == [1, 2, 50, 51, 51, 51]
    # two copies at the centre give the old opacity back: 1 - (1 - o')^2 = o
    o2 = values32(F([0.5]), np.full((1, 3), 0.1, F), [1], 0.005, False)["o"].astype(np.float64)
    assert abs(1 - (1 - o2[0]) ** 2 - 0.5) < 1e-6


def test_grow_layout():
    rec = designed_cloud()
    g = grow_ref(rec, 0.005, 3, 10)
    assert g.counts[0] == 16 and g.cnt.sum() == 10 and np.all(g.cnt[[0, 1, 4]] == 0)
    assert list(g.offset) == list(np.cumsum(np.concatenate([[0], 1 + g.cnt]))[:-1]) and len(g.parent) == 16
    rec[:, 15] = 0.0
    assert grow_ref(rec, 0.005, 3, 10).counts == (6, 0)
    assert grow_ref(designed_cloud(), 0.005, 3, 0).counts == (6, 0)


def test_noise_is_sigma_z():
    """noise_ref against M M^T z written out, and the gate: a transparent splat moves, an opaque one stays."""
    rng = np.random.default_rng(1)
    rec = np.zeros((5, 84), F)
    rec[:, 0:3] = rng.uniform(-1, 1, (5, 3))
    rec[:, 4:7] = rng.uniform(0.01, 0.3, (5, 3))
    q = rng.standard_normal((5, 4))
    rec[:, 8:12] = q / np.linalg.norm(q, axis=1, keepdims=True)
    rec[:, 15] = [0.001, 0.001, 0.5, 0.99, 0.004]
    g = np.arange(5)
    pos, bound = noise_ref(rec, g, 0.5, 100.0, 0.995, 11)
    z = normals(11, g)[:, 0, :]
    for k in range(5):
        M = rot_matrix(rec[k, 8:12].astype(np.float64)) * rec[k, 4:7].astype(np.float64)
        gate = 1 / (1 + math.exp(-100.0 * ((1 - float(rec[k, 15])) - float(F(0.995)))))
        assert np.allclose(pos[k], rec[k, 0:3] + (M @ M.T @ z[k]) * gate * 0.5, rtol=1e-12, atol=1e-15)
    moved = np.abs(pos - rec[:, 0:3]).max(1)
    assert moved[0] > 1e-6 and moved[2] < 1e-12 * max(moved[0], 1) and np.all(bound >= 0)


def test_mcmc_entry_points_refuse_a_null_context():
    L = _lib.lib()
    assert L.gs_relocate_device(None, 1, None, None, None, 1, 0.005, 0, None, 0, 1) == _lib.GS_ERR_INVALID
    assert L.gs_grow_device(None, 1, None, None, None, 1, 0.005, 0, 0, None, None, None, None, 0, 1) == _lib.GS_ERR_INVALID
    assert L.gs_position_noise_device(None, 1, None, 1, None, None, 0, 1.0, 100.0, 0.995, 0) == _lib.GS_ERR_INVALID
