"""The designed scenes of tests/test_project_records_gpu.py, proven on the CPU oracle: k_project stores the raster records of a
chunk of consecutive splats (a quarter wave of 16, or a wave of 64) only when one of them emits a list element, so the scenes put
whole runs of 64 and of 16 splats into one class each -- culled, kept without an element (the margin between |ndc| 1.0 and the
1.3 cull), emitting -- and a second camera swaps the emitting and the margin class, so that chunks stored in the first frame go
stale in the second.  Here every splat is shown to be of the class its place claims, under both cameras; no GPU."""
import functools

import numpy as np
import pytest

CULLED, MARGIN, EMITS = 0, 1, 2
WAVE, QUARTER = 64, 16
RAGGED = 37
# wave by wave; a string names the class of all 64 splats, a tuple (class of the wave, class of the odd ones, their lanes)
LAYOUT = (
    ("all emitting", EMITS),
    ("all in the margin", MARGIN),
    ("all culled", CULLED),
    ("one emitter at lane 0 among margin splats", (MARGIN, EMITS, (0,))),
    ("one emitter at lane 63 among margin splats", (MARGIN, EMITS, (63,))),
    ("one emitter in quarter 0", (MARGIN, EMITS, (5,))),
    ("one emitter in quarter 1", (MARGIN, EMITS, (16,))),
    ("one emitter in quarter 2", (MARGIN, EMITS, (47,))),
    ("one emitter in quarter 3", (MARGIN, EMITS, (48,))),
    ("one margin splat among culled ones", (CULLED, MARGIN, (21,))),
    ("a class per quarter: emitting, margin, culled, margin", "quarters"),
    ("a ragged last wave of margin splats", "ragged"),
)
N = (len(LAYOUT) - 1) * WAVE + RAGGED
CAMERA_1 = dict(pos=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0)
FRAMES = ((64, 48), (128, 96))


def designed_classes():
    """The class each splat is placed for under CAMERA_1, [N]."""
    cls = np.empty(N, np.int64)
    for w, (_, what) in enumerate(LAYOUT):
        lanes = slice(w * WAVE, min((w + 1) * WAVE, N))
        if what == "quarters":
            cls[lanes] = np.repeat([EMITS, MARGIN, CULLED, MARGIN], QUARTER)
        elif what == "ragged":
            cls[lanes] = MARGIN
        elif isinstance(what, tuple):
            cls[lanes] = what[0]
            cls[w * WAVE + np.array(what[2])] = what[1]
        else:
            cls[lanes] = what
    return cls


def _matrix(flat):
    return np.asarray(flat, np.float64).reshape(4, 4).T          # the flat arrays are column-major


def _world_of(view, proj, ndc_x, ndc_y, depth):
    """World position that CAMERA_1 sees at (ndc_x, ndc_y), `depth` in front of it (float64; the oracle judges the float32)."""
    V, P = _matrix(view), _matrix(proj)
    # q = P (X, Y, -depth, 1): q.x = ndc_x q.w and q.y = ndc_y q.w, two linear equations in X and Y
    rows = np.stack([P[0] - ndc_x * P[3], P[1] - ndc_y * P[3]])
    rhs = -(rows[:, 2] * -depth + rows[:, 3])
    X, Y = np.linalg.solve(rows[:, :2], rhs)
    return (np.linalg.inv(V) @ np.array([X, Y, -depth, 1.0]))[:3]


@functools.lru_cache(maxsize=None)
def scene(w, h):
    """(aos [N][84], designed classes [N]) for a w x h frame; never modified.  Emitting splats sit around the middle of the
    screen, margin splats at ndc x = 1.17 +- 0.04 beside its right edge and high up (so that CAMERA_2 finds them on the screen),
    culled ones half behind the camera and half at ndc x = 1.6.  All are small (a radius of a few pixels) and round; all 16 SH
    coefficients are non-zero."""
    import oracle
    import vk3dgaussiansplatting_amd as gs
    view, proj = oracle.camera_matrices(np.zeros(3, np.float32), 0.0, 0.0, w / h)
    cls = designed_classes()
    rng = np.random.default_rng(w * 1000 + h)
    aos = np.zeros((N, 84), np.float32)
    for g in range(N):
        depth = rng.uniform(3.0, 5.0)
        jx, jy = rng.uniform(-0.04, 0.04, 2)
        if cls[g] == EMITS:
            p = _world_of(view, proj, 0.4 * jx, 0.4 * jy, depth)
        elif cls[g] == MARGIN:
            p = _world_of(view, proj, 1.17 + jx, MARGIN_NDC_Y + jy, depth)
        elif g % 2:
            p = _world_of(view, proj, 1.6 + jx, 4 * jy, depth)
        else:
            p = _world_of(view, proj, 4 * jx, 4 * jy, -depth)          # behind the camera
        aos[g] = gs.makeGaussian(p, (0.04, 0.04, 0.04, 0.0), sh0=(0.0, 0.0, 0.0, rng.uniform(0.3, 0.9)))
    sh_rgb = np.array([12 + 4 * k + c for k in range(16) for c in range(3)])
    aos[:, sh_rgb] = (rng.uniform(0.1, 0.3, (N, 48)) * rng.choice([-1.0, 1.0], (N, 48))).astype(np.float32)
    aos.setflags(write=False)
    cls.setflags(write=False)
    return aos, cls


# The second camera: turned so that the margin splats of CAMERA_1 come onto the screen and its emitting splats leave it across
# the bottom edge.  (Across the left or the top edge they would still emit: the reference's tile extents truncate towards zero,
# so a splat up to 16 px outside those edges lands in tile column / row 0.)
MARGIN_NDC_Y = 0.75
CAMERA_2 = dict(pos=(0.0, 0.0, 0.0), yaw=-0.2, pitch=0.86)


def oracle_classes(oracle, aos, w, h, cam, **rows):
    """Per splat, what the oracle's InitSortList makes of it: CULLED, MARGIN (passes both culls, touches no tile) or EMITS; and
    the |ndc| of the kept ones, from the screen position it stores."""
    view, proj = oracle.camera_matrices(np.asarray(cam["pos"], np.float32), cam["yaw"], cam["pitch"], w / h)
    p = oracle.make_params(w, h, view, proj, cam["pos"], **rows)
    s = oracle.init_sort_list(p, aos)["splats"]
    tiles = (s["max_x"].astype(np.int64) - s["min_x"]) * (s["max_y"].astype(np.int64) - s["min_y"])
    cls = np.where(s["visible"] == 0, CULLED, np.where(tiles == 0, MARGIN, EMITS))
    ndc = np.stack([s["screen_x"] / np.float32(w) * 2 - 1, s["screen_y"] / np.float32(h) * 2 - 1], axis=1)
    return cls, ndc


def chunk_classes(cls, chunk):
    """Per chunk of `chunk` consecutive splats: does it hold an emitting splat (its records are stored)."""
    pad = np.full(-len(cls) % chunk, CULLED)
    return (np.concatenate([cls, pad]).reshape(-1, chunk) == EMITS).any(axis=1)


@pytest.mark.parametrize("w,h", FRAMES)
def test_every_splat_is_of_the_class_its_place_claims(oracle_mod, w, h):
    aos, want = scene(w, h)
    assert N == 11 * 64 + 37 and N > 2 * 256 and N % 256 and N % 64 == RAGGED          # crosses two block boundaries, ragged
    got, ndc = oracle_classes(oracle_mod, aos, w, h, CAMERA_1)
    assert np.array_equal(got, want)
    # the margin splats lie between |ndc| 1.05 and 1.25 (in x; inside the screen in y), the emitting ones on the screen
    m = want == MARGIN
    assert np.all((np.abs(ndc[m, 0]) > 1.05) & (np.abs(ndc[m, 0]) < 1.25) & (np.abs(ndc[m, 1]) < 1.0))
    assert np.all(np.abs(ndc[want == EMITS]) < 1.0)
    # both kinds of culled splat
    view, _ = oracle_mod.camera_matrices(np.zeros(3, np.float32), 0.0, 0.0, w / h)
    z = (np.c_[aos[:, :3].astype(np.float64), np.ones(N)] @ _matrix(view).T)[:, 2]
    c = want == CULLED
    assert np.count_nonzero(c & (z > 0)) > 40 and np.count_nonzero(c & (z < 0)) > 40


@pytest.mark.parametrize("w,h", FRAMES)
def test_waves_and_quarters_are_of_the_designed_kinds(oracle_mod, w, h):
    """What a build that stores by waves and one that stores by quarter waves each keep: the designed scenes tell them apart."""
    aos, _ = scene(w, h)
    cls, _ = oracle_classes(oracle_mod, aos, w, h, CAMERA_1)
    waves, quarters = chunk_classes(cls, WAVE), chunk_classes(cls, QUARTER)
    assert waves.tolist() == [True, False, False, True, True, True, True, True, True, False, True, False]
    q = quarters.reshape(-1, 4) if len(quarters) % 4 == 0 else np.concatenate([quarters, [False] * (-len(quarters) % 4)]).reshape(-1, 4)
    assert q[0].all() and not q[1].any() and not q[2].any()
    assert q[3].tolist() == [True, False, False, False] and q[4].tolist() == [False, False, False, True]
    for k in range(4):
        assert q[5 + k].tolist() == [j == k for j in range(4)]
    assert not q[9].any() and q[10].tolist() == [True, False, False, False] and not q[11].any()
    # a wave with a margin splat among culled ones, and wholly culled chunks next to kept ones
    assert np.count_nonzero(cls[9 * WAVE:10 * WAVE] == MARGIN) == 1 and np.count_nonzero(cls[9 * WAVE:10 * WAVE] == CULLED) == 63


@pytest.mark.parametrize("w,h", FRAMES)
def test_the_second_camera_swaps_the_emitting_and_the_margin_class(oracle_mod, w, h):
    aos, first = scene(w, h)
    second, ndc = oracle_classes(oracle_mod, aos, w, h, CAMERA_2)
    assert np.all(second[first == EMITS] == MARGIN) and np.all(second[first == MARGIN] == EMITS)
    m = second == MARGIN
    assert np.all((np.abs(ndc[m]).max(axis=1) > 1.05) & (np.abs(ndc[m]).max(axis=1) < 1.25))
    # chunks stored in the first frame and not in the second (their records go stale), and the other way round
    for chunk in (WAVE, QUARTER):
        a, b = chunk_classes(first, chunk), chunk_classes(second, chunk)
        assert np.count_nonzero(a & ~b) >= 1 and np.count_nonzero(b & ~a) >= 2
