"""Pass 0 of a frame's depth sort inside InitSortList (k_emit<false, true>) through the C-ABI, on the designed scenes of
tests/test_emit_pass0_cpu.py.  Every case draws the scene on a context that takes the path (GS_SORT_RADIX4, GS_COUNT_PER_PASS --
GS_COUNT_AUTO would feed the counts of lists this short --, record_timings = 1) and on one that does not (record_timings = 2: pass 0
as two launches) and checks: gs_debug_read(GS_BUF_PASS0_OFFSETS) is readable on the first alone and equals the numpy table; sorted
tile words, depth words, ids, ranges and the image equal the oracle's; they equal the other context's bit for bit; the element
counts and the overflow flag agree.

An overflowing frame (the list is cut by LIST index, which the digit rows do not know) writes the plain list and runs pass 0 as
launches: the same lists, and no table to read.  The case of a heavy block whose helper records find no room (kEmitNoHelp) cannot
be reached without overflow: the helper list holds capacity / 4096 + 1 records and a frame registers at most elements / 4096 of
them, so it is not run here.  The non-temporal k_project instantiations are chosen by scene size (above 256 MiB of records):
the full-size frames of tests/test_bench_gpu.py run them."""
import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from test_parity_gpu import make_scene
from test_designed_lengths_cpu import WIDE_CAPACITY, cached, wide_frame, wide_scene
from test_emit_pass0_cpu import OH, OVERFLOWS, OW, overflow_scene, pass0_table, scene

pytestmark = pytest.mark.gpu

SH = gs.SphericalHarmonicsMode
GS_ERR_INVALID = -1

LISTS = (("tile", gs.BUF_SORTED_TILE), ("depth", gs.BUF_SORTED_DEPTH), ("id", gs.BUF_SORTED_ID), ("ranges", gs.BUF_RANGES))


def renderer(sc, w, h, record_timings=1, count=gs.GS_COUNT_PER_PASS, **constants):
    r = gs.Renderer(w, h, warmup_frames=0, sort_algorithm=gs.GS_SORT_RADIX4, record_timings=record_timings, count_launches=count,
                    **constants)
    r.init(sc.getResourceManager())
    r.initForScene(sc)
    return r


def oracle_ref(oracle, key, sc, w, h, constants=None):
    """oracle.full_pipeline of the scene under its camera and constants, with keys and element counts per splat; cached by key."""
    def make():
        cam = sc.getCamera()
        p = oracle.make_params(w, h, cam.getViewMatrix(), cam.getProjectionMatrix(), cam.getPosition(), sh_mode=int(cam.getShMode()))
        for k, v in (constants or {}).items():
            setattr(p, k, v)
        ref = oracle.full_pipeline(p, sc.getResourceManager().getGaussians())
        return with_counts(ref)
    return cached(("pass0_ref", key), make)


def with_counts(ref):
    sp = ref["stage1"]["splats"]
    ref["keys"] = sp["depth_key"]
    ref["counts"] = np.where(sp["visible"] != 0, (sp["max_x"] - sp["min_x"]).astype(np.int64) * (sp["max_y"] - sp["min_y"]).astype(np.int64), 0)
    return ref


def table_of(r):
    return r.debugRead(gs.BUF_PASS0_OFFSETS)


def no_table(r):
    with pytest.raises(gs.GsplatError) as e:
        table_of(r)
    assert e.value.code == GS_ERR_INVALID


def products(r, sc):
    out = dict(image=r.draw(sc).copy(), status=r.lastStatus)
    for name, which in LISTS:
        out[name] = r.debugRead(which)
    t = r.timings()
    out["counts"] = (t.num_sort_elements, t.emitted_elements, t.overflowed)
    return out


def check(fused, plain, sc, ref, pixels=True):
    """One frame on both contexts: the table, the oracle, each other.  -> the products of the context under test."""
    a, b = products(fused, sc), products(plain, sc)
    e, counter = ref["e"], ref["stage1"]["counter"]
    over = counter > ref["stage1"]["capacity"]
    if over:
        no_table(fused)
    else:
        assert np.array_equal(table_of(fused), pass0_table(ref["keys"], ref["counts"]))
    no_table(plain)
    assert a["counts"] == b["counts"] == (e, counter, int(over)) and a["status"] == b["status"] == (gs.GS_WARN_OVERFLOW if over else gs.GS_OK)
    for name, _ in LISTS:
        want = ref[name] if name == "ranges" else ref[name][:e]
        assert np.array_equal(a[name], want), name
        assert np.array_equal(a[name], b[name]), name
    assert np.array_equal(a["image"], b["image"])
    if pixels:
        assert np.array_equal(a["image"], ref["image"])
    return a


@pytest.mark.parametrize("name", ["mixed", "mixed_far", "n257", "one_digit", "alternating", "heavy", "holes", "nothing"])
def test_designed_scene(oracle_mod, name):
    """Cases 1 - 6 of the scene list: sixteen digits mixed in every block (default planes, and far_plane = 10000), a second block of one
    splat, one digit, two digits alternating, a block of 9984 elements in three slices between light ones, empty blocks, nothing."""
    aos, w, h, constants = scene(oracle_mod, name)
    sc = make_scene(aos, w, h)
    ref = oracle_ref(oracle_mod, name, sc, w, h, constants)
    fused, plain = renderer(sc, w, h, **constants), renderer(sc, w, h, record_timings=2, **constants)
    for _ in range(2):                                  # the second frame replays the captured chain
        check(fused, plain, sc, ref)
    if name == "one_digit":
        t = table_of(fused)
        assert np.count_nonzero(t[:-1].any(axis=0)) == 1 and set(t[-1].tolist()) <= {0, ref["e"]}
    fused.cleanup()
    plain.cleanup()


@pytest.mark.parametrize("delta", OVERFLOWS, ids=[str(d) for d in OVERFLOWS])
def test_overflow(oracle_mod, delta):
    """Case 7: the recipe of test_overflow_truncates_like_reference as it is, trimmed to capacity - 1, capacity and capacity + 1, and
    with a whole-frame splat across the capacity between splats of other digits."""
    aos = overflow_scene(oracle_mod, delta)
    sc = make_scene(aos, OW, OH)
    ref = oracle_ref(oracle_mod, ("overflow", delta), sc, OW, OH)
    assert (ref["stage1"]["counter"] > ref["stage1"]["capacity"]) == (delta not in (-1, 0))
    fused, plain = renderer(sc, OW, OH), renderer(sc, OW, OH, record_timings=2)
    for _ in range(2):
        check(fused, plain, sc, ref)
    fused.cleanup()
    plain.cleanup()


def test_more_than_65535_tiles(oracle_mod):
    """Case 8: 257 x 256 tiles, 32-bit tile words, the unpacked layouts of pass 0."""
    aos, w, h, _ = wide_scene(oracle_mod)
    ref = with_counts(dict(wide_frame(oracle_mod)))
    sc = make_scene(aos, w, h)
    r = renderer(sc, w, h)
    info = r.sceneInfo()
    assert (info.capacity, info.tile_word_bytes) == (WIDE_CAPACITY, 4)
    a = products(r, sc)
    assert np.array_equal(table_of(r), pass0_table(ref["keys"], ref["counts"]))
    e = ref["e"]
    assert a["counts"] == (e, ref["stage1"]["counter"], 0)
    for name, _ in LISTS:
        assert np.array_equal(a[name], ref[name] if name == "ranges" else ref[name][:e]), name
    assert np.array_equal(a["image"], ref["image"])
    r.cleanup()


def test_one_context_several_frames(oracle_mod):
    """Case 9: poses A, B, A through one context (the captured chain replays over the rows an earlier frame left), fed counts on a
    second context, a band of tile rows and back."""
    aos, w, h, _ = scene(oracle_mod, "mixed")
    poses = dict(A=make_scene(aos, w, h), B=make_scene(aos, w, h, pos=(0.03, -0.02, -0.05), yaw=0.15, pitch=-0.1))
    refs = {k: oracle_ref(oracle_mod, ("mixed", k), sc, w, h) for k, sc in poses.items()}
    assert not np.array_equal(pass0_table(refs["A"]["keys"], refs["A"]["counts"]), pass0_table(refs["B"]["keys"], refs["B"]["counts"]))
    fused, plain, fed = renderer(poses["A"], w, h), renderer(poses["A"], w, h, record_timings=2), renderer(poses["A"], w, h, count=gs.GS_COUNT_FED)
    for k in "ABA":
        a = check(fused, plain, poses[k], refs[k])
        b = products(fed, poses[k])
        no_table(fed)
        assert all(np.array_equal(a[name], b[name]) for name in ("tile", "depth", "id", "ranges", "image")) and a["counts"] == b["counts"]
    gh = fused.sceneInfo().tiles_y
    fused.setTileRows(3, 9)
    band = fused.draw(poses["A"])
    no_table(fused)
    assert np.array_equal(band[48:144], refs["A"]["image"][48:144])
    fused.setTileRows(0, gh)
    check(fused, plain, poses["A"], refs["A"])
    for r in (fused, plain, fed):
        r.cleanup()


INSTANCES = [(sh, aa, depth) for sh in (SH.ONLY_FIRST_BAND, SH.DEGREE_1, SH.DEGREE_2, SH.ALL_BANDS)
             for aa, depth in ((False, False), (True, True))] + [(SH.ALL_BANDS, True, False), (SH.ALL_BANDS, False, True)]


@pytest.mark.parametrize("sh_mode,antialias,depth", INSTANCES)
def test_every_project_instantiation(oracle_mod, sh_mode, antialias, depth):
    """Case 10: SH degree 0 - 3, anti-alias on, the depth output on, on the scene of case 1.  The lists and the table do not depend on
    colour or opacity; the pixels are compared with the oracle's where it draws the same frame (no anti-alias, a mode it knows)."""
    aos, w, h, _ = scene(oracle_mod, "mixed")
    known = sh_mode in (SH.ONLY_FIRST_BAND, SH.ALL_BANDS)
    sc = make_scene(aos, w, h, sh_mode=int(sh_mode))
    ref = oracle_ref(oracle_mod, ("mixed", "sh", int(sh_mode) if known else 0), make_scene(aos, w, h, sh_mode=int(sh_mode) if known else 0), w, h)
    fused, plain = renderer(sc, w, h), renderer(sc, w, h, record_timings=2)
    for r in (fused, plain):
        r.setAntialias(antialias)
        r.setOutputs(depth=depth)
    check(fused, plain, sc, ref, pixels=known and not antialias)
    if depth:
        assert np.array_equal(fused.readOutput(gs.GS_OUTPUT_DEPTH).view(np.uint32), plain.readOutput(gs.GS_OUTPUT_DEPTH).view(np.uint32))
    fused.cleanup()
    plain.cleanup()
