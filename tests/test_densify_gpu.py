"""Adaptive density control on the MI355X (include/gsplat.h): gs_densify_stats_device against the float64 reference of the
screen gradient and the radius NumPy computes from GS_BUF_COV, gs_densify_device bit for bit against the NumPy restatement
(tests/test_densify_cpu.py) on the designed statistics array at n = 1, 255, 256, 257 and 70 000, the refusals of both, and
autograd.VisibleAdam(track_density=True).densify() end to end."""
import ctypes as C
import functools

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_parity_gpu import ALL_SORTS, make_renderer, make_scene
from test_outputs_cpu import SCENES, camera_params, load_scene
from test_backward_cpu import (check_overflowing, frozen_of, list_offsets, overflow_tiles, overflowing_scene,
                               sampled_decisions, tile_weights)
from frame64 import frame_decisions, weights
from test_backward_fullsize_gpu import oracle_list
from test_adam_gpu import frame_state
from test_train_chain_gpu import LAMBDA, bits, new_renderer
from test_densify_cpu import (D, DEFAULTS, DESIGN, DESIGN_PARAMS, VARIANTS, densify_ref, screen_gradient, screen_norm,
                              variant_inputs)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = np.float32
DEV = "cuda:0"


def up(a):
    """A host array on the device, bits kept whatever they spell (uint32 / float32 as int32 storage)."""
    a = np.ascontiguousarray(a)
    return torch.tensor(a.view(np.int32) if a.dtype.itemsize == 4 else a, device=DEV)


def down(t, dtype):
    return t.cpu().numpy().view(dtype)


# ---- 1. the statistics ------------------------------------------------------------------------------------------------------

def radius_of(cov):
    """ceilf(3 sqrtf(max(lambda0, lambda1))) of the frame's 2-D covariances (GS_BUF_COV), in float32 as k_project writes it."""
    c0, c1, c2 = (cov[:, k].astype(F) for k in range(3))
    with np.errstate(invalid="ignore"):
        det = c0 * c2 - c1 * c1
        m = (c0 + c2) * F(0.5)
        d = m * m - det
        root = np.sqrt(np.where(d > 0, d, F(0)))
        l0, l1 = m + root, m - root
        return np.ceil(F(3) * np.sqrt(np.where(l0 > l1, l0, l1))).astype(F)


class Frame:
    """A drawn frame with the visible-row backward done on it: the renderer, and ids / rows / count on the device."""

    def __init__(self, aos, w, h, cam=None, sort=gs.GS_SORT_RADIX4, seed=1, grads=None, sc=None, constants=None):
        """sc: a scene with a camera of its own instead of make_scene(aos, w, h, **cam); constants: Renderer's camera constants."""
        self.n, self.w, self.h = len(aos), w, h
        self.sc = sc if sc is not None else make_scene(aos, w, h, **(cam or {}))
        self.r = make_renderer(self.sc, w, h, sort=sort, **(constants or {}))
        self.r.draw(self.sc)
        self.wr, self.wd = grads if grads is not None else weights(h, w, seed)
        self.g_rgba, self.g_depth = up(self.wr), up(self.wd)
        self.ids = torch.full((self.n,), -1, dtype=torch.int32, device=DEV)
        self.rows = torch.zeros(self.n, 84, device=DEV)
        self.count = torch.zeros(1, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        self.backward()

    def backward(self):
        self.r.backwardVisibleDevice(self.g_rgba.data_ptr(), self.g_depth.data_ptr(), self.ids.data_ptr(), self.rows.data_ptr(),
                                     self.n, self.count.data_ptr())

    def stats(self, arrays, max_rows=None, ids=None, count=None, n=None):
        a, s, m = arrays
        self.r.densifyStatsDevice((ids if ids is not None else self.ids).data_ptr(),
                                  (count if count is not None else self.count).data_ptr(),
                                  self.n if max_rows is None else max_rows, self.n if n is None else n,
                                  a.data_ptr(), s.data_ptr(), m.data_ptr())
        self.r.synchronize()
        return down(a, F), down(s, np.uint32), down(m, F)

    def visible(self):
        self.r.synchronize()
        k = int(down(self.count, np.uint32)[0])
        return down(self.ids, np.uint32)[:k].astype(np.int64)


def zeros(n):
    a = (torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, device=DEV))
    torch.cuda.synchronize()
    return a


def sentinels(n):
    a = (torch.full((n,), 7.5, device=DEV), torch.full((n,), 11, dtype=torch.int32, device=DEV), torch.full((n,), -1.0, device=DEV))
    torch.cuda.synchronize()
    return a


def assert_norm(got, want, keep, what):
    """compare_with_reference's bound on the one column: |got - want| <= 2e-2 |want| + 2e-3 max|want| on the splats `keep`."""
    a, b = got[keep].astype(np.float64), want[keep]
    scale = np.abs(b).max()
    assert scale > 0, what
    tol = 2e-2 * np.abs(b) + 2e-3 * scale
    print(f"{what}: worst |gpu - ref| / tolerance {float((np.abs(a - b) / tol).max()):.4f} over {int(keep.sum())} splats")
    assert np.all(np.abs(a - b) <= tol), (what, int(np.argmax(np.abs(a - b) - tol)))


@pytest.mark.parametrize("scene", ["ragged", "dense", "ragged@pose"])
def test_stats_after_one_step(oracle_mod, tmp_path, scene):
    """One call from zeros: seen is 1 exactly on V (the oracle's splats with a non-empty tile box) and 0 elsewhere;
    max_radius equals, bit for bit, the radius NumPy computes from GS_BUF_COV on V and is 0 elsewhere; grad_accum is the norm
    of the float64 screen gradient in NDC units within the gradient tolerance, exactly 0 outside V.  A second call on the
    same frame gives fl(a + a), seen == 2 and the same radius."""
    aos, w, h, cam = load_scene(scene)
    f = Frame(aos, w, h, cam)
    arrays = zeros(f.n)
    accum, seen, radius = (a.copy() for a in f.stats(arrays))
    cov = f.r.debugRead(gs.BUF_COV)
    accum2, seen2, radius2 = f.stats(arrays)
    V = f.visible()
    f.r.cleanup()
    p = camera_params(oracle_mod, f.sc, w, h)
    ref, flags = frame_decisions(tmp_path, p, aos)
    touched, _ = list_offsets(ref)
    assert np.array_equal(V, np.flatnonzero(touched != 0)) and 500 < len(V) <= f.n
    inV = np.zeros(f.n, bool)
    inV[V] = True
    assert np.array_equal(seen, inV.astype(np.uint32))
    want_r = radius_of(cov)
    assert np.array_equal(bits(radius[inV]), bits(want_r[inV])) and not bits(radius[~inV]).any()
    assert radius[inV].min() >= 1 and len(np.unique(radius[inV])) > 5
    fz = frozen_of(scene.partition("@")[0], aos)
    ds, _ = screen_gradient(p, aos, ref, flags, f.wr.astype(np.float64), f.wd.astype(np.float64), fz if fz.any() else None)
    want = screen_norm(ds, w, h)
    assert not bits(accum[~inV]).any() and np.all(np.isfinite(accum)) and np.all(accum >= 0)
    assert np.count_nonzero(want) > 100
    assert_norm(accum, want, ~fz, scene)
    assert np.array_equal(bits(accum2), bits(accum + accum)) and np.array_equal(seen2, 2 * seen)
    assert np.array_equal(bits(radius2), bits(radius))


def test_stats_zero_det_excludes_the_needles(oracle_mod, tmp_path):
    """The zero_det scene: the frozen needles (a float32 determinant dominated by rounding) are not compared, as in
    tests/test_backward_gpu.py; every other splat is within the tolerance."""
    aos, w, h, cam = load_scene("zero_det")
    f = Frame(aos, w, h, cam)
    accum, seen, radius = f.stats(zeros(f.n))
    f.r.cleanup()
    p = camera_params(oracle_mod, f.sc, w, h)
    ref, flags = frame_decisions(tmp_path, p, aos)
    fz = frozen_of("zero_det", aos)
    ds, _ = screen_gradient(p, aos, ref, flags, f.wr.astype(np.float64), f.wd.astype(np.float64), fz)
    assert_norm(accum, screen_norm(ds, w, h), ~fz, "zero_det")


def test_stats_on_the_overflowing_scene(oracle_mod, tmp_path):
    """overflowing_scene of tests/test_backward_cpu.py (800 000 frame-filling splats, element counter past 2^32): seen is 1
    on every splat with a tile box, also on those wholly past the capacity, whose accumulator stays exactly 0 (their slots
    are not elements of the list: offsets saturate); the splat the capacity cuts sums its surviving rows only; by value on
    the union of the sampled tiles' lists against the float64 screen gradient under tile weights."""
    aos, w, h = overflowing_scene()
    sc = make_scene(aos, w, h)
    p = camera_params(oracle_mod, sc, w, h)
    gw, gh = oracle_mod.grid(w, h)
    s1, e, ot, od, oi, oranges = oracle_list(oracle_mod, p, aos, want_splats=True)
    across, past, victims = check_overflowing(s1)
    tiles = overflow_tiles(oranges, gw, gh, ot[:e], oi[:e], across)
    sub_ids, sub_ranges, flags = sampled_decisions(tmp_path, p, aos, s1, oi[:e], oranges, tiles)
    twr, twd = tile_weights(w, h, tiles, seed=4)
    uniq, inverse = np.unique(sub_ids, return_inverse=True)
    sub = dict(stage1=dict(color=np.asarray(s1["color"])[uniq], cov=np.asarray(s1["cov"])[uniq]), id=inverse.reshape(-1),
               ranges=sub_ranges, e=len(sub_ids))
    ds, _ = screen_gradient(p, aos[uniq], sub, flags, twr.astype(np.float64), twd.astype(np.float64))
    want = screen_norm(ds, w, h)
    f = Frame(aos, w, h, grads=(twr, twd))
    assert f.r.lastStatus == gs.GS_WARN_OVERFLOW
    accum, seen, radius = f.stats(zeros(f.n))
    V = f.visible()
    f.r.cleanup()
    touched, _ = list_offsets(dict(stage1=s1))
    assert np.array_equal(V, np.flatnonzero(touched != 0))
    assert np.array_equal(seen, (touched != 0).astype(np.uint32)) and np.all(seen[past] == 1)
    assert not bits(accum[past]).any() and not bits(accum[victims]).any()
    outside = np.ones(f.n, bool)
    outside[uniq] = False
    assert not bits(accum[outside]).any() and accum[across] != 0 and np.count_nonzero(want) >= 500
    assert np.all(radius[touched != 0] >= 1)
    assert_norm(accum[uniq], want, np.ones(len(uniq), bool), "past 2^32")


def test_stats_bits_do_not_depend_on_the_sorter():
    aos, w, h = SCENES["ragged"]()
    first = None
    for sort in ALL_SORTS:
        f = Frame(aos, w, h, sort=sort)
        got = [a.copy() for a in f.stats(zeros(f.n))]
        f.r.cleanup()
        if first is None:
            first = got
            assert first[0].any()
        else:
            for a, b in zip(got, first):
                assert np.array_equal(bits(a), bits(b)), sort


def test_stats_max_rows_and_foreign_ids():
    """With max_rows < |V| only the first max_rows ids move (sentinels elsewhere keep their bits); a count below max_rows
    stops the list; an id >= n is skipped; max_rows == 0 launches nothing and takes NULL pointers."""
    aos, w, h = SCENES["ragged"]()
    f = Frame(aos, w, h)
    V = f.visible()
    full = [a.copy() for a in f.stats(zeros(f.n))]
    for max_rows, count in ((100, None), (257, None), (len(V) + 50, 300), (0, None)):
        arrays = sentinels(f.n + 8)                                  # 8 guard entries behind n
        cnt = None if count is None else up(np.array([count], np.uint32))
        torch.cuda.synchronize()
        accum, seen, radius = f.stats(arrays, max_rows=max_rows, count=cnt)
        k = min(max_rows, len(V) if count is None else count)
        moved = np.zeros(f.n + 8, bool)
        moved[V[:k]] = True
        assert np.all(accum[~moved] == F(7.5)) and np.all(seen[~moved] == 11) and np.all(radius[~moved] == F(-1)), max_rows
        assert np.array_equal(bits(accum[moved]), bits(F(7.5) + full[0][V[:k]])) and np.all(seen[moved] == 12), max_rows
        assert np.array_equal(bits(radius[moved]), bits(full[2][V[:k]])), max_rows
    L = _lib.lib()
    assert L.gs_densify_stats_device(f.r._ctx.handle, None, None, 0, f.n, None, None, None) == _lib.GS_OK
    a, b = int(V[3]), int(V[40])
    ids = up(np.array([a, f.n, b, 0xFFFFFFFF, f.n + 1, int(V[41])], np.uint32))
    cnt = up(np.array([5], np.uint32))
    arrays = sentinels(f.n + 8)
    accum, seen, radius = f.stats(arrays, max_rows=6, ids=ids, count=cnt)
    moved = np.zeros(f.n + 8, bool)
    moved[[a, b]] = True
    assert np.all(seen[moved] == 12) and np.all(seen[~moved] == 11) and np.all(accum[~moved] == F(7.5)) and np.all(radius[~moved] == F(-1))
    f.r.cleanup()


def test_stats_refusals():
    """Nothing is enqueued by a refused call: after gs_visible_count alone, after a new frame without a backward, after an
    upload (in place, in full and of rows), with a NULL pointer, with an n other than the scene's; and what gs_backward
    refuses (a FAST context) with its message."""
    aos, w, h = SCENES["dense"]()
    aos = np.ascontiguousarray(aos, F)
    sc = make_scene(aos, w, h)
    r = make_renderer(sc, w, h)
    n, L = len(aos), _lib.lib()
    hdl = r._ctx.handle
    accum, seen, radius = arrays = sentinels(n)
    ids = torch.zeros(n, dtype=torch.int32, device=DEV)
    rows = torch.zeros(n, 84, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    grad, d_aos = up(weights(h, w, 2)[0]), up(aos)
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def stats(i=ids, c=count, max_rows=n, nn=n, a=accum, s=seen, m=radius):
        return L.gs_densify_stats_device(hdl, vp(i), vp(c), max_rows, nn, vp(a), vp(s), vp(m))

    def refused(rc, word):
        msg = L.gs_last_error(hdl).decode()
        assert rc == _lib.GS_ERR_INVALID and word in msg, (rc, word, msg)

    def backward():
        r.backwardVisibleDevice(grad.data_ptr(), None, ids.data_ptr(), rows.data_ptr(), n, count.data_ptr())

    refused(stats(), "no frame since")                                       # no frame at all
    r.draw(sc)
    refused(stats(), "no gs_backward* on this frame")
    assert r.visibleCount() > 0
    refused(stats(), "no gs_backward* on this frame")                        # the scan alone wrote no rows
    backward()
    assert stats() == _lib.GS_OK
    r.draw(sc)
    refused(stats(), "no gs_backward* on this frame")                        # a new frame, no backward
    backward()
    r.uploadDevice(d_aos.data_ptr(), n)
    refused(stats(), "no frame since")                                       # an upload
    r.draw(sc); backward()
    r.uploadRowsDevice(d_aos.data_ptr(), n, ids.data_ptr(), count.data_ptr(), n)
    refused(stats(), "no frame since")
    r.draw(sc); backward()
    for k in ("i", "c", "a", "s", "m"):
        refused(stats(**{k: None}), "gs_densify_stats_device: null")
    refused(stats(nn=n - 1), "n differs from the scene's")
    refused(stats(nn=n + 1), "n differs from the scene's")
    r.synchronize()
    listed = down(ids, np.uint32)[:int(down(count, np.uint32)[0])]
    assert np.count_nonzero(down(seen, np.uint32) == 12) == len(listed) and np.all(down(seen, np.uint32)[listed] == 12)   # the one valid call
    assert np.count_nonzero(down(seen, np.uint32) == 11) == n - len(listed)
    assert stats() == _lib.GS_OK                                             # a refusal costs the frame nothing
    assert r.backward(weights(h, w, 2)[0]).any()                             # the dense form sets the flag too
    assert stats() == _lib.GS_OK
    r.synchronize()
    assert np.all(down(seen, np.uint32)[down(ids, np.uint32)[:5]] == 14)
    r.cleanup()
    fast = make_renderer(sc, w, h, mode=gs.GS_RENDER_FAST)
    fast.draw(sc)
    hdl = fast._ctx.handle
    refused(stats(), "only GS_RENDER_EXACT frames can be differentiated")
    fast.cleanup()


# ---- 2. the new cloud -------------------------------------------------------------------------------------------------------

GUARD = 3                      # sentinel rows behind max_out
SENT = F(-12345.5)


@pytest.fixture(scope="module")
def bare():
    """A context without a scene and without a resolution: all gs_densify_device needs."""
    r = gs.Renderer(64, 64, record_timings=False)
    r.init(gs.ResourceManager())
    yield r
    r.cleanup()


@functools.lru_cache(maxsize=None)
def case(name, n):
    """Inputs and the restatement's answer; float 83 of record g carries g, so that every output row names its parent."""
    rec, m, v, st = variant_inputs(name, n)
    rec.view(np.uint32)[:, 83] = np.arange(n)
    ref = densify_ref(rec, m, v, st, VARIANTS[name])
    for a in (rec, m, v, *st.values(), *(x for x in ref.values() if isinstance(x, np.ndarray))):
        a.setflags(write=False)
    return rec, m, v, st, ref


def run_densify(r, rec, m, v, st, params, max_out, moments=True):
    """gs_densify_device on device copies; returns (records_out, m_out, v_out [max_out + GUARD, 84], counts [4])."""
    n = len(rec)
    d = [up(rec), up(m), up(v), up(st["grad_accum"]), up(st["seen"]), up(st["max_radius"])]
    outs = [torch.full((max_out + GUARD, 84), float(SENT), device=DEV) for _ in range(3)]
    counts = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    p = gs.default_densify_params(**params)
    ptr = lambda t: t.data_ptr()
    r.densifyDevice(ptr(d[0]), ptr(d[1]) if moments else None, ptr(d[2]) if moments else None, n, ptr(d[3]), ptr(d[4]), ptr(d[5]), p,
                    ptr(outs[0]), ptr(outs[1]) if moments else None, ptr(outs[2]) if moments else None, max_out, ptr(counts))
    r.synchronize()
    for t, a in zip(d, (rec, m, v, st["grad_accum"], st["seen"], st["max_radius"])):
        assert np.array_equal(t.cpu().numpy().view(np.uint32).reshape(-1), bits(a).reshape(-1))      # the inputs are only read
    return [down(o, F) for o in outs] + [down(counts, np.uint32)]


def position_error(got, ref, rows):
    """max over the children `rows` of |pos - ref| / (2e-5 sum_k |R[i][k] s[k]| + 4 ulp(pos)); NaN positions (a NaN scale) must be
    NaN in both."""
    want, bound = ref["pos64"][rows], ref["bound"][rows]
    g = got[rows, 0:3].astype(np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(g), nan)
    tol = 2e-5 * bound + 4 * np.spacing(np.abs(want).astype(F)).astype(np.float64)
    return float((np.abs(g - want)[~nan] / tol[~nan]).max()) if (~nan).any() else 0.0


def assert_equals_ref(got, ref, n, max_out, moments=True):
    """The outputs below min(n_out, max_out) against the restatement, the sentinels behind them; returns the position error."""
    rec_o, m_o, v_o, counts = got
    assert tuple(int(c) for c in counts) == ref["counts"]
    n_out = ref["counts"][0]
    k = min(n_out, max_out)
    for a in (rec_o, m_o, v_o):
        assert np.all(a[k:] == SENT)
    if not moments:
        assert np.all(m_o == SENT) and np.all(v_o == SENT)
    parent, child = ref["parent"][:k], ref["child"][:k]
    # stable: every row names its parent, the k(g) outputs of g before those of g + 1
    assert np.array_equal(bits(rec_o[:k])[:, 83], parent.astype(np.uint32))
    plain = child < 0
    assert np.array_equal(bits(rec_o[:k][plain]), bits(ref["records"][:k][plain]))
    kids, want_kids = rec_o[:k][~plain], ref["records"][:k][~plain]
    rest = np.r_[3, 7:84]                                            # everything but the position and the scale
    assert np.array_equal(bits(kids[:, rest]), bits(want_kids[:, rest]))
    nan = np.isnan(want_kids[:, 4:7])                                # (the quotient of a NaN scale is a NaN: its payload is no contract)
    assert np.array_equal(np.isnan(kids[:, 4:7]), nan) and np.array_equal(bits(kids[:, 4:7])[~nan], bits(want_kids[:, 4:7])[~nan])
    if moments:
        assert np.array_equal(bits(m_o[:k]), bits(ref["m"][:k])) and np.array_equal(bits(v_o[:k]), bits(ref["v"][:k]))
    rows = np.flatnonzero(~plain)
    err = position_error(rec_o, ref, rows) if len(rows) else 0.0
    assert err <= 1.0, err
    return err


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70_000, 262_144, 262_145])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_densify_against_the_restatement(bare, name, n):
    """The designed statistics array tiled over n records -- 1, 255, 256: one block of 256 splats, part and full; 257: two blocks;
    70 000: 274 blocks, one for each of the first 274 of the 1024 threads of the one-workgroup scan, the other threads idle;
    262 144: 1024 blocks, one per thread, none idle; 262 145: 1025 blocks, so two per thread, and the upper half of the threads
    own nothing --
    as designed and with parameters that keep, prune or split every splat: the four counts, every kept and cloned record,
    the m and v rows (copies and zeros), the children's scales and every float of theirs but the position bit for bit, the
    order stable, the sentinel rows behind the outputs intact, the inputs unchanged.  Child positions within
    2e-5 sum_k |R[i][k] s[k]| + 4 ulp(pos) of the float64 restatement (about five times what a cosine argument rounded to
    float32 at 2 pi, 5e-7 absolute, costs a draw of radius 5.77).  Measured on an MI355X, the worst ratio to that bound:
    0.30 (all_split, n = 70 000: 140 000 children), 0.11 (designed, n = 70 000), 0.08 (designed, n = 255 .. 257)."""
    rec, m, v, st, ref = case(name, n)
    got = run_densify(bare, rec, m, v, st, VARIANTS[name], 2 * n)
    err = assert_equals_ref(got, ref, n, 2 * n)
    print(f"{name} n {n}: counts {ref['counts']}, worst child position error / bound {err:.4f}")
    want = {"all_kept": (n, 0, 0, 0), "all_pruned": (0, 0, 0, n), "all_split": (2 * n, 0, n, 0)}.get(name)
    assert want is None or ref["counts"] == want
    if name == "designed" and n >= D:
        assert min(ref["counts"][1:]) >= 3 and {d[2] for d in DESIGN} == set(ref["kind"][:D].tolist())


def test_densify_capacity_seed_and_null_moments(bare):
    """max_out at n_out - 1 and at 0: nothing at or past the cut is written and counts_out[0] is not truncated.  The same
    seed gives the same bits; another seed (either half) changes child positions and nothing else.  With m, v, m_out and
    v_out NULL the records are the same."""
    n = 257
    rec, m, v, st, ref = case("designed", n)
    n_out = ref["counts"][0]
    base = run_densify(bare, rec, m, v, st, DESIGN_PARAMS, 2 * n)
    for max_out in (n_out - 1, n_out, 0, 1):
        assert_equals_ref(run_densify(bare, rec, m, v, st, DESIGN_PARAMS, max_out), ref, n, max_out)
    again = run_densify(bare, rec, m, v, st, DESIGN_PARAMS, 2 * n)
    for a, b in zip(again, base):
        assert np.array_equal(bits(a), bits(b))
    children = np.flatnonzero(ref["child"] >= 0)
    finite = children[~np.isnan(ref["pos64"][children]).any(1)]
    for seed in (DESIGN_PARAMS["seed"] ^ 1, DESIGN_PARAMS["seed"] ^ (1 << 32)):
        other = run_densify(bare, rec, m, v, st, dict(DESIGN_PARAMS, seed=seed), 2 * n)
        differ = bits(other[0]) != bits(base[0])
        assert np.all(differ[finite, 0:3].any(1)) and not differ[:, 3:].any()
        assert set(np.flatnonzero(differ.any(1)).tolist()) <= set(children.tolist())
        for k in (1, 2, 3):
            assert np.array_equal(bits(other[k]), bits(base[k]))
        assert_equals_ref(other, densify_ref(rec, m, v, st, dict(DESIGN_PARAMS, seed=seed)), n, 2 * n)
    alone = run_densify(bare, rec, m, v, st, DESIGN_PARAMS, 2 * n, moments=False)
    assert np.array_equal(bits(alone[0]), bits(base[0])) and np.array_equal(alone[3], base[3])
    assert_equals_ref(alone, ref, n, 2 * n, moments=False)


def test_densify_refusals(bare):
    """Every refusal of the header returns GS_ERR_INVALID with a message and enqueues nothing; a valid call afterwards works."""
    n = 40
    rec, m, v, st, ref = case("designed", n)
    L, hdl = _lib.lib(), bare._ctx.handle
    d = dict(rec=up(rec), m=up(m), v=up(v), a=up(st["grad_accum"]), s=up(st["seen"]), r=up(st["max_radius"]),
             rec_o=torch.full((2 * n, 84), float(SENT), device=DEV), m_o=torch.full((2 * n, 84), float(SENT), device=DEV),
             v_o=torch.full((2 * n, 84), float(SENT), device=DEV), c=torch.full((4,), -1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    vp = lambda x: None if x is None else C.c_void_p(x if isinstance(x, int) else x.data_ptr())

    def call(p=None, n_=n, max_out=2 * n, null_params=False, **swap):
        a = dict(d, **swap)
        p = gs.default_densify_params(**DESIGN_PARAMS) if p is None else p
        return L.gs_densify_device(hdl, vp(a["rec"]), vp(a["m"]), vp(a["v"]), n_, vp(a["a"]), vp(a["s"]), vp(a["r"]),
                                   None if null_params else C.byref(p), vp(a["rec_o"]), vp(a["m_o"]), vp(a["v_o"]), max_out, vp(a["c"]))

    def refused(rc, word):
        msg = L.gs_last_error(hdl).decode()
        assert rc == _lib.GS_ERR_INVALID and word in msg, (rc, word, msg)

    for k in ("rec", "a", "s", "r", "c"):
        refused(call(**{k: None}), "gs_densify_device: null")
    refused(call(rec_o=None), "null records_out")
    refused(call(null_params=True), "null gs_densify_params")
    refused(call(n_=0), "n is 0")
    refused(call(n_=1 << 31), "below 2^31")
    for size in (0, 36, 44):
        p = gs.default_densify_params()
        p.struct_size = size
        refused(call(p), "struct_size")
    refused(call(gs.default_densify_params(grad_threshold=float("nan"))), "grad_threshold")
    for bad in (0.0, -1.6, float("nan")):
        refused(call(gs.default_densify_params(split_shrink=bad)), "split_shrink")
    for part in (("m",), ("v",), ("m_o",), ("v_o",), ("m", "v"), ("m_o", "v_o"), ("m", "m_o")):
        refused(call(**{k: None for k in part}), "all together")
    refused(call(rec_o=d["rec"]), "aliases an input")
    refused(call(m_o=d["m"]), "aliases an input")
    refused(call(v_o=d["a"]), "aliases an input")
    refused(call(rec_o=d["rec"].data_ptr() + 336 * (n - 1)), "aliases an input")           # the last input row only
    refused(call(rec_o=d["rec"].data_ptr() - 336 * 2 * n + 4), "aliases an input")         # the first input float only
    refused(call(c=d["s"]), "aliases an input")
    refused(call(c=d["rec_o"]), "alias each other")
    refused(call(m_o=d["v_o"]), "alias each other")
    bare.synchronize()
    for k in ("rec_o", "m_o", "v_o"):
        assert np.all(down(d[k], F) == SENT)
    assert np.all(down(d["c"], np.int32) == -1)
    # adjacent is not aliased; max_out == 0 needs no output rows; infinite thresholds are parameters, not errors
    assert call(rec_o=d["rec"].data_ptr() + 336 * n, m_o=None, v_o=None, m=None, v=None, max_out=0) == _lib.GS_OK
    assert call(rec_o=None, m_o=None, v_o=None, max_out=0) == _lib.GS_OK
    assert call(gs.default_densify_params(grad_threshold=float("inf"), prune_opacity=float("-inf"))) == _lib.GS_OK
    assert call() == _lib.GS_OK
    bare.synchronize()
    assert tuple(down(d["c"], np.uint32).tolist()) == ref["counts"]
    assert np.array_equal(bits(down(d["m_o"], F)[:ref["counts"][0]]), bits(ref["m"]))


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------

STEPS_BEFORE = 4


def test_visible_adam_densifies():
    """VisibleAdam(track_density=True) on the dense scene: four steps gather the statistics (seen counts the steps a splat
    was rasterised in); densify() with thresholds taken from those statistics -- the median mean gradient of the seen splats,
    the median largest scale, the 98th percentile of the largest radius -- clones, splits and prunes, with the counts and
    the records, m and v of the restatement on the CPU; t and the hyper-parameters stay, the statistics restart from zero.
    A further step runs: its numbers and the records, m and v it leaves are the bits of a fresh VisibleAdam seeded with the
    same records, m, v and t, and the renderer's scene is the fresh full upload of the new records."""
    from vk3dgaussiansplatting_amd.autograd import VisibleAdam
    aos, w, h = SCENES["dense"]()
    aos = np.ascontiguousarray(aos, F)
    n = len(aos)
    rng = np.random.default_rng(3)
    truth = aos.copy()
    truth[:, 12:15] += 0.3 * rng.standard_normal((n, 3)).astype(F)
    truth[:, 0:3] += 0.01 * rng.standard_normal((n, 3)).astype(F)
    sc_truth, sc = make_scene(truth, w, h), make_scene(aos, w, h)
    r = new_renderer(sc_truth, w, h, gs.GS_SORT_RADIX4, False)
    r.draw(sc_truth)
    target = torch.tensor(np.ascontiguousarray(r.readOutput(gs.GS_OUTPUT_RGBA32F)[..., :3]), device=DEV)
    r.cleanup()
    cam = gs.Renderer._camera_args(sc.getCamera())
    r = new_renderer(sc, w, h, gs.GS_SORT_RADIX4, False)
    opt = VisibleAdam(torch.tensor(aos, device=DEV), renderer=r, track_density=True)
    for _ in range(STEPS_BEFORE):
        opt.step(*cam, target, LAMBDA)
    opt.stream.synchronize()
    st = dict(grad_accum=opt.grad_accum.cpu().numpy(), seen=opt.seen.cpu().numpy().view(np.uint32), max_radius=opt.max_radius.cpu().numpy())
    rec0, m0, v0 = (t.cpu().numpy() for t in (opt.records, opt.m, opt.v))
    was_seen = st["seen"] > 0
    assert 500 < was_seen.sum() < n and st["seen"].max() == STEPS_BEFORE and np.all(st["max_radius"][was_seen] >= 1)
    mean = st["grad_accum"][was_seen] / st["seen"][was_seen].astype(F)
    params = dict(grad_threshold=float(np.median(mean)), split_scale=float(np.median(rec0[:, 4:7].max(1))), prune_opacity=0.005,
                  prune_radius=float(np.percentile(st["max_radius"][was_seen], 98)), seed=2024)
    ref = densify_ref(rec0, m0, v0, st, dict(DEFAULTS, **params))
    assert min(ref["counts"][1:]) > 20, ref["counts"]                    # clone, split and prune all occur
    t_before = opt.t
    counts = opt.densify(**params)
    print(f"densify: {n} -> {counts}")
    assert counts == ref["counts"] and opt.t == t_before == STEPS_BEFORE
    n_out = counts[0]
    assert n_out != n and opt.records.shape == (n_out, 84) and opt.records.is_contiguous() and opt.max_rows == n_out
    assert opt.ids.shape == (n_out,) and opt.rows.shape == (n_out, 84) and opt.grad_accum.shape == (n_out,)
    assert not opt.grad_accum.any() and not opt.seen.any() and not opt.max_radius.any()
    got = [opt.records.cpu().numpy(), opt.m.cpu().numpy(), opt.v.cpu().numpy()]
    plain = ref["child"] < 0
    assert np.array_equal(bits(got[0][plain]), bits(ref["records"][plain]))
    assert np.array_equal(bits(got[0][~plain][:, 3:]), bits(ref["records"][~plain][:, 3:])) and not np.isnan(rec0).any()
    assert np.array_equal(bits(got[1]), bits(ref["m"])) and np.array_equal(bits(got[2]), bits(ref["v"]))
    assert position_error(got[0], ref, np.flatnonzero(~plain)) <= 1.0
    # the step after: against a fresh optimiser seeded with the same state
    R0, M0, V0 = opt.records.clone(), opt.m.clone(), opt.v.clone()
    torch.cuda.synchronize()
    numbers = opt.step(*cam, target, LAMBDA)
    opt.stream.synchronize()
    assert np.all(np.isfinite(numbers.cpu().numpy())) and opt.t == STEPS_BEFORE + 1
    assert int(opt.count.cpu()[0]) > 500 and opt.seen.sum().item() == int(opt.count.cpu()[0])
    r2 = new_renderer(sc, w, h, gs.GS_SORT_RADIX4, False)
    fresh = VisibleAdam(R0.clone(), renderer=r2, track_density=True)
    fresh.m.copy_(M0); fresh.v.copy_(V0); fresh.t = opt.t - 1
    torch.cuda.synchronize()
    numbers2 = fresh.step(*cam, target, LAMBDA)
    fresh.stream.synchronize()
    assert np.array_equal(bits(numbers.cpu().numpy()), bits(numbers2.cpu().numpy()))
    for a, b in ((opt.records, fresh.records), (opt.m, fresh.m), (opt.v, fresh.v), (opt.grad_accum, fresh.grad_accum)):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
    assert not np.array_equal(bits(opt.records.cpu().numpy()), bits(R0.cpu().numpy()))
    # the renderer's scene is R0, uploaded in full at that step: the same frame and buffers as a fresh upload of R0
    r.setStream(None)
    B = make_renderer(sc, w, h)
    B.uploadDevice(R0.data_ptr(), n_out)
    a, b = frame_state(r, sc), frame_state(B, sc)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name
    assert r.sceneInfo().num_gaussians == n_out == B.sceneInfo().num_gaussians
    r2.setStream(None)
    for x in (r, r2, B):
        x.cleanup()
