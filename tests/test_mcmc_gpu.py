"""The MCMC calls on the MI355X (include/gsplat.h): gs_relocate_device, gs_grow_device and gs_position_noise_device against
mcmc_ref (tests/test_mcmc_cpu.py) -- the sampler, the layouts, the counts and every untouched float bit for bit, the values
under the allowances derived below --, at the edges of the 64-bit scan, on designed clouds, twice and on two sorters, through
the frame, the refusals, and autograd.VisibleAdam.relocate / grow / add_noise."""
import functools

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_adam_cpu import UNTOUCHED
from test_backward_cpu import screen_splat, small_scene
from test_mcmc_cpu import F, mcmc_ref
from test_parity_gpu import make_renderer, make_scene
from test_raw_cpu import FLT_MIN, act_ref, random_raw
from test_raw_gpu import fields_equal
from test_train_chain_gpu import LAMBDA, bits, new_renderer
from test_trainer_calls_gpu import Recorder

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
MIN_OP = 0.005
SEED = 0x0123456789ABCDEF
SENTINEL = 0xFFC54321                 # a NaN with a payload, in the floats nothing reads and behind every output
SENTINEL_I32 = SENTINEL - (1 << 32)
VALUES = [4, 5, 6, 15]                # the floats a source changes
OTHERS = [c for c in range(84) if c not in VALUES]


def up(a):
    a = np.ascontiguousarray(a)
    return torch.tensor(a.view(np.int32) if a.dtype.itemsize == 4 else a, device=DEV)


def down(t, dtype=np.float32):
    return t.cpu().numpy().view(dtype)


def filled(shape, dtype=torch.float32):
    shape = shape if isinstance(shape, tuple) else (shape,)
    return torch.full(shape, SENTINEL_I32, dtype=torch.int32, device=DEV).view(dtype)


def make_context(sort=gs.GS_SORT_RADIX4):
    r = gs.Renderer(64, 64, sort_algorithm=sort, record_timings=False)
    r.init(gs.ResourceManager())
    return r


@pytest.fixture(scope="module")
def bare():
    """A context without a scene and without a resolution: all the MCMC calls need."""
    r = make_context()
    yield r
    r.cleanup()


# ---- clouds -----------------------------------------------------------------------------------------------------------------

def alive_mask(n, kind, rng):
    alive = np.zeros(n, bool)
    if kind == "edges":               # alive only at the block edges, runs of dead splats between them
        alive[[g for g in (0, 255, 256, 511, n - 1) if g < n]] = True
    elif kind == "mixed":
        alive = rng.random(n) >= 0.2
    elif kind == "one_alive":
        alive[17 % n] = True
    elif kind == "no_dead":
        alive[:] = True
    else:
        assert kind == "all_dead"
    return alive


@functools.lru_cache(maxsize=None)
def cloud(n, kind, space):
    """records (and raw, with records == act(raw) in the fields), m, v [n, 84]: ordinary rows, the opacity of an alive splat in
    (0.12, 0.97), of a dead one 3.4e-4; the sentinel in the 25 floats no call computes with, non-zero moments."""
    rng = np.random.default_rng(n * 7 + len(kind))
    alive = alive_mask(n, kind, rng)
    raw = random_raw(rng, n)
    raw[:, 15] = np.where(alive, rng.uniform(-2.0, 3.5, n), -8.0)
    rec = act_ref(raw, np.float32)
    m, v = (rng.standard_normal((n, 84)).astype(F) for _ in range(2))
    for a in (raw, rec, m, v):
        bits(a)[:, UNTOUCHED] = SENTINEL
    assert np.array_equal(rec[:, 15] > F(MIN_OP), alive)
    return rec, (raw if space == "raw" else None), m, v


def special_cloud():
    """Records space: an opacity equal to min_opacity (dead), a NaN (dead), 1.5 and 1 (alive, weight 2^24), 0 and -1 (dead), and
    the float next above min_opacity (alive)."""
    rec, _, m, v = cloud(300, "no_dead", "records")
    rec = rec.copy()
    rec[[0, 1, 2, 100, 255, 256, 299], 15] = [MIN_OP, np.nan, 1.5, 1.0, 0.0, -1.0, np.nextafter(F(MIN_OP), F(1))]
    return rec, None, m, v


# ---- the values of a source, under the allowances ---------------------------------------------------------------------------

def logf_bound(theta):
    """What tests/test_raw_gpu.py allows gs_raw_from_records_device for the device's logf: 2 ulp(theta) + 2^-22."""
    return 2 * np.spacing(np.abs(theta).astype(F)).astype(np.float64) + 2.0 ** -22


def check_values(old_rec, new_rec, new_raw, cnt, what):
    """old_rec: the sources' rows before [k, 84]; new_rec / new_raw: their rows after; cnt [k] > 0."""
    if len(cnt) == 0:
        return
    r = mcmc_ref.ratio(cnt)
    o_old, s_old = old_rec[:, 15], old_rec[:, 4:7]
    oc64 = mcmc_ref.opacity64(o_old, r, MIN_OP)
    got_o = new_rec[:, 15]
    if new_raw is None:
        # log1pf and expm1f are one ulp each, plus one division; |x| e^x / (1 - e^x) <= 1 for x <= 0 does not amplify the error
        # of the exponent: 8 * 2^-24 relative is about twice the sum
        err = np.abs(got_o.astype(np.float64) - oc64) / oc64
        print(f"{what}: worst opacity error {float(err.max()) / 2.0 ** -24:.2f} x 2^-24 (allowed 8)")
        assert np.all(err <= 8 * 2.0 ** -24)
    else:
        # the logit of an oc that is 8 * 2^-24 relative off moves by at most 8 * 2^-24 / (1 - oc): d logit / d oc = 1 / (oc (1 - oc))
        theta = np.log(oc64 / (1 - oc64))
        err = np.abs(new_raw[:, 15].astype(np.float64) - theta)
        tol = logf_bound(theta) + 8 * 2.0 ** -24 / (1 - oc64)
        print(f"{what}: worst logit error / allowance {float((err / tol).max()):.3f}")
        assert np.all(err <= tol)
    # the scales restated from the opacity bits the device stored: the recurrence has no transcendental in it
    s32, c = mcmc_ref.scales32(o_old, s_old, got_o, r)
    assert np.all(c > 0) and np.all(c[o_old <= 1] <= 1)
    if new_raw is None:
        assert np.array_equal(bits(new_rec[:, 4:7]), bits(s32)), what
    else:
        theta = np.log(np.maximum(s32, FLT_MIN).astype(np.float64))
        err = np.abs(new_raw[:, 4:7].astype(np.float64) - theta)
        print(f"{what}: worst log-scale error / allowance {float((err / logf_bound(theta)).max()):.3f}")
        assert np.all(err <= logf_bound(theta))
        fields_equal(new_rec, act_ref(new_raw, np.float32), (what, "records == act(raw)"))
    # act(logit(oc)) may round one ulp below an oc clamped at min_opacity: the bound holds for the value that was clamped
    assert np.all(got_o < np.minimum(o_old, 1.0)) and np.all(got_o >= F(MIN_OP) * (F(1) - F(2.0 ** -22) if new_raw is not None else 1))


# ---- gs_relocate_device -----------------------------------------------------------------------------------------------------

def run_relocate(r, arrays, seed=SEED, max_rows=None, min_opacity=MIN_OP):
    rec, raw, m, v = arrays
    n = len(rec)
    max_rows = n if max_rows is None else max_rows
    d = [None if a is None else up(a) for a in arrays]
    ids, counts = filled(max_rows + 4, torch.int32), filled(3, torch.int32)
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else t.data_ptr()
    r.relocateDevice(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), n, min_opacity, seed, ids.data_ptr() if max_rows else None,
                     max_rows, counts.data_ptr())
    r.synchronize()
    return [None if t is None else down(t) for t in d], down(ids, np.uint32), tuple(int(x) for x in down(counts, np.uint32))


def check_relocate(r, arrays, what, max_rows=None, seed=SEED):
    rec, raw, m, v = arrays
    n = len(rec)
    ref = mcmc_ref.relocate_ref(rec, MIN_OP, seed)
    (g_rec, g_raw, g_m, g_v), ids, counts = run_relocate(r, arrays, seed, max_rows)
    assert counts == ref.counts, (what, counts, ref.counts)
    k = min(counts[0], n if max_rows is None else max_rows)
    assert np.array_equal(ids[:k], ref.ids[:k]) and np.all(ids[k:] == SENTINEL), what
    changed = np.zeros(n, bool)
    changed[ref.ids] = True
    src, dead = ref.cnt > 0, ref.src_of >= 0
    # untouched: every float of every array keeps its bits; a source keeps all but its four values
    for old, new in ((rec, g_rec), (raw, g_raw), (m, g_m), (v, g_v)):
        if old is not None:
            assert np.array_equal(bits(new[~changed]), bits(old[~changed])), what
    for old, new in ((rec, g_rec), (raw, g_raw)):
        if old is not None:
            assert np.array_equal(bits(new[src][:, OTHERS]), bits(old[src][:, OTHERS])), what
    # cnt, seen through which sources changed, and their values
    moved = bits(g_rec[:, 15]) != bits(rec[:, 15])
    assert np.array_equal(moved & ~dead, src), what
    check_values(rec[src], g_rec[src], None if raw is None else g_raw[src], ref.cnt[src], what)
    # src(d), seen through which row every dead d received: all 84 floats as they now stand
    d = np.flatnonzero(dead)
    assert np.array_equal(bits(g_rec[d]), bits(g_rec[ref.src_of[d]])), what
    if raw is not None:
        assert np.array_equal(bits(g_raw[d]), bits(g_raw[ref.src_of[d]])), what
    if len(d) and len(np.unique(ref.src_of[d])) > 1:
        assert len(np.unique(bits(g_rec[d])[:, 0])) > 1               # the copies are not all of one source
    assert not bits(g_m[changed]).any() and not bits(g_v[changed]).any(), what
    return ref, (g_rec, g_raw, g_m, g_v), ids, counts


SIZES = [1, 255, 256, 257, 262_145]       # 262 145: the first n with more than 1024 block sums -- two blocks per scanning thread


@pytest.mark.parametrize("space", ["records", "raw"])
@pytest.mark.parametrize("n", SIZES)
def test_relocate_at_the_edges_of_the_scan(bare, n, space):
    """Alive splats only at g in {0, 255, 256, 511, n - 1}: every draw is resolved at a block edge, and a dead splat between two
    alive ones is never chosen.  Everything check_relocate compares, bit for bit or under the derived allowances."""
    ref, _, _, counts = check_relocate(bare, cloud(n, "edges", space), ("edges", n, space))
    alive = [g for g in (0, 255, 256, 511, n - 1) if g < n]
    assert counts[1] == n - len(set(alive))
    if counts[1]:
        assert set(np.unique(ref.src_of[ref.src_of >= 0])) <= set(alive) and counts[0] == n
        if n >= 257:
            assert counts[2] == len(set(alive))                        # with this many draws every alive splat is a source


@pytest.mark.parametrize("space", ["records", "raw"])
@pytest.mark.parametrize("n,kind", [(255, "mixed"), (257, "mixed"), (3000, "mixed"), (60, "one_alive"), (300, "all_dead"),
                                    (300, "no_dead")])
def test_relocate_on_designed_clouds(bare, n, kind, space):
    """A fifth of the splats dead (small ratios, r = 2, 3, ...); one alive splat and 59 dead ones (the ratio clamps at 51); all
    dead (nothing changes, counts {0, n, 0}); no dead splat (nothing changes, counts {0, 0, 0})."""
    arrays = cloud(n, kind, space)
    ref, got, ids, counts = check_relocate(bare, arrays, (kind, n, space))
    if kind == "mixed":
        assert 1 < ref.cnt.max() < 50 and counts[2] > 5
    elif kind == "one_alive":
        assert counts == (60, 59, 1) and ref.cnt.max() == 59 and mcmc_ref.ratio(ref.cnt.max()) == 51
    elif kind == "all_dead":
        assert counts == (0, n, 0)
    else:
        assert counts == (0, 0, 0)
    if kind in ("all_dead", "no_dead"):
        for old, new in zip(arrays, got):
            assert old is None or np.array_equal(bits(old), bits(new))


def test_relocate_special_opacities_and_a_short_list(bare):
    """An opacity equal to min_opacity and a NaN are dead, 1.5 and 1 are alive with weight 2^24; max_rows below the
    number of changed rows: ids_out holds the first max_rows, the count is not clamped; max_rows == 0 with a NULL ids_out."""
    arrays = special_cloud()
    ref, _, _, counts = check_relocate(bare, arrays, "special")
    assert list(np.flatnonzero(ref.dead)) == [0, 1, 255, 256] and ref.w[2] == ref.w[100] == 2 ** 24 and ref.w[299] > 0
    assert counts[1] == 4 and 5 <= counts[0] <= 8
    check_relocate(bare, arrays, "short list", max_rows=3)
    check_relocate(bare, arrays, "no list", max_rows=0)
    other = check_relocate(bare, arrays, "another seed", seed=SEED + 1)[0]
    assert not np.array_equal(other.src_of, ref.src_of) or counts[2] == 1


# ---- gs_grow_device ---------------------------------------------------------------------------------------------------------

def run_grow(r, arrays, n_add, max_out, seed=SEED):
    n = len(arrays[0])
    d = [None if a is None else up(a) for a in arrays]
    out = [None if a is None else filled((max_out + 2, 84)) for a in arrays]
    counts = filled(2, torch.int32)
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else t.data_ptr()
    r.growDevice(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), n, MIN_OP, seed, n_add, ptr(out[0]), ptr(out[1]), ptr(out[2]),
                 ptr(out[3]), max_out, counts.data_ptr())
    r.synchronize()
    for a, t in zip(arrays, d):
        assert a is None or np.array_equal(bits(a), bits(down(t)))           # the inputs are only read
    return [None if t is None else down(t) for t in out], tuple(int(x) for x in down(counts, np.uint32))


def check_grow(r, arrays, n_add, what, short=0):
    rec, raw, m, v = arrays
    n = len(rec)
    ref = mcmc_ref.grow_ref(rec, MIN_OP, SEED, n_add)
    n_out = ref.counts[0]
    max_out = n_out - short
    (g_rec, g_raw, g_m, g_v), counts = run_grow(r, arrays, n_add, max_out)
    assert counts == ref.counts, (what, counts, ref.counts)
    for a in (g_rec, g_raw, g_m, g_v):
        assert a is None or np.all(bits(a[max_out:]) == SENTINEL), what      # rows >= max_out are not written
    parent = ref.parent[:max_out]
    plain = ref.cnt[parent] == 0
    # the row placement: a row nobody drew is copied bit for bit, moments included
    for old, new in ((rec, g_rec), (raw, g_raw), (m, g_m), (v, g_v)):
        if old is not None:
            assert np.array_equal(bits(new[:max_out][plain]), bits(old[parent[plain]])), what
    # a source: all its outputs identical, its row but for the four values, zero moments
    first = ref.offset[parent]
    for old, new in ((rec, g_rec), (raw, g_raw)):
        if old is not None:
            assert np.array_equal(bits(new[:max_out]), bits(new[first])), what
            assert np.array_equal(bits(new[:max_out][:, OTHERS]), bits(old[parent][:, OTHERS])), what
    assert not bits(g_m[:max_out][~plain]).any() and not bits(g_v[:max_out][~plain]).any(), what
    src = np.flatnonzero((ref.cnt > 0) & (ref.offset < max_out))
    check_values(rec[src], g_rec[ref.offset[src]], None if raw is None else g_raw[ref.offset[src]], ref.cnt[src], what)
    return ref, counts


@pytest.mark.parametrize("space", ["records", "raw"])
@pytest.mark.parametrize("n,kind,n_add", [(1, "no_dead", 3), (257, "mixed", 40), (257, "edges", 700), (3000, "mixed", 150),
                                          (60, "one_alive", 100), (262_145, "edges", 1000)])
def test_grow(bare, n, kind, n_add, space):
    """gs_grow_device against grow_ref: the counts, the row placement (the copies beside their source), plain copies bit for bit,
    the sources' values, zero moments; with max_out three rows short, the rows past it are not written."""
    arrays = cloud(n, kind, space)
    ref, counts = check_grow(bare, arrays, n_add, (kind, n, n_add, space))
    assert counts[0] == n + n_add and np.all(ref.w[ref.cnt > 0] > 0)
    if n < 10_000:
        check_grow(bare, arrays, n_add, (kind, n, n_add, space, "short"), short=3)


def test_grow_without_draws(bare):
    """n_add == 0 is a plain copy; with every splat dead no draw is made and the outputs number n."""
    for kind, n_add in (("mixed", 0), ("all_dead", 50)):
        arrays = cloud(300, kind, "raw")
        ref, counts = check_grow(bare, arrays, n_add, (kind, n_add))
        assert counts == (300, 0)


# ---- gs_position_noise_device -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def noise_cloud():
    rng = np.random.default_rng(77)
    n = 300
    raw = random_raw(rng, n + 1)
    raw[:, 15] = rng.uniform(-9.0, -4.0, n + 1)              # opacities of 1e-4 .. 0.018: gates from 0.2 to 1
    raw[:, 4:7] = rng.uniform(-4.0, -1.0, (n + 1, 3))
    rec = act_ref(raw, np.float32)
    for a in (raw, rec):
        bits(a)[:, UNTOUCHED] = SENTINEL
    return rec, raw, n


@pytest.mark.parametrize("form", ["listed", "count_cuts", "max_rows_cuts", "all_rows", "records_alone"])
def test_position_noise(bare, form):
    """The positions of the listed rows within 2e-5 gate scale sum_k |R[i][k]| s_k^2 sum_j |R[j][k]| + 4 ulp(pos) of the float64
    restatement -- the allowance per unit normal that tests/test_densify_gpu.py gives a split child, carried through the second
    product --, the same bits in raw; nothing else is touched: an id >= n is skipped, rows past min(count, max_rows) and the
    blocks past the count leave memory alone, row n is never written; ids == NULL touches every row."""
    rec, raw, n = noise_cloud()
    scale, gate_k, gate_x0 = 0.5, 100.0, 0.995
    listed = np.array([5, 299, n, 0, 64, 255, 256, 17, 130, 131, 200, 77], dtype=np.uint32)
    count, max_rows = {"listed": (12, 700), "count_cuts": (5, 700), "max_rows_cuts": (12, 7), "all_rows": (0, 0),
                       "records_alone": (12, 12)}[form]
    ids = np.full(max(max_rows, 12) + 4, 3, np.uint32)       # behind the list: ids that would move splat 3
    ids[:12] = listed
    d_rec, d_raw = up(rec), (None if form == "records_alone" else up(raw))
    d_ids, d_count = up(ids), torch.tensor([count], dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    if form == "all_rows":
        bare.positionNoiseDevice(d_rec.data_ptr(), d_raw.data_ptr(), n, None, None, 0, scale, gate_k, gate_x0, SEED)
        touched = np.arange(n)
    else:
        bare.positionNoiseDevice(d_rec.data_ptr(), None if d_raw is None else d_raw.data_ptr(), n, d_ids.data_ptr(),
                                 d_count.data_ptr(), max_rows, scale, gate_k, gate_x0, SEED)
        touched = np.array([g for g in listed[:min(count, max_rows)] if g < n], dtype=np.int64)
    bare.synchronize()
    g_rec = down(d_rec)
    want, bound = mcmc_ref.noise_ref(rec, touched, scale, gate_k, gate_x0, SEED)
    got = g_rec[touched, 0:3].astype(np.float64)
    tol = 2e-5 * bound + 4 * np.spacing(np.abs(want).astype(F)).astype(np.float64)
    print(f"{form}: worst |gpu - ref| / allowance {float((np.abs(got - want) / tol).max()):.3f}; "
          f"largest move {float(np.abs(want - rec[touched, 0:3]).max()):.3g}")
    assert np.all(np.abs(got - want) <= tol)
    assert np.median(np.abs(want - rec[touched, 0:3]).max(1) / tol.max(1)) > 100      # the noise is far above the allowance
    rest = np.ones(n + 1, bool)
    rest[touched] = False
    assert np.array_equal(bits(g_rec[rest]), bits(rec[rest])) and np.array_equal(bits(g_rec[:, 3:]), bits(rec[:, 3:]))
    if d_raw is not None:
        g_raw = down(d_raw)
        assert np.array_equal(bits(g_raw[:, 0:3]), bits(g_rec[:, 0:3])) and np.array_equal(bits(g_raw[:, 3:]), bits(raw[:, 3:]))
    assert np.array_equal(down(d_ids, np.uint32), ids) and int(d_count.cpu()[0]) == count


# ---- reproducibility --------------------------------------------------------------------------------------------------------

def test_the_same_bits_twice_and_on_two_sorters(bare):
    other = make_context(gs.GS_SORT_TILE_BUCKET)
    try:
        arrays = cloud(3000, "mixed", "raw")
        rec, raw, n = noise_cloud()
        runs = []
        for r in (bare, bare, other):
            reloc = run_relocate(r, arrays)
            grown = run_grow(r, arrays, 150, 3150)
            d_rec, d_raw = up(rec), up(raw)
            torch.cuda.synchronize()
            r.positionNoiseDevice(d_rec.data_ptr(), d_raw.data_ptr(), n, None, None, 0, 0.5, 100.0, 0.995, SEED)
            r.synchronize()
            flat = [a for a in reloc[0] + [reloc[1]] + grown[0] + [down(d_rec), down(d_raw)]]
            runs.append((b"".join(bits(a).tobytes() for a in flat), reloc[2], grown[1]))
        assert runs[0] == runs[1] == runs[2]
    finally:
        other.cleanup()


# ---- through the frame ------------------------------------------------------------------------------------------------------

def test_listed_rows_upload_gives_the_frame_of_a_full_upload():
    """The small scene with a few splats killed: relocate, then gs_upload_rows_device with the call's own ids and count; the
    frame is byte for byte that of a full upload of the same records."""
    aos, w, h = small_scene()
    aos = np.ascontiguousarray(aos, dtype=F).copy()
    n = len(aos)
    kill = [3, 50, 120, 299]
    aos[kill, 15] = 0.001
    sc = make_scene(aos, w, h)
    r = make_renderer(sc, w, h)
    rec = up(aos)
    ids, counts = filled(n, torch.int32), filled(3, torch.int32)
    torch.cuda.synchronize()
    r.relocateDevice(rec.data_ptr(), None, None, None, n, MIN_OP, SEED, ids.data_ptr(), n, counts.data_ptr())
    r.uploadRowsDevice(rec.data_ptr(), n, ids.data_ptr(), counts.data_ptr(), n)
    listed = r.draw(sc).copy()
    r.uploadDevice(rec.data_ptr(), n)
    full = r.draw(sc).copy()
    r.cleanup()
    changed, dead, sources = (int(x) for x in down(counts, np.uint32))
    assert dead == len(kill) and 1 <= sources <= 4 and changed == dead + sources
    assert np.array_equal(listed, full)


def test_two_copies_conserve_the_pixels(oracle_mod):
    """A source sampled once (r = 2) with its one copy: every pixel the source covered in the frame BEFORE relocation -- and
    every other pixel, where both frames hold the background -- is within one 8-bit step of that frame, in every channel
    (the dead splat lies off the screen, so only that splat covers the pixels).
    The colour is chosen so that the bound can hold at the rim too.  The rasteriser skips an entry whose alpha is below
    1 / 255, so the copies (o' = 1 - sqrt(1 - o) = 0.163 against o = 0.3, scales times c = 0.9746) cover a slightly smaller
    disc than the splat did.  Where a copy's alpha falls to 1 / 255 the old splat's alpha is o (255 o')^(-c^2) = 2.21 / 255,
    its largest value in the ring that no copy covers; with a colour of at most 0.55 the old frame holds at most 1.22 steps
    there, which rounds to 1.  Inside the disc the two copies differ from the splat by at most 0.47 steps of alpha."""
    w, h = 64, 48
    aos = np.stack([screen_splat(oracle_mod, w, h, 30.0, 22.0, 3.0, 9.0, 0.3, colour=(0.18, 0.0, -0.6)),
                    screen_splat(oracle_mod, w, h, -4000.0, 22.0, 3.0, 2.0, 0.001)]).astype(F)
    sc = make_scene(aos, w, h)
    r = make_renderer(sc, w, h)
    before = r.draw(sc).copy()
    rec = up(aos)
    counts = filled(3, torch.int32)
    torch.cuda.synchronize()
    r.relocateDevice(rec.data_ptr(), None, None, None, 2, MIN_OP, SEED, None, 0, counts.data_ptr())
    r.uploadDevice(rec.data_ptr(), 2)
    after = r.draw(sc).copy()
    r.cleanup()
    got = down(rec)
    assert tuple(down(counts, np.uint32)) == (2, 1, 1) and np.array_equal(bits(got[0]), bits(got[1]))
    assert got[0, 15] < 0.3 and np.all(got[0, 4:6] < aos[0, 4:6])
    diff = np.abs(after.astype(np.int32) - before.astype(np.int32))
    covered = before[..., :3].max(-1) > 0                              # by the source, in the frame before
    lost = covered & (after[..., :3].max(-1) == 0)
    print("two copies: largest pixel difference", int(diff[covered].max()), "over the", int(covered.sum()), "pixels the source",
          "covered, peak", int(before[..., :3].max()), ";", int(lost.sum()), "of them no copy covers;", int(diff[~covered].max()),
          "elsewhere")
    assert before[..., :3].max() > 35 and covered.sum() > 200
    assert diff[covered].max() <= 1
    assert diff[~covered].max() <= 1                                   # the same bound everywhere else


# ---- the refusals -----------------------------------------------------------------------------------------------------------

def test_refusals(bare):
    """Every refusal of the header with its message; nothing was enqueued: every array keeps its bits."""
    n = 8
    pool = filled((8 * n, 84))
    rec, raw, m, v, o_rec, o_raw, o_m, o_v = (pool[k * n:(k + 1) * n] for k in range(8))
    ids, counts = filled(n + 3, torch.int32), filled(3, torch.int32)
    torch.cuda.synchronize()
    P = lambda t: t.data_ptr()
    reloc = lambda **kw: bare.relocateDevice(**{**dict(records_ptr=P(rec), raw_ptr=P(raw), m_ptr=P(m), v_ptr=P(v), n=n,
                                                       min_opacity=MIN_OP, seed=1, ids_out_ptr=P(ids), max_rows=n,
                                                       counts_ptr=P(counts)), **kw})
    grow = lambda **kw: bare.growDevice(**{**dict(records_ptr=P(rec), raw_ptr=P(raw), m_ptr=P(m), v_ptr=P(v), n=n,
                                                  min_opacity=MIN_OP, seed=1, n_add=2, records_out_ptr=P(o_rec),
                                                  raw_out_ptr=P(o_raw), m_out_ptr=P(o_m), v_out_ptr=P(o_v), max_out=n,
                                                  counts_ptr=P(counts)), **kw})
    noise = lambda **kw: bare.positionNoiseDevice(**{**dict(records_ptr=P(rec), raw_ptr=P(raw), n=n, ids_ptr=P(ids),
                                                            count_ptr=P(counts), max_rows=n, scale=1.0), **kw})
    nan, inf = float("nan"), float("inf")
    cases = [
        (reloc, dict(records_ptr=None), "gs_relocate_device: null records or counts_out"),
        (reloc, dict(counts_ptr=None), "gs_relocate_device: null records or counts_out"),
        (reloc, dict(m_ptr=None), "gs_relocate_device: m and v must be given together or not at all"),
        (reloc, dict(v_ptr=None), "gs_relocate_device: m and v must be given together or not at all"),
        (reloc, dict(n=0), "gs_relocate_device: n is 0"),
        (reloc, dict(n=2 ** 31), "gs_relocate_device: n must be below 2^31"),
        (reloc, dict(min_opacity=2.0 ** -25), "gs_relocate_device: min_opacity must lie in [2^-24, 1)"),
        (reloc, dict(min_opacity=1.0), "gs_relocate_device: min_opacity must lie in [2^-24, 1)"),
        (reloc, dict(min_opacity=nan), "gs_relocate_device: min_opacity must lie in [2^-24, 1)"),
        (reloc, dict(ids_out_ptr=None), "gs_relocate_device: null ids_out with max_rows > 0"),
        (reloc, dict(raw_ptr=P(rec) + 336), "gs_relocate_device: two arrays alias each other"),
        (reloc, dict(v_ptr=P(m)), "gs_relocate_device: two arrays alias each other"),
        (reloc, dict(counts_ptr=P(ids) + 4), "gs_relocate_device: two arrays alias each other"),
        (grow, dict(records_ptr=None), "gs_grow_device: null records or counts_out"),
        (grow, dict(counts_ptr=None), "gs_grow_device: null records or counts_out"),
        (grow, dict(records_out_ptr=None), "gs_grow_device: null records_out with max_out > 0"),
        (grow, dict(raw_out_ptr=None), "gs_grow_device: raw, m and v must each be null together with their own output"),
        (grow, dict(m_ptr=None), "gs_grow_device: raw, m and v must each be null together with their own output"),
        (grow, dict(m_ptr=None, m_out_ptr=None), "gs_grow_device: m and v must be given together or not at all"),
        (grow, dict(n=0), "gs_grow_device: n is 0"),
        (grow, dict(n=2 ** 31), "gs_grow_device: n must be below 2^31"),
        (grow, dict(min_opacity=0.0), "gs_grow_device: min_opacity must lie in [2^-24, 1)"),
        (grow, dict(n_add=2 ** 31 - n), "gs_grow_device: n + n_add must be below 2^31"),
        (grow, dict(records_out_ptr=P(rec) + 336 * (n - 1)), "gs_grow_device: an output array aliases an input"),
        (grow, dict(counts_ptr=P(v)), "gs_grow_device: an output array aliases an input"),
        (grow, dict(m_out_ptr=P(o_v) + 4), "gs_grow_device: two output arrays alias each other"),
        (noise, dict(records_ptr=None), "gs_position_noise_device: null records"),
        (noise, dict(n=0), "gs_position_noise_device: n is 0"),
        (noise, dict(scale=inf), "gs_position_noise_device: scale, gate_k and gate_x0 must be finite"),
        (noise, dict(gate_k=nan), "gs_position_noise_device: scale, gate_k and gate_x0 must be finite"),
        (noise, dict(gate_x0=-inf), "gs_position_noise_device: scale, gate_k and gate_x0 must be finite"),
        (noise, dict(count_ptr=None), "gs_position_noise_device: null count with ids and max_rows > 0"),
    ]
    for call, change, message in cases:
        with pytest.raises(gs.GsplatError) as ei:
            call(**change)
        assert ei.value.code == _lib.GS_ERR_INVALID and message in str(ei.value), (change, str(ei.value))
    bare.synchronize()
    for t in (pool, ids, counts):
        assert np.all(down(t, np.uint32) == SENTINEL)
    # legal: a listed form with max_rows == 0 launches nothing; a count query of grow writes the counts alone
    noise(max_rows=0, count_ptr=None)
    bare.synchronize()
    assert np.all(down(pool, np.uint32) == SENTINEL)


# ---- autograd.VisibleAdam ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["records", "raw"])
def test_visible_adam_relocates_grows_and_adds_noise(space, monkeypatch):
    """On the small scene: a step, add_noise() on its rows, a few splats killed, relocate() -- no host wait: the counts stay a
    device tensor --, a step, grow(n_add=k): the cloud has n + k rows and the next step runs."""
    from vk3dgaussiansplatting_amd.autograd import VisibleAdam
    aos, w, h = small_scene()
    aos = np.ascontiguousarray(aos, dtype=F).copy()
    n = len(aos)
    aos[[10, 20, 30, 40, 60], 15] = 0.006                               # nearly transparent: the noise gate is open
    truth = aos.copy()
    truth[:, 12:15] += 0.3 * np.random.default_rng(3).standard_normal((n, 3)).astype(F)
    sc_truth, sc = make_scene(truth, w, h), make_scene(aos, w, h)
    r = new_renderer(sc_truth, w, h, gs.GS_SORT_RADIX4, False)
    r.draw(sc_truth)
    target = torch.tensor(np.ascontiguousarray(r.readOutput(gs.GS_OUTPUT_RGBA32F)[..., :3]), device=DEV)
    r.cleanup()
    cam = gs.Renderer._camera_args(sc.getCamera())
    r = new_renderer(sc, w, h, gs.GS_SORT_RADIX4, False)
    opt = VisibleAdam(torch.tensor(aos, device=DEV), renderer=r, space=space)
    host = lambda t: t.cpu().numpy()
    opt.step(*cam, target, LAMBDA)
    opt.stream.synchronize()
    pos0, k0 = host(opt.records)[:, 0:3].copy(), int(host(opt.count).view(np.uint32)[0])
    opt.add_noise(5e5)
    opt.stream.synchronize()
    pos1 = host(opt.records)[:, 0:3]
    listed = np.zeros(n, bool)
    listed[host(opt.ids).view(np.uint32)[:k0]] = True
    assert k0 > 50 and np.array_equal(bits(pos1[~listed]), bits(pos0[~listed])) and np.any(bits(pos1[listed]) != bits(pos0[listed]))
    if space == "raw":
        assert np.array_equal(bits(host(opt.raw)[:, 0:3]), bits(pos1))
    kill = [3, 50, 120, 299]
    with torch.cuda.stream(opt.stream):
        if space == "raw":
            opt.raw[kill, 15] = -8.0
            opt.records[kill, 15] = float(act_ref(np.full((1, 84), -8.0, F), np.float32)[0, 15])
        else:
            opt.records[kill, 15] = 0.001
    opt.reset_upload()
    # relocate() and add_noise() wait for nothing and read nothing back: every Renderer call, every torch wait and every
    # Tensor.cpu / .item is logged while they run (the recorder of tests/test_trainer_calls_gpu.py)
    rec = Recorder(r, [])
    rec.opt = opt
    Recorder.log_torch_waits(monkeypatch)
    for name in ("cpu", "item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, (lambda fn, name: lambda self, *a, **kw: (
            Recorder.running.calls.append(["Tensor." + name, [], {}]) if Recorder.running is not None else None, fn(self, *a, **kw))[1])(
            getattr(torch.Tensor, name), name))
    with rec.method("relocate") as calls:
        opt.relocate(seed=5)
    n_ = opt.records.shape[0]
    names = [c[0] for c in calls]
    assert names[-2:] == ["relocateDevice", "uploadRowsDevice"] and names[0] == "uploadDevice", names
    assert not [x for x in names if "synchronize" in x or x.startswith("Tensor.")], names
    assert calls[-1][1] == ["records", n_, "relocated_ids", "relocated", n_], calls[-1]
    assert calls[-2][1][-3:] == ["relocated_ids", n_, "relocated"], calls[-2]
    with rec.method("add_noise") as calls:
        opt.add_noise(5e5)
    assert [c[0] for c in calls] == ["positionNoiseDevice"], calls
    assert opt.relocated.is_cuda and opt.relocated_ids.is_cuda
    numbers = opt.step(*cam, target, LAMBDA)
    opt.stream.synchronize()
    changed, dead, sources = (int(x) for x in host(opt.relocated).view(np.uint32))
    assert dead == len(kill) and 1 <= sources <= 4 and changed == dead + sources and np.all(np.isfinite(host(numbers)))
    n_out, sources = opt.grow(n_add=7)
    assert n_out == n + 7 and 1 <= sources <= 7
    assert opt.records.shape == opt.m.shape == opt.v.shape == (n + 7, 84) and opt.max_rows == n + 7
    if space == "raw":
        assert opt.raw.shape == (n + 7, 84)
        fields_equal(host(opt.records), act_ref(host(opt.raw), np.float32), "records == act(raw) after grow")
    assert opt.grow(cap_max=n + 7) == (n + 7, 0)                            # at the cap: n_add = 0, a plain copy
    numbers = opt.step(*cam, target, LAMBDA)
    opt.add_noise(5e5, all_rows=True)
    assert opt._full_upload
    numbers2 = opt.step(*cam, target, LAMBDA)
    opt.stream.synchronize()
    assert np.all(np.isfinite(host(numbers))) and np.all(np.isfinite(host(numbers2))) and r.sceneInfo().num_gaussians == n + 7
    r.setStream(None)
    r.cleanup()
