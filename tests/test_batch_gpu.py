"""gs_rows_accumulate_device and gs_rows_collect_device on the MI355X (include/gsplat.h): both calls bit for bit against their
NumPy float32 restatements (tests/test_batch_cpu.py) on designed lists and marks, on the lists of two real frames, enqueued
without a host wait against the same calls with a wait after each, as autograd.VisibleAdam.step_batch uses them, and the
refusals.  Every comparison is of bits; a NaN in a field is compared by position."""
import ctypes as C
import functools

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_adam_cpu import FIELDS, UNTOUCHED, adam_rows_ref, params_dict
from test_adam_gpu import same_floats
from test_backward_gpu import SCENES
from test_batch_cpu import SENTINEL, rows_accumulate_ref, rows_collect_ref
from test_parity_gpu import make_scene
from test_train_chain_gpu import CAMERAS, LAMBDA, SENTINEL_ID, SENTINEL_ROW, bits, new_renderer

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def bare():
    """A context without a scene and without a resolution: all that both calls need."""
    pytest.importorskip("torch")
    r = gs.Renderer(64, 64, record_timings=False)
    r.init(gs.ResourceManager())
    yield r
    r.cleanup()


def up(a):
    """A host array on the device as its bits (int32 storage), whatever they spell."""
    import torch
    return torch.tensor(np.ascontiguousarray(a).view(np.int32), device="cuda:0")


def down(t, dtype=np.float32):
    return t.cpu().numpy().view(dtype)


# ---- 1. accumulate against the restatement ---------------------------------------------------------------------------------

N = 300                                    # not a multiple of 64; every array has N + 1 rows and n = N is passed
CANARY = 42                                # a valid row no list names: ids past count point at it
# three lists of 78 distinct ids that overlap: 0, N - 1, one id == N (skipped), a run of 70, isolated ids.  64 and 250 are in
# all three, 0, 7 and parts of the runs in two.  Rows 12 and 13 of each list lie in its run: in the mapping of 19 lanes per row
# they straddle the first 256-thread block (lanes 228..246 and 247..265).
LISTS = ([0, 7, 31, N, 64] + list(range(100, 170)) + [200, 250, N - 1],
         [0, 5, 64, N, 33] + list(range(135, 205)) + [250, 260, 1],
         [64, N - 1, 7, 2, N] + list(range(60, 64)) + list(range(65, 131)) + [250, 270, 280])
K = len(LISTS[0])
WEIGHTS = (1.0, 0.5, 1.0 / 3.0)
CASES = [(0, 8), (1, 1), (63, 64), (64, 64), (65, 64), (K, N)]


@functools.lru_cache(maxsize=None)
def accumulate_inputs():
    """acc [N + 1, 84]: NaN in the fields (a first touch must not read them), the sentinel in the other 25 floats; three frames'
    rows [N, 84]: magnitudes over six decades (products and sums round differently from a fused multiply-add), exact zeros,
    -0.0f, one NaN, the sentinel in the floats that are never read."""
    assert all(len(l) == K == len(set(l)) for l in LISTS)
    rng = np.random.default_rng(77)
    acc = np.full((N + 1, 84), np.nan, F)
    bits(acc)[:, UNTOUCHED] = SENTINEL
    frames = []
    for t in range(3):
        g = (rng.standard_normal((N, 84)) * 10.0 ** rng.integers(-4, 3, (N, 84))).astype(F)
        g[rng.random((N, 84)) < 0.1] = 0.0
        g[rng.random((N, 84)) < 0.05] = -0.0
        bits(g)[:, UNTOUCHED] = SENTINEL
        frames.append(g)
    frames[1][2, 8] = np.nan                                            # row 2 of the second list: splat 64, touched by all three
    return acc, frames


def ids_for(k, count):
    ids = np.full(N, CANARY, np.uint32)
    c = min(count, K)
    ids[:c] = LISTS[k][:c]
    return ids


@pytest.mark.parametrize("count,max_rows", CASES)
def test_accumulate_bits_against_the_restatement(bare, count, max_rows):
    """Three frames into one accumulator, weights 1, 1/2, 1/3: after every call acc and mark equal rows_accumulate_ref bit for bit
    -- rows with one, two and three touches, a first touch over NaN, the spare row N (the lists name it: an id == n is skipped),
    the canary, the 25 sentinel floats of every row -- and ids, rows and count keep their bits."""
    import torch
    acc, frames = accumulate_inputs()
    mark = np.zeros(N + 1, np.uint32)
    d_acc, d_mark = up(acc), up(mark)
    d_count = torch.tensor([count], dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    want = (acc, mark)
    for k in range(3):
        ids = ids_for(k, count)
        d_ids, d_rows = up(ids), up(frames[k])
        torch.cuda.synchronize()
        want = rows_accumulate_ref(*want, N, ids, frames[k], count, max_rows, WEIGHTS[k])
        bare.rowsAccumulateDevice(d_acc.data_ptr(), d_mark.data_ptr(), N, d_ids.data_ptr(), d_rows.data_ptr(), d_count.data_ptr(),
                                  max_rows, WEIGHTS[k])
        bare.synchronize()
        same_floats(down(d_acc), want[0], ("acc", "frame", k))
        assert np.array_equal(down(d_mark, np.uint32), want[1]), ("mark", "frame", k)
        assert np.array_equal(down(d_rows, np.uint32), bits(frames[k])) and np.array_equal(down(d_ids, np.uint32), ids)
        assert int(d_count.cpu()[0]) == count
    got, marks = down(d_acc), down(d_mark, np.uint32)
    assert np.all(bits(got)[:, UNTOUCHED] == SENTINEL) and marks[N] == 0 and marks[CANARY] == 0
    assert np.isnan(got[[CANARY, N]][:, FIELDS]).all()                   # never listed: still the NaN they started with
    touched = np.flatnonzero(marks)
    k = min(count, max_rows)
    assert set(touched) == {g for l in LISTS for g in l[:k] if g < N}
    if k == K:
        assert set(marks[touched]) == {1, 2, 3} and marks[64] == 3 and marks[0] == 2 and marks[31] == 1
    # the one NaN of the rows (row 2 of the second list, splat 64) where it is listed, nothing of acc's own
    assert np.sum(np.isnan(got[touched][:, FIELDS])) == (1 if k >= 3 else 0) and (k < 3 or np.isnan(got[64, 8]))


# ---- 2. collect against the restatement ------------------------------------------------------------------------------------

BIG = 262144 + 257                          # 1026 blocks of 256 splats: the first size at which a thread of the block scan owns two
SIZES = [1, 255, 256, 257, 300, BIG]


def mark_patterns(n):
    rng = np.random.default_rng(n)
    edges = np.array(sorted({g for b in range(256, n + 1, 256) for g in (b - 1, b) if g < n}), dtype=np.int64)
    pats = {"none": np.zeros(0, np.int64), "all": np.arange(n), "first": np.array([0]), "last": np.array([n - 1]),
            "block_edges": edges, "random_half": np.flatnonzero(rng.random(n) < 0.5)}
    for name, members in pats.items():
        m = np.zeros(n + 1, np.uint32)
        m[members] = rng.integers(1, 5, len(members)).astype(np.uint32) if name != "all" else 1
        m[n] = 7                                                        # beyond n: no member, never cleared
        yield name, m


@pytest.mark.parametrize("n", SIZES)
def test_collect_bits_against_the_restatement(bare, n):
    """Every mark pattern (none, all, only splat 0, only splat n - 1, both sides of every block boundary, a random half) with
    max_rows 0, |U| - 1, |U| and |U| + 5: count_out is |U| unclamped, ids and rows equal rows_collect_ref bit for bit -- the fields
    are acc's bits (arbitrary ones: acc is random words), the other 25 floats +0 -- rows and ids past min(|U|, max_rows) keep
    their sentinels, mark is zero below n and untouched at n, acc is unchanged."""
    import torch
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n)
    d_acc = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + 1, 84), dtype=torch.int32, device=dev, generator=gen)     # filled on the device
    acc = down(d_acc)
    for name, mark in mark_patterns(n):
        size = int(np.count_nonzero(mark[:n]))
        for max_rows in sorted({0, max(size - 1, 0), size, size + 5}):
            what = (name, "max_rows", max_rows)
            d_mark = up(mark)
            d_ids = torch.full((max_rows + 3,), SENTINEL_ID, dtype=torch.int32, device=dev)
            d_rows = torch.full((max_rows + 3, 84), SENTINEL_ROW, dtype=torch.float32, device=dev)
            d_count = torch.full((1,), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            bare.rowsCollectDevice(d_acc.data_ptr(), d_mark.data_ptr(), n, d_ids.data_ptr() if max_rows else None,
                                   d_rows.data_ptr() if max_rows else None, max_rows, d_count.data_ptr())
            bare.synchronize()
            ids0 = np.full(max_rows + 3, SENTINEL_ID, np.int32).view(np.uint32)
            rows0 = np.full((max_rows + 3, 84), SENTINEL_ROW, F)
            w_ids, w_rows, w_count, w_mark = rows_collect_ref(acc, mark, n, ids0 if max_rows else None, rows0 if max_rows else None, max_rows)
            assert w_count == size
            assert int(down(d_count, np.uint32)[0]) == size, what
            assert np.array_equal(down(d_mark, np.uint32), w_mark), what
            if max_rows:
                assert np.array_equal(down(d_ids, np.uint32), w_ids), what
                assert np.array_equal(down(d_rows, np.uint32), bits(w_rows)), what
                k = min(size, max_rows)
                assert not bits(w_rows)[:k][:, UNTOUCHED].any() and np.all(w_rows[k:] == F(SENTINEL_ROW))
            else:
                assert np.all(down(d_ids, np.int32) == SENTINEL_ID) and np.all(down(d_rows) == F(SENTINEL_ROW)), what
    assert np.array_equal(down(d_acc, np.uint32), bits(acc))             # only read


# ---- 3., 4., 5. real frames, the chain without a wait, the trainer -----------------------------------------------------------

BATCH_STEPS = 3


@functools.lru_cache(maxsize=None)
def dense_inputs():
    aos, w, h = SCENES["dense"]()
    aos = np.ascontiguousarray(aos, dtype=np.float32)
    target = np.random.default_rng(11).uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
    return aos, target, w, h


def run_batches(how, steps, weights, cams=(0, 1), space="records", track_density=False):
    """`steps` optimiser steps on the dense scene, each on the views CAMERAS[c] for c in cams: the upload (full, then the rows of
    the union the step before listed), per view frame -> loss -> visible-row gradients -> gs_rows_accumulate_device, then one
    gs_rows_collect_device and one Adam step.  Host copies of what every step left: per view the numbers and the frame's own
    (ids, rows, count), the union (ids, rows, count), the records; and the final records, m, v (and seen).
    how = "waiting": the calls by hand on the context's own stream, a wait after every one (the answer);
          "caller_stream": the same calls on a torch stream handed to gs_set_stream, nothing waited for until the end;
          "step_batch": autograd.VisibleAdam.step_batch, nothing waited for; "step": VisibleAdam.step (one view)."""
    import torch
    from vk3dgaussiansplatting_amd.autograd import VisibleAdam
    aos, target_np, w, h = dense_inputs()
    n, B = len(aos), len(cams)
    dev = torch.device("cuda:0")
    scenes = [make_scene(aos, w, h, **CAMERAS[c]) for c in cams]
    cameras = [gs.Renderer._camera_args(sc.getCamera())[:3] for sc in scenes]
    r = new_renderer(scenes[0], w, h, gs.GS_SORT_RADIX4, False)
    records = torch.tensor(aos, device=dev)
    target0 = torch.tensor(target_np, device=dev)
    targets = [[target0 * (1.0 - 0.05 * (s * B + b)) for b in range(B)] for s in range(steps)]
    numbers = [torch.full((B, 3), float("nan"), device=dev) for _ in range(steps)]
    hist = dict(view_ids=[[torch.full((n,), SENTINEL_ID, dtype=torch.int32, device=dev) for _ in cams] for _ in range(steps)],
                view_rows=[[torch.full((n, 84), SENTINEL_ROW, device=dev) for _ in cams] for _ in range(steps)],
                view_count=[[torch.full((1,), -1, dtype=torch.int32, device=dev) for _ in cams] for _ in range(steps)],
                ids=[torch.full((n,), SENTINEL_ID, dtype=torch.int32, device=dev) for _ in range(steps)],
                rows=[torch.full((n, 84), SENTINEL_ROW, device=dev) for _ in range(steps)],
                count=[torch.full((1,), -1, dtype=torch.int32, device=dev) for _ in range(steps)],
                records=[torch.full((n, 84), float("nan"), device=dev) for _ in range(steps)])
    seen = None
    torch.cuda.synchronize()
    if how in ("step_batch", "step"):
        opt = VisibleAdam(records, renderer=r, space=space, track_density=track_density)
        for s in range(steps):
            if how == "step":
                numbers[s] = opt.step(*cameras[0], 0, targets[s][0], LAMBDA, None)[None]
            else:
                numbers[s] = opt.step_batch(cameras, targets[s], 0, LAMBDA, None, weights)
            with torch.cuda.stream(opt.stream):
                hist["ids"][s].copy_(opt.ids)
                hist["count"][s].copy_(opt.count)
                hist["records"][s].copy_(opt.records)
        records, m, v = opt.records, opt.m, opt.v
        seen = opt.seen if track_density else None
    else:
        waiting = how == "waiting"
        m, v = torch.zeros_like(records), torch.zeros_like(records)
        ids = torch.zeros(n, dtype=torch.int32, device=dev)
        rows = torch.zeros(n, 84, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        grad = torch.zeros(h, w, 4, device=dev)
        acc = torch.full((n, 84), float("nan"), device=dev)               # never initialised, as far as the calls know
        mark = torch.zeros(n, dtype=torch.int32, device=dev)
        # the union's own buffers (the trainer reuses ids / rows / count): what the collect leaves alone still holds the sentinel
        u_ids = torch.full((n,), SENTINEL_ID, dtype=torch.int32, device=dev)
        u_rows = torch.full((n, 84), SENTINEL_ROW, device=dev)
        u_count = torch.full((1,), -1, dtype=torch.int32, device=dev)
        stream = None if waiting else torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        if stream is not None:
            r.setStream(stream.cuda_stream)

        def wait():
            if waiting:
                torch.cuda.synchronize()
                r.synchronize()

        def chain():
            for s in range(steps):
                if s == 0:
                    r.uploadDevice(records.data_ptr(), n)
                else:
                    r.uploadRowsDevice(records.data_ptr(), n, u_ids.data_ptr(), u_count.data_ptr(), n)
                wait()
                for b in range(B):
                    r.drawCamera(*cameras[b], 0, sync=False)
                    wait()
                    r.photometricLossDevice(None, targets[s][b].data_ptr(), LAMBDA, None, numbers[s][b].data_ptr(), grad.data_ptr())
                    wait()
                    r.backwardVisibleDevice(grad.data_ptr(), None, ids.data_ptr(), rows.data_ptr(), n, count.data_ptr())
                    wait()
                    hist["view_ids"][s][b].copy_(ids)
                    hist["view_rows"][s][b].copy_(rows)
                    hist["view_count"][s][b].copy_(count)
                    wait()
                    r.rowsAccumulateDevice(acc.data_ptr(), mark.data_ptr(), n, ids.data_ptr(), rows.data_ptr(), count.data_ptr(), n, weights[b])
                    wait()
                r.rowsCollectDevice(acc.data_ptr(), mark.data_ptr(), n, u_ids.data_ptr(), u_rows.data_ptr(), n, u_count.data_ptr())
                wait()
                hist["ids"][s].copy_(u_ids)
                hist["rows"][s].copy_(u_rows)
                hist["count"][s].copy_(u_count)
                wait()
                r.adamRowsDevice(records.data_ptr(), m.data_ptr(), v.data_ptr(), n, u_ids.data_ptr(), u_rows.data_ptr(), u_count.data_ptr(), n,
                                 gs.default_adam_params(step=s + 1))
                wait()
                hist["records"][s].copy_(records)
                wait()

        if stream is not None:
            with torch.cuda.stream(stream):
                chain()
        else:
            chain()
    torch.cuda.synchronize()                                            # the one wait of the unsynchronised forms
    r.synchronize()
    out = dict(numbers=np.stack([t.cpu().numpy() for t in numbers]), final_records=records.cpu().numpy(), m=m.cpu().numpy(),
               v=v.cpu().numpy(), seen=None if seen is None else seen.cpu().numpy().view(np.uint32))
    for key, val in hist.items():
        out[key] = [[t.cpu().numpy() for t in x] if isinstance(x, list) else x.cpu().numpy() for x in val]
    r.setStream(None)
    r.cleanup()
    return out


def view_list(a, s, b):
    """The frame's own list of step s, view b, from a by-hand run: ids uint32 [count], rows [count, 84], count."""
    count = int(a["view_count"][s][b].view(np.uint32)[0])
    return a["view_ids"][s][b].view(np.uint32)[:count], a["view_rows"][s][b][:count], count


def union_ref(a, s, weights, n):
    """The NumPy restatement on the host copies of step s's per-view lists: (ids, rows, count) of the union, and the marks
    before the collect."""
    acc, mark = np.full((n, 84), np.nan, F), np.zeros(n, np.uint32)
    for b, w in enumerate(weights):
        ids, rows, count = view_list(a, s, b)
        acc, mark = rows_accumulate_ref(acc, mark, n, ids, rows, count, n, w)
    ids, rows, count, _ = rows_collect_ref(acc, mark, n, np.full(n, SENTINEL_ID, np.int32).view(np.uint32), np.full((n, 84), SENTINEL_ROW, F), n)
    return ids, rows, count, mark


@functools.lru_cache(maxsize=None)
def two_view_answer():
    """Three steps on two views with a wait after every call, checked not to be trivial: the two views list different splats,
    some in common; the numbers are finite and change; the union has the size the two lists and their overlap give, below the cloud's."""
    a = run_batches("waiting", BATCH_STEPS, (0.5, 0.5))
    n = len(dense_inputs()[0])
    for s in range(BATCH_STEPS):
        assert np.all(np.isfinite(a["numbers"][s])) and a["numbers"][s].all()
        (i0, r0, c0), (i1, r1, c1) = view_list(a, s, 0), view_list(a, s, 1)
        common = np.intersect1d(i0, i1)
        union = int(a["count"][s].view(np.uint32)[0])
        assert len(common) > 0 and not np.array_equal(i0, i1) and min(c0, c1) < union == c0 + c1 - len(common) < n, (s, c0, c1, len(common), union)
        assert np.any(r0 != 0) and np.any(r1 != 0)
        if s:
            assert not np.array_equal(bits(a["numbers"][s]), bits(a["numbers"][s - 1]))
    return a


def test_two_real_frames_against_the_restatement():
    """The dense scene under the two cameras: the device chain of two accumulates (weights 1/2 each) and one collect gives the
    ids, rows and count that the restatement makes of the two frames' own lists read back to the host -- at every step, the
    later ones over an accumulator that still holds the sums of the step before.  At the first step the union's buffers still hold
    their sentinel past the count."""
    pytest.importorskip("torch")
    a = two_view_answer()
    n = len(dense_inputs()[0])
    for s in range(BATCH_STEPS):
        ids, rows, count, _ = union_ref(a, s, (0.5, 0.5), n)
        assert int(a["count"][s].view(np.uint32)[0]) == count
        assert np.array_equal(a["ids"][s].view(np.uint32)[:count], ids[:count]), s
        assert np.array_equal(bits(a["rows"][s][:count]), bits(rows[:count])), s
        if s == 0:                                                      # nothing past the written rows is touched
            assert np.array_equal(a["ids"][s].view(np.uint32), ids) and np.array_equal(bits(a["rows"][s]), bits(rows))


def test_one_real_frame_at_weight_one_comes_back_bit_for_bit():
    """One camera, weight 1: collect returns the frame's own ids, rows and count."""
    pytest.importorskip("torch")
    a = run_batches("waiting", 1, (1.0,), cams=(1,))
    ids, rows, count = view_list(a, 0, 0)
    assert count > 0 and int(a["count"][0].view(np.uint32)[0]) == count
    assert np.array_equal(a["ids"][0].view(np.uint32)[:count], ids) and np.all(a["ids"][0][count:] == SENTINEL_ID)
    assert np.array_equal(bits(a["rows"][0][:count]), bits(rows)) and np.all(a["rows"][0][count:] == F(SENTINEL_ROW))
    assert not bits(rows)[:, UNTOUCHED].any() and np.any(rows[:, FIELDS] != 0)


@pytest.mark.parametrize("how", ["caller_stream", "step_batch"])
def test_three_batches_enqueued_without_waiting(how):
    """Three steps of two views each, enqueued back to back on a caller's stream -- by hand, and by VisibleAdam.step_batch -- with
    nothing waited for until one final synchronize give the bits of the same calls with a wait after each: the numbers of every
    view, the union's count and ids and the records after every step, and the final records, m and v."""
    pytest.importorskip("torch")
    want = two_view_answer()
    got = run_batches(how, BATCH_STEPS, (0.5, 0.5))
    assert np.array_equal(bits(got["numbers"]), bits(want["numbers"]))
    for s in range(BATCH_STEPS):
        count = int(want["count"][s].view(np.uint32)[0])
        assert np.array_equal(got["count"][s], want["count"][s]), ("step", s, "count")
        assert np.array_equal(got["ids"][s][:count], want["ids"][s][:count]), ("step", s, "ids")
        assert np.array_equal(bits(got["records"][s]), bits(want["records"][s])), ("step", s, "records")
    for name in ("final_records", "m", "v"):
        assert np.array_equal(bits(got[name]), bits(want[name])), name


@pytest.mark.parametrize("space", ["records", "raw"])
def test_step_batch_of_one_view_is_step(space):
    """B = 1 with weights [1.0]: after three steps records, m and v (and the numbers) are the bits step() leaves."""
    pytest.importorskip("torch")
    want = run_batches("step", BATCH_STEPS, None, cams=(1,), space=space)
    got = run_batches("step_batch", BATCH_STEPS, [1.0], cams=(1,), space=space)
    assert np.array_equal(bits(got["numbers"]), bits(want["numbers"])) and np.all(np.isfinite(want["numbers"]))
    for name in ("final_records", "m", "v"):
        assert np.array_equal(bits(got[name]), bits(want[name])), name
    assert want["v"].any() and not np.array_equal(bits(want["final_records"]), bits(dense_inputs()[0]))


def test_step_batch_is_adam_on_the_host_computed_union():
    """B = 2, the default weights 1/2: one step_batch moves records, m and v as adam_rows_ref (tests/test_adam_cpu.py) does with the
    union the restatement makes of the two frames' lists; with track_density, seen counts the views that listed a splat."""
    pytest.importorskip("torch")
    a = two_view_answer()
    aos = dense_inputs()[0]
    n = len(aos)
    ids, rows, count, mark = union_ref(a, 0, (0.5, 0.5), n)
    zeros = np.zeros_like(aos)
    want = adam_rows_ref(aos, zeros, zeros, ids, rows, count, n, n, params_dict(gs.default_adam_params(step=1)), np.float32)
    got = run_batches("step_batch", 1, None, track_density=True)
    for name, w in zip(("final_records", "m", "v"), want):
        same_floats(got[name], w, name)
    assert np.array_equal(got["seen"], mark) and set(np.unique(mark)) == {0, 1, 2}


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------

def test_refusals(bare):
    """Every refusal of the header returns GS_ERR_INVALID with its message and enqueues nothing: acc, mark and the sentinel-filled
    outputs are unchanged after gs_synchronize; the valid calls afterwards work."""
    import torch
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n = 10
    acc = torch.full((n, 84), 3.0, device=dev)
    mark = torch.ones(n, dtype=torch.int32, device=dev)
    rows = torch.ones(n, 84, device=dev)
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    count = torch.tensor([n], dtype=torch.int32, device=dev)
    ids_out = torch.full((n,), SENTINEL_ID, dtype=torch.int32, device=dev)
    rows_out = torch.full((n, 84), SENTINEL_ROW, device=dev)
    count_out = torch.full((1,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    h = bare._ctx.handle
    vp = lambda x: C.c_void_p(x) if x else None
    inf, nan = float("inf"), float("nan")

    def accumulate(a, weight=1.0):
        return L.gs_rows_accumulate_device(h, vp(a[0]), vp(a[1]), a[2], vp(a[3]), vp(a[4]), vp(a[5]), a[6], weight)

    def collect(a):
        return L.gs_rows_collect_device(h, vp(a[0]), vp(a[1]), a[2], vp(a[3]), vp(a[4]), a[5], vp(a[6]))

    def refused(rc, word):
        msg = L.gs_last_error(h).decode()
        assert rc == _lib.GS_ERR_INVALID and word in msg, (rc, word, msg)

    def unchanged():
        bare.synchronize()
        assert torch.all(acc == 3.0) and torch.all(mark == 1) and torch.all(ids_out == SENTINEL_ID)
        assert torch.all(rows_out == SENTINEL_ROW) and int(count_out[0]) == -1

    good = [acc.data_ptr(), mark.data_ptr(), n, ids.data_ptr(), rows.data_ptr(), count.data_ptr(), n]
    for k in (0, 1, 3, 4, 5):                                               # any NULL pointer with max_rows > 0
        a = list(good)
        a[k] = 0
        refused(accumulate(a), "gs_rows_accumulate_device: null")
    a = list(good)
    a[2] = 0
    refused(accumulate(a), "n is 0")
    for bad in (inf, -inf, nan):
        refused(accumulate(good, bad), "weight")
    a = list(good)
    a[4] = acc.data_ptr() + 336 * (n - 1)                                   # grad_rows inside acc
    refused(accumulate(a), "acc aliases grad_rows")
    a[0], a[4] = rows.data_ptr() + 4, rows.data_ptr()                       # acc inside grad_rows
    refused(accumulate(a), "acc aliases grad_rows")
    unchanged()

    good_c = [acc.data_ptr(), mark.data_ptr(), n, ids_out.data_ptr(), rows_out.data_ptr(), n, count_out.data_ptr()]
    for k in (0, 1, 6):
        a = list(good_c)
        a[k] = 0
        refused(collect(a), "gs_rows_collect_device: null acc, mark or count_out")
    for bad_n, word in ((0, "n is 0"), (2 ** 31, "below 2^31"), (2 ** 32 - 1, "below 2^31")):
        a = list(good_c)
        a[2] = bad_n
        refused(collect(a), word)
    for k in (3, 4):
        a = list(good_c)
        a[k] = 0
        refused(collect(a), "gs_rows_collect_device: null ids_out or rows_out with max_rows > 0")
    a = list(good_c)
    a[4] = acc.data_ptr() + 336 * (n - 1)
    refused(collect(a), "rows_out aliases acc")
    a = list(good_c)
    a[3] = mark.data_ptr() + 4 * (n - 1)
    refused(collect(a), "aliases mark")
    a = list(good_c)
    a[6] = mark.data_ptr() + 4
    refused(collect(a), "aliases mark")
    unchanged()

    # max_rows == 0: the accumulate launches nothing (NULL arrays allowed); the collect counts and clears
    assert accumulate([0, 0, n, 0, 0, 0, 0]) == _lib.GS_OK and accumulate(good[:6] + [0]) == _lib.GS_OK
    unchanged()
    assert collect([acc.data_ptr(), mark.data_ptr(), n, 0, 0, 0, count_out.data_ptr()]) == _lib.GS_OK
    bare.synchronize()
    assert int(count_out[0]) == n and not mark.any() and torch.all(acc == 3.0) and torch.all(rows_out == SENTINEL_ROW)
    # and the valid pair: a first touch stores 2 * 1 over the 3s, the collect lists all ten
    assert accumulate(good, 2.0) == _lib.GS_OK and collect(good_c) == _lib.GS_OK
    bare.synchronize()
    got = rows_out.cpu().numpy()
    assert int(count_out[0]) == n and np.array_equal(ids_out.cpu().numpy(), np.arange(n)) and not mark.any()
    assert np.all(got[:, FIELDS] == 2.0) and not bits(got)[:, UNTOUCHED].any()
