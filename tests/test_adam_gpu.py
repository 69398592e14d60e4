"""gs_adam_rows_device and gs_upload_rows_device on the MI355X (include/gsplat.h): the Adam step bit for bit against its NumPy
float32 restatement (tests/test_adam_cpu.py), the sparse in-place upload bit for bit against the full one, the refusals, the
five-call training step enqueued without a host wait against the same steps with a wait after every call, and
autograd.VisibleAdam training a small scene."""
import ctypes as C
import functools

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_adam_cpu import FIELDS, UNTOUCHED, adam_rows_ref, params_dict
from test_backward_gpu import SCENES
from test_loss_cpu import BG
from test_parity_gpu import make_renderer, make_scene
from test_train_chain_gpu import CAMERAS, LAMBDA, STEPS, bits, chain_inputs, new_renderer

pytestmark = pytest.mark.gpu

# ---- 1. bits against the restatement --------------------------------------------------------------------------------------

N = 300                                    # not a multiple of 64; every tensor has N + 1 rows and n = N is passed
CANARY = 42                                # a valid row no list names: ids past count point at it
SENTINEL = 0xFFC12345                      # a NaN with a payload: arithmetic on it, or a float load and store that canonicalises, shows
LISTED = [0, 7, 31, N, 64] + list(range(100, 170)) + [200, 250, N - 1]      # 0, N - 1, a run of 70, isolated ids, one id == N
K = len(LISTED)
CASES = [(0, 8), (1, 1), (63, 64), (64, 64), (65, 64), (K, N)]
ADAM_STEPS = 3
# every group its own rate; beta2 = 0.95 so that a gradient of 1e20 takes v' to +inf: (0.05 * 1e20) * 1e20 > FLT_MAX
TEST_PARAMS = dict(beta1=0.8, beta2=0.95, lr=[1e-3, 5e-3, 2e-3, 3e-3, 1.5, 7e-4])


@functools.lru_cache(maxsize=None)
def adam_inputs():
    """records / m / v [N + 1, 84] with the sentinel in the 25 untouched floats (m, v zero in the fields), and the gradient
    rows [N, 84] of three steps: random magnitudes over six decades with exact zeros, and in rows 0..2 the designed values --
    1e-30 and 3e-21 (v' underflows to 0 / is subnormal), 1e20 (v' = +inf: the field must not move), a scale pushed below lo,
    opacities pushed beyond hi and below lo, one NaN."""
    rng = np.random.default_rng(2024)
    f = np.float32
    rec = rng.uniform(0.05, 1.0, (N + 1, 84)).astype(f)
    rec[0, 4] = 1e-3                        # one scale step of 5e-3 takes it below lo = 1e-7
    rec[0, 15], rec[7, 15] = 0.99, 0.01     # one opacity step of 1.5 takes them beyond hi = 1 / below lo = 0
    m, v = np.zeros_like(rec), np.zeros_like(rec)
    for a in (rec, m, v):
        a.view(np.uint32)[:, UNTOUCHED] = SENTINEL
    grads = []
    for t in range(ADAM_STEPS):
        g = (rng.standard_normal((N, 84)) * 10.0 ** rng.integers(-4, 3, (N, 84))).astype(f)
        g[rng.random((N, 84)) < 0.1] = 0.0
        g.view(np.uint32)[:, UNTOUCHED] = SENTINEL                     # never read
        g[0, 0], g[0, 1], g[0, 2], g[0, 5] = 0.0, 1e-30, 1e20, 3e-21
        g[0, 4] = 2.0                                                  # scale 1e-3 -> below lo
        g[0, 15] = -1.0 if t != 1 else 40.0                            # opacity 0.99 -> above hi, then (m turns) below lo
        g[1, 15] = 3.0                                                 # row 1 is splat 7: opacity 0.01 -> below lo
        g[2, 8] = np.nan if t == 1 else g[2, 8]                        # one NaN, from the second step on it stays
        grads.append(g)
    return rec, m, v, grads


def ids_for(count):
    """The id buffer of a case: the list up to count, the canary behind it."""
    ids = np.full(N, CANARY, np.uint32)
    k = min(count, K)
    ids[:k] = LISTED[:k]
    return ids


def same_floats(got, want, what):
    """Bit equality; in the 59 fields a NaN is compared by position only."""
    gb, wb = bits(got), bits(want)
    assert np.array_equal(gb[:, UNTOUCHED], wb[:, UNTOUCHED]), (what, "untouched floats")
    g, w = got[:, FIELDS], want[:, FIELDS]
    assert np.array_equal(np.isnan(g), np.isnan(w)), (what, "NaN positions")
    ok = ~np.isnan(w)
    assert np.array_equal(gb[:, FIELDS][ok], wb[:, FIELDS][ok]), (what, "fields", int(np.sum(gb[:, FIELDS][ok] != wb[:, FIELDS][ok])))


@pytest.fixture(scope="module")
def bare():
    """A context without a scene and without a resolution: all gs_adam_rows_device needs."""
    pytest.importorskip("torch")
    r = gs.Renderer(64, 64, record_timings=False)
    r.init(gs.ResourceManager())
    yield r
    r.cleanup()


@pytest.mark.parametrize("count,max_rows", CASES)
def test_adam_bits_against_the_restatement(bare, count, max_rows):
    """Three consecutive steps (step = 1, 2, 3) on N = 300 records: records, m and v equal adam_rows_ref(float32) bit for bit
    after every step; every unlisted row, the canary, the spare row N (the list names it: an id == n is skipped), the 25
    sentinel floats of every row, and the gradient rows, ids and count themselves keep their bits."""
    import torch
    rec, m, v, grads = adam_inputs()
    ids = ids_for(count)
    dev = torch.device("cuda:0")
    up = lambda a: torch.tensor(a.view(np.int32), device=dev)           # bits, whatever they spell
    d_rec, d_m, d_v, d_ids = up(rec), up(m), up(v), up(ids)
    d_count = torch.tensor([count], dtype=torch.int32, device=dev)
    d_grads = [up(g) for g in grads]
    down = lambda t: t.cpu().numpy().view(np.float32)
    torch.cuda.synchronize()
    want = (rec, m, v)
    moved = set(int(i) for i in ids[:min(count, max_rows)] if i < N)
    for t in range(ADAM_STEPS):
        p = gs.default_adam_params(step=t + 1, **TEST_PARAMS)
        want = adam_rows_ref(*want, ids, grads[t], count, max_rows, N, params_dict(p), np.float32)
        bare.adamRowsDevice(d_rec.data_ptr(), d_m.data_ptr(), d_v.data_ptr(), N, d_ids.data_ptr(), d_grads[t].data_ptr(),
                            d_count.data_ptr(), max_rows, p)
        bare.synchronize()
        for name, got, w in zip(("records", "m", "v"), (down(d_rec), down(d_m), down(d_v)), want):
            same_floats(got, w, (name, "step", t + 1))
        assert np.array_equal(d_grads[t].cpu().numpy(), grads[t].view(np.int32)) and np.array_equal(d_ids.cpu().numpy(), ids.view(np.int32))
        assert int(d_count.cpu()[0]) == count
    # the answer itself: what was listed moved, nothing else did, and the designed values did what they were designed for
    got = down(d_rec)
    untouched_rows = [g for g in range(N + 1) if g not in moved]
    assert CANARY in untouched_rows and N in untouched_rows
    for name, start, end in (("records", rec, got), ("m", m, down(d_m)), ("v", v, down(d_v))):
        assert np.array_equal(bits(end[untouched_rows]), bits(start[untouched_rows])), name
        assert np.all(bits(end)[:, UNTOUCHED] == SENTINEL), name
    for g in moved:
        assert not np.array_equal(bits(got[g]), bits(rec[g])), g
    if count >= 1:
        assert np.isinf(down(d_v)[0, 2]) and got[0, 2] == rec[0, 2] and got[0, 4] == np.float32(1e-7) and got[0, 15] == 0.0
        assert want[0][0, 15] == 0.0 and adam_rows_ref(rec, m, v, ids, grads[0], count, max_rows, N,
                                                       params_dict(gs.default_adam_params(step=1, **TEST_PARAMS)), np.float32)[0][0, 15] == 1.0
    if count >= 3 and max_rows >= 3:
        assert got[7, 15] == 0.0 and np.isnan(got[31, 8]) and not np.isnan(got[31, 9])


# ---- 2. the sparse upload equals the full upload ----------------------------------------------------------------------------

BAND = (0, 2)                               # tile rows of the second comparison
BUFFERS = ("BUF_COLOR", "BUF_COV", "BUF_SORTED_TILE", "BUF_SORTED_DEPTH", "BUF_SORTED_ID", "BUF_RANGES")


def frame_state(r, sc):
    out = {"frame": r.draw(sc).copy()}
    for name in BUFFERS:
        out[name] = r.debugRead(getattr(gs, name)).copy()
    return out


@functools.lru_cache(maxsize=None)
def upload_case():
    """The dense scene, the listed rows and their new records.  One listed splat moves onto a splat the band's list holds
    (position, scale and rotation: the same footprint), from a 64-splat block none of whose splats the band lists and whose
    box does not contain the new position."""
    aos, w, h = SCENES["dense"]()
    aos = np.ascontiguousarray(aos, dtype=np.float32)
    n = len(aos)
    sc = make_scene(aos, w, h)
    r = make_renderer(sc, w, h)
    r.setTileRows(*BAND)
    r.draw(sc)
    in_band = np.unique(r.debugRead(gs.BUF_SORTED_ID))
    r.cleanup()
    assert 0 < len(in_band) < n
    blocks = np.setdiff1d(np.arange(n // 64), np.unique(in_band // 64))
    mover = donor = None
    for b in blocks:
        box_lo, box_hi = aos[b * 64:(b + 1) * 64, 0:3].min(0), aos[b * 64:(b + 1) * 64, 0:3].max(0)
        for d in in_band:
            if np.any(aos[d, 0:3] < box_lo - 0.5) or np.any(aos[d, 0:3] > box_hi + 0.5):
                mover, donor = int(b) * 64 + 17, int(d)
                break
        if mover is not None:
            break
    assert mover is not None, "no block outside the band"
    rng = np.random.default_rng(9)
    others = np.setdiff1d(rng.choice(n, 220, replace=False), [mover, 3000])
    ids = np.unique(np.concatenate([[0, n - 1, mover], np.arange(640, 700), others])).astype(np.uint32)
    ids = np.concatenate([ids, [n]]).astype(np.uint32)                   # one id == n: skipped
    changed = aos.copy()
    listed = ids[:-1]
    changed[listed, 0:3] += 0.02 * rng.standard_normal((len(listed), 3)).astype(np.float32)
    changed[listed, 4:7] *= rng.uniform(0.7, 1.4, (len(listed), 3)).astype(np.float32)
    changed[listed[5], 8:12] = (0.3, -0.2, 0.5, 0.8)                   # a rotation, not unit
    changed[listed, 12:76] += 0.05 * rng.standard_normal((len(listed), 64)).astype(np.float32)     # SH and opacity
    changed[listed, 15] = np.clip(changed[listed, 15], 0.05, 0.99)
    changed[mover, 0:3], changed[mover, 4:7], changed[mover, 8:12] = aos[donor, 0:3], aos[donor, 4:7], aos[donor, 8:12]
    changed[3000, 0:16] += 0.25                                         # an UNLISTED row: must not be uploaded
    assert 3000 not in listed
    full = aos.copy()
    full[listed] = changed[listed]
    return aos, w, h, ids, changed, full, mover


@pytest.mark.parametrize("sort", [gs.GS_SORT_RADIX4, gs.GS_SORT_RADIX4_SPLAT_FIRST], ids=["radix4", "radix4_splat_first"])
def test_sparse_upload_equals_full_upload(sort):
    """Context A uploads the listed rows of the changed records in place; context B uploads, in full, the original records
    with only the listed rows replaced.  The frame, GS_BUF_COLOR, GS_BUF_COV, the sorted list and the ranges are equal byte
    for byte on the whole frame, and again on a band of tile rows that the moved splat enters: a context that owns a band
    culls whole 64-splat blocks by their boxes, so stale block bounds would lose the moved splat there."""
    torch = pytest.importorskip("torch")
    aos, w, h, ids, changed, full, mover = upload_case()
    n = len(aos)
    sc = make_scene(aos, w, h)
    dev = torch.device("cuda:0")
    d_changed = torch.tensor(np.concatenate([changed, np.full((1, 84), np.nan, np.float32)]), device=dev)      # row n: never read
    d_full = torch.tensor(full, device=dev)
    d_ids = torch.tensor(np.concatenate([ids, np.full(50, 3000, np.uint32)]).view(np.int32), device=dev)       # past count: the unlisted row
    d_count = torch.tensor([len(ids)], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    A, B = make_renderer(sc, w, h, sort=sort), make_renderer(sc, w, h, sort=sort)
    before = frame_state(A, sc)
    # a frame is drawn: gs_backward would work now; after the sparse upload it is refused until the next frame, like after a full one
    A.uploadRowsDevice(d_changed.data_ptr(), n, d_ids.data_ptr(), d_count.data_ptr(), len(d_ids))
    with pytest.raises(gs.GsplatError) as ei:
        A.backward(np.ones((h, w, 4), np.float32))
    assert ei.value.code == _lib.GS_ERR_INVALID and "no frame since" in str(ei.value)
    B.uploadDevice(d_full.data_ptr(), n)
    a, b = frame_state(A, sc), frame_state(B, sc)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), ("whole frame", name)
    assert a["frame"].tobytes() != before["frame"].tobytes() and not np.array_equal(a["BUF_SORTED_ID"], before["BUF_SORTED_ID"])
    assert A.backward(np.ones((h, w, 4), np.float32)).any()                 # the new frame can be differentiated
    for r in (A, B):
        r.setTileRows(*BAND)
    a, b = frame_state(A, sc), frame_state(B, sc)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), ("band", name)
    assert mover in a["BUF_SORTED_ID"]                                      # it entered the band: its block's box was rebuilt
    A.cleanup()
    B.cleanup()


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------

def test_refusals(bare):
    """Every refusal of the header returns its code with a message and enqueues nothing; a valid call afterwards works."""
    import torch
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n = 10
    rec = torch.rand(n, 84, device=dev)
    m, v = torch.zeros_like(rec), torch.zeros_like(rec)
    rows = torch.ones(n, 84, device=dev)
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    count = torch.tensor([n], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    start = rec.cpu().numpy().copy()
    h = bare._ctx.handle
    good = [rec.data_ptr(), m.data_ptr(), v.data_ptr(), n, ids.data_ptr(), rows.data_ptr(), count.data_ptr(), n]
    vp = lambda x: C.c_void_p(x) if x else None

    def adam(args, p):
        a = list(args)
        return L.gs_adam_rows_device(h, vp(a[0]), vp(a[1]), vp(a[2]), a[3], vp(a[4]), vp(a[5]), vp(a[6]), a[7], None if p is None else C.byref(p))

    def refused(rc, word, code=_lib.GS_ERR_INVALID):
        msg = L.gs_last_error(h).decode()
        assert rc == code and word in msg, (rc, word, msg)

    inf, nan = float("inf"), float("nan")
    for k in (0, 1, 2, 4, 5, 6):                                            # any NULL pointer with max_rows > 0
        a = list(good)
        a[k] = 0
        refused(adam(a, gs.default_adam_params()), "gs_adam_rows_device: null")
    refused(adam(good, None), "null gs_adam_params")
    a = list(good)
    a[3] = 0
    refused(adam(a, gs.default_adam_params()), "n is 0")
    for size in (0, 88, 96):
        p = gs.default_adam_params()
        p.struct_size = size
        refused(adam(good, p), "struct_size")
    refused(adam(good, gs.default_adam_params(step=0)), "step")
    for kw in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan), dict(beta2=1.0), dict(beta2=-1e-3), dict(beta2=nan)):
        refused(adam(good, gs.default_adam_params(**kw)), "beta")
    for bad in (-1e-3, inf, nan):
        refused(adam(good, gs.default_adam_params(lr={gs.GS_ADAM_SH_DC: bad})), "lr")
        refused(adam(good, gs.default_adam_params(eps=bad)), "eps")
    refused(adam(good, gs.default_adam_params(lo={gs.GS_ADAM_SCALE: 2.0}, hi={gs.GS_ADAM_SCALE: 1.0})), "lo")
    refused(adam(good, gs.default_adam_params(lo={gs.GS_ADAM_POSITION: nan})), "lo")
    refused(adam(good, gs.default_adam_params(hi={gs.GS_ADAM_SH_REST: nan})), "lo")
    bare.synchronize()
    assert np.array_equal(bits(rec.cpu().numpy()), bits(start))              # nothing was enqueued
    a = list(good)
    a[7] = 0
    assert adam(a, gs.default_adam_params()) == _lib.GS_OK and adam([0, 0, 0, n, 0, 0, 0, 0], gs.default_adam_params()) == _lib.GS_OK
    bare.synchronize()
    assert np.array_equal(bits(rec.cpu().numpy()), bits(start))              # max_rows == 0: GS_OK, nothing launched
    assert adam(good, gs.default_adam_params()) == _lib.GS_OK
    bare.synchronize()
    assert np.all(rec.cpu().numpy()[:, FIELDS] != start[:, FIELDS])

    # gs_upload_rows_device
    upload = lambda hh, ptr, nn, i, c, mr: L.gs_upload_rows_device(hh, vp(ptr), nn, vp(i), vp(c), mr)
    refused(upload(h, rec.data_ptr(), n, ids.data_ptr(), count.data_ptr(), n), "no gaussians uploaded", _lib.GS_ERR_NO_SCENE)
    aos, w, hgt = SCENES["dense"]()
    sc = make_scene(aos, w, hgt)
    r = make_renderer(sc, w, hgt)
    hs, ns = r._ctx.handle, len(aos)
    d_aos = torch.tensor(np.ascontiguousarray(aos, dtype=np.float32), device=dev)
    torch.cuda.synchronize()

    def refused_s(rc, word, code=_lib.GS_ERR_INVALID):
        msg = L.gs_last_error(hs).decode()
        assert rc == code and word in msg, (rc, word, msg)

    r.draw(sc)
    refused_s(upload(hs, 0, ns, ids.data_ptr(), count.data_ptr(), n), "gs_upload_rows_device: null")
    refused_s(upload(hs, d_aos.data_ptr(), ns, 0, count.data_ptr(), n), "gs_upload_rows_device: null")
    refused_s(upload(hs, d_aos.data_ptr(), ns, ids.data_ptr(), 0, n), "gs_upload_rows_device: null")
    refused_s(upload(hs, d_aos.data_ptr(), 0, ids.data_ptr(), count.data_ptr(), n), "n is 0")
    refused_s(upload(hs, d_aos.data_ptr(), ns - 1, ids.data_ptr(), count.data_ptr(), n), "differs from the scene's")
    assert r.backward(np.ones((hgt, w, 4), np.float32)).any()                 # a refusal does not cost the frame its backward
    assert upload(hs, 0, ns, 0, 0, 0) == _lib.GS_OK                           # max_rows == 0
    seen = np.unique(r.debugRead(gs.BUF_SORTED_ID))[:n].astype(np.int64)     # splats that pass the culls: GS_BUF_COLOR shows their colour
    colour0 = r.debugRead(gs.BUF_COLOR)[seen].copy()
    d_seen = torch.tensor(seen, device=dev)
    d_aos[d_seen, 12:15] += 0.5
    ids_seen = d_seen.to(torch.int32)
    torch.cuda.synchronize()
    assert upload(hs, d_aos.data_ptr(), ns, ids_seen.data_ptr(), count.data_ptr(), n) == _lib.GS_OK
    r.draw(sc)
    assert len(seen) == n and np.all(np.any(r.debugRead(gs.BUF_COLOR)[seen] != colour0, axis=1))
    r.cleanup()


# ---- 4. and 5. the training step without waiting ------------------------------------------------------------------------------

def run_training(r, aos, scenes, make_target, lam, bg, how, adam_kw, history):
    """len(scenes) steps of upload (full, then rows) -> frame -> loss -> visible-row gradients -> Adam on the renderer r, the
    records starting as aos.  Returns host copies: numbers [steps][3], the final records / m / v, and with history the
    count, ids and records after every step (device-to-device copies on the working stream).
    how = "waiting": the context's own stream, a wait after every torch op and every library call (the answer);
          "caller_stream": a torch stream handed to gs_set_stream, nothing waited for between the first upload and the final
                           synchronize;
          "visible_adam": autograd.VisibleAdam.step, the targets made on the current stream, nothing waited for."""
    import torch
    from vk3dgaussiansplatting_amd.autograd import VisibleAdam
    steps, n = len(scenes), len(aos)
    h, w = r.height, r.width
    dev = torch.device("cuda:0")
    records = torch.tensor(aos, device=dev)
    numbers = [torch.full((3,), float("nan"), device=dev) for _ in range(steps)]
    hist = dict(count_hist=[torch.full((1,), -1, dtype=torch.int32, device=dev) for _ in range(steps)],
                ids_hist=[torch.full((n,), -1, dtype=torch.int32, device=dev) for _ in range(steps)],
                rows_hist=[torch.full((n, 84), float("nan"), device=dev) for _ in range(steps)],
                records_hist=[torch.full((n, 84), float("nan"), device=dev) for _ in range(steps)]) if history else None
    keep = []
    waiting = how == "waiting"

    def wait():
        if waiting:
            torch.cuda.synchronize()
            r.synchronize()

    if how == "visible_adam":
        opt = VisibleAdam(records, renderer=r, **adam_kw)
        for s in range(steps):
            target = make_target(s)
            keep.append(target)
            view, proj, pos, sh_mode = gs.Renderer._camera_args(scenes[s].getCamera())
            numbers[s] = opt.step(view, proj, pos, sh_mode, target, lam, bg)
        m, v = opt.m, opt.v
    else:
        m, v = torch.zeros_like(records), torch.zeros_like(records)
        ids = torch.zeros(n, dtype=torch.int32, device=dev)
        rows = torch.zeros(n, 84, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        grad = torch.zeros(h, w, 4, device=dev)
        stream = torch.cuda.Stream(device=dev) if how == "caller_stream" else None
        torch.cuda.synchronize()
        if stream is not None:
            r.setStream(stream.cuda_stream)

        def chain():
            for s in range(steps):
                if s == 0:
                    r.uploadDevice(records.data_ptr(), n)
                else:
                    r.uploadRowsDevice(records.data_ptr(), n, ids.data_ptr(), count.data_ptr(), n)
                wait()
                r.drawDevice(scenes[s], None, sync=False)
                wait()
                target = make_target(s)
                keep.append(target)
                wait()
                r.photometricLossDevice(None, target.data_ptr(), lam, bg, numbers[s].data_ptr(), grad.data_ptr())
                wait()
                r.backwardVisibleDevice(grad.data_ptr(), None, ids.data_ptr(), rows.data_ptr(), n, count.data_ptr())
                wait()
                r.adamRowsDevice(records.data_ptr(), m.data_ptr(), v.data_ptr(), n, ids.data_ptr(), rows.data_ptr(), count.data_ptr(), n,
                                 gs.default_adam_params(step=s + 1, **adam_kw))
                wait()
                if history:
                    hist["count_hist"][s].copy_(count)
                    hist["ids_hist"][s].copy_(ids)
                    hist["rows_hist"][s].copy_(rows)
                    hist["records_hist"][s].copy_(records)
                    wait()

        if stream is not None:
            with torch.cuda.stream(stream):
                chain()
        else:
            chain()
    torch.cuda.synchronize()                                            # the one wait of the unsynchronised forms
    r.synchronize()
    out = dict(numbers=np.stack([t.cpu().numpy() for t in numbers]), records=records.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy())
    if history:
        out.update({k: [t.cpu().numpy() for t in hist[k]] for k in hist})
    r.setStream(None)
    r.cleanup()
    return out


def run_chain(sort, timers, how):
    """The six steps of tests/test_train_chain_gpu.py's inputs: the camera alternates between its two poses, sh_mode cycles
    0, 1, 2, the target is a scaled image made by a torch op just before the loss reads it."""
    import torch
    aos, _, target_np, w, h = chain_inputs()
    scenes = [make_scene(aos, w, h, sh_mode=s % 3, **CAMERAS[s % 2]) for s in range(STEPS)]
    r = new_renderer(scenes[0], w, h, sort, timers)
    target0 = torch.tensor(target_np, device="cuda:0")
    torch.cuda.synchronize()
    return run_training(r, aos, scenes, lambda s: target0 * (1.0 - 0.05 * s), LAMBDA, BG, how, {}, history=True), aos


@functools.lru_cache(maxsize=None)
def chain_answer(timers):
    """The waiting form, checked not to be trivial: finite numbers that change from step to step; every step lists splats,
    ascending; the records a step changed are rows it listed, most of them; rows never listed keep their bits."""
    a, aos = run_chain(gs.GS_SORT_RADIX4, timers, "waiting")
    n = len(aos)
    prev, ever = aos, np.zeros(n, bool)
    for s in range(STEPS):
        assert np.all(np.isfinite(a["numbers"][s])) and a["numbers"][s].all()
        if s:
            assert not np.array_equal(bits(a["numbers"][s]), bits(a["numbers"][s - 1]))
        count = int(a["count_hist"][s].view(np.uint32)[0])
        ids = a["ids_hist"][s].view(np.uint32)[:count].astype(np.int64)
        assert 0 < count <= n and np.all(np.diff(ids) > 0) and ids[-1] < n
        changed = np.flatnonzero(np.any(bits(a["records_hist"][s]) != bits(prev), axis=1))
        with_gradient = ids[np.any(a["rows_hist"][s][:count] != 0, axis=1)]        # (a splat the frame cut off has a zero row)
        assert len(with_gradient) > 0 and np.all(np.isin(changed, ids)) and np.all(np.isin(with_gradient, changed)), (s, len(changed), count)
        assert np.all(np.isfinite(a["records_hist"][s]))
        ever[ids] = True
        prev = a["records_hist"][s]
    assert 0 < ever.sum() < n and np.array_equal(bits(a["records"][~ever]), bits(aos[~ever]))
    assert np.array_equal(bits(a["records"]), bits(prev))
    assert not a["m"][~ever].any() and not a["v"][~ever].any() and a["v"][ever].any()
    return a


@pytest.mark.parametrize("timers", [False, True], ids=["radix4-no_timers", "radix4-timers"])
def test_six_training_steps_enqueued_without_waiting(timers):
    """Upload (the first in full, the others of the rows the step before listed), frame, loss, visible-row gradients and the
    Adam step, six times on a caller's torch stream with nothing waited for between the first upload and one final
    synchronize, give the bits of the same steps with a wait after every call: the three numbers, count and ids[:count] of
    every step, and the final records, m and v."""
    pytest.importorskip("torch")
    want = chain_answer(timers)
    got, _ = run_chain(gs.GS_SORT_RADIX4, timers, "caller_stream")
    assert np.array_equal(bits(got["numbers"]), bits(want["numbers"]))
    for s in range(STEPS):
        count = int(want["count_hist"][s].view(np.uint32)[0])
        assert np.array_equal(got["count_hist"][s], want["count_hist"][s]), ("step", s, "count")
        assert np.array_equal(got["ids_hist"][s][:count], want["ids_hist"][s][:count]), ("step", s, "ids")
        assert np.array_equal(bits(got["records_hist"][s]), bits(want["records_hist"][s])), ("step", s, "records")
    for name in ("records", "m", "v"):
        assert np.array_equal(bits(got[name]), bits(want[name])), name


TRAIN_STEPS = 20


def test_visible_adam_trains():
    """autograd.VisibleAdam on the dense scene against a frame rendered from perturbed colours (the SH constant term moved
    by noise of 0.3), twenty steps at the default rates: the loss of step 20 is below that of step 1.  step() waits for
    nothing: its numbers and the final records, m and v are the bits of the five calls made by hand with a wait after each."""
    torch = pytest.importorskip("torch")
    aos, w, h = SCENES["dense"]()
    aos = np.ascontiguousarray(aos, dtype=np.float32)
    rng = np.random.default_rng(3)
    truth = aos.copy()
    truth[:, 12:15] += 0.3 * rng.standard_normal((len(aos), 3)).astype(np.float32)
    sc_truth, sc = make_scene(truth, w, h), make_scene(aos, w, h)
    r = new_renderer(sc_truth, w, h, gs.GS_SORT_RADIX4, False)
    r.draw(sc_truth)
    target_np = np.ascontiguousarray(r.readOutput(gs.GS_OUTPUT_RGBA32F)[..., :3])
    r.cleanup()
    target = torch.tensor(target_np, device="cuda:0")
    torch.cuda.synchronize()
    scenes = [sc] * TRAIN_STEPS
    out = {}
    for how in ("waiting", "visible_adam"):
        r = new_renderer(sc, w, h, gs.GS_SORT_RADIX4, False)
        out[how] = run_training(r, aos, scenes, lambda s: target, LAMBDA, None, how, {}, history=False)
    want, got = out["waiting"], out["visible_adam"]
    print("loss per step:", [float(x) for x in want["numbers"][:, 0]])
    assert np.all(np.isfinite(want["numbers"])) and np.all(np.isfinite(want["records"]))
    for name in ("numbers", "records", "m", "v"):
        assert np.array_equal(bits(got[name]), bits(want[name])), name
    assert want["numbers"][TRAIN_STEPS - 1, 0] < want["numbers"][0, 0], want["numbers"][:, 0]
