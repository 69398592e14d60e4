"""The raw parameter space on the MI355X (include/gsplat.h): gs_adam_rows_raw_device bit for bit against its NumPy float32
restatement (tests/test_raw_cpu.py), the two conversions, the opacity reset, the refusals, autograd.VisibleAdam(space="raw")
enqueued without a host wait against the same calls with a wait after each, training, density control and the .ply it saves."""
import ctypes as C
import functools

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_adam_cpu import FIELDS, UNTOUCHED, params_dict
from test_adam_gpu import CANARY, CASES, LISTED, N, SENTINEL, ids_for, same_floats
from test_backward_cpu import small_scene
from test_backward_gpu import SCENES
from test_loss_cpu import BG
from test_parity_gpu import make_scene
from test_raw_cpu import (F32, FLT_MIN, act_ref, adam_rows_raw_ref, convert_ply, first_leg_bounds, random_raw,
                          raw_from_records_ref)
from test_train_chain_gpu import CAMERAS, LAMBDA, STEPS, bits, chain_inputs, new_renderer

pytestmark = pytest.mark.gpu

ADAM_STEPS = 3
# every group its own rate; beta2 = 0.95 so that a gradient of 1e20 takes v' to +inf; the opacity group clamped to [-3, 3]:
# the clamp acts on the LOGIT
TEST_PARAMS = dict(beta1=0.8, beta2=0.95, lr=[1e-3, 5e-3, 2e-3, 3e-3, 1.5, 7e-4], lo={gs.GS_ADAM_OPACITY: -3.0},
                   hi={gs.GS_ADAM_OPACITY: 3.0})
LOGIT_PLUS_40, LOGIT_MINUS_40, TINY_ROT, HUGE_ROT, CLAMPED_UP = LISTED[1], LISTED[2], LISTED[4], LISTED[5], LISTED[6]


def sentinel_rest(a):
    a.view(np.uint32)[:, UNTOUCHED] = SENTINEL


def fields_equal(got, want, what):
    """Bit equality of the 59 fields; a NaN is compared by position only."""
    g, w = got[:, FIELDS], want[:, FIELDS]
    assert np.array_equal(np.isnan(g), np.isnan(w)), (what, "NaN positions")
    ok = ~np.isnan(w)
    assert np.array_equal(bits(g)[ok], bits(w)[ok]), (what, int(np.sum(bits(g)[ok] != bits(w)[ok])))


@functools.lru_cache(maxsize=None)
def raw_adam_inputs():
    """raw / records / m / v [N + 1, 84], records = act(raw) in the fields, the sentinel in the 25 floats no call touches, and
    the gradient rows [N, 84] of three steps (row i belongs to LISTED[i]).  The designed rows: splat 0 has the log-scales -200
    and +100 (the two clamps of E) and the position gradients 0, 1e-30, 1e20; splats 7 and 31 the logits +40 and -40; splat 64
    a rotation of length 1e-3, splat 100 one of length 1e3; splat 101 a logit the step pushes through hi = 3; list row 2
    (splat 31) has a NaN gradient on a position field in the second step alone (the field and its moments stay NaN after it)."""
    rng = np.random.default_rng(2025)
    raw = random_raw(rng, N + 1)
    raw[0, 4], raw[0, 5] = -200.0, 100.0
    raw[LOGIT_PLUS_40, 15], raw[LOGIT_MINUS_40, 15] = 40.0, -40.0
    raw[TINY_ROT, 8:12] *= F32(1e-3) / np.linalg.norm(raw[TINY_ROT, 8:12]).astype(F32)
    raw[HUGE_ROT, 8:12] *= F32(1e3) / np.linalg.norm(raw[HUGE_ROT, 8:12]).astype(F32)
    raw[CLAMPED_UP, 15] = 2.5
    rec = act_ref(raw, F32)
    m, v = np.zeros_like(raw), np.zeros_like(raw)
    for a in (raw, rec, m, v):
        sentinel_rest(a)
    grads = []
    for t in range(ADAM_STEPS):
        g = (rng.standard_normal((N, 84)) * 10.0 ** rng.integers(-4, 3, (N, 84))).astype(F32)
        g[rng.random((N, 84)) < 0.1] = 0.0
        sentinel_rest(g)                                                # never read
        g[0, 0], g[0, 1], g[0, 2] = 0.0, 1e-30, 1e20
        g[0, 4], g[0, 5] = 1.0, 1e-30                                   # times the scales 2^-126 and 2^126
        g[6, 15] = -1.0                                                 # list row 6 is splat 101: the logit 2.5 goes up by 1.5
        g[1, 15], g[2, 15] = -1.0, 1.0                                  # splats 7 and 31: pushed further out, held by hi and lo
        g[2, 0] = np.nan if t == 1 else g[2, 0]
        grads.append(g)
    return raw, rec, m, v, grads


@pytest.fixture(scope="module")
def bare():
    """A context without a scene and without a resolution: all the raw-space calls need."""
    pytest.importorskip("torch")
    r = gs.Renderer(64, 64, record_timings=False)
    r.init(gs.ResourceManager())
    yield r
    r.cleanup()


def up(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a).view(np.int32), device="cuda:0")      # bits, whatever they spell


def down(t):
    return t.cpu().numpy().view(np.float32)


# ---- 1. the Adam step bit for bit -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count,max_rows", CASES)
def test_raw_adam_bits_against_the_restatement(bare, count, max_rows):
    """Three consecutive steps on N = 300 rows (19 quads a row against 256 lanes a block: block edges fall inside rows): raw,
    records, m and v equal adam_rows_raw_ref(float32) bit for bit after every step, and records[listed] == act_ref(raw[listed])
    -- the invariant the next step's chain stands on.  Unlisted rows, the canary behind the count, row N (an id == n is
    skipped), the 25 sentinel floats of every row, the gradient rows, ids and count keep their bits."""
    import torch
    raw, rec, m, v, grads = raw_adam_inputs()
    ids = ids_for(count)
    d = [up(a) for a in (raw, rec, m, v)]
    d_ids, d_count = up(ids), torch.tensor([count], dtype=torch.int32, device="cuda:0")
    d_grads = [up(g) for g in grads]
    torch.cuda.synchronize()
    want = (raw, rec, m, v)
    moved = sorted(set(int(i) for i in ids[:min(count, max_rows)] if i < N))
    names = ("raw", "records", "m", "v")
    for t in range(ADAM_STEPS):
        p = gs.default_adam_params(space="raw", step=t + 1, **TEST_PARAMS)
        want = adam_rows_raw_ref(*want, ids, grads[t], count, max_rows, N, params_dict(p), F32)
        bare.adamRowsRawDevice(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), N, d_ids.data_ptr(),
                               d_grads[t].data_ptr(), d_count.data_ptr(), max_rows, p)
        bare.synchronize()
        got = [down(x) for x in d]
        for name, g_, w_ in zip(names, got, want):
            same_floats(g_, w_, (name, "step", t + 1))
        if moved:
            fields_equal(got[1][moved], act_ref(got[0][moved], F32), ("records == act(raw)", "step", t + 1))
        assert np.array_equal(d_grads[t].cpu().numpy(), grads[t].view(np.int32)) and np.array_equal(d_ids.cpu().numpy(), ids.view(np.int32))
        assert int(d_count.cpu()[0]) == count
    got = [down(x) for x in d]
    untouched_rows = [g for g in range(N + 1) if g not in moved]
    assert CANARY in untouched_rows and N in untouched_rows
    for name, start, end in zip(names, (raw, rec, m, v), got):
        assert np.array_equal(bits(end[untouched_rows]), bits(start[untouched_rows])), name
        assert np.all(bits(end)[:, UNTOUCHED] == SENTINEL), name
    for g in moved:
        assert not np.array_equal(bits(got[0][g]), bits(raw[g])) and not np.array_equal(bits(got[1][g]), bits(rec[g])), g
    # the designed values did what they were designed for
    if count >= 1:
        assert rec[0, 4] == F32(2.0 ** -126) and rec[0, 5] == F32(2.0 ** 126)                 # the two clamps of E
        assert np.isinf(got[3][0, 2]) and got[0][0, 2] == raw[0, 2] and got[1][0, 2] == raw[0, 2]    # 1e20: v' = +inf, no move
        assert np.all(np.isfinite(got[0][0, 4:7])) and np.all(got[1][0, 4:7] > 0)
    if count >= 7 and max_rows >= 7:
        assert rec[LOGIT_PLUS_40, 15] == 1.0 and 0 < rec[LOGIT_MINUS_40, 15] < 1e-17
        assert got[0][LOGIT_PLUS_40, 15] == 3.0 and got[0][LOGIT_MINUS_40, 15] == -3.0        # +40: o = 1, a zero chain gradient; -40: one of 4e-18; hi and lo hold the raw values
        assert got[0][CLAMPED_UP, 15] == 3.0 and got[1][CLAMPED_UP, 15] == act_ref(got[0][[CLAMPED_UP]], F32)[0, 15] and 0.95 < got[1][CLAMPED_UP, 15] < 0.96
        for g, length in ((TINY_ROT, 1e-3), (HUGE_ROT, 1e3)):
            assert abs(np.linalg.norm(raw[g, 8:12].astype(np.float64)) / length - 1) < 1e-6
            assert abs(np.linalg.norm(got[1][g, 8:12].astype(np.float64)) - 1) < 2.0 ** -22 and np.all(np.isfinite(got[0][g, 8:12]))
        assert np.isnan(got[0][LISTED[2], 0]) and np.isnan(got[1][LISTED[2], 0]) and not np.isnan(got[0][LISTED[2], 1])


# ---- 2. the conversions -----------------------------------------------------------------------------------------------------------

def test_conversions(bare):
    """n = 300 (no multiple of 64 or 256) of 301 rows.  gs_records_from_raw_device equals act_ref(float32) bit for bit on every
    row.  gs_raw_from_records_device against the float64 restatement within 2 ulp(theta) + 2^-22: one ulp for the device's
    logf, one for the rounding, the additive term for the rounded quotient of the logit (measured on an MI355X: the worst
    error is 0.73 of the bound, 3.1e-6 at log FLT_MIN); opacities of exactly 0 and 1 and a
    scale of 0 land on the documented clamps.  Both leave row n and the 25 other floats of every output row alone."""
    import torch
    raw, rec, _, _, _ = raw_adam_inputs()                                # designed rows included: both clamps of E, logits of +-40
    out = np.zeros((N + 1, 84), F32)
    out.view(np.uint32)[:] = SENTINEL
    d_raw, d_out = up(raw), up(out)
    torch.cuda.synchronize()
    bare.recordsFromRawDevice(d_raw.data_ptr(), d_out.data_ptr(), N)
    bare.synchronize()
    got = down(d_out)
    want = act_ref(raw, F32)
    fields_equal(got[:N], want[:N], "records_from_raw")
    assert not np.isnan(got[:N, FIELDS]).any()
    assert np.all(bits(got)[:, UNTOUCHED] == SENTINEL) and np.all(bits(got[N]) == SENTINEL)
    assert np.array_equal(bits(down(d_raw)), bits(raw))

    rng = np.random.default_rng(8)
    records = act_ref(random_raw(rng, N + 1), F32)
    records[:, 4:7] = np.exp(rng.uniform(np.log(1e-7), np.log(1e4), (N + 1, 3))).astype(F32)
    records[:, 15] = rng.uniform(0, 1, N + 1).astype(F32)
    records[0, 15], records[1, 15], records[2, 4], records[3, 5] = 0.0, 1.0, 0.0, 1e-42      # the clamps; a subnormal scale
    records[4, 15], records[5, 15] = 1e-9, F32(1.0 - 2.0 ** -24)
    sentinel_rest(records)
    d_rec, d_out = up(records), up(out)
    torch.cuda.synchronize()
    bare.rawFromRecordsDevice(d_rec.data_ptr(), d_out.data_ptr(), N)
    bare.synchronize()
    got = down(d_out)
    theta = raw_from_records_ref(records, np.float64)
    ident = [c for c in FIELDS if not (4 <= c < 7 or c == 15)]
    assert np.array_equal(bits(got[:N, ident]), bits(records[:N, ident]))                  # rotation and the rest: the same bits
    cols = [4, 5, 6, 15]
    err = np.abs(got[:N, cols].astype(np.float64) - theta[:N, cols])
    bound = 2 * np.spacing(np.abs(theta[:N, cols]).astype(F32)).astype(np.float64) + 2.0 ** -22
    print("raw_from_records: worst error / bound =", float(np.max(err / bound)), "worst |error| =", float(err.max()))
    assert np.all(err <= bound), float(np.max(err / bound))
    assert abs(got[0, 15] + 24 * np.log(2)) < 1e-5 and abs(got[1, 15] - 24 * np.log(2)) < 1e-5 and np.all(np.abs(got[:N, 15]) <= 16.7)
    assert abs(got[2, 4] - np.log(float(FLT_MIN))) < 1e-5 and abs(got[3, 5] - np.log(float(FLT_MIN))) < 1e-5
    assert np.all(bits(got)[:, UNTOUCHED] == SENTINEL) and np.all(bits(got[N]) == SENTINEL)
    assert np.array_equal(bits(down(d_rec)), bits(records))


# ---- 3. the opacity reset -----------------------------------------------------------------------------------------------------------

def test_opacity_reset(bare):
    """n = 300 of 301 rows with opacities on both sides of 0.01 and one exactly 0.01, which is kept: float 15 of raw and
    records matches the restatement bit for bit, float 15 of m and v is zero in every row, every other float of the four arrays
    keeps its bits.  The form without moments; the refusals."""
    import oracle
    import torch
    rng = np.random.default_rng(4)
    raw = random_raw(rng, N + 1)
    raw[:, 15] = rng.uniform(-9, 3, N + 1)
    rec = act_ref(raw, F32)
    cap = F32(0.01)
    rec[5, 15] = cap                                                    # exactly max_opacity: kept
    m, v = (rng.standard_normal((N + 1, 84)).astype(F32) for _ in range(2))
    for a in (raw, rec, m, v):
        sentinel_rest(a)
    above = np.flatnonzero(rec[:N, 15] > cap)
    assert 20 < len(above) < N - 20 and 5 not in above
    L = F32(np.log(float(cap) / (1.0 - float(cap))))
    want_raw, want_rec, want_m, want_v = (a.copy() for a in (raw, rec, m, v))
    want_raw[above, 15] = L
    want_rec[above, 15] = F32(1) / (F32(1) + oracle.exp(F32([-L]))[0])
    want_m[:N, 15] = 0.0
    want_v[:N, 15] = 0.0
    d = [up(a) for a in (raw, rec, m, v)]
    torch.cuda.synchronize()
    bare.resetOpacityRawDevice(*(x.data_ptr() for x in d), N, 0.01)
    bare.synchronize()
    for name, got, want in zip(("raw", "records", "m", "v"), d, (want_raw, want_rec, want_m, want_v)):
        assert np.array_equal(bits(down(got)), bits(want)), name
    assert down(d[1])[:N, 15].max() <= F32(0.0100001) and down(d[1])[5, 15] == cap and abs(want_rec[above[0], 15] - 0.01) < 1e-8
    # without moments
    d2 = [up(a) for a in (raw, rec)]
    torch.cuda.synchronize()
    bare.resetOpacityRawDevice(d2[0].data_ptr(), d2[1].data_ptr(), None, None, N, 0.01)
    bare.synchronize()
    assert np.array_equal(bits(down(d2[0])), bits(want_raw)) and np.array_equal(bits(down(d2[1])), bits(want_rec))


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals(bare):
    """Every refusal of the header returns its code with a message and enqueues nothing; a valid call afterwards works."""
    import torch
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n = 10
    raw = torch.tensor(random_raw(np.random.default_rng(1), n), device=dev)
    rec, m, v = torch.zeros_like(raw), torch.zeros_like(raw), torch.zeros_like(raw)
    rows = torch.ones(n, 84, device=dev)
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    count = torch.tensor([n], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    bare.recordsFromRawDevice(raw.data_ptr(), rec.data_ptr(), n)
    bare.synchronize()
    state = lambda: [bits(t.cpu().numpy()).copy() for t in (raw, rec, m, v)]
    start = state()
    h = bare._ctx.handle
    vp = lambda x: C.c_void_p(x) if x else None
    good = [raw.data_ptr(), rec.data_ptr(), m.data_ptr(), v.data_ptr(), n, ids.data_ptr(), rows.data_ptr(), count.data_ptr(), n]

    def adam(a, p):
        return L.gs_adam_rows_raw_device(h, vp(a[0]), vp(a[1]), vp(a[2]), vp(a[3]), a[4], vp(a[5]), vp(a[6]), vp(a[7]), a[8],
                                         None if p is None else C.byref(p))

    def refused(rc, word, code=_lib.GS_ERR_INVALID):
        msg = L.gs_last_error(h).decode()
        assert rc == code and word in msg, (rc, word, msg)

    dp = lambda **kw: gs.default_adam_params(space="raw", **kw)
    inf, nan = float("inf"), float("nan")
    for k in (0, 1, 2, 3, 5, 6, 7):                                        # any NULL pointer with max_rows > 0
        a = list(good)
        a[k] = 0
        refused(adam(a, dp()), "gs_adam_rows_raw_device: null")
    refused(adam(good, None), "gs_adam_rows_raw_device: null gs_adam_params")
    a = list(good)
    a[4] = 0
    refused(adam(a, dp()), "n is 0")
    for size in (0, 88, 96):
        p = dp()
        p.struct_size = size
        refused(adam(good, p), "struct_size")
    refused(adam(good, dp(step=0)), "step")
    for kw in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan), dict(beta2=1.0), dict(beta2=-1e-3), dict(beta2=nan)):
        refused(adam(good, dp(**kw)), "beta")
    for bad in (-1e-3, inf, nan):
        refused(adam(good, dp(lr={gs.GS_ADAM_SH_DC: bad})), "lr")
        refused(adam(good, dp(eps=bad)), "eps")
    refused(adam(good, dp(lo={gs.GS_ADAM_SCALE: 2.0}, hi={gs.GS_ADAM_SCALE: 1.0})), "lo")
    refused(adam(good, dp(lo={gs.GS_ADAM_POSITION: nan})), "lo")
    for k in (0, 2, 3):                                                    # records shares bytes with raw, m or v
        a = list(good)
        a[1] = a[k] + 336 * (n - 1)                                        # the last row of that array is the first of "records"
        refused(adam(a, dp()), "aliases")
    # the conversions
    conv = lambda f, a, b, nn: f(h, vp(a), vp(b), nn)
    for f, name in ((L.gs_records_from_raw_device, "gs_records_from_raw_device"), (L.gs_raw_from_records_device, "gs_raw_from_records_device")):
        refused(conv(f, 0, rec.data_ptr(), n), name + ": null")
        refused(conv(f, raw.data_ptr(), 0, n), name + ": null")
        refused(conv(f, raw.data_ptr(), rec.data_ptr(), 0), "n is 0")
        refused(conv(f, raw.data_ptr(), raw.data_ptr(), n), "aliases")
        refused(conv(f, raw.data_ptr(), raw.data_ptr() + 336 * (n - 1), n), "aliases")
    # the reset
    reset = lambda a, b, c_, d_, nn, cap: L.gs_reset_opacity_raw_device(h, vp(a), vp(b), vp(c_), vp(d_), nn, cap)
    ptrs = [t.data_ptr() for t in (raw, rec, m, v)]
    refused(reset(0, ptrs[1], ptrs[2], ptrs[3], n, 0.01), "gs_reset_opacity_raw_device: null")
    refused(reset(ptrs[0], 0, ptrs[2], ptrs[3], n, 0.01), "gs_reset_opacity_raw_device: null")
    refused(reset(ptrs[0], ptrs[1], ptrs[2], 0, n, 0.01), "together")
    refused(reset(ptrs[0], ptrs[1], 0, ptrs[3], n, 0.01), "together")
    refused(reset(*ptrs, 0, 0.01), "n is 0")
    for cap in (0.0, 1.0, -0.5, 1.5, nan):
        refused(reset(*ptrs, n, cap), "max_opacity")
    bare.synchronize()
    for a, b in zip(state(), start):
        assert np.array_equal(a, b)                                         # nothing was enqueued
    a = list(good)
    a[8] = 0
    assert adam(a, dp()) == _lib.GS_OK and adam([0, 0, 0, 0, n, 0, 0, 0, 0], dp()) == _lib.GS_OK     # max_rows == 0: nothing launched
    bare.synchronize()
    for a, b in zip(state(), start):
        assert np.array_equal(a, b)
    assert adam(good, dp()) == _lib.GS_OK
    bare.synchronize()
    after = state()
    assert np.all(after[0][:, FIELDS] != start[0][:, FIELDS]) and np.all(after[1][:, FIELDS] != start[1][:, FIELDS])
    assert reset(*ptrs, n, 0.5) == _lib.GS_OK
    assert conv(L.gs_raw_from_records_device, rec.data_ptr(), raw.data_ptr(), n) == _lib.GS_OK
    bare.synchronize()
    assert rec.cpu().numpy()[:, 15].max() <= 0.5 and np.all(raw.cpu().numpy()[:, 15] <= 0.0)


# ---- 5. the training step without waiting -------------------------------------------------------------------------------------------

def run_training_raw(r, aos, scenes, make_target, lam, bg, how, params=None, keep_first=False):
    """len(scenes) raw-space steps on the renderer r from the records aos: raw made by gs_raw_from_records_device, records
    rewritten as act(raw), then upload (full, then rows) -> frame -> loss -> visible-row gradients -> gs_adam_rows_raw_device.
    how = "waiting": the five calls by hand on the context's own stream with a wait after every call (the answer);
          "visible_adam": autograd.VisibleAdam(space="raw").step, nothing waited for.
    Returns host copies of the numbers and the final raw / records / m / v; with keep_first also the arrays before the first
    step and the ids, rows and count that step left."""
    import torch
    from vk3dgaussiansplatting_amd.autograd import VisibleAdam
    steps, n = len(scenes), len(aos)
    dev = torch.device("cuda:0")
    records = torch.tensor(aos, device=dev)
    numbers = [torch.full((3,), float("nan"), device=dev) for _ in range(steps)]
    first, keep = {}, []
    host = lambda t: t.cpu().numpy().copy()
    kw = params or {}
    if how == "visible_adam":
        opt = VisibleAdam(records, renderer=r, space="raw", **kw)
        for s in range(steps):
            target = make_target(s)
            keep.append(target)
            numbers[s] = opt.step(*gs.Renderer._camera_args(scenes[s].getCamera()), target, lam, bg)
        raw, m, v = opt.raw, opt.m, opt.v
    else:
        raw, m, v = torch.zeros_like(records), torch.zeros_like(records), torch.zeros_like(records)
        ids = torch.zeros(n, dtype=torch.int32, device=dev)
        rows = torch.zeros(n, 84, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        grad = torch.zeros(r.height, r.width, 4, device=dev)

        def wait():
            torch.cuda.synchronize()
            r.synchronize()

        wait()
        r.rawFromRecordsDevice(records.data_ptr(), raw.data_ptr(), n)
        wait()
        r.recordsFromRawDevice(raw.data_ptr(), records.data_ptr(), n)
        wait()
        if keep_first:
            first.update(raw0=host(raw), records0=host(records))
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
            r.adamRowsRawDevice(raw.data_ptr(), records.data_ptr(), m.data_ptr(), v.data_ptr(), n, ids.data_ptr(), rows.data_ptr(),
                                count.data_ptr(), n, gs.default_adam_params(space="raw", step=s + 1, **kw))
            wait()
            if keep_first and s == 0:
                first.update(ids=host(ids).view(np.uint32), rows=host(rows), count=int(host(count).view(np.uint32)[0]),
                             raw1=host(raw), records1=host(records), m1=host(m), v1=host(v))
    torch.cuda.synchronize()
    r.synchronize()
    out = dict(numbers=np.stack([host(t) for t in numbers]), raw=host(raw), records=host(records), m=host(m), v=host(v), **first)
    r.setStream(None)
    r.cleanup()
    return out


def test_six_raw_steps_without_waiting():
    """VisibleAdam(space="raw").step six times on chain_inputs()'s scene, the camera alternating and sh_mode cycling, against
    the same five calls made by hand with a wait after every one: the numbers and the final raw, records, m and v are equal bit
    for bit.  And with the ids, rows and count step 1 left on the device, adam_rows_raw_ref(float32) applied to the starting
    arrays gives raw, records, m and v after step 1 bit for bit: the chain against real gradient rows."""
    torch = pytest.importorskip("torch")
    aos, _, target_np, w, h = chain_inputs()
    n = len(aos)
    scenes = [make_scene(aos, w, h, sh_mode=s % 3, **CAMERAS[s % 2]) for s in range(STEPS)]
    target0 = torch.tensor(target_np, device="cuda:0")
    torch.cuda.synchronize()
    make_target = lambda s: target0 * (1.0 - 0.05 * s)
    out = {}
    for how in ("waiting", "visible_adam"):
        r = new_renderer(scenes[0], w, h, gs.GS_SORT_RADIX4, False)
        out[how] = run_training_raw(r, aos, scenes, make_target, LAMBDA, BG, how, keep_first=how == "waiting")
    want, got = out["waiting"], out["visible_adam"]
    assert np.all(np.isfinite(want["numbers"])) and want["numbers"].all()
    for name in ("numbers", "raw", "records", "m", "v"):
        assert np.array_equal(bits(got[name]), bits(want[name])), name
    fields_equal(want["records"], act_ref(want["raw"], F32), "records == act(raw) at the end")
    count = want["count"]
    assert 0 < count <= n and np.any(want["rows"][:count] != 0)
    p = params_dict(gs.default_adam_params(space="raw", step=1))
    zeros = np.zeros((n, 84), F32)
    ref = adam_rows_raw_ref(want["raw0"], want["records0"], zeros, zeros, want["ids"], want["rows"], count, n, n, p, F32)
    for name, a in zip(("raw1", "records1", "m1", "v1"), ref):
        assert np.array_equal(bits(want[name]), bits(a)), name
    assert not np.array_equal(bits(want["raw1"]), bits(want["raw0"]))


# ---- 6. it trains, with the geometry moving -----------------------------------------------------------------------------------------

TRAIN_STEPS = 20


def train_series(aos, truth, w, h, space):
    """Twenty steps of VisibleAdam(space) at its default rates from aos against the frame of truth -> (numbers, the optimiser's
    final records on the host)."""
    import torch
    from vk3dgaussiansplatting_amd.autograd import VisibleAdam
    sc_truth, sc = make_scene(truth, w, h), make_scene(aos, w, h)
    r = new_renderer(sc_truth, w, h, gs.GS_SORT_RADIX4, False)
    r.draw(sc_truth)
    target = torch.tensor(np.ascontiguousarray(r.readOutput(gs.GS_OUTPUT_RGBA32F)[..., :3]), device="cuda:0")
    r.cleanup()
    torch.cuda.synchronize()
    r = new_renderer(sc, w, h, gs.GS_SORT_RADIX4, False)
    opt = VisibleAdam(torch.tensor(aos, device="cuda:0"), renderer=r, space=space)
    cam = gs.Renderer._camera_args(sc.getCamera())
    numbers = [opt.step(*cam, target, LAMBDA) for _ in range(TRAIN_STEPS)]
    opt.stream.synchronize()
    series = np.stack([t.cpu().numpy() for t in numbers])
    records = opt.records.cpu().numpy()
    r.setStream(None)
    r.cleanup()
    return series, records


def test_raw_space_trains():
    """VisibleAdam(space="raw") on the dense scene at the default raw rates, twenty steps against the frame of the cloud with
    its SH constant term moved by noise of 0.3 (the case test_visible_adam_trains shows to descend in record space): the loss of
    step 20 is below that of step 1; every record stays finite, scales > 0, opacities in [0, 1], every record rotation within
    2^-22 of unit length.  The same with the log-scales of the truth moved by +-0.3 is printed next to the record-space series
    under the same rates: recorded in profiles/raw_space_training.txt, not asserted."""
    pytest.importorskip("torch")
    aos, w, h = SCENES["dense"]()
    aos = np.ascontiguousarray(aos, dtype=F32)
    rng = np.random.default_rng(3)
    truth = aos.copy()
    truth[:, 12:15] += 0.3 * rng.standard_normal((len(aos), 3)).astype(F32)
    series, rec = train_series(aos, truth, w, h, "raw")
    print("raw space, SH truth, loss per step:", [round(float(x), 6) for x in series[:, 0]])
    assert np.all(np.isfinite(series)) and np.all(np.isfinite(rec[:, FIELDS]))
    assert np.all(rec[:, 4:7] > 0) and np.all(rec[:, 15] >= 0) and np.all(rec[:, 15] <= 1)
    assert np.all(np.abs(np.linalg.norm(rec[:, 8:12].astype(np.float64), axis=1) - 1) <= 2.0 ** -22)
    assert series[TRAIN_STEPS - 1, 0] < series[0, 0], series[:, 0]
    truth = aos.copy()
    truth[:, 4:7] *= np.exp(rng.choice(F32([-0.3, 0.3]), (len(aos), 3))).astype(F32)
    for space in ("raw", "records"):
        series, _ = train_series(aos, truth, w, h, space)
        print(f"{space} space, log-scale truth, loss per step:", [round(float(x), 6) for x in series[:, 0]])


# ---- 7. density control, the reset and the .ply in raw space ----------------------------------------------------------------------------

def test_raw_space_densify_reset_and_save(tmp_path):
    """VisibleAdam(space="raw", track_density=True) on the small scene, put into the loader's order first.  save_ply then
    gs_convert_ply gives opt.records under the bounds of the first leg of the CPU round trip, in the same order.  After
    densify() raw has n_out rows, records == act_ref(raw) bit for bit, a split child's log-scale is within 4 ulp of
    log(parent / 1.6), and the next step runs as a new scene.  After reset_opacity(0.01) no record opacity exceeds sigmoid(L)
    and the next frame shows it: the full upload happened."""
    torch = pytest.importorskip("torch")
    import oracle
    from vk3dgaussiansplatting_amd.autograd import VisibleAdam
    aos, w, h = small_scene()
    p0 = str(tmp_path / "start.ply")
    gs.write_ply(p0, np.ascontiguousarray(aos, dtype=F32), "records")
    aos = convert_ply(p0)                                               # the loader's Morton order
    n = len(aos)
    rng = np.random.default_rng(3)
    truth = aos.copy()
    truth[:, 12:15] += 0.3 * rng.standard_normal((n, 3)).astype(F32)
    truth[:, 0:3] += 0.01 * rng.standard_normal((n, 3)).astype(F32)
    sc_truth, sc = make_scene(truth, w, h), make_scene(aos, w, h)
    r = new_renderer(sc_truth, w, h, gs.GS_SORT_RADIX4, False)
    r.draw(sc_truth)
    target = torch.tensor(np.ascontiguousarray(r.readOutput(gs.GS_OUTPUT_RGBA32F)[..., :3]), device="cuda:0")
    r.cleanup()
    cam = gs.Renderer._camera_args(sc.getCamera())
    r = new_renderer(sc, w, h, gs.GS_SORT_RADIX4, False)
    opt = VisibleAdam(torch.tensor(aos, device="cuda:0"), renderer=r, space="raw", track_density=True)
    host = lambda t: t.cpu().numpy()
    fields_equal(host(opt.records), act_ref(host(opt.raw), F32), "records == act(raw) from the start")
    # save_ply: the parameters exactly, the loader gives the records again, in the same order
    p1 = str(tmp_path / "saved.ply")
    opt.save_ply(p1)
    back = convert_ply(p1)
    assert back.shape == (n, 84) and np.array_equal(bits(back[:, 0:3]), bits(host(opt.records)[:, 0:3]))      # the same order
    first_leg_bounds(back, host(opt.raw), "save_ply")
    assert np.allclose(back[:, FIELDS], host(opt.records)[:, FIELDS], rtol=3e-6, atol=1e-7)
    for _ in range(4):
        opt.step(*cam, target, LAMBDA)
    opt.stream.synchronize()
    opt.save_ply(p1)                                                   # after training: matched by position, which moved
    back, rec = convert_ply(p1), host(opt.records)
    where = {rec[g, 0:3].tobytes(): g for g in range(n)}
    assert len(where) == n
    order = np.array([where[back[k, 0:3].tobytes()] for k in range(n)])
    first_leg_bounds(back, host(opt.raw)[order], "save_ply after four steps")
    # densify
    rec0 = rec
    seen = host(opt.seen).view(np.uint32) > 0
    mean = host(opt.grad_accum)[seen] / host(opt.seen).view(np.uint32)[seen].astype(F32)
    split_scale = float(np.median(rec0[:, 4:7].max(1)))
    n_out, cloned, split, pruned = opt.densify(grad_threshold=float(np.median(mean)), split_scale=split_scale, seed=7)
    print(f"densify in raw space: {n} -> {n_out} (cloned {cloned}, split {split}, pruned {pruned})")
    assert split > 0 and cloned > 0 and n_out == n + cloned + split - pruned
    raw1, rec1 = host(opt.raw), host(opt.records)
    assert raw1.shape == rec1.shape == (n_out, 84) and opt.m.shape == (n_out, 84)
    fields_equal(rec1, act_ref(raw1, F32), "records == act(raw) after densify")
    # split children: two consecutive rows with equal scales, the parent's divided by 1.6; the parent is the row of rec0 whose
    # SH constant term they carry
    sh = {rec0[g, 12:15].tobytes(): g for g in range(n)}
    children = 0
    for k in range(n_out - 1):
        g = sh.get(rec1[k, 12:15].tobytes())
        if g is None or not np.array_equal(rec1[k, 12:15], rec1[k + 1, 12:15]) or np.array_equal(rec1[k, 0:3], rec1[k + 1, 0:3]):
            continue
        for c in (k, k + 1):
            want = np.log(rec0[g, 4:7].astype(np.float64) / 1.6)
            assert np.all(np.abs(raw1[c, 4:7] - want) <= 4 * np.spacing(np.abs(want).astype(F32))), (c, raw1[c, 4:7], want)
        children += 2
    assert children == 2 * split
    numbers = opt.step(*cam, target, LAMBDA)                            # a new scene of n_out splats
    opt.stream.synchronize()
    assert np.all(np.isfinite(host(numbers))) and r.sceneInfo().num_gaussians == n_out
    fields_equal(host(opt.records), act_ref(host(opt.raw), F32), "records == act(raw) after the step on the new cloud")
    # the reset
    max_opacity = F32(0.01)
    L = F32(np.log(float(max_opacity) / (1.0 - float(max_opacity))))   # the header's L, from the float the call receives
    cap = F32(1) / (F32(1) + oracle.exp(F32([-L]))[0])
    before = host(numbers)
    raw_b, rec_b = host(opt.raw).copy(), host(opt.records).copy()
    above = rec_b[:, 15] > max_opacity
    assert above.sum() > 10 and opt.m[:, 15].any() and opt.v[:, 15].any()
    opt.reset_opacity(0.01)
    opt.stream.synchronize()
    raw_r, rec_r = host(opt.raw), host(opt.records)
    assert rec_r[:, 15].max() <= cap and np.all(rec_r[above, 15] == cap)          # no record opacity exceeds sigmoid(L)
    assert np.all(raw_r[above, 15] == L)
    assert np.array_equal(bits(raw_r[~above]), bits(raw_b[~above])) and np.array_equal(bits(rec_r[~above]), bits(rec_b[~above]))
    others = [c for c in range(84) if c != 15]
    assert np.array_equal(bits(raw_r[:, others]), bits(raw_b[:, others])) and np.array_equal(bits(rec_r[:, others]), bits(rec_b[:, others]))
    assert not opt.m[:, 15].any() and not opt.v[:, 15].any()
    assert opt._full_upload                                             # the next step uploads every record
    numbers = opt.step(*cam, target, LAMBDA)
    opt.stream.synchronize()
    rec2 = host(opt.records)
    # the step after the reset moved the listed logits by at most the rate 0.05 from L
    assert np.all(host(opt.raw)[:, 15] <= L + F32(0.0500001)) and rec2[:, 15].max() <= 0.0106
    assert host(numbers)[0] > before[0] and host(numbers)[1] > 1.05 * before[1]      # a nearly transparent cloud: the frame changed
    r.setStream(None)
    r.cleanup()
