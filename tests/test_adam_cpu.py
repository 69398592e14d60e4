"""gs_adam_rows_device / gs_upload_rows_device (include/gsplat.h) without a GPU: the restatement of the Adam step in NumPy
that tests/test_adam_gpu.py compares the kernel with bit for bit, pinned here against torch.optim.SparseAdam in float64; the
table of field groups; the defaults; the refusals that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib

GROUP = np.array(gs.ADAM_GROUP_OF_FLOAT)
FIELDS = np.flatnonzero(GROUP >= 0)               # the 59 floats of a record the optimiser moves
UNTOUCHED = np.flatnonzero(GROUP < 0)             # the other 25


def params_dict(p):
    """A GsAdamParams as the plain values adam_rows_ref takes."""
    return dict(step=int(p.step), beta1=float(p.beta1), beta2=float(p.beta2), eps=float(p.eps), lr=[float(x) for x in p.lr],
                lo=[float(x) for x in p.lo], hi=[float(x) for x in p.hi])


def adam_rows_ref(records, m, v, ids, rows, count, max_rows, n, params, dtype):
    """gs_adam_rows_device restated (the header's arithmetic, operation by operation, every operand of `dtype`): returns the
    new (records, m, v); the inputs stay.  records / m / v: [>= n, 84]; ids: the listed splats; rows: [>= min(count,
    max_rows), 84] gradient rows; params: step, beta1, beta2, eps and lr / lo / hi per group.  With dtype = np.float32 this
    is the kernel's answer bit for bit (IEEE + - * / sqrt, nothing contracted); with np.float64 it is SparseAdam's rule."""
    D = dtype
    rec, mm, vv = (np.array(a, dtype=D, copy=True) for a in (records, m, v))
    b1, b2, eps = D(params["beta1"]), D(params["beta2"]), D(params["eps"])
    c1, c2 = D(1) - b1, D(1) - b2
    t = float(params["step"])
    root2, bias1 = math.sqrt(1.0 - math.pow(float(b2), t)), 1.0 - math.pow(float(b1), t)        # in double, like the host code
    grp = GROUP[FIELDS]
    step = np.array([D(float(D(lr)) * root2 / bias1) for lr in params["lr"]], dtype=D)[grp]
    lo = np.array(params["lo"], dtype=D)[grp]
    hi = np.array(params["hi"], dtype=D)[grp]
    k = min(int(count), int(max_rows))
    listed = [i for i in range(k) if int(ids[i]) < n]                  # an id >= n is skipped
    if not listed:
        return rec, mm, vv
    idx = np.asarray(ids, dtype=np.int64)[listed]
    at = np.ix_(idx, FIELDS)
    g = np.asarray(rows, dtype=D)[np.ix_(listed, FIELDS)]
    with np.errstate(all="ignore"):
        m1 = b1 * mm[at] + c1 * g
        v1 = b2 * vv[at] + (c2 * g) * g
        p1 = rec[at] - step * (m1 / (np.sqrt(v1) + eps))
        p1 = np.where(p1 < lo, lo, np.where(p1 > hi, hi, p1))         # a NaN stays a NaN
    assert m1.dtype == v1.dtype == p1.dtype == D
    rec[at], mm[at], vv[at] = p1, m1, v1
    return rec, mm, vv


def test_group_table_marks_the_59_fields():
    assert len(gs.ADAM_GROUP_OF_FLOAT) == 84 and len(FIELDS) == 59 and len(UNTOUCHED) == 25
    sizes = [int(np.sum(GROUP == g)) for g in range(6)]
    assert sizes == [3, 3, 4, 3, 1, 45]
    assert (gs.GS_ADAM_POSITION, gs.GS_ADAM_SCALE, gs.GS_ADAM_ROTATION, gs.GS_ADAM_SH_DC, gs.GS_ADAM_OPACITY, gs.GS_ADAM_SH_REST) == tuple(range(6))
    assert list(np.flatnonzero(GROUP == gs.GS_ADAM_POSITION)) == [0, 1, 2] and list(np.flatnonzero(GROUP == gs.GS_ADAM_SCALE)) == [4, 5, 6]
    assert list(np.flatnonzero(GROUP == gs.GS_ADAM_ROTATION)) == [8, 9, 10, 11] and list(np.flatnonzero(GROUP == gs.GS_ADAM_SH_DC)) == [12, 13, 14]
    assert list(np.flatnonzero(GROUP == gs.GS_ADAM_OPACITY)) == [15]
    assert list(np.flatnonzero(GROUP == gs.GS_ADAM_SH_REST)) == [16 + 4 * k + c for k in range(15) for c in range(3)]
    assert list(UNTOUCHED) == sorted([3, 7] + [19 + 4 * k for k in range(15)] + list(range(76, 84)))


def test_default_params_and_struct_size():
    L = _lib.lib()
    p = _lib.GsAdamParams()
    L.gs_default_adam_params(C.byref(p))
    f = np.float32
    assert p.struct_size == C.sizeof(_lib.GsAdamParams) == 92 and p.step == 1
    assert (f(p.beta1), f(p.beta2), f(p.eps)) == (f(0.9), f(0.999), f(1e-15))
    assert [f(x) for x in p.lr] == [f(1.6e-4), f(5e-3), f(1e-3), f(2.5e-3), f(5e-2), f(1.25e-4)]
    inf = float("inf")
    assert list(p.lo) == [-inf, float(f(1e-7)), -inf, -inf, 0.0, -inf] and list(p.hi) == [inf, inf, inf, inf, 1.0, inf]
    L.gs_default_adam_params(None)                                     # tolerated, like gs_default_config(NULL)
    q = gs.default_adam_params(step=3, beta1=0.5, lr={gs.GS_ADAM_OPACITY: 0.25}, hi=[1, 2, 3, 4, 5, 6])
    assert (q.step, q.beta1, q.lr[4], q.lr[0], list(q.hi)) == (3, 0.5, 0.25, p.lr[0], [1, 2, 3, 4, 5, 6])
    with pytest.raises(TypeError):
        gs.default_adam_params(learning_rate=1.0)
    with pytest.raises(ValueError):
        gs.default_adam_params(lr=[1.0, 2.0])


def test_null_context_is_refused_by_both_entry_points():
    L = _lib.lib()
    p = gs.default_adam_params()
    assert L.gs_adam_rows_device(None, None, None, None, 4, None, None, None, 0, C.byref(p)) == _lib.GS_ERR_INVALID
    assert L.gs_adam_rows_device(None, None, None, None, 0, None, None, None, 7, None) == _lib.GS_ERR_INVALID
    assert L.gs_upload_rows_device(None, None, 4, None, None, 0) == _lib.GS_ERR_INVALID
    assert L.gs_upload_rows_device(None, None, 0, None, None, 7) == _lib.GS_ERR_INVALID


@pytest.mark.parametrize("steps", [1, 2, 3])
def test_restatement_in_float64_is_sparse_adam(steps):
    """One rate for all groups, no clamps: `steps` steps of adam_rows_ref(float64) over changing lists of rows against
    torch.optim.SparseAdam in float64 on the CPU, within 1e-12 * (|p| + lr): about ten double roundings of 1.1e-16 on
    either side leave four orders of slack.  Rows keep their moments while they are not listed, fields with a zero gradient
    move, and the bias correction counts the optimiser's steps, not a row's."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(steps)
    n, lr, eps = 40, 1e-2, 1e-9
    inf = float("inf")
    params = dict(beta1=0.9, beta2=0.999, eps=eps, lr=[lr] * 6, lo=[-inf] * 6, hi=[inf] * 6)
    rec = rng.standard_normal((n, 84))
    m, v = np.zeros((n, 84)), np.zeros((n, 84))
    p = torch.tensor(rec, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.SparseAdam([p], lr=lr, betas=(0.9, 0.999), eps=eps)
    for t in range(1, steps + 1):
        k = int(rng.integers(5, 25))
        ids = np.sort(rng.choice(n, k, replace=False)).astype(np.uint32)
        rows = np.zeros((k + 3, 84))
        rows[:k, FIELDS] = rng.standard_normal((k, 59)) * 10.0 ** rng.integers(-4, 3, (k, 59))
        rows[:k, FIELDS[::7]] = 0.0                                   # zero gradients inside listed rows
        rec, m, v = adam_rows_ref(rec, m, v, ids, rows, k, k + 3, n, dict(params, step=t), np.float64)
        p.grad = torch.sparse_coo_tensor(torch.tensor(ids.astype(np.int64))[None], torch.tensor(rows[:k]), size=(n, 84))
        opt.step()
        got, want = rec[:, FIELDS], p.detach().numpy()[:, FIELDS]
        assert np.all(np.abs(got - want) <= 1e-12 * (np.abs(want) + lr)), (t, np.abs(got - want).max())
    assert np.array_equal(rec[:, UNTOUCHED], p.detach().numpy()[:, UNTOUCHED])           # zero gradient and zero moments: SparseAdam keeps them too


def test_restatement_skips_and_clamps():
    """The parts SparseAdam has no counterpart for: count / max_rows, an id >= n, the clamps, NaN."""
    f = np.float32
    n = 5
    rec = np.full((n + 1, 84), 0.5, f)
    m, v = np.zeros_like(rec), np.zeros_like(rec)
    ids = np.array([1, 5, 3, 2], np.uint32)
    rows = np.ones((4, 84), f)
    rows[2, 15] = np.nan
    params = params_dict(gs.default_adam_params(lr=[0.25, 1.0, 0.25, 0.25, 1.0, 0.25]))
    r1, m1, v1 = adam_rows_ref(rec, m, v, ids, rows, 3, 8, n, params, f)
    assert r1.dtype == f and np.array_equal(rec, np.full((n + 1, 84), 0.5, f))           # the inputs stay
    assert np.array_equal(r1[[0, 2, 4, 5]], rec[[0, 2, 4, 5]])                          # unlisted, past count, id >= n
    assert np.array_equal(r1[1][UNTOUCHED], rec[1][UNTOUCHED]) and np.all(m1[:, UNTOUCHED] == 0)
    assert np.all(r1[1, 4:7] == f(1e-7)) and r1[1, 15] == 0.0 and np.isnan(r1[3, 15]) and np.isnan(m1[3, 15])
    assert np.allclose(r1[1, 0:3], 0.25, rtol=1e-5)                                      # step 1: p - lr * g / |g|
    r2, _, _ = adam_rows_ref(rec, m, v, ids, rows, 4, 2, n, params, f)                  # max_rows cuts the list
    assert np.array_equal(r2[[0, 2, 3, 4, 5]], rec[[0, 2, 3, 4, 5]]) and not np.array_equal(r2[1], rec[1])
