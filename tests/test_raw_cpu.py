"""The raw parameter space of include/gsplat.h without a GPU: the NumPy restatements of act, of gs_adam_rows_raw_device and of
gs_raw_from_records_device that tests/test_raw_gpu.py compares the kernels with, pinned here against torch (exp, sigmoid,
normalize, SparseAdam) in float64; the defaults; the refusals that need no device; gs_write_ply against the loader; the writer
under the host sanitizers."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_adam_cpu import FIELDS, UNTOUCHED, adam_rows_ref, params_dict
from test_library import ROOT, _build_and_run

F32 = np.float32
FLT_MIN = F32(np.finfo(np.float32).tiny)
OPACITY_LO, OPACITY_HI = F32(2.0 ** -24), F32(1.0 - 2.0 ** -24)         # 0x1p-24f, 0x1.fffffep-1f


def E(x, dtype):
    """The header's E: the pinned exp in float32 (oracle.exp, gso_exp), the real one in float64."""
    return oracle.exp(x) if dtype is np.float32 else np.exp(x)


def act_ref(raw, dtype):
    """act of the header on every row of raw [k, 84], operation by operation, every operand of `dtype`: the record the raw
    row stands for.  The floats that are not fields are copied."""
    D = dtype
    r = np.array(raw, dtype=D, copy=True)
    out = r.copy()
    with np.errstate(all="ignore"):
        out[:, 4:7] = E(r[:, 4:7], D)
        out[:, 15] = D(1) / (D(1) + E(-r[:, 15], D))
        t = r[:, 8:12] * r[:, 8:12]
        inv = D(1) / np.sqrt((t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3]))
        out[:, 8:12] = r[:, 8:12] * inv[:, None]
    assert out.dtype == D
    return out


def raw_from_records_ref(records, dtype):
    """gs_raw_from_records_device restated; np.log stands for the device's logf, so float64 is the form to compare with."""
    D = dtype
    r = np.array(records, dtype=D, copy=True)
    out = r.copy()
    with np.errstate(all="ignore"):
        s = r[:, 4:7]
        out[:, 4:7] = np.log(np.where(s < D(FLT_MIN), D(FLT_MIN), s))
        o = r[:, 15]
        c = np.where(o < D(OPACITY_LO), D(OPACITY_LO), np.where(o > D(OPACITY_HI), D(OPACITY_HI), o))
        out[:, 15] = np.log(c / (D(1) - c))
    return out


def adam_rows_raw_ref(raw, records, m, v, ids, rows, count, max_rows, n, params, dtype):
    """gs_adam_rows_raw_device restated: the chain from dL/d(record) to dL/d(raw) with the record's current values, then
    adam_rows_ref on (raw, m, v), then records[listed, fields] = act(raw').  Returns the new (raw, records, m, v)."""
    D = dtype
    raw0, rec = np.array(raw, dtype=D, copy=True), np.array(records, dtype=D, copy=True)
    k = min(int(count), int(max_rows))
    listed = [i for i in range(k) if int(ids[i]) < n]
    if not listed:
        return raw0, rec, np.array(m, dtype=D, copy=True), np.array(v, dtype=D, copy=True)
    idx = np.asarray(ids, dtype=np.int64)[listed]
    g = np.array(np.asarray(rows, dtype=D)[listed], copy=True)
    R, W = rec[idx], raw0[idx]
    gt = g.copy()
    with np.errstate(all="ignore"):
        gt[:, 4:7] = g[:, 4:7] * R[:, 4:7]
        o = R[:, 15]
        gt[:, 15] = (g[:, 15] * o) * (D(1) - o)
        t = W[:, 8:12] * W[:, 8:12]
        inv = D(1) / np.sqrt((t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3]))            # of the OLD raw rotation
        q, gq = R[:, 8:12], g[:, 8:12]
        d = (gq[:, 0] * q[:, 0] + gq[:, 1] * q[:, 1]) + (gq[:, 2] * q[:, 2] + gq[:, 3] * q[:, 3])
        gt[:, 8:12] = (gq - q * d[:, None]) * inv[:, None]
    assert gt.dtype == D
    chained = np.zeros((k, 84), dtype=D)
    chained[listed] = gt
    raw1, m1, v1 = adam_rows_ref(raw0, m, v, ids, chained, count, max_rows, n, params, D)
    rec[np.ix_(idx, FIELDS)] = act_ref(raw1[idx], D)[:, FIELDS]
    return raw1, rec, m1, v1


def random_raw(rng, n, dtype=np.float32):
    """n raw rows of ordinary values: log-scales in [-9, 1], logits in [-8, 8], rotations of length 0.3 .. 3, SH in +-2,
    distinct positions; the floats that are not fields are zero."""
    raw = np.zeros((n, 84), dtype)
    raw[:, FIELDS] = rng.uniform(-2, 2, (n, 59))
    raw[:, 0:3] = rng.uniform(-5, 5, (n, 3))
    raw[:, 4:7] = rng.uniform(-9, 1, (n, 3))
    raw[:, 15] = rng.uniform(-8, 8, n)
    q = rng.standard_normal((n, 4))
    raw[:, 8:12] = q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.3, 3.0, (n, 1))
    return raw


def test_pinned_exp_serves_act():
    """What the header says of E on the ranges act uses it on: within 1e-6 relative of exp on [-20, 6], the sigmoid built
    from it within 1e-6 relative on [-20, 20]; the clamps at both ends, and a NaN sent to the lower clamp.  This checks the
    oracle's gso_exp, which act_ref and the header's text stand on, and calls nothing of the library: unlike the other tests of
    this file it passes without the raw-space calls."""
    x = np.linspace(-20, 6, 4001).astype(F32)
    assert np.max(np.abs(oracle.exp(x).astype(np.float64) / np.exp(x.astype(np.float64)) - 1)) < 1e-6
    z = np.linspace(-20, 20, 4001).astype(F32)
    sig = (F32(1) / (F32(1) + oracle.exp(-z))).astype(np.float64)
    assert np.max(np.abs(sig * (1 + np.exp(-z.astype(np.float64))) - 1)) < 1e-6
    assert list(oracle.exp(F32([-np.inf, np.inf, np.nan, -200, 100]))) == [F32(2.0 ** -126), F32(2.0 ** 126), F32(2.0 ** -126), F32(2.0 ** -126), F32(2.0 ** 126)]


@pytest.mark.parametrize("steps", [3])
def test_raw_restatement_in_float64_is_sparse_adam_through_torch_activations(steps):
    """A torch float64 leaf `raw`; records = exp of floats 4..6, sigmoid of float 15, normalize of floats 8..11, the rest
    identity; the loss (rows * records).sum() over the listed rows; one SparseAdam step on the sparse gradient of raw.
    Three steps over changing lists equal adam_rows_raw_ref(float64) within the 1e-12 * (|p| + lr) of
    test_restatement_in_float64_is_sparse_adam: the same count of double roundings, plus a handful for the chain."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(11)
    n = 40
    # the library's raw defaults (no clamp in any group: SparseAdam has none) with one rate; the float32 values they hold
    params = params_dict(gs.default_adam_params(space="raw", lr=[1e-2] * 6, eps=1e-9))
    assert all(x == -np.inf for x in params["lo"]) and all(x == np.inf for x in params["hi"])
    lr, eps = params["lr"][0], params["eps"]
    raw = random_raw(rng, n, np.float64)
    rec = act_ref(raw, np.float64)
    m, v = np.zeros((n, 84)), np.zeros((n, 84))
    p = torch.tensor(raw, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.SparseAdam([p], lr=lr, betas=(params["beta1"], params["beta2"]), eps=eps)
    for t in range(1, steps + 1):
        k = int(rng.integers(5, 25))
        ids = np.sort(rng.choice(n, k, replace=False)).astype(np.uint32)
        rows = np.zeros((k + 3, 84))
        rows[:k, FIELDS] = rng.standard_normal((k, 59)) * 10.0 ** rng.integers(-4, 3, (k, 59))
        rows[:k, FIELDS[::7]] = 0.0
        raw, rec, m, v = adam_rows_raw_ref(raw, rec, m, v, ids, rows, k, k + 3, n, dict(params, step=t), np.float64)
        records = torch.cat([p[:, 0:4], torch.exp(p[:, 4:7]), p[:, 7:8], torch.nn.functional.normalize(p[:, 8:12], dim=1, eps=0.0),
                             p[:, 12:15], torch.sigmoid(p[:, 15:16]), p[:, 16:]], dim=1)
        t_ids = torch.tensor(ids.astype(np.int64))
        loss = (torch.tensor(rows[:k]) * records[t_ids]).sum()
        (dense,) = torch.autograd.grad(loss, p)
        p.grad = torch.sparse_coo_tensor(t_ids[None], dense[t_ids], size=(n, 84))
        opt.step()
        got, want = raw[:, FIELDS], p.detach().numpy()[:, FIELDS]
        assert np.all(np.abs(got - want) <= 1e-12 * (np.abs(want) + lr)), (t, np.abs(got - want).max())
        # and the records the restatement keeps are act of its raw: the invariant the next step's chain stands on
        assert np.array_equal(rec, act_ref(raw, np.float64))
    assert np.array_equal(raw[:, UNTOUCHED], p.detach().numpy()[:, UNTOUCHED])


def test_restatements_skip_clamp_and_invert():
    """count / max_rows and an id >= n as in adam_rows_ref; lo / hi act on the raw value; raw_from_records_ref inverts
    act_ref up to rounding and lands on the documented clamps."""
    rng = np.random.default_rng(5)
    n = 6
    raw = random_raw(rng, n + 1)
    rec = act_ref(raw, F32)
    m, v = np.zeros_like(raw), np.zeros_like(raw)
    ids = np.array([1, 6, 3, 2], np.uint32)
    rows = np.ones((4, 84), F32)
    p = params_dict(gs.default_adam_params(space="raw", lr=[0.25] * 6, lo={gs.GS_ADAM_OPACITY: -1.0}, hi={gs.GS_ADAM_OPACITY: 1.0}))
    raw[1, 15], raw[3, 15] = 0.9, -0.9
    rec = act_ref(raw, F32)
    rows[2, 15] = -1.0                                                   # row 3's logit goes up, row 1's down
    r1, c1, m1, v1 = adam_rows_raw_ref(raw, rec, m, v, ids, rows, 3, 8, n, p, F32)
    assert r1.dtype == c1.dtype == F32
    assert np.array_equal(r1[[0, 2, 4, 5, 6]], raw[[0, 2, 4, 5, 6]]) and np.array_equal(c1[[0, 2, 4, 5, 6]], rec[[0, 2, 4, 5, 6]])
    assert np.allclose([r1[1, 15], r1[3, 15]], [0.65, -0.65], rtol=1e-5)    # step 1 moves by lr against the sign; inside [-1, 1]
    p2 = dict(p, lr=[5.0] * 6)
    r2, c2, _, _ = adam_rows_raw_ref(raw, rec, m, v, ids, rows, 3, 8, n, p2, F32)
    assert r2[1, 15] == -1.0 and r2[3, 15] == 1.0                         # the clamps hold the LOGIT
    assert c2[1, 15] == F32(1) / (F32(1) + oracle.exp(F32([1.0]))[0]) and np.array_equal(c2[[1, 3]][:, FIELDS], act_ref(r2[[1, 3]], F32)[:, FIELDS])
    back = raw_from_records_ref(rec, np.float64)
    assert np.allclose(back[:, 4:7], raw[:, 4:7], rtol=0, atol=1e-5) and np.allclose(back[:, 15], raw[:, 15], rtol=0, atol=2e-3)
    edge = rec.copy()
    edge[0, 15], edge[1, 15], edge[2, 4] = 0.0, 1.0, 0.0
    b = raw_from_records_ref(edge, np.float64)
    assert abs(b[0, 15] + 24 * np.log(2)) < 1e-6 and abs(b[1, 15] - 24 * np.log(2)) < 1e-6 and abs(b[2, 4] + 126 * np.log(2)) < 1e-9
    assert np.all(np.abs(b[:, 15]) <= 16.7)


def test_default_params_raw_and_struct_size():
    L = _lib.lib()
    p, q = _lib.GsAdamParams(), _lib.GsAdamParams()
    L.gs_default_adam_params(C.byref(p))
    L.gs_default_adam_params_raw(C.byref(q))
    inf = float("inf")
    assert q.struct_size == C.sizeof(_lib.GsAdamParams) == 92 and q.step == 1
    assert (q.beta1, q.beta2, q.eps, list(q.lr)) == (p.beta1, p.beta2, p.eps, list(p.lr))
    assert list(q.lo) == [-inf] * 6 and list(q.hi) == [inf] * 6
    L.gs_default_adam_params_raw(None)                                   # tolerated, like gs_default_adam_params(NULL)
    r = gs.default_adam_params(space="raw", step=4, lr={gs.GS_ADAM_SCALE: 0.5}, hi={gs.GS_ADAM_OPACITY: 3.0})
    assert (r.step, r.lr[1], r.lr[0], list(r.hi), list(r.lo)) == (4, 0.5, p.lr[0], [inf, inf, inf, inf, 3.0, inf], [-inf] * 6)
    assert list(gs.default_adam_params().lo) == list(p.lo) and list(gs.default_adam_params(space="records").hi) == list(p.hi)
    with pytest.raises(ValueError):
        gs.default_adam_params(space="logit")
    assert (_lib.GS_PLY_FROM_RECORDS, _lib.GS_PLY_FROM_RAW) == (0, 1)


def test_null_context_is_refused_by_every_device_call():
    """The code alone, as the existing entry points answer a NULL context; gs_write_ply has no context and refuses its
    arguments by themselves."""
    L = _lib.lib()
    p = gs.default_adam_params(space="raw")
    bad = _lib.GS_ERR_INVALID
    assert L.gs_adam_rows_raw_device(None, None, None, None, None, 4, None, None, None, 0, C.byref(p)) == bad
    assert L.gs_adam_rows_raw_device(None, None, None, None, None, 0, None, None, None, 7, None) == bad
    assert L.gs_records_from_raw_device(None, None, None, 4) == bad
    assert L.gs_raw_from_records_device(None, None, None, 4) == bad
    assert L.gs_reset_opacity_raw_device(None, None, None, None, None, 4, 0.01) == bad
    rows = np.zeros((1, 84), F32)
    assert L.gs_write_ply(None, rows.ctypes.data_as(C.c_void_p), 1, 0) == bad


# ---- gs_write_ply against the loader ------------------------------------------------------------------------------------------

INRIA_ORDER = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(45)]
               + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])


def convert_ply(path):
    L = _lib.lib()
    n = C.c_uint32(0)
    assert L.gs_convert_ply(os.fsencode(path), None, 0, C.byref(n)) == _lib.GS_OK
    out = np.zeros((n.value, 84), F32)
    assert L.gs_convert_ply(os.fsencode(path), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)) == _lib.GS_OK
    return out


def first_leg_bounds(got, raw, what):
    """Records that came through gs_write_ply(FROM_RAW) and the loader, against act of the raw rows they were written from:
    positions, SH and rotation bit-equal to act_ref(float32); scale within 1 ulp of the float64 exp (the host libm's
    documented bound); opacity within 2^-23 absolute of the float64 sigmoid."""
    a32, a64 = act_ref(raw, F32), act_ref(raw, np.float64)
    same = [c for c in FIELDS if not (4 <= c < 7 or c == 15)]
    assert np.array_equal(got[:, same].view(np.uint32), a32[:, same].view(np.uint32)), what
    ulp = np.spacing(np.abs(got[:, 4:7])).astype(np.float64)
    assert np.all(np.abs(got[:, 4:7].astype(np.float64) - a64[:, 4:7]) <= ulp), what
    assert np.all(np.abs(got[:, 15].astype(np.float64) - a64[:, 15]) <= 2.0 ** -23), what


def test_ply_round_trip(tmp_path):
    """1000 random raw rows: FROM_RAW then the loader gives act of them (A) under first_leg_bounds; A written FROM_RECORDS and
    loaded again (B) keeps the order, positions and SH bit for bit, and scale, opacity and rotation within one rounding of
    the log amplified by exp plus an ulp of each libm call.  The header lists the 62 INRIA properties and the file has the
    size that implies.  The error codes."""
    L = _lib.lib()
    rng = np.random.default_rng(77)
    n = 1000
    raw = random_raw(rng, n)
    assert len(np.unique(raw[:, 0:3].view(np.uint32), axis=0)) == n
    pa, pb = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    gs.write_ply(pa, raw, "raw")
    data = open(pa, "rb").read()
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode().split("\n")
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {n}"] and lines[-1] == ""
    assert lines[3:-1] == [f"property float {name}" for name in INRIA_ORDER] and len(INRIA_ORDER) == 62
    assert len(body) == n * 62 * 4
    vertex = np.frombuffer(body, "<f4").reshape(n, 62)
    assert not vertex[:, 3:6].any()                                                         # the normals
    assert np.array_equal(vertex[:, 54], raw[:, 15]) and np.array_equal(vertex[:, 55:58], raw[:, 4:7])   # the parameters exactly
    A = convert_ply(pa)
    assert A.shape == (n, 84)
    where = {raw[g, 0:3].tobytes(): g for g in range(n)}
    order = np.array([where[A[k, 0:3].tobytes()] for k in range(n)])
    assert sorted(order) == list(range(n))
    first_leg_bounds(A, raw[order], "first leg")
    assert not A[:, UNTOUCHED].any()
    gs.write_ply(pb, A, "records")
    B = convert_ply(pb)
    ident = [c for c in FIELDS if not (4 <= c < 12 or c == 15)]
    assert np.array_equal(B[:, ident].view(np.uint32), A[:, ident].view(np.uint32))         # same order, positions and SH bit for bit
    a_s = A[:, 4:7].astype(np.float64)
    assert np.all(np.abs(B[:, 4:7].astype(np.float64) - a_s) <= a_s * 2.0 ** -23 * (np.abs(np.log(a_s)) + 2))
    assert np.all(np.abs(B[:, 15].astype(np.float64) - A[:, 15]) <= 2.0 ** -22)
    assert np.all(np.abs(B[:, 8:12].astype(np.float64) - A[:, 8:12]) <= 2.0 ** -22)
    # errors
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.gs_write_ply(os.fsencode(str(tmp_path / "no_such_dir" / "a.ply")), ptr(raw), n, _lib.GS_PLY_FROM_RAW) == _lib.GS_ERR_IO
    assert b"no_such_dir" in L.gs_ply_last_error()
    with pytest.raises(gs.GsplatError) as ei:
        gs.write_ply(str(tmp_path / "no_such_dir" / "a.ply"), raw, "records")
    assert ei.value.code == _lib.GS_ERR_IO and "no_such_dir" in str(ei.value)
    assert L.gs_write_ply(None, ptr(raw), n, 0) == _lib.GS_ERR_INVALID
    assert L.gs_write_ply(os.fsencode(pa), None, n, 0) == _lib.GS_ERR_INVALID
    assert L.gs_write_ply(os.fsencode(pa), ptr(raw), 0, 0) == _lib.GS_ERR_INVALID
    assert L.gs_write_ply(os.fsencode(pa), ptr(raw), n, 2) == _lib.GS_ERR_INVALID
    assert open(pa, "rb").read() == data                                                   # a refused call does not touch the file
    with pytest.raises(ValueError):
        gs.write_ply(pa, raw, "logit")


def test_ply_writer_under_sanitizers(tmp_path):
    """tests/host/sanitize_ply_write.cpp + gs_ply.cpp with -fsanitize=address,undefined, as a program of its own: both
    spaces written and converted back at sizes around the writer's chunk, the clamps, the error paths."""
    csrc = os.path.join(ROOT, "vk3dgaussiansplatting_amd", "csrc")
    out = _build_and_run(tmp_path, "san_ply_write", "g++",
                         ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                         [os.path.join(ROOT, "tests", "host", "sanitize_ply_write.cpp"), os.path.join(csrc, "gs_ply.cpp")],
                         [str(tmp_path)])
    assert "sanitize_ply_write ok" in out
