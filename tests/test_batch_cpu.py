"""gs_rows_accumulate_device / gs_rows_collect_device (include/gsplat.h) without a GPU: the NumPy float32 restatements, written
from the header's text alone, that tests/test_batch_gpu.py compares the kernels with bit for bit, and the properties the header
derives from the arithmetic checked on the restatements themselves; the refusal that needs no device."""
import numpy as np
import pytest

from vk3dgaussiansplatting_amd import _lib
from test_adam_cpu import FIELDS, UNTOUCHED

SENTINEL = 0xFFC12345                      # a NaN with a payload, in the 25 floats no call may read or write
F = np.float32


@pytest.fixture(autouse=True)
def library_has_both_calls():
    """Every test of this file is about the two calls: without their symbols there is nothing to restate."""
    L = _lib.lib()
    assert hasattr(L, "gs_rows_accumulate_device") and hasattr(L, "gs_rows_collect_device")
    assert {"gs_rows_accumulate_device", "gs_rows_collect_device"} <= set(_lib.EXPORTS)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def rows_accumulate_ref(acc, mark, n, ids, rows, count, max_rows, weight):
    """gs_rows_accumulate_device restated: returns the new (acc, mark); the inputs stay.  acc: float32 [>= n, 84]; mark:
    uint32 [>= n]; ids, rows, count: a frame's list.  Float32, a multiply and then an add; a first touch stores."""
    acc, mark = np.array(acc, dtype=F, copy=True), np.array(mark, dtype=np.uint32, copy=True)
    rows = np.asarray(rows, dtype=F)
    w = F(weight)
    with np.errstate(all="ignore"):
        for i in range(min(int(count), int(max_rows))):
            g = int(ids[i])
            if g >= n:                                                  # compared, never dereferenced
                continue
            term = w * rows[i, FIELDS]
            assert term.dtype == F
            acc[g, FIELDS] = term if mark[g] == 0 else acc[g, FIELDS] + term
            mark[g] += 1
    return acc, mark


def rows_collect_ref(acc, mark, n, ids_out, rows_out, max_rows):
    """gs_rows_collect_device restated: returns the new (ids_out, rows_out, count, mark); the inputs stay.  ids_out, rows_out:
    what the buffers held before (None with max_rows == 0).  Rows move as bits."""
    mark = np.array(mark, dtype=np.uint32, copy=True)
    U = np.flatnonzero(mark[:n] != 0)
    k = min(len(U), int(max_rows))
    if max_rows:
        ids_out, rows_out = np.array(ids_out, dtype=np.uint32, copy=True), np.array(rows_out, dtype=F, copy=True)
        ids_out[:k] = U[:k]
        out = bits(rows_out)
        out[:k] = 0                                                     # +0.0f in the 25 other floats
        out[:k, FIELDS] = bits(np.asarray(acc, dtype=F))[U[:k]][:, FIELDS]
    mark[:n] = 0
    return ids_out, rows_out, len(U), mark


def frame(rng, n, k):
    """A list of k distinct ids below n (ascending, as the backward writes them) and its rows: six decades, exact zeros,
    -0.0f, the sentinel in the floats that are never read."""
    ids = np.sort(rng.choice(n, k, replace=False)).astype(np.uint32)
    rows = (rng.standard_normal((k, 84)) * 10.0 ** rng.integers(-3, 3, (k, 84))).astype(F)
    rows[rng.random((k, 84)) < 0.1] = 0.0
    rows[rng.random((k, 84)) < 0.05] = -0.0
    bits(rows)[:, UNTOUCHED] = SENTINEL
    return ids, rows


def blank(n):
    """An accumulator nobody initialised: NaN in the fields, the sentinel elsewhere; zero marks."""
    acc = np.full((n, 84), np.nan, F)
    bits(acc)[:, UNTOUCHED] = SENTINEL
    return acc, np.zeros(n, np.uint32)


def test_first_touch_is_a_store_and_the_other_floats_stay():
    rng = np.random.default_rng(1)
    n = 40
    acc0, mark0 = blank(n)
    ids, rows = frame(rng, n, 17)
    acc, mark = rows_accumulate_ref(acc0, mark0, n, ids, rows, 17, 17, 0.5)
    assert not np.isnan(acc[ids][:, FIELDS]).any()                      # the NaN underneath was never read
    rest = np.setdiff1d(np.arange(n), ids)
    assert np.array_equal(bits(acc[rest]), bits(acc0[rest]))            # unlisted rows: unchanged
    assert np.all(bits(acc)[:, UNTOUCHED] == SENTINEL)                  # the 25 non-fields: never written, never read
    assert np.array_equal(mark, np.isin(np.arange(n), ids).astype(np.uint32))
    assert np.array_equal(acc[ids][:, FIELDS], F(0.5) * rows[:, FIELDS])
    assert np.isnan(acc0[ids][:, FIELDS]).all() and not mark0.any()     # the inputs stay


def test_one_frame_at_weight_one_gives_the_rows_bits():
    rng = np.random.default_rng(2)
    n = 30
    ids, rows = frame(rng, n, 30)
    assert np.any(bits(rows[:, FIELDS]) == 0x80000000)                  # -0.0f is among the values
    acc, mark = rows_accumulate_ref(*blank(n), n, ids, rows, 30, 30, 1.0)
    assert np.array_equal(bits(acc[ids][:, FIELDS]), bits(rows[:, FIELDS]))
    out_ids, out_rows, count, mark1 = rows_collect_ref(acc, mark, n, np.zeros(30, np.uint32), np.full((30, 84), 7.0, F), 30)
    assert count == 30 and np.array_equal(out_ids, ids) and not mark1.any()
    assert np.array_equal(bits(out_rows)[:, FIELDS], bits(rows)[:, FIELDS]) and not bits(out_rows)[:, UNTOUCHED].any()


def test_count_max_rows_and_ids_beyond_n():
    rng = np.random.default_rng(3)
    n = 20
    ids, rows = frame(rng, n + 1, n + 1)                                # every id 0..n: the last one is == n
    assert ids[-1] == n
    acc0, mark0 = blank(n + 1)
    acc, mark = rows_accumulate_ref(acc0, mark0, n, ids, rows, n + 1, n + 1, 1.0)
    assert mark[n] == 0 and np.array_equal(bits(acc[n]), bits(acc0[n])) and np.all(mark[:n] == 1)
    acc, mark = rows_accumulate_ref(acc0, mark0, n, ids, rows, 9, 5, 1.0)      # max_rows cuts the list, then the count
    assert mark.sum() == 5
    acc, mark = rows_accumulate_ref(acc0, mark0, n, ids, rows, 3, 5, 1.0)
    assert mark.sum() == 3
    acc, mark = rows_accumulate_ref(acc0, mark0, n, ids, rows, 3, 0, 1.0)
    assert mark.sum() == 0 and np.array_equal(bits(acc), bits(acc0))


def test_order_of_the_frames_changes_the_association_only():
    """Two frames: a + b is b + a in IEEE arithmetic, so both orders give the same bits.  Three frames: each order is its own
    association, (w0 r0 + w1 r1) + w2 r2 against (w2 r2 + w1 r1) + w0 r0, and the two differ in some last bits."""
    rng = np.random.default_rng(4)
    n = 50
    ids = np.arange(n, dtype=np.uint32)
    frames = [(ids, frame(rng, n, n)[1], w) for w in (1.0, 0.5, 1.0 / 3.0)]

    def run(order):
        acc, mark = blank(n)
        for k in order:
            acc, mark = rows_accumulate_ref(acc, mark, n, frames[k][0], frames[k][1], n, n, frames[k][2])
        return acc, mark

    (a01, m01), (a10, m10) = run((0, 1)), run((1, 0))
    assert np.array_equal(bits(a01), bits(a10)) and np.all(m01 == 2) and np.array_equal(m01, m10)
    t = [F(w) * r[:, FIELDS] for _, r, w in frames]
    assert np.array_equal(bits(a01[:, FIELDS]), bits(t[0] + t[1]))
    (a012, m012), (a210, _) = run((0, 1, 2)), run((2, 1, 0))
    assert np.all(m012 == 3)
    assert np.array_equal(bits(a012[:, FIELDS]), bits((t[0] + t[1]) + t[2]))
    assert np.array_equal(bits(a210[:, FIELDS]), bits((t[2] + t[1]) + t[0]))
    assert np.any(bits(a012[:, FIELDS]) != bits(a210[:, FIELDS]))


def test_collect_truncates_counts_and_clears():
    rng = np.random.default_rng(5)
    n = 64
    acc = rng.standard_normal((n + 1, 84)).astype(F)
    bits(acc)[:, UNTOUCHED] = SENTINEL
    mark = np.zeros(n + 1, np.uint32)
    U = np.array([0, 3, 4, 31, 32, 63])
    mark[U] = [1, 2, 1, 7, 1, 1]
    mark[n] = 9                                                         # beyond n: not a member, not cleared
    ids0, rows0 = np.full(10, 0xDEADBEEF, np.uint32), np.full((10, 84), -12345.5, F)
    for max_rows in (0, 5, 6, 10):
        none = max_rows == 0
        ids, rows, count, mark1 = rows_collect_ref(acc, mark, n, None if none else ids0[:max_rows], None if none else rows0[:max_rows], max_rows)
        assert count == 6 and not mark1[:n].any() and mark1[n] == 9      # not clamped; members beyond max_rows are cleared too
        if none:
            assert ids is None and rows is None
            continue
        k = min(6, max_rows)
        assert np.array_equal(ids[:k], U[:k]) and np.all(ids[k:] == 0xDEADBEEF) and np.all(rows[k:] == F(-12345.5))
        assert np.array_equal(bits(rows[:k])[:, FIELDS], bits(acc[U[:k]])[:, FIELDS]) and not bits(rows[:k])[:, UNTOUCHED].any()
    ids, rows, count, mark1 = rows_collect_ref(acc, np.zeros(n, np.uint32), n, ids0, rows0, 10)
    assert count == 0 and np.array_equal(ids, ids0) and np.array_equal(rows, rows0)
    assert mark[U[0]] == 1                                              # the inputs stay


def test_null_context_is_refused_by_both_entry_points():
    L = _lib.lib()
    assert L.gs_rows_accumulate_device(None, None, None, 4, None, None, None, 0, 1.0) == _lib.GS_ERR_INVALID
    assert L.gs_rows_collect_device(None, None, None, 4, None, None, 0, None) == _lib.GS_ERR_INVALID
