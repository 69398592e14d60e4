"""What tests/test_band_backward_gpu.py (gradients of a tile-row band, include/gsplat.h gs_set_band_gradients) rests on,
checked without a GPU: the entry point and its bindings, the dealings of the band tests, and -- on the oracle alone -- the
precondition of the stale-scratch test and the identity that the V_band of a dealing's bands unite to V of the frame."""
import os
import subprocess

import numpy as np

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from conftest import ROOT
from test_outputs_cpu import SCENES, oracle_params
from test_band_cull_cpu import C_BAND, H, W, cameras, cloud_c, emits_into, oracle_run

# The dealings of `ragged`'s 12 tile rows (333 x 190: 21 x 12 tiles, the last row partial).  ("rows", begin, end) is
# gs_set_tile_rows, ("il", phase, stride, compact_output) gs_set_tile_rows_interleaved.
DEALINGS = {
    "thirds": [("rows", 0, 4), ("rows", 4, 8), ("rows", 8, 12)],
    "edges": [("rows", 0, 1), ("rows", 1, 11), ("rows", 11, 12)],       # a single top row, the ragged last row alone
    "empty": [("rows", 5, 5)],
    "stride2": [("il", 0, 2, 0), ("il", 1, 2, 0)],
    "stride5": [("il", k, 5, 0) for k in range(5)],
    "stride2_compact": [("il", 0, 2, 1), ("il", 1, 2, 1)],
}


def rows_of(spec, gh):
    """The tile rows a context with the rows `spec` owns in a grid of gh rows."""
    return list(range(spec[1], spec[2])) if spec[0] == "rows" else list(range(spec[1], gh, spec[2]))


def v_band(s, rows):
    """Per splat of the oracle's whole-frame records: at least one tile of its box lies in the tile rows `rows`."""
    box = (s["visible"] == 1) & (s["min_x"] < s["max_x"])
    lo, hi = s["min_y"].astype(np.int64), s["max_y"].astype(np.int64)
    hit = np.zeros(box.shape, bool)
    for row in rows:
        hit |= (lo <= row) & (row < hi)
    return box & hit


def test_dealings_cover_every_row_once():
    for name, dealing in DEALINGS.items():
        owned = sorted(row for spec in dealing for row in rows_of(spec, 12))
        assert owned == ([] if name == "empty" else list(range(12))), name
    assert [len(rows_of(spec, 12)) for spec in DEALINGS["stride5"]] == [3, 3, 2, 2, 2]


def test_entry_point_and_bindings():
    """gs_set_band_gradients refuses a NULL context with the code alone; the symbol is exported and declared (the export
    test of test_library.py then holds the header to it); the Python wrapper has the method."""
    L = _lib.lib()
    assert L.gs_set_band_gradients(None, 1) == _lib.GS_ERR_INVALID
    assert L.gs_set_band_gradients(None, 0) == _lib.GS_ERR_INVALID
    assert "gs_set_band_gradients" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    assert "int gs_set_band_gradients(gs_ctx* ctx, uint32_t enable);" in hdr
    assert hasattr(gs.Renderer, "setBandGradients")
    assert _lib.API_VERSION == 7


def test_cpp_wrapper_has_the_method(tmp_path):
    """include/gsplat.hpp compiles as plain C++17 with a call of setBandGradients and links with the library."""
    src = tmp_path / "t.cpp"
    src.write_text('#include "gsplat.hpp"\nint main() { gsplat::Renderer r(64, 64); int rc = r.init();\n'
                   '  if (rc != GS_OK) return rc == GS_ERR_NO_DEVICE ? 0 : 1;\n'
                   '  return r.setBandGradients(true) == GS_OK && r.setBandGradients(false) == GS_OK ? 0 : 2; }\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lgsplat_hip", f"-Wl,-rpath,{libdir}"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_stale_counts_would_be_nonzero(oracle_mod):
    """The precondition of the stale-scratch test: under `rigid`, every splat of block 0 of cloud_c(63) emits nothing into
    C_BAND (k_band_cull rejects the block: its four waves are out waves), and at least one of them emits into the whole
    frame -- so the count a whole-grid frame left for it is not zero."""
    aos, in_mask = cloud_c(63)
    s = oracle_run(("C", 63, False), aos, cameras()["rigid"], W, H)["splats"]
    block0 = slice(0, 256)
    assert not in_mask[block0].any()
    assert not emits_into(s, *C_BAND)[block0].any()
    assert emits_into(s, 0, (H + 15) // 16)[block0].any()
    # some other block is kept, so the band's list is not empty and slots follow the rejected block
    assert emits_into(s, *C_BAND)[256:].any()


def test_union_of_v_band_is_v(oracle_mod):
    """On the oracle: over every dealing of `ragged`, the union of V_band is V of the whole frame, and a band's V_band is a
    proper subset."""
    import oracle
    aos, w, h = SCENES["ragged"]()
    s = oracle.full_pipeline(oracle_params(oracle_mod, w, h), aos)["stage1"]["splats"]
    gh = (h + 15) // 16
    v = v_band(s, range(gh))
    assert np.array_equal(v, emits_into(s, 0, gh)) and 0 < v.sum() < len(aos)
    for name, dealing in DEALINGS.items():
        if name == "empty":
            assert not v_band(s, rows_of(dealing[0], gh)).any()
            continue
        union = np.zeros_like(v)
        for spec in dealing:
            mine = v_band(s, rows_of(spec, gh))
            assert 0 < mine.sum() < v.sum(), (name, spec)
            assert not (mine & ~v).any()
            union |= mine
        assert np.array_equal(union, v), name
