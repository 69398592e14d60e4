"""The active SH degree as host arithmetic: gs_sh_mode_of_degree through the library (which loads without a GPU), the Python
helper over it, and VisibleAdam's degree schedule -- none of it needs a context."""
import ctypes as C

import pytest

from vk3dgaussiansplatting_amd import _lib

MODE_OF_DEGREE = {0: 2, 1: 5, 2: 4, 3: 0}
MODES = (0, 1, 2, 4, 5)          # 3 names no mode: refused before the degrees existed, and still


def test_the_five_modes_are_named():
    assert (_lib.GS_SH_ALL_BANDS, _lib.GS_SH_SKIP_FIRST_BAND, _lib.GS_SH_ONLY_FIRST_BAND, _lib.GS_SH_DEGREE_1,
            _lib.GS_SH_DEGREE_2) == (0, 1, 2, 5, 4)
    import vk3dgaussiansplatting_amd as gs
    cam = gs.Camera(1.5)
    for mode in MODES:
        cam.setShMode(mode)
        assert int(cam.getShMode()) == mode
    assert [int(m) for m in list(gs.SphericalHarmonicsMode)[:3]] == [0, 1, 2]
    for bad in (3, 6):
        with pytest.raises(ValueError):
            cam.setShMode(bad)


def test_mode_of_degree_through_the_library():
    L = _lib.lib()
    for degree, want in MODE_OF_DEGREE.items():
        mode = C.c_uint32(77)
        assert L.gs_sh_mode_of_degree(degree, C.byref(mode)) == _lib.GS_OK and mode.value == want
    for bad in (4, 5, 0xFFFFFFFF):
        mode = C.c_uint32(77)
        assert L.gs_sh_mode_of_degree(bad, C.byref(mode)) == _lib.GS_ERR_INVALID and mode.value == 77
    for degree in (0, 3, 4):
        assert L.gs_sh_mode_of_degree(degree, None) == _lib.GS_ERR_INVALID


def test_python_helper_agrees():
    for degree, want in MODE_OF_DEGREE.items():
        assert _lib.sh_mode_of_degree(degree) == want
    for bad in (4, -1, 1 << 32):
        with pytest.raises(ValueError):
            _lib.sh_mode_of_degree(bad)


def test_visible_adam_schedule_without_a_device():
    """sh_degree, oneup_sh_degree() and frame_sh_mode() are host state: checked on an object that never saw a context."""
    pytest.importorskip("torch")
    from vk3dgaussiansplatting_amd.autograd import VisibleAdam
    opt = VisibleAdam.__new__(VisibleAdam)
    assert opt.sh_degree == 3 and opt.frame_sh_mode(None) == 0           # the default: what a step drew before the degree existed
    opt.sh_degree = 0
    seen = []
    for _ in range(5):
        seen.append((opt.sh_degree, opt.frame_sh_mode(None), opt.frame_sh_mode()))
        opt.oneup_sh_degree()
    assert seen == [(0, 2, 2), (1, 5, 5), (2, 4, 4), (3, 0, 0), (3, 0, 0)]
    assert opt.oneup_sh_degree() == 3
    for explicit in MODES:                                            # an explicit integer is taken as it is
        assert opt.frame_sh_mode(explicit) == explicit
    opt.sh_degree = 4
    with pytest.raises(ValueError):
        opt.frame_sh_mode(None)
