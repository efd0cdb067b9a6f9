"""SH colours in the multi-view batch: what can be checked without a device -- the new entry point is declared,
exported and listed, it keeps ABI 125, its host checks answer before anything touches the GPU, and the Python keyword is there."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gsr_sh_backward_views"


def _settings(V, degree=3, coeffs=16):
    from diff_gaussian_rasterization import _hip
    arr = (_hip.GsrSettings * V)()
    for v in range(V):
        arr[v].image_height, arr[v].image_width = 8, 8
        arr[v].sh_degree, arr[v].sh_coeffs = degree, coeffs
    return arr


def test_entry_point_is_declared_exported_and_listed():
    from diff_gaussian_rasterization import _hip
    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, hdr), "not declared in include/gsr.h"
    assert NAME in _hip.EXPORTS
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), NAME), "not exported by libgsr_hip.so"
    lib = _hip.load_library()
    assert lib.gsr_sh_backward_views.restype is ctypes.c_int and len(lib.gsr_sh_backward_views.argtypes) == 11
    # the header says what the call is for: it completes the batch backward, and it adds to dL_dmeans3D
    doc = hdr[hdr.index("SH colours in the multi-view call"):hdr.index("int " + NAME)]
    assert "gsr_backward_batch_ex" in doc and "dL_dcolors_views" in doc and "ACCUMULATED" in doc and "must be those of that forward" in doc
    assert "with SH use gsr_backward per view" not in hdr


def test_abi_version_is_still_125():
    from diff_gaussian_rasterization import _hip
    assert _hip.load_library().gsr_version() == 125


def test_host_checks_answer_minus_two_with_a_message():
    from diff_gaussian_rasterization import _hip
    lib = _hip.load_library()
    none8 = [None] * 8
    assert lib.gsr_sh_backward_views(2, None, 10, *none8) == -2                       # NULL settings
    assert NAME.encode() in lib.gsr_last_error() and b"settings" in lib.gsr_last_error()
    for V in (0, 17):
        assert lib.gsr_sh_backward_views(V, _settings(max(V, 1)), 10, *none8) == -2   # V outside 1..GSR_MAX_BATCH
        assert NAME.encode() in lib.gsr_last_error() and b"1..16" in lib.gsr_last_error()
    assert lib.gsr_sh_backward_views(2, _settings(2), 10, *none8) == -2               # NULL tables, P > 0
    assert NAME.encode() in lib.gsr_last_error() and b"NULL" in lib.gsr_last_error()
    assert lib.gsr_sh_backward_views(1, _settings(1, degree=3, coeffs=9), 10, *none8) == -2   # degree 3 needs 16 coefficients
    assert NAME.encode() in lib.gsr_last_error() and b"sh_degree" in lib.gsr_last_error()
    s = _settings(2)
    s[1].sh_degree = 2
    assert lib.gsr_sh_backward_views(2, s, 10, *none8) == -2                          # the views disagree
    assert NAME.encode() in lib.gsr_last_error() and b"view 1" in lib.gsr_last_error()


def test_no_gaussians_is_zero_without_a_launch():
    from diff_gaussian_rasterization import _hip
    lib = _hip.load_library()
    assert lib.gsr_sh_backward_views(3, _settings(3), 0, *([None] * 8)) == 0


def test_python_keyword_is_on_the_public_signature():
    from diff_gaussian_rasterization import rasterize_gaussians_views
    p = inspect.signature(rasterize_gaussians_views).parameters
    assert "batched_sh" in p and p["batched_sh"].default is False
    assert "batched_sh" in (rasterize_gaussians_views.__doc__ or "") and "camera_gradients=True" in rasterize_gaussians_views.__doc__
