"""Device ray queries (vmx_query / vmx_query_device) without a GPU: the symbols, the constants, the argument
checks that come before any device work, and the float form of RayCastCollision's `ii.t > 1e-3`."""
import ctypes as C
import os
import re

import numpy as np

from vermilion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vermilion_hip.h")


def test_query_symbols_and_constants(hip_lib):
    for name in ("vmx_query", "vmx_query_device"):
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
    src = open(HEADER).read()
    consts = {k: int(v, 0) for k, v in re.findall(r"#define (VMX_QUERY_[A-Z_]+)\s+(0x[0-9a-fA-F]+|\d+)u", src)}
    assert consts == {"VMX_QUERY_NEAREST": 0, "VMX_QUERY_ANY": 1, "VMX_QUERY_COLLISION": 2,
                      "VMX_QUERY_FETCH_PER_LANE": 0x100}
    for k, v in consts.items():
        assert getattr(L, k) == v, k
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src)


def _err(lib):
    return lib.vmx_last_error().decode()


def test_query_argument_errors_do_not_need_a_gpu(hip_lib):
    """Every check below fires before the scene is looked at (a NULL scene is the last check), so each is seen
    on its own, on a box without a device."""
    o = np.zeros((4, 3), np.float32)
    tri = np.zeros(4, np.int32)
    t = np.zeros(4, np.float32)
    hit = np.zeros(4, np.uint8)
    O, T, I, H = o.ctypes.data, t.ctypes.data, tri.ctypes.data, hit.ctypes.data
    for fn in (hip_lib.vmx_query, hip_lib.vmx_query_device):
        extra = () if fn is hip_lib.vmx_query else (None,)
        cases = [
            ((None, 0, O, O, None, 4, I, T, H), "NULL scene"),
            ((None, 3, O, O, None, 4, I, T, H), "unknown query mode"),
            ((None, 0x200, O, O, None, 4, I, T, H), "unknown query mode"),
            ((None, 0, None, O, None, 4, I, T, H), "NULL rays"),
            ((None, 2, O, None, None, 4, I, T, H), "NULL rays"),
            ((None, 0, O, O, None, 4, None, None, None), "no output"),
            ((None, 1, O, O, None, 4, I, None, H), "VMX_QUERY_ANY returns hit only"),
            ((None, 1, O, O, None, 4, None, T, H), "VMX_QUERY_ANY returns hit only"),
            ((None, 1 | 0x100, O, O, None, 4, None, T, None), "VMX_QUERY_ANY returns hit only"),
        ]
        for args, msg in cases:
            assert fn(*(args + extra)) == L.VMX_ERR_INVALID, (fn, args)
            assert msg in _err(hip_lib), (args, _err(hip_lib))
        # n == 0 needs no rays and no outputs, but still a scene
        assert fn(*((None, 0, None, None, None, 0, None, None, None) + extra)) == L.VMX_ERR_INVALID
        assert "NULL scene" in _err(hip_lib)


def test_python_layer_rejects_bad_modes_before_the_library():
    import vermilion_amd as va
    sc = va.Scene.__new__(va.Scene)  # no device needed: the mode is checked first
    try:
        sc.query(np.zeros((1, 3)), np.ones((1, 3)), mode="occlusion")
    except ValueError as e:
        assert "mode" in str(e)
    else:
        raise AssertionError("unknown mode accepted")


def test_collision_threshold_float_form_is_exact():
    """RayCastCollision tests `ii.t > 1e-3` with a float t and the double literal 1e-3 (meshEngine.cpp:202).  The
    kernel's float test is t >= 1e-3f: exhaustively over every float from 2^-11 to 2^-9 (the binades around 1e-3,
    4.2 M values), plus zero, subnormals, negatives, the extremes, inf and NaN."""
    lo = np.float32(2.0 ** -11).view(np.uint32)
    hi = np.float32(2.0 ** -9).view(np.uint32)
    bits = np.arange(lo, hi + 1, dtype=np.uint32)
    special = np.array([0.0, -0.0, 1e-45, 1e-38, -1e-3, 1e-3, 1.0, 3.4e38, np.inf, -np.inf, np.nan], np.float32).view(np.uint32)
    t = np.concatenate([bits, special]).view(np.float32)
    with np.errstate(invalid="ignore"):
        ref = t.astype(np.float64) > 1e-3
        kernel = t >= np.float32(1e-3)
    assert np.array_equal(ref, kernel)
    # and why not `>`: 1e-3f itself lies above the double 1e-3, the float below it does not
    f = np.float32(1e-3)
    assert float(f) > 1e-3 and float(np.nextafter(f, np.float32(0))) < 1e-3
    assert not (f > np.float32(1e-3)) and float(f) > 1e-3
