"""MeshEngine::RayCast of device batches (vmx_raycast_device / vmx_raycast_camera_device) without a GPU: the symbols,
the header, the argument checks that come before any device work, and the Python layer's input checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import vermilion_amd as va
from vermilion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vermilion_hip.h")
ENTRIES = ("vmx_raycast_device", "vmx_raycast_camera_device")


def _err(lib):
    return lib.vmx_last_error().decode()


def test_raycast_symbols_are_declared_and_bound(hip_lib):
    src = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, src), name
    # additive: no new ABI version, no new query constant
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src)
    assert set(re.findall(r"#define (VMX_QUERY_[A-Z_]+)", src)) == {
        "VMX_QUERY_NEAREST", "VMX_QUERY_ANY", "VMX_QUERY_COLLISION", "VMX_QUERY_FETCH_PER_LANE"}
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER], check=True)


def test_raycast_argument_errors_do_not_need_a_gpu(hip_lib):
    """Each check fires before the scene is looked at (a NULL scene is the last check), so each is seen alone."""
    rays = np.zeros((8, 3), np.float32)
    out = np.zeros(8 * 16 + 4, np.float32)
    base = out.ctypes.data
    aligned = base + (-base) % 16
    R = rays.ctypes.data
    fn = hip_lib.vmx_raycast_device
    cases = [
        ((None, R, R, 4, aligned, 0, None), "NULL scene"),
        ((None, R, R, 4, aligned, 0x100, None), "NULL scene"),  # VMX_QUERY_FETCH_PER_LANE is a valid flag
        ((None, R, R, 4, aligned, 1, None), "unknown raycast flags"),
        ((None, R, R, 4, aligned, 0x200, None), "unknown raycast flags"),
        ((None, None, R, 4, aligned, 0, None), "NULL rays"),
        ((None, R, None, 4, aligned, 0, None), "NULL rays"),
        ((None, R, R, 4, None, 0, None), "NULL d_out"),
        ((None, R, R, 4, aligned + 4, 0, None), "16-byte aligned"),
        ((None, R, R, 0x80000000, aligned, 0, None), "more than 2^31 - 1 rays"),
        ((None, R, R, 0xFFFFFFFF, aligned, 0, None), "more than 2^31 - 1 rays"),
        ((None, R, R, 4, R - (R % 16), 0, None), "overlaps the rays"),
        ((None, aligned + 64, R, 4, aligned, 0, None), "overlaps the rays"),
        ((None, R, aligned + 200, 4, aligned, 0, None), "overlaps the rays"),
    ]
    for args, msg in cases:
        assert fn(*args) == L.VMX_ERR_INVALID, args
        assert msg in _err(hip_lib), (args, _err(hip_lib))
    # n == 0 needs no rays and no output, but still a scene
    assert fn(None, None, None, 0, None, 0, None) == L.VMX_ERR_INVALID
    assert "NULL scene" in _err(hip_lib)

    cam = va.make_camera((0, 0, 0), (0, 0, 0), 16, 8, 8)
    opts = va.make_opts(seed=3)
    fc = hip_lib.vmx_raycast_camera_device
    P = C.byref
    bad_spp = va.make_camera((0, 0, 0), (0, 0, 0), 16, 8, 3)
    bad_units = va.make_camera((0, 0, 0), (0, 0, 0), 16, 8, 8)
    bad_units.rotation_units = 7
    world2 = va.make_opts(seed=3, world=2)
    cases = [
        ((None, P(cam), P(opts), 0, aligned, 0, None), "NULL scene"),
        ((None, P(cam), P(opts), 7, aligned, 0x100, None), "NULL scene"),  # k = kmax - 1
        ((None, P(cam), P(opts), 0, aligned, 2, None), "unknown raycast flags"),
        ((None, None, P(opts), 0, aligned, 0, None), "NULL camera or opts"),
        ((None, P(cam), None, 0, aligned, 0, None), "NULL camera or opts"),
        ((None, P(cam), P(opts), 0, None, 0, None), "NULL d_out"),
        ((None, P(cam), P(opts), 0, aligned + 8, 0, None), "16-byte aligned"),
        ((None, P(bad_spp), P(opts), 0, aligned, 0, None), "rays_per_pixel < 4"),
        ((None, P(bad_units), P(opts), 0, aligned, 0, None), "unknown rotation_units"),
        ((None, P(cam), P(world2), 0, aligned, 0, None), "world > 1"),
        ((None, P(cam), P(opts), 8, aligned, 0, None), "sample index out of range"),
        ((None, P(cam), P(opts), 0xFFFFFFFF, aligned, 0, None), "sample index out of range"),
    ]
    for args, msg in cases:
        assert fc(*args) == L.VMX_ERR_INVALID, args
        assert msg in _err(hip_lib), (args, _err(hip_lib))


def test_python_layer_rejects_mixed_and_misshaped_inputs_before_the_library():
    torch = pytest.importorskip("torch")

    class NoLib:  # any call into the library fails the test
        def __getattr__(self, name):
            raise AssertionError(f"library called: {name}")

    sc = va.Scene.__new__(va.Scene)
    sc._lib, sc._h, sc.device = NoLib(), None, 0
    o = np.zeros((4, 3), np.float32)
    t = torch.zeros((4, 3), dtype=torch.float32)  # a CPU tensor: not on the scene's device
    with pytest.raises(ValueError, match="mix"):
        sc.raycast(t, o)
    with pytest.raises(ValueError, match="mix"):
        sc.raycast(o, t)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        sc.raycast(t.reshape(-1), t.reshape(-1))
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        sc.raycast(t[:, :2], t)
    with pytest.raises(ValueError, match="float32"):
        sc.raycast(t.double(), t)
    with pytest.raises(ValueError, match="contiguous"):
        sc.raycast(t, torch.zeros((3, 4)).t())
    with pytest.raises(ValueError, match="both be"):
        sc.raycast(t, t[:3])
    with pytest.raises(ValueError, match="cuda"):
        sc.raycast(t, t)
    m = va.MeshEngine.__new__(va.MeshEngine)
    m.sceneAccelerator = sc
    with pytest.raises(ValueError, match="mix"):
        m.RayCast(t, o)
