"""Light sampling (vmx_render_nee*, vmx_radiance_nee) without a GPU: the symbols, the header, and the argument checks that
come before any device work — each fires before the scene is looked at (a NULL scene is the last check), so each is seen
alone."""
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
ENTRIES = ("vmx_render_nee", "vmx_render_nee_device", "vmx_radiance_nee")
CORRECTED = L.VMX_SAMPLING_CORRECTED


def _err(lib):
    return lib.vmx_last_error().decode()


def _opts(**kw):
    kw.setdefault("sampling", CORRECTED)
    kw.setdefault("early_stop", False)
    return va.make_opts(seed=3, **kw)


def _calls(lib, opts, cam=None):
    """the three entries with valid buffers, a NULL scene and the given options"""
    cam = cam or va.make_camera((0, 0, 0), (0, 0, 0), 16, 8, 8)
    frame = np.zeros((8, 16, 5), np.float32)
    o, d, out = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32), np.zeros((4, 4), np.float32)
    st = L.Stats()
    return {
        "vmx_render_nee": lambda: lib.vmx_render_nee(None, C.byref(cam), C.byref(opts), frame.ctypes.data, C.byref(st)),
        "vmx_render_nee_device": lambda: lib.vmx_render_nee_device(None, C.byref(cam), C.byref(opts), frame.ctypes.data,
                                                                   C.byref(st), None),
        "vmx_radiance_nee": lambda: lib.vmx_radiance_nee(None, o.ctypes.data, d.ctypes.data, 4, C.byref(opts), out.ctypes.data,
                                                         C.byref(st)),
    }


def test_nee_symbols_are_declared_and_bound(hip_lib):
    src = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, src), name
    for name in ("render_nee", "render_nee_device", "radiance_nee"):
        assert callable(getattr(va.Scene, name))
    # additive: no new ABI version, no new kernel slot in vmx_timings
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src) and hip_lib.vmx_abi_version() == 2
    assert re.search(r"#define VMX_K_COUNT 10\b", src) and len(L.K_NAMES) == 10
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER], check=True)


def test_nee_null_arguments(hip_lib):
    cam = va.make_camera((0, 0, 0), (0, 0, 0), 16, 8, 8)
    opts = _opts()
    buf = np.zeros(16 * 8 * 5, np.float32)
    P = C.byref
    st = L.Stats()
    for args in ((None, P(opts), buf.ctypes.data), (P(cam), None, buf.ctypes.data), (P(cam), P(opts), None)):
        assert hip_lib.vmx_render_nee(None, args[0], args[1], args[2], P(st)) == L.VMX_ERR_INVALID
        assert "NULL argument" in _err(hip_lib)
        assert hip_lib.vmx_render_nee_device(None, args[0], args[1], args[2], P(st), None) == L.VMX_ERR_INVALID
        assert "NULL argument" in _err(hip_lib)
    o = np.zeros((4, 3), np.float32)
    for args in ((None, o.ctypes.data, P(opts), buf.ctypes.data), (o.ctypes.data, None, P(opts), buf.ctypes.data),
                 (o.ctypes.data, o.ctypes.data, None, buf.ctypes.data), (o.ctypes.data, o.ctypes.data, P(opts), None)):
        assert hip_lib.vmx_radiance_nee(None, args[0], args[1], 4, args[2], args[3], None) == L.VMX_ERR_INVALID
        assert "NULL argument" in _err(hip_lib)
    # everything else valid: the scene is the last thing looked at
    for name, call in _calls(hip_lib, opts).items():
        assert call() == L.VMX_ERR_INVALID, name
        assert "NULL scene" in _err(hip_lib), name


REJECTED = [
    ("parity", dict(sampling=L.VMX_SAMPLING_PARITY), "VMX_SAMPLING_CORRECTED"),
    ("unknown_mode", dict(sampling=2), "unknown sampling mode"),
    ("unknown_bit", dict(sampling=CORRECTED | 0x400), "unknown sampling mode"),
    ("elide_dead", dict(sampling=CORRECTED | L.VMX_SAMPLING_ELIDE_DEAD), "VMX_SAMPLING_ELIDE_DEAD"),
    ("early_stop", dict(early_stop=True), "early_stop"),
    ("world", dict(world=2, rank=1), "world"),
    ("collect_counters", dict(collect_counters=True), "collect_counters"),
    ("reserved0", dict(pipeline=1), "reserved[0]"),
]


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_nee_rejected_options_name_what_was_rejected(hip_lib, case):
    _, kw, word = case
    for name, call in _calls(hip_lib, _opts(**kw)).items():
        assert call() == L.VMX_ERR_INVALID, name
        assert word in _err(hip_lib), (name, _err(hip_lib))


def test_nee_accepted_options_reach_the_scene_check(hip_lib):
    for kw in (dict(), dict(sampling=CORRECTED | L.VMX_SAMPLING_LIBM_DOUBLE), dict(samples_per_batch=1), dict(world=1)):
        for name, call in _calls(hip_lib, _opts(**kw)).items():
            assert call() == L.VMX_ERR_INVALID and "NULL scene" in _err(hip_lib), (name, kw)


def test_nee_radiance_of_no_rays_is_ok(hip_lib):
    o = np.zeros((1, 3), np.float32)
    opts = _opts()
    assert hip_lib.vmx_radiance_nee(None, o.ctypes.data, o.ctypes.data, 0, C.byref(opts), o.ctypes.data, None) == L.VMX_OK
    # ... but its options are still checked
    bad = _opts(early_stop=True)
    assert hip_lib.vmx_radiance_nee(None, o.ctypes.data, o.ctypes.data, 0, C.byref(bad), o.ctypes.data, None) == L.VMX_ERR_INVALID
