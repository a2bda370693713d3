"""Light-sampled progressive handles and budgeted steps (vmx_progressive_begin_nee, vmx_sampling_budget_default_params,
vmx_progressive_budget_device / step_budget_device / step_budgeted) without a GPU: the symbols, the struct layout against
the header, the defaults, and the argument checks that come before any device work, each seen alone.  (The refusals by kind
of handle need a handle, hence a device: tests/test_gpu_nee_progressive.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import budget_spec as BS
import vermilion_amd as va
from vermilion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vermilion_hip.h")
ENTRIES = ("vmx_progressive_begin_nee", "vmx_sampling_budget_default_params", "vmx_progressive_budget_device",
           "vmx_progressive_step_budget_device", "vmx_progressive_step_budgeted")
CORRECTED = L.VMX_SAMPLING_CORRECTED
F = np.float32
N = None


def _err(lib):
    return lib.vmx_last_error().decode()


def _opts(**kw):
    kw.setdefault("sampling", CORRECTED)
    kw.setdefault("early_stop", False)
    return va.make_opts(seed=3, **kw)


def refused(lib, fn, args, what):
    assert getattr(lib, fn)(*args) == L.VMX_ERR_INVALID, (fn, what)
    assert what in _err(lib), (fn, what, _err(lib))


def test_symbols_are_declared_and_bound(hip_lib):
    src = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
        decl = re.search(r"\bint %s\((.*?)\);" % name, src, re.S)
        assert decl, name
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1)).split(",")) == len(L.SYMBOLS[name][1]), name
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src) and hip_lib.vmx_abi_version() == 2
    assert "make_sampling_budget_params" in va.__all__ and hasattr(va, "make_sampling_budget_params")
    assert callable(va.Scene.progressive_nee)
    for name in ("budget_device", "step_budget", "step_budgeted"):
        assert hasattr(va.Progressive, name), name
    # the header states what the budgets select, and what stays out of scope
    assert "b_p != 0 exactly where select_device writes 1" in src
    assert "per-pixel sample budgets within one step" not in src
    assert re.search(r"Out of scope: budgeted steps on plain handles", src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER], check=True)


def test_budget_params_layout_matches_header(tmp_path):
    fields = [n for n, _ in L.SamplingBudgetParams._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vermilion_hip.h"\nint main(void){\n'
    prog += 'printf("size %zu\\n", sizeof(vmx_sampling_budget_params));\n'
    for n in fields:
        prog += f'printf("{n} %zu\\n", offsetof(vmx_sampling_budget_params, {n}));\n'
    prog += "return 0;}\n"
    src = tmp_path / "sz.c"
    src.write_text(prog)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(L.SamplingBudgetParams) == 48
    assert [int(out[n]) for n in fields] == [getattr(L.SamplingBudgetParams, n).offset for n in fields] == [0, 32, 36]


def test_default_params(hip_lib):
    p = L.SamplingBudgetParams()
    p.select.threshold, p.select.min_samples, p.max_step, p.reserved[1] = 9.0, 9, 9, 9
    assert hip_lib.vmx_sampling_budget_default_params(C.byref(p)) == L.VMX_OK
    s = L.SamplingParams()
    assert hip_lib.vmx_sampling_default_params(C.byref(s)) == L.VMX_OK
    assert p.select.as_dict() == s.as_dict() and p.max_step == 0 and list(p.reserved) == [0, 0, 0]
    assert (F(p.select.threshold), F(p.select.floor), p.select.min_samples, p.select.radius, p.max_step) == \
        (F(BS.DEFAULTS["threshold"]), F(BS.DEFAULTS["floor"]), BS.DEFAULTS["min_samples"], BS.DEFAULTS["radius"], BS.DEFAULTS["max_step"])
    assert hip_lib.vmx_sampling_budget_default_params(None) == L.VMX_ERR_INVALID
    q = va.make_sampling_budget_params(threshold=2, radius=3, max_step=5)
    assert (q.select.threshold, q.select.min_samples, q.select.radius, q.max_step) == (2.0, 8, 3, 5)


# ---- vmx_progressive_begin_nee -----------------------------------------------------------------------------------------------
def _begin(lib, cam, opts, flags=0, out=True):
    h = C.c_void_p()
    return lib.vmx_progressive_begin_nee(None, None if cam is None else C.byref(cam), None if opts is None else C.byref(opts), flags,
                                         None, C.byref(h) if out else None)


def test_begin_nee_null_arguments_and_flags(hip_lib):
    cam, opts = va.make_camera((0, 0, 0), (0, 0, 0), 16, 8, 8), _opts()
    for c, o in ((None, opts), (cam, None)):
        assert _begin(hip_lib, c, o) == L.VMX_ERR_INVALID and "NULL argument" in _err(hip_lib)
    assert _begin(hip_lib, cam, opts, out=False) == L.VMX_ERR_INVALID and "NULL out" in _err(hip_lib)
    for flags in (2, 3, 1 << 31):
        assert _begin(hip_lib, cam, opts, flags) == L.VMX_ERR_INVALID and "unknown flag" in _err(hip_lib)
    # everything else valid, with and without moments: the scene is the last thing looked at
    for flags in (0, L.VMX_PROGRESSIVE_MOMENTS):
        assert _begin(hip_lib, cam, opts, flags) == L.VMX_ERR_INVALID and "NULL scene" in _err(hip_lib)
    # the order: cam / opts, out, flags, opts contents, frame, scene
    bad_opts, bad_cam = _opts(early_stop=True), va.make_camera((0, 0, 0), (0, 0, 0), 16, 8, 2)
    assert _begin(hip_lib, None, bad_opts, 2, out=False) == L.VMX_ERR_INVALID and "NULL argument" in _err(hip_lib)
    assert _begin(hip_lib, bad_cam, bad_opts, 2, out=False) == L.VMX_ERR_INVALID and "NULL out" in _err(hip_lib)
    assert _begin(hip_lib, bad_cam, bad_opts, 2) == L.VMX_ERR_INVALID and "unknown flag" in _err(hip_lib)
    assert _begin(hip_lib, bad_cam, bad_opts) == L.VMX_ERR_INVALID and "early_stop" in _err(hip_lib)
    assert _begin(hip_lib, bad_cam, opts) == L.VMX_ERR_INVALID and "rays_per_pixel < 4" in _err(hip_lib)


REJECTED = [
    ("parity", dict(sampling=L.VMX_SAMPLING_PARITY), "light sampling: sampling must be VMX_SAMPLING_CORRECTED"),
    ("unknown_mode", dict(sampling=2), "unknown sampling mode"),
    ("elide_dead", dict(sampling=CORRECTED | L.VMX_SAMPLING_ELIDE_DEAD), "light sampling: VMX_SAMPLING_ELIDE_DEAD does not apply"),
    ("early_stop", dict(early_stop=True), "light sampling: early_stop is not supported"),
    ("world", dict(world=2, rank=1), "light sampling: world > 1 is not supported"),
    ("collect_counters", dict(collect_counters=True), "light sampling: collect_counters is not supported"),
    ("reserved0", dict(pipeline=1), "light sampling: reserved[0] must be 0"),
]


@pytest.mark.parametrize("case", REJECTED, ids=[c[0] for c in REJECTED])
def test_begin_nee_refuses_what_render_nee_refuses_with_its_messages(hip_lib, case):
    _, kw, message = case
    cam, opts = va.make_camera((0, 0, 0), (0, 0, 0), 16, 8, 8), _opts(**kw)
    frame = np.zeros((8, 16, 5), np.float32)
    assert hip_lib.vmx_render_nee(None, C.byref(cam), C.byref(opts), frame.ctypes.data, None) == L.VMX_ERR_INVALID
    assert _err(hip_lib) == message
    for flags in (0, L.VMX_PROGRESSIVE_MOMENTS):
        assert _begin(hip_lib, cam, opts, flags) == L.VMX_ERR_INVALID
        assert _err(hip_lib) == message


def test_begin_nee_accepted_options_reach_the_scene_check(hip_lib):
    cam = va.make_camera((0, 0, 0), (0, 0, 0), 16, 8, 8)
    for kw in (dict(), dict(sampling=CORRECTED | L.VMX_SAMPLING_LIBM_DOUBLE), dict(samples_per_batch=1), dict(world=1)):
        assert _begin(hip_lib, cam, _opts(**kw)) == L.VMX_ERR_INVALID and "NULL scene" in _err(hip_lib), kw


def test_begin_ex_still_refuses_unknown_flags(hip_lib):
    cam, opts = va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 16), va.make_opts(seed=1, early_stop=False)
    out = C.c_void_p()
    for flags in (2, 3, 1 << 31):
        refused(hip_lib, "vmx_progressive_begin_ex", (N, C.byref(cam), C.byref(opts), flags, N, C.byref(out)),
                "vmx_progressive_begin_ex: unknown flag")


# ---- the budget entries ---------------------------------------------------------------------------------------------------------
def test_budget_checks_do_not_need_a_gpu(hip_lib):
    """params first, then the pointers (NULL, alignment, buffers that meet), then the handle"""
    buf = np.zeros(64, np.float32)
    ptr = (buf.ctypes.data + 15) & ~15
    lib = hip_lib
    refused(lib, "vmx_progressive_budget_device", (N, N, N, N), "NULL d_budget")
    refused(lib, "vmx_progressive_budget_device", (N, N, ptr + 2, N), "d_budget must be 4-byte aligned")
    refused(lib, "vmx_progressive_budget_device", (N, N, ptr, ptr + 20), "d_total must be 8-byte aligned")
    refused(lib, "vmx_progressive_budget_device", (N, N, ptr + 4, ptr), "d_budget and d_total overlap")
    refused(lib, "vmx_progressive_budget_device", (N, N, ptr, ptr), "d_budget and d_total overlap")
    refused(lib, "vmx_progressive_budget_device", (N, N, ptr + 8, ptr), "NULL handle")
    refused(lib, "vmx_progressive_budget_device", (N, N, ptr, N), "NULL handle")
    refused(lib, "vmx_progressive_step_budget_device", (N, N, N, N), "NULL d_budget")
    refused(lib, "vmx_progressive_step_budget_device", (N, ptr + 1, N, N), "d_budget must be 4-byte aligned")
    refused(lib, "vmx_progressive_step_budget_device", (N, ptr, N, N), "NULL handle")
    refused(lib, "vmx_progressive_step_budgeted", (N, N, N, N), "NULL handle")
    # the order: a misaligned pointer is seen before the NULL handle, bad params before a NULL pointer
    refused(lib, "vmx_progressive_budget_device", (N, N, ptr + 4, ptr + 4), "d_total must be 8-byte aligned")
    bad = [dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold=-0.5),
           dict(floor=float("nan")), dict(floor=float("inf")), dict(floor=0.0), dict(floor=-0.1),
           dict(min_samples=0), dict(min_samples=1), dict(radius=4), dict(radius=1 << 31)]
    for kw in bad:
        p = va.make_sampling_budget_params(**kw)
        for fn, args in (("vmx_progressive_budget_device", (N, C.byref(p), N, N)), ("vmx_progressive_step_budgeted", (N, C.byref(p), N, N))):
            refused(lib, fn, args, "vmx_sampling_params")
            assert list(kw)[0] in _err(lib), (kw, _err(lib))
    for i in range(4):
        p = va.make_sampling_budget_params()
        p.select.reserved[i] = 1
        refused(lib, "vmx_progressive_budget_device", (N, C.byref(p), ptr, N), "vmx_sampling_params: reserved")
    for i in range(3):
        p = va.make_sampling_budget_params()
        p.reserved[i] = 1
        refused(lib, "vmx_progressive_budget_device", (N, C.byref(p), N, N), "vmx_sampling_budget_params: reserved")
        refused(lib, "vmx_progressive_step_budgeted", (N, C.byref(p), N, N), "vmx_sampling_budget_params: reserved")
    # every max_step is a count (no bit of it is reserved): what is valid reaches the handle check
    for ms in (0, 1, 7, 0xFFFFFFFF):
        ok = va.make_sampling_budget_params(threshold=0.0, min_samples=2, radius=0, max_step=ms)
        refused(lib, "vmx_progressive_budget_device", (N, C.byref(ok), ptr, N), "NULL handle")
        refused(lib, "vmx_progressive_step_budgeted", (N, C.byref(ok), N, N), "NULL handle")
