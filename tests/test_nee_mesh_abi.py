"""Emissive triangles (vmx_scene_set_emitters, vmx_scene_emitters, vmx_multi_set_emitters, vmx_emitters_check) without a
GPU: the symbols, the structs, the header, and every refusal that comes before any device work, each seen alone and in the
order the header states.  A scene cannot exist here, so the refusals after the NULL scene are seen through
vmx_emitters_check, the routine vmx_scene_set_emitters runs them with (tests/test_gpu_nee_mesh.py sees them on a scene)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vermilion_hip.h")
ENTRIES = ("vmx_scene_set_emitters", "vmx_scene_emitters", "vmx_multi_set_emitters", "vmx_emitters_check")
NTRIS = 10


def _err(lib):
    return lib.vmx_last_error().decode()


def refused(lib, code, what):
    assert code == L.VMX_ERR_INVALID, what
    assert what in _err(lib), (what, _err(lib))


def table(ids, radiance=(1.0, 1.0, 1.0)):
    return S.emitter_table(ids, radiance)


def test_symbols_structs_and_header(hip_lib):
    src = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(hip_lib, name) and name in L.SYMBOLS, name
        decl = re.search(r"\bint %s\((.*?)\);" % name, src, re.S)
        assert decl, name
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1)).split(",")) == len(L.SYMBOLS[name][1]), name
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src) and hip_lib.vmx_abi_version() == 2
    assert re.search(r"#define VMX_MAX_EMITTERS 65536u\b", src) and L.VMX_MAX_EMITTERS == 65536
    # the structs as declared: 16 and 40 bytes, the doubles 8-byte aligned
    assert C.sizeof(L.Emitter) == 16 and C.sizeof(L.EmitterInfo) == 40 == S.EMITTER_DTYPE.itemsize
    assert [L.EmitterInfo.area.offset, L.EmitterInfo.weight.offset, L.EmitterInfo.cdf.offset] == [16, 24, 32]
    assert [S.EMITTER_DTYPE.fields[k][1] for k in ("tri_id", "radiance", "area", "weight", "cdf")] == [0, 4, 16, 24, 32]
    probe = ('#include "%s"\n_Static_assert(sizeof(vmx_emitter) == 16 && sizeof(vmx_emitter_info) == 40, "sizes");\n' % HEADER)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-"], input=probe.encode(), check=True)
    # the header says who sees the table and who does not
    flat = src.replace("\n * ", " ")
    assert "The table means something to the LIGHT-SAMPLED integrator only" in flat
    assert "see ordinary unlit triangles, exactly as before" in flat
    for name in ("set_emitters", "emitters"):
        assert callable(getattr(va.Scene, name)), name
    assert callable(va.MultiScene.set_emitters)


def test_null_handles_come_first(hip_lib):
    lib = hip_lib
    tb, n = table([1, 2])
    n_out = C.c_uint32(7)
    # the NULL scene before everything else: a NULL table with n > 0, too many, a bad id
    for args in ((tb, n), (None, 3), (None, 0), (tb, L.VMX_MAX_EMITTERS + 1)):
        refused(lib, lib.vmx_scene_set_emitters(None, *args), "NULL scene")
        refused(lib, lib.vmx_multi_set_emitters(None, *args), "NULL vmx_multi")
    refused(lib, lib.vmx_scene_emitters(None, None, 0, C.byref(n_out)), "NULL scene")
    refused(lib, lib.vmx_scene_emitters(None, None, 0, None), "NULL scene")
    assert n_out.value == 7


def test_every_refusal_in_the_documented_order(hip_lib):
    lib = hip_lib

    def check(tb, n, ntris=NTRIS):
        return lib.vmx_emitters_check(tb, n, ntris)

    good, n = table([0, 9, 4])
    assert check(good, n) == L.VMX_OK and check(None, 0) == L.VMX_OK and check(good, 0) == L.VMX_OK
    assert check(None, 0, 0) == L.VMX_OK
    refused(lib, check(None, 1), "NULL emitters with n > 0")
    refused(lib, check(None, L.VMX_MAX_EMITTERS + 1), "NULL emitters with n > 0")  # (before the count)
    many, m = table(list(range(NTRIS + 1)))
    refused(lib, check(many, m), "more emitters than the scene has triangles")
    big = (L.Emitter * (L.VMX_MAX_EMITTERS + 1))()
    for i, e in enumerate(big):
        e.tri_id = i
    refused(lib, check(big, len(big), 1 << 20), "more than VMX_MAX_EMITTERS emitters")
    refused(lib, check(big, len(big), 5), "more than VMX_MAX_EMITTERS emitters")  # (before n > ntris)
    assert check(big, L.VMX_MAX_EMITTERS, 1 << 20) == L.VMX_OK
    # a count above ntris before a bad id among them
    refused(lib, check(many, m, 3), "more emitters than the scene has triangles")
    bad_id, k = table([0, NTRIS])
    refused(lib, check(bad_id, k), "is not below the scene's triangle count")
    # a bad id before a repeated one, a repeated one before a bad radiance
    both, k = table([3, 3, NTRIS])
    refused(lib, check(both, k), "is not below the scene's triangle count")
    twice, k = table([3, 5, 3], [[1, 1, 1], [-1, 1, 1], [1, 1, 1]])
    refused(lib, check(twice, k), "triangle id 3 is listed more than once")
    for bad in (-1.0, -0.0 - 1e-30, float("nan"), float("inf"), float("-inf")):
        for comp in range(3):
            rad = np.ones((2, 3), np.float32)
            rad[1, comp] = bad
            tb, k = table([2, 7], rad)
            refused(lib, check(tb, k), "emitter 1: a radiance component is negative or not finite")
    zero, k = table([2, 7], [0.0, 0.0, 0.0])
    assert check(zero, k) == L.VMX_OK  # black is a radiance
