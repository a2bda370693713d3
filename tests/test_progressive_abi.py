"""Progressive rendering (vmx_progressive_*) without a GPU: the symbols, the header, the struct layout, the argument
checks that come before any device work, and the Python layer's checks of the device preview's tensors."""
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
ENTRIES = ("vmx_progressive_begin", "vmx_progressive_step", "vmx_progressive_info_get", "vmx_progressive_preview_device",
           "vmx_progressive_preview", "vmx_progressive_end")


def _err(lib):
    return lib.vmx_last_error().decode()


def test_progressive_symbols_are_declared_and_bound(hip_lib):
    src = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, src), name
    # additive: no new ABI version, no new kernel slot in vmx_timings
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src) and hip_lib.vmx_abi_version() == 2
    assert re.search(r"#define VMX_K_COUNT 10\b", src) and len(L.K_NAMES) == 10
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER], check=True)


def test_progressive_info_layout_matches_header(tmp_path):
    fields = [n for n, _ in L.ProgressiveInfo._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vermilion_hip.h"\nint main(void){\n'
    prog += 'printf("size %zu\\n", sizeof(vmx_progressive_info));\n'
    for n in fields:
        prog += f'printf("{n} %zu\\n", offsetof(vmx_progressive_info, {n}));\n'
    prog += "return 0;}\n"
    src = tmp_path / "sz.c"
    src.write_text(prog)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(L.ProgressiveInfo) == 40
    for n in fields:
        assert int(out[n]) == getattr(L.ProgressiveInfo, n).offset, n


def test_progressive_argument_errors_do_not_need_a_gpu(hip_lib):
    """Each check of begin fires before the scene is looked at (a NULL scene is the last check), so each is seen alone;
    cam / opts get vmx_render's checks and messages."""
    P = C.byref
    cam = va.make_camera((0, 0, 0), (0, 0, 0), 16, 8, 8)
    opts = va.make_opts(seed=3)
    h = C.c_void_p()
    bad_spp = va.make_camera((0, 0, 0), (0, 0, 0), 16, 8, 3)
    bad_units = va.make_camera((0, 0, 0), (0, 0, 0), 16, 8, 8)
    bad_units.rotation_units = 7
    bad_res = va.make_camera((0, 0, 0), (0, 0, 0), 0, 8, 8)
    cases = [
        ((None, P(cam), P(opts), None, P(h)), "NULL scene"),
        ((None, P(cam), P(va.make_opts(sampling=L.VMX_SAMPLING_CORRECTED | 0x300)), None, P(h)), "NULL scene"),  # valid bits
        ((None, P(cam), P(va.make_opts(world=3, rank=2, stripe_rows=4)), None, P(h)), "NULL scene"),
        ((None, None, P(opts), None, P(h)), "NULL argument"),
        ((None, P(cam), None, None, P(h)), "NULL argument"),
        ((None, P(bad_spp), P(opts), None, P(h)), "rays_per_pixel < 4"),
        ((None, P(bad_units), P(opts), None, P(h)), "unknown rotation_units"),
        ((None, P(bad_res), P(opts), None, P(h)), "image resolution must be non-zero"),
        ((None, P(cam), P(va.make_opts(sampling=2)), None, P(h)), "unknown sampling mode"),
        ((None, P(cam), P(va.make_opts(sampling=0x400)), None, P(h)), "unknown sampling mode"),
        ((None, P(cam), P(va.make_opts(world=2, rank=2)), None, P(h)), "rank must be < world"),
        ((None, P(cam), P(va.make_opts(world=4, rank=7)), None, P(h)), "rank must be < world"),
        ((None, P(cam), P(opts), None, None), "NULL out"),
    ]
    for args, msg in cases:
        assert hip_lib.vmx_progressive_begin(*args) == L.VMX_ERR_INVALID, msg
        assert msg in _err(hip_lib), (msg, _err(hip_lib))
    assert not h.value
    st = L.Stats()
    info = L.ProgressiveInfo()
    frame = np.zeros(8, np.float32)
    for fn, args in ((hip_lib.vmx_progressive_step, (None, 4, P(st))),
                     (hip_lib.vmx_progressive_step, (None, 0, None)),
                     (hip_lib.vmx_progressive_info_get, (None, P(info))),
                     (hip_lib.vmx_progressive_preview, (None, frame.ctypes.data, None)),
                     (hip_lib.vmx_progressive_preview_device, (None, frame.ctypes.data, None)),
                     (hip_lib.vmx_progressive_end, (None,))):
        assert fn(*args) == L.VMX_ERR_INVALID, fn
        assert "NULL handle" in _err(hip_lib), _err(hip_lib)
    # both outputs NULL: checked before the handle, so it is seen alone
    for fn in (hip_lib.vmx_progressive_preview, hip_lib.vmx_progressive_preview_device):
        assert fn(None, None, None) == L.VMX_ERR_INVALID
        assert "no output" in _err(hip_lib), _err(hip_lib)


class NoLib:  # any call into the library fails the test
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def _handle(shape=(41, 70)):
    sc = va.Scene.__new__(va.Scene)
    sc._lib, sc._h, sc.device = NoLib(), None, 0
    p = va.Progressive.__new__(va.Progressive)
    p._scene, p._lib, p._h, p.device, p.shape, p._stream = sc, sc._lib, None, 0, shape, None
    return p


def test_python_layer_rejects_bad_preview_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    p = _handle()
    f = torch.zeros((41, 70, 5), dtype=torch.float32)  # CPU tensors: not on the scene's device
    q = torch.zeros((41, 70, 4), dtype=torch.uint8)
    with pytest.raises(ValueError, match="both None"):
        p.preview_device()
    with pytest.raises(ValueError, match="torch tensor"):
        p.preview_device(rgbaz=np.zeros((41, 70, 5), np.float32))
    with pytest.raises(ValueError, match="float32"):
        p.preview_device(rgbaz=f.double())
    with pytest.raises(ValueError, match="uint8"):
        p.preview_device(rgba8=q.int())
    with pytest.raises(ValueError, match=r"\[41, 70, 5\]"):
        p.preview_device(rgbaz=f.reshape(-1, 5))
    with pytest.raises(ValueError, match=r"\[41, 70, 5\]"):
        p.preview_device(rgbaz=torch.zeros((41, 70, 4)))
    with pytest.raises(ValueError, match=r"\[41, 70, 4\]"):
        p.preview_device(rgbaz=None, rgba8=torch.zeros((70, 41, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="contiguous"):
        p.preview_device(rgbaz=torch.zeros((70, 41, 5)).transpose(0, 1))
    with pytest.raises(ValueError, match="contiguous"):
        p.preview_device(rgba8=torch.zeros((41, 70, 8), dtype=torch.uint8)[:, :, ::2])
    with pytest.raises(ValueError, match="cuda"):
        p.preview_device(rgbaz=f)
    with pytest.raises(ValueError, match="cuda"):
        p.preview_device(rgba8=q)
    with pytest.raises(ValueError, match="cuda"):
        p.preview_device(f, q)
    p._h = None  # (nothing to end: __del__ must not reach the library either)
