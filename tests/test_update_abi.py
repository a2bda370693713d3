"""In-place geometry updates (vmx_scene_update / vmx_scene_update_device / vmx_multi_update) without a GPU: the
symbols, the constants, and the argument checks that come before any device work."""
import os
import re

import numpy as np
import pytest

from vermilion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vermilion_hip.h")
NAMES = ("vmx_scene_update", "vmx_scene_update_device", "vmx_multi_update")


def test_update_symbols_and_constants(hip_lib):
    src = open(HEADER).read()
    for name in NAMES:
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, src), name
    consts = {k: int(v, 0) for k, v in re.findall(r"#define (VMX_UPDATE_[A-Z_]+)\s+(0x[0-9a-fA-F]+|\d+)u", src)}
    assert consts == {"VMX_UPDATE_REFIT": 0, "VMX_UPDATE_REBUILD": 1}
    for k, v in consts.items():
        assert getattr(L, k) == v, k
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src)
    assert hip_lib.vmx_abi_version() == 2


def _err(lib):
    return lib.vmx_last_error().decode()


@pytest.mark.parametrize("name", NAMES)
def test_update_argument_errors_do_not_need_a_gpu(hip_lib, name):
    """Each check fires before the scene is looked at (a NULL scene is the last check), so each is seen on its own,
    on a box without a device."""
    fn = getattr(hip_lib, name)
    extra = (None,) if name == "vmx_scene_update_device" else ()
    a = np.zeros((4, 9), np.float32)
    P = a.ctypes.data
    cases = [
        ((None, P, P, None, 4, 0), "NULL scene"),
        ((None, P, None, None, 4, 1), "NULL scene"),  # REBUILD is a known flag
        ((None, P, P, P, 4, 2), "unknown update flags"),
        ((None, P, None, None, 4, 0x80000000), "unknown update flags"),
        ((None, None, None, None, 4, 0), "pos, nrm and uv are all NULL"),
        ((None, None, None, None, 4, 1), "pos, nrm and uv are all NULL"),
        ((None, P, None, None, 0, 0), "ntris is 0"),
        ((None, None, None, P, 0, 1), "ntris is 0"),
    ]
    for args, msg in cases:
        assert fn(*(args + extra)) == L.VMX_ERR_INVALID, (name, args)
        assert msg in _err(hip_lib), (name, args, _err(hip_lib))


def test_python_layer_rejects_empty_updates_before_the_library():
    import vermilion_amd as va
    sc = va.Scene.__new__(va.Scene)  # no device needed: the arguments are checked first
    with pytest.raises(ValueError, match="nothing to update"):
        sc.update()
    sc.ntris = 4
    with pytest.raises(ValueError, match="another count"):
        sc.update(pos=np.zeros((5, 9), np.float32))
    ms = va.MultiScene.__new__(va.MultiScene)
    ms.ntris = 4
    with pytest.raises(ValueError, match="nothing to update"):
        ms.update()
    with pytest.raises(ValueError, match="another count"):
        ms.update(uv=np.zeros((5, 6), np.float32))
