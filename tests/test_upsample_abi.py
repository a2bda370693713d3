"""G-buffer-guided upsampling (vmx_upsample_*) without a GPU: the symbols, the struct layout against the header, the
defaults, the argument checks that come before any device work, the Python layer's checks of its tensors — and the
conditions the restatement itself (tests/upsample_spec.py, what the GPU tests compare with) is held to, on oracle data
and on synthetic cases, so that the yardstick cannot drift."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import filter_spec as FS
import oracle_lib as O
import upsample_spec as US
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vermilion_hip.h")
ENTRIES = ("vmx_upsample_default_params", "vmx_upsample_create", "vmx_upsample_destroy", "vmx_upsample_set_guides_device",
           "vmx_upsample_apply_device")


def _err(lib):
    return lib.vmx_last_error().decode()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_upsample_symbols_are_declared_and_bound(hip_lib):
    src = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, src), name
    # additive: no new ABI version
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src) and hip_lib.vmx_abi_version() == 2
    for name in ("Upsample", "make_upsample_params", "low_camera"):
        assert name in va.__all__ and hasattr(va, name)


def test_upsample_params_layout_matches_header(tmp_path):
    fields = [n for n, _ in L.UpsampleParams._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vermilion_hip.h"\nint main(void){\n'
    prog += 'printf("size %zu\\n", sizeof(vmx_upsample_params));\n'
    for n in fields:
        prog += f'printf("{n} %zu\\n", offsetof(vmx_upsample_params, {n}));\n'
    prog += "return 0;}\n"
    src = tmp_path / "sz.c"
    src.write_text(prog)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(L.UpsampleParams) == 32
    for n in fields:
        assert int(out[n]) == getattr(L.UpsampleParams, n).offset, n
    assert [int(out[n]) for n in fields] == [0, 4, 8]


def test_default_params(hip_lib):
    p = L.UpsampleParams(9, 9.0, (C.c_uint32 * 6)(1, 2, 3, 4, 5, 6))
    assert hip_lib.vmx_upsample_default_params(C.byref(p)) == L.VMX_OK
    assert p.normal_squarings == 5 and np.float32(p.sigma_depth) == np.float32(0.1)
    assert list(p.reserved) == [0] * 6
    assert hip_lib.vmx_upsample_default_params(None) == L.VMX_ERR_INVALID
    q = va.make_upsample_params(sigma_depth=0.5)
    assert (q.normal_squarings, q.sigma_depth) == (5, 0.5)
    assert va.make_upsample_params(normal_squarings=2).normal_squarings == 2
    # the restatement's defaults are the library's
    lib_defaults, spec_defaults = US.params_of(va.make_upsample_params()), US.params_of()
    assert all(np.float32(lib_defaults[k]) == np.float32(spec_defaults[k]) for k in spec_defaults)


def test_low_camera_replaces_image_res_only():
    c = scenes.cornell_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], 72, 40, 16)
    low = va.low_camera(cam, 36, 20)
    assert tuple(low.image_res) == (36, 20) and tuple(cam.image_res) == (72, 40)
    low.image_res[:] = [72, 40]
    assert bytes(low) == bytes(cam)


def test_create_and_null_handles_do_not_need_a_gpu(hip_lib):
    h = C.c_void_p()
    create = hip_lib.vmx_upsample_create
    # a zero size is refused before the device is looked at
    for lw, lh, w, hh in ((0, 4, 8, 8), (4, 0, 8, 8), (4, 4, 0, 8), (4, 4, 8, 0), (0, 0, 0, 0)):
        assert create(0, lw, lh, w, hh, C.byref(h)) == L.VMX_ERR_INVALID
        assert "resolution must be non-zero" in _err(hip_lib) and not h.value
    # the size limits, each named: the low frame no larger than the full one, the full one at most 4 times the low one
    for lw, lh, w, hh in ((9, 4, 8, 8), (4, 9, 8, 8)):
        assert create(0, lw, lh, w, hh, C.byref(h)) == L.VMX_ERR_INVALID
        assert "low_width <= width" in _err(hip_lib) and not h.value
    for lw, lh, w, hh in ((2, 4, 9, 8), (4, 2, 8, 9), (1, 1, 5, 1)):
        assert create(0, lw, lh, w, hh, C.byref(h)) == L.VMX_ERR_INVALID
        assert "width <= 4 * low_width" in _err(hip_lib) and not h.value
    assert create(0, 1 << 15, 1 << 15, 1 << 16, 1 << 16, C.byref(h)) == L.VMX_ERR_INVALID  # make_frame's size check
    assert "image too large" in _err(hip_lib)
    assert create(0, 4, 4, 8, 8, None) == L.VMX_ERR_INVALID
    # no such device: an ordinal no machine has; without any device, device 0 as well
    assert create(1 << 20, 4, 4, 8, 8, C.byref(h)) == L.VMX_ERR_NO_DEVICE and not h.value
    if hip_lib.vmx_device_count() == 0:
        assert create(0, 4, 4, 8, 8, C.byref(h)) == L.VMX_ERR_NO_DEVICE and not h.value
        assert "no CPU path" in _err(hip_lib)
        with pytest.raises(va.VmxError) as e:
            va.Upsample(4, 4, 8, 8)
        assert e.value.code == L.VMX_ERR_NO_DEVICE
    buf = np.zeros(64, np.float32)
    ptr = buf.ctypes.data
    aligned = ptr + (-ptr % 16)
    for fn, args in ((hip_lib.vmx_upsample_destroy, (None,)),
                     (hip_lib.vmx_upsample_set_guides_device, (None, aligned, aligned, None)),
                     (hip_lib.vmx_upsample_apply_device, (None, ptr, ptr, None, None, None))):
        assert fn(*args) == L.VMX_ERR_INVALID, fn
        assert "NULL handle" in _err(hip_lib), _err(hip_lib)
    # checks that come before the handle, so that each is seen alone: outputs, then parameters
    assert hip_lib.vmx_upsample_apply_device(None, ptr, None, None, None, None) == L.VMX_ERR_INVALID
    assert "no output" in _err(hip_lib)
    bad = [dict(normal_squarings=9), dict(sigma_depth=0.0), dict(sigma_depth=float("nan")), dict(sigma_depth=float("inf")),
           dict(sigma_depth=-1.0)]
    for kw in bad:
        p = va.make_upsample_params(**kw)
        assert hip_lib.vmx_upsample_apply_device(None, ptr, ptr, None, C.byref(p), None) == L.VMX_ERR_INVALID, kw
        assert "vmx_upsample_params" in _err(hip_lib), (kw, _err(hip_lib))
        # ... and the outputs come before the parameters
        assert hip_lib.vmx_upsample_apply_device(None, ptr, None, None, C.byref(p), None) == L.VMX_ERR_INVALID, kw
        assert "no output" in _err(hip_lib), (kw, _err(hip_lib))
    p = va.make_upsample_params()
    p.reserved[4] = 1
    assert hip_lib.vmx_upsample_apply_device(None, ptr, ptr, None, C.byref(p), None) == L.VMX_ERR_INVALID
    assert "reserved" in _err(hip_lib)
    # pointers: NULL and alignment, before the handle
    assert hip_lib.vmx_upsample_apply_device(None, None, ptr, None, None, None) == L.VMX_ERR_INVALID
    assert "NULL d_low_rgbaz" in _err(hip_lib)
    assert hip_lib.vmx_upsample_apply_device(None, ptr + 2, ptr, None, None, None) == L.VMX_ERR_INVALID
    assert "4-byte aligned" in _err(hip_lib)
    for args, msg in (((None, aligned), "NULL d_rayhit_low"), ((aligned, None), "NULL d_rayhit_full"),
                      ((aligned + 4, aligned), "16-byte aligned"), ((aligned, aligned + 8), "16-byte aligned")):
        assert hip_lib.vmx_upsample_set_guides_device(None, *args, None) == L.VMX_ERR_INVALID
        assert msg in _err(hip_lib), (msg, _err(hip_lib))


class NoLib:  # any call into the library fails the test
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_layer_rejects_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    u = va.Upsample.__new__(va.Upsample)
    u._lib, u._h, u.device, u.low_shape, u.shape = NoLib(), None, 0, (28, 47), (41, 70)
    low = torch.zeros((28, 47, 5), dtype=torch.float32)  # CPU tensors: not on the handle's device
    with pytest.raises(ValueError, match="torch tensor"):
        u.apply(np.zeros((28, 47, 5), np.float32))
    with pytest.raises(ValueError, match="float32"):
        u.apply(low.double())
    with pytest.raises(ValueError, match=r"\[28, 47, 5\]"):
        u.apply(torch.zeros((41, 70, 5)))  # a full-size frame is not the input
    with pytest.raises(ValueError, match="contiguous"):
        u.apply(torch.zeros((47, 28, 5)).transpose(0, 1))
    with pytest.raises(ValueError, match="cuda"):
        u.apply(low)
    with pytest.raises(ValueError, match="torch tensor"):
        u.set_guides(np.zeros((28, 47, 16), np.float32), torch.zeros((41, 70, 16)))
    with pytest.raises(ValueError, match=r"\[28, 47, 16\]"):
        u.set_guides(torch.zeros((41, 70, 16)), torch.zeros((41, 70, 16)))
    with pytest.raises(ValueError, match="cuda"):
        u.set_guides(torch.zeros((28, 47, 16)), torch.zeros((41, 70, 16)))


# ---- the restatement's own conditions, on oracle data ----------------------------------------------------------------
def _oracle_case(name):
    if name == "cornell8":
        pos, nrm, uv = scenes.cornell8()
        c, (w, h), (lw, lh) = scenes.cornell_camera(), (72, 40), (36, 20)
    else:
        pos, nrm, uv = scenes.lattice()
        c, (w, h), (lw, lh) = scenes.lattice_camera(), (64, 48), (32, 24)
    return (O.OracleScene(pos, nrm, uv), (lambda spp: va.make_camera(c["position"], c["rotation_deg"], w, h, spp)), (w, h),
            (lw, lh))


def _mse(a, conv):
    return float(np.mean((a[..., :3].astype(np.float64) - conv) ** 2))


@pytest.mark.parametrize("name", ["cornell8", "lattice"])
def test_spec_quality_on_oracle_frames(name):
    """(a) corrected sampling, early stop off, seeds 3-6, default spheres.  The low frame: 64 spp at half size, filtered
    with filter_spec under the low guide; both guides from the oracle's sample-0 camera rays; the reference the oracle's
    2048-spp frame at full size, seed 1.  Per seed mse(up) / mse(raw full-size 16 spp) <= 0.08 (a prototype measured
    0.021-0.032: the cap stops a broken spec passing and is no tuning target) and mse(up) < mse(the full-size 16-spp
    frame filtered with filter_spec) — the same ray count; over the mean of the four seeds mse(up) < mse(pixel
    replication); and at most 15 % of the full pixels take the fallback."""
    osc, cam_of, (w, h), (lw, lh) = _oracle_case(name)
    corrected = L.VMX_SAMPLING_CORRECTED
    conv, _ = osc.render(cam_of(2048), va.make_opts(seed=1, early_stop=False, sampling=corrected))
    conv = conv[..., :3].astype(np.float64)
    ups, reps = [], []
    for seed in (3, 4, 5, 6):
        opts = va.make_opts(seed=seed, early_stop=False, sampling=corrected)
        cam = cam_of(16)
        lcam = va.low_camera(cam_of(64), lw, lh)
        raw, _ = osc.render(cam, opts)
        low, _ = osc.render(lcam, opts)
        assert raw.shape == (h, w, 5) and low.shape == (lh, lw, 5)
        n_hi, z_hi = FS.guide_of(osc.raycast(*O.primary_rays(cam, opts, 0)).reshape(h, w))
        n_lo, z_lo = FS.guide_of(osc.raycast(*O.primary_rays(lcam, opts, 0)).reshape(lh, lw))
        low_f = FS.filtered_frame(low, n_lo, z_lo)
        up, fell, _ = US.upsample(low_f, n_lo, z_lo, n_hi, z_hi, details=True)
        full_f = FS.filtered_frame(raw, n_hi, z_hi)
        mse_raw, mse_full, mse_up = _mse(raw, conv), _mse(full_f, conv), _mse(up, conv)
        mse_rep = _mse(US.replicated(low_f, w, h), conv)
        print(f"{name} seed {seed}: mse raw {mse_raw:.6f}; of it: full-size filtered {mse_full / mse_raw:.4f}, upsampled "
              f"{mse_up / mse_raw:.4f}, replicated {mse_rep / mse_raw:.4f}; fallback {fell.mean():.4f}")
        assert mse_up / mse_raw <= 0.08, (name, seed, mse_up / mse_raw)
        assert mse_up < mse_full, (name, seed, mse_up, mse_full)
        assert fell.mean() <= 0.15, (name, seed, fell.mean())
        ups.append(mse_up), reps.append(mse_rep)
    print(f"{name}: mean over the seeds: upsampled {np.mean(ups):.6f} replicated {np.mean(reps):.6f}")
    assert np.mean(ups) < np.mean(reps), (name, np.mean(ups), np.mean(reps))
    osc.close()


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - np.broadcast_to(b, a.shape).copy().view(np.int32))


def test_spec_keeps_an_edge_between_perpendicular_normals():
    """(b) 12 x 8 from 6 x 4: the left half normal +z and colour A, the right half normal +x and colour B, one depth, the
    edge on a low-pixel boundary.  No tap across the edge has w > 0 (the dot product is 0), so every full pixel is
    within 1 ulp of its own side's colour; with the edge taken out of the full guide the pixels beside it move: the edge
    is kept by the guide, not the colours."""
    A, B = np.float32([0.7, 0.4, 0.2]), np.float32([0.1, 0.3, 0.9])
    lo = np.zeros((4, 6, 5), np.float32)
    lo[:, :3, :3], lo[:, 3:, :3] = A, B
    lo[..., 3] = 1
    n_lo, n_hi = np.zeros((4, 6, 3), np.float32), np.zeros((8, 12, 3), np.float32)
    n_lo[:, :3, 2] = 1
    n_lo[:, 3:, 0] = 1
    n_hi[:, :6, 2] = 1
    n_hi[:, 6:, 0] = 1
    z_lo, z_hi = np.full((4, 6), 10, np.float32), np.full((8, 12), 10, np.float32)
    out, fell, _ = US.upsample(lo, n_lo, z_lo, n_hi, z_hi, details=True)
    d = max(int(_ulps(out[:, :6, :3], A).max()), int(_ulps(out[:, 6:, :3], B).max()))
    print("largest distance of a pixel from its own side's colour:", d, "ulp;", int(fell.sum()), "fallback pixels")
    assert d <= 1 and not fell.any()
    # the full guide without the edge: one normal everywhere, the bisector of the two, which sees both low sides alike
    # (dot = sqrt(1/2) with each).  Column 5 lies half way between low columns 2 and 3 and now takes both.
    flat = np.zeros_like(n_hi)
    flat[..., 0] = flat[..., 2] = np.sqrt(np.float32(0.5))
    bled = US.upsample(lo, n_lo, z_lo, flat, z_hi)
    moved = np.abs(bled[:, 5, :3] - A).max(axis=-1)
    print("without the edge, column 5 moves by", float(moved.min()), "to", float(moved.max()))
    assert moved.min() > 1e-3
    assert np.abs(bled[:, :5, :3] - A).max() <= 1e-6 and np.abs(bled[:, 6:, :3] - B).max() <= 1e-6  # (only there)


ODD = np.array([0x7FC12345, 0x7F812345, 0xFFC00001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000],
               np.uint32).view(np.float32)  # NaN payloads (quiet, signalling, negative), -0, denormals, +-inf


def test_spec_takes_alpha_and_depth_from_the_anchor_bitwise():
    """(c) 7 x 5 from 2 x 2 with odd bit patterns in alpha and depth: each full pixel has its anchor's, bitwise — the
    inside tap of largest tent weight, the earlier one on a tie.  At ratio 1 (9 x 4) every pixel is its own anchor."""
    rng = np.random.RandomState(8)
    lo = rng.uniform(0, 1, (2, 2, 5)).astype(np.float32)
    lo[..., 3] = ODD[:4].reshape(2, 2)
    lo[..., 4] = ODD[4:].reshape(2, 2)
    n_lo, n_hi = np.zeros((2, 2, 3), np.float32), np.zeros((5, 7, 3), np.float32)
    n_lo[..., 1] = n_hi[..., 1] = 1
    z_lo, z_hi = np.full((2, 2), 3, np.float32), np.full((5, 7), 3, np.float32)
    out, _, (ay, ax) = US.upsample(lo, n_lo, z_lo, n_hi, z_hi, details=True)
    # the anchors, worked out in exact rational arithmetic: low coordinate x*2/7 and y*2/5, nearest tap, ties to the first
    want_x = [(x * 2) // 7 + (1 if ((x * 2) % 7) * 2 > 7 and (x * 2) // 7 + 1 < 2 else 0) for x in range(7)]
    want_y = [(y * 2) // 5 + (1 if ((y * 2) % 5) * 2 > 5 and (y * 2) // 5 + 1 < 2 else 0) for y in range(5)]
    assert [int(v) for v in ax[0]] == want_x and [int(v) for v in ay[:, 0]] == want_y
    assert len(set(want_x)) == 2 and len(set(want_y)) == 2
    assert np.array_equal(bits(out[..., 3:]), bits(lo[ay, ax][..., 3:]))
    assert np.isnan(out[..., 3:]).any() and np.isinf(out[..., 3:]).any()
    lo1 = rng.uniform(0, 1, (4, 9, 5)).astype(np.float32)
    lo1[..., 3].reshape(-1)[:8] = ODD
    lo1[..., 4].reshape(-1)[20:28] = ODD
    n1 = np.zeros((4, 9, 3), np.float32)
    n1[..., 0] = 1
    z1 = rng.uniform(1, 2, (4, 9)).astype(np.float32)
    out1, _, (ay, ax) = US.upsample(lo1, n1, z1, n1, z1, details=True)
    assert np.array_equal(ay, np.arange(4)[:, None].repeat(9, 1)) and np.array_equal(ax, np.arange(9)[None].repeat(4, 0))
    assert np.array_equal(bits(out1[..., 3:]), bits(lo1[..., 3:]))
    # ... and with one guide for both sizes the only tap of weight > 0 is the pixel itself: colours within 1 ulp
    assert _ulps(out1[..., :3], lo1[..., :3]).max() <= 1


def test_spec_fallback_is_the_anchor_colour():
    """(d) 12 x 8 from 6 x 4.  A full hit pixel whose four taps are all misses, a NaN full normal, and a z_p so small
    that isz overflows: each takes the anchor's colour, bitwise."""
    rng = np.random.RandomState(9)
    lo = rng.uniform(0, 1, (4, 6, 5)).astype(np.float32)
    lo[0, 0, 0] = ODD[0]  # a NaN colour leaves through the fallback with its payload
    n_lo, n_hi = np.zeros((4, 6, 3), np.float32), np.zeros((8, 12, 3), np.float32)
    n_lo[..., 2] = n_hi[..., 2] = 1
    z_lo, z_hi = np.full((4, 6), 5, np.float32), np.full((8, 12), 5, np.float32)
    z_lo[:2, :2] = -1  # full pixel (1, 1) lies between low pixels (0..1, 0..1), each with tent weight 1/4: all misses
    n_lo[:2, :2] = 0
    plain, fell0, _ = US.upsample(lo, n_lo, z_lo, n_hi, z_hi, details=True)
    n_hi[4, 7] = np.nan             # a NaN full normal: d is NaN, fails d > 0, and every weight is 0
    z_hi[6, 3] = np.float32(1e-40)  # isz = 1 / (0.1f * 1e-40f) overflows: t and g are infinite, every weight is 0
    with np.errstate(all="ignore"):
        assert np.isinf(np.float32(1) / (np.float32(0.1) * z_hi[6, 3]))
    out, fell, (ay, ax) = US.upsample(lo, n_lo, z_lo, n_hi, z_hi, details=True)
    # the anchors: (1, 1) ties four ways and keeps tap (0, 0); (4, 7) and (6, 3) lie between two low columns of one row
    # (fy = 0) and keep the first; row 4 of the low image does not exist
    for (y, x), (qy, qx) in (((1, 1), (0, 0)), ((4, 7), (2, 3)), ((6, 3), (3, 1))):
        assert fell[y, x], (y, x)
        assert (int(ay[y, x]), int(ax[y, x])) == (qy, qx), (y, x)
        assert np.array_equal(bits(out[y, x]), bits(lo[qy, qx])), (y, x)
    assert bits(out[1, 1])[0] == bits(ODD)[0]
    # without the two oddities the fallback pixels are the full hit pixels whose taps of weight > 0 are all misses: the
    # 3 x 3 corner (row and column 2 have fy = 0 and fx = 0, so only low row and column 1 weigh)
    want = np.zeros((8, 12), bool)
    want[:3, :3] = True
    assert np.array_equal(fell0, want)
    want[4, 7] = want[6, 3] = True
    assert np.array_equal(fell, want)
    # every other pixel is what it is without the oddities
    others = np.ones((8, 12), bool)
    others[4, 7] = others[6, 3] = False
    assert FS.same_bits(out[others], plain[others])
