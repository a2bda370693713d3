"""Albedo-demodulated denoising (vmx_albedo_camera_device, vmx_filter_apply_demodulated_device,
vmx_progressive_preview_demodulated*) without a GPU: the symbols, the argument checks that come before any device work,
the Python layer's checks of its tensors — and the conditions the restatement itself (tests/demod_spec.py, what the GPU
tests compare with) is held to on oracle data, so that the yardstick cannot drift.

Where demodulation pays: resolved textures on surfaces wider than the filter's footprint (the textured Cornell set
below).  Thin bars with a minified texture (the lattice) are the known limit: there it is no better than the plain
filter, and the cap on that case only lets a regression show.  (The overlap checks need a handle's image size, hence a
device: they are in tests/test_gpu_demod.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import demod_spec as DS
import filter_spec as FS
import oracle_lib as O
import temporal_spec as TS
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vermilion_hip.h")
ENTRIES = ("vmx_albedo_camera_device", "vmx_filter_apply_demodulated_device",
           "vmx_progressive_preview_demodulated_device", "vmx_progressive_preview_demodulated")


def _err(lib):
    return lib.vmx_last_error().decode()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_demod_symbols_are_declared_and_bound(hip_lib):
    src = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, src), name
    # additive: no new ABI version
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src) and hip_lib.vmx_abi_version() == 2
    m = re.search(r"#define VMX_ALBEDO_FLOOR ([0-9.e+-]+)f\b", src)
    assert m and float(m.group(1)) == 2.0 ** -10
    assert va.ALBEDO_FLOOR == 2.0 ** -10 == float(DS.ALBEDO_FLOOR) and "ALBEDO_FLOOR" in va.__all__
    assert hasattr(va.Scene, "albedo_camera")


def test_albedo_argument_checks_come_before_any_device_work(hip_lib):
    alb = hip_lib.vmx_albedo_camera_device
    buf = np.zeros(8 * 8 * 4 + 4, np.float32)
    ptr = (buf.ctypes.data + 15) & ~15
    cam = va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 18)  # kmax = 4 * (18 / 4) = 16
    opts = va.make_opts(seed=1)

    def refused(what, *args):
        assert alb(*args) == L.VMX_ERR_INVALID, what
        assert what in _err(hip_lib), (what, _err(hip_lib))

    refused("NULL scene", None, C.byref(cam), C.byref(opts), 0, 4, ptr, None)  # last: everything else was fine
    refused("NULL camera or opts", None, None, C.byref(opts), 0, 4, ptr, None)
    refused("NULL camera or opts", None, C.byref(cam), None, 0, 4, ptr, None)
    refused("NULL d_albedo", None, C.byref(cam), C.byref(opts), 0, 4, None, None)
    for off in (4, 8, 12, 1):
        refused("16-byte", None, C.byref(cam), C.byref(opts), 0, 4, ptr + off, None)
    # the camera and opts, as vmx_raycast_camera_device checks its own (make_frame)
    for bad_cam, what in ((va.make_camera((0, 0, 0), (0, 0, 0), 0, 8, 16), "resolution must be non-zero"),
                          (va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 3), "rays_per_pixel < 4"),
                          (va.make_camera((0, 0, 0), (0, 0, 0), 1 << 16, 1 << 16, 16), "image too large")):
        refused(what, None, C.byref(bad_cam), C.byref(opts), 0, 4, ptr, None)
        same = hip_lib.vmx_raycast_camera_device(None, C.byref(bad_cam), C.byref(opts), 0, ptr, 0, None)
        assert same == L.VMX_ERR_INVALID and what in _err(hip_lib)
    units = va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 16)
    units.rotation_units = 2
    refused("rotation_units", None, C.byref(units), C.byref(opts), 0, 4, ptr, None)
    refused("unknown sampling mode", None, C.byref(cam), C.byref(va.make_opts(sampling=7)), 0, 4, ptr, None)
    refused("world > 1", None, C.byref(cam), C.byref(va.make_opts(world=2, rank=1)), 0, 4, ptr, None)
    refused("nsamples must be at least 1", None, C.byref(cam), C.byref(opts), 0, 0, ptr, None)
    for first, n in ((0, 17), (16, 1), (13, 4), (0xFFFFFFFF, 1), (1, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF)):
        refused("sample range", None, C.byref(cam), C.byref(opts), first, n, ptr, None)
    # the ends of the range are inside it
    for first, n in ((0, 16), (15, 1), (12, 4), (0, 1)):
        refused("NULL scene", None, C.byref(cam), C.byref(opts), first, n, ptr, None)


def test_demodulated_apply_and_preview_argument_checks(hip_lib):
    app = hip_lib.vmx_filter_apply_demodulated_device
    buf = np.zeros(256, np.float32)
    ptr = (buf.ctypes.data + 15) & ~15
    assert app(None, ptr, ptr + 512, ptr, None, None, None) == L.VMX_ERR_INVALID and "NULL handle" in _err(hip_lib)
    # checks that come before the handle, in vmx_filter_apply_device's order, each seen alone
    bad = [dict(iterations=0), dict(iterations=11), dict(normal_squarings=9), dict(sigma_colour=0.0),
           dict(sigma_colour=float("nan")), dict(sigma_depth=float("inf")), dict(sigma_depth=-1.0)]
    previews = (hip_lib.vmx_progressive_preview_demodulated, hip_lib.vmx_progressive_preview_demodulated_device)
    for kw in bad:
        p = va.make_filter_params(**kw)
        assert app(None, ptr, ptr + 512, ptr, None, C.byref(p), None) == L.VMX_ERR_INVALID, kw
        assert "vmx_filter_params" in _err(hip_lib), (kw, _err(hip_lib))
        for fn in previews:
            assert fn(None, ptr, None, C.byref(p), 4) == L.VMX_ERR_INVALID, kw
            assert "vmx_filter_params" in _err(hip_lib), (kw, _err(hip_lib))
    p = va.make_filter_params()
    p.reserved[1] = 1
    assert app(None, ptr, ptr + 512, ptr, None, C.byref(p), None) == L.VMX_ERR_INVALID and "reserved" in _err(hip_lib)
    assert app(None, None, ptr + 512, ptr, None, None, None) == L.VMX_ERR_INVALID and "NULL d_in_rgbaz" in _err(hip_lib)
    assert app(None, ptr, None, ptr, None, None, None) == L.VMX_ERR_INVALID and "NULL d_albedo" in _err(hip_lib)
    assert app(None, ptr, ptr + 512, None, None, None, None) == L.VMX_ERR_INVALID and "no output" in _err(hip_lib)
    for args in ((ptr + 2, ptr + 512, ptr, None), (ptr, ptr + 512, ptr + 2, None), (ptr, ptr + 512, None, ptr + 1)):
        assert app(None, *args, None, None) == L.VMX_ERR_INVALID and "4-byte" in _err(hip_lib), args
    for off in (4, 8, 12):
        assert app(None, ptr, ptr + 512 + off, ptr, None, None, None) == L.VMX_ERR_INVALID
        assert "d_albedo must be 16-byte aligned" in _err(hip_lib)
    # the plain call is the call it was: no albedo, nothing asked of one
    assert hip_lib.vmx_filter_apply_device(None, ptr, ptr, None, None, None) == L.VMX_ERR_INVALID
    assert "NULL handle" in _err(hip_lib)
    for fn in previews:
        assert fn(None, None, None, None, 4) == L.VMX_ERR_INVALID and "no output" in _err(hip_lib)
        for samples in (0, 4, 1 << 30):  # (its range is the handle's kmax: seen with a handle, on the device)
            assert fn(None, ptr, None, None, samples) == L.VMX_ERR_INVALID and "NULL handle" in _err(hip_lib)
    assert previews[1](None, ptr + 2, None, None, 4) == L.VMX_ERR_INVALID and "NULL handle" in _err(hip_lib)


class NoLib:  # any call into the library fails the test
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_layer_rejects_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")

    class OnDevice:  # a tensor that passes every check but its address: the later arguments are reached
        def __init__(self, shape, dtype, ptr=0):
            self.shape, self.dtype, self.device, self.ptr = shape, dtype, torch.device("cuda", 0), ptr

        def data_ptr(self):
            return self.ptr

        def is_contiguous(self):
            return True

    OnDevice.__module__ = "torch"
    f = va.Filter.__new__(va.Filter)
    f._lib, f._h, f.device, f.shape = NoLib(), None, 0, (41, 70)
    ok_frame = OnDevice((41, 70, 5), torch.float32)
    plane = torch.zeros((41, 70, 4), dtype=torch.float32)  # a CPU tensor: not on the filter's device
    with pytest.raises(ValueError, match="albedo must be a torch tensor"):
        f.apply(ok_frame, albedo=np.zeros((41, 70, 4), np.float32))
    with pytest.raises(ValueError, match="albedo must be torch.float32"):
        f.apply(ok_frame, albedo=plane.double())
    with pytest.raises(ValueError, match=r"albedo must be \[41, 70, 4\]"):
        f.apply(ok_frame, albedo=torch.zeros((41, 70, 3)))
    with pytest.raises(ValueError, match="albedo must be contiguous"):
        f.apply(ok_frame, albedo=torch.zeros((70, 41, 4)).transpose(0, 1))
    with pytest.raises(ValueError, match="albedo must be on cuda"):
        f.apply(ok_frame, albedo=plane)
    with pytest.raises(ValueError, match="albedo must be 16-byte aligned"):
        f.apply(ok_frame, albedo=OnDevice((41, 70, 4), torch.float32, ptr=0x1008))
    with pytest.raises(ValueError, match="rgbaz must be on cuda"):  # the frame is still checked first
        f.apply(torch.zeros((41, 70, 5)), albedo=OnDevice((41, 70, 4), torch.float32))
    sc = va.Scene.__new__(va.Scene)
    sc._lib, sc._h, sc.device = NoLib(), None, 0
    cam, opts = va.make_camera((0, 0, 0), (0, 0, 0), 70, 41, 16), va.make_opts()
    with pytest.raises(ValueError, match="samples must be at least 1"):
        sc.albedo_camera(cam, opts, samples=0)
    with pytest.raises(ValueError, match="first must not be negative"):
        sc.albedo_camera(cam, opts, first=-1)
    with pytest.raises(ValueError, match="out must be a torch tensor"):
        sc.albedo_camera(cam, opts, out=np.zeros((41, 70, 4), np.float32))
    with pytest.raises(ValueError, match=r"out must be \[41, 70, 4\]"):
        sc.albedo_camera(cam, opts, out=torch.zeros((70, 41, 4)))
    with pytest.raises(ValueError, match="out must be on cuda"):
        sc.albedo_camera(cam, opts, out=plane)
    with pytest.raises(ValueError, match="out must be 16-byte aligned"):
        sc.albedo_camera(cam, opts, out=OnDevice((41, 70, 4), torch.float32, ptr=0x2004))
    p = va.Progressive.__new__(va.Progressive)
    p._scene, p._lib, p._h, p.device, p.shape, p._stream = sc, sc._lib, None, 0, (41, 70), None
    with pytest.raises(ValueError, match="albedo_samples must be at least 1"):
        p.preview_filtered(albedo_samples=0)
    with pytest.raises(ValueError, match="albedo_samples must be at least 1"):
        p.preview_filtered_device(rgbaz=ok_frame, albedo_samples=0)
    with pytest.raises(ValueError, match="rgbaz must be on cuda"):
        p.preview_filtered_device(rgbaz=torch.zeros((41, 70, 5)), albedo_samples=4)


# ---- the restatement's own conditions, on oracle data ----------------------------------------------------------------
def checker_texture():
    """32 x 32 x 3: 4-texel checks in red and green, 2-texel stripes in blue"""
    y, x = np.mgrid[0:32, 0:32]
    chk = ((x // 4 + y // 4) & 1).astype(np.float32)
    tex = np.stack([0.25 + 0.7 * chk, 0.9 - 0.6 * chk, 0.3 + 0.5 * ((x // 2) & 1)], axis=-1)
    return np.ascontiguousarray(tex, np.float32)


def _oracle_case(name, textured=True):
    if name == "cornell8":
        pos, nrm, uv = scenes.cornell8()
        c, (w, h) = scenes.cornell_camera(), (70, 41)
    else:
        pos, nrm, uv = scenes.lattice()
        c, (w, h) = scenes.lattice_camera(), (64, 48)
    tex = checker_texture() if textured else None
    osc = O.OracleScene(pos, nrm, uv)
    if textured:
        osc.bind_texture(tex)

    def cam_of(spp, i=0, motion=(0.0, 0.0)):
        p, r = c["position"], c["rotation_deg"]
        return va.make_camera((p[0] + motion[0] * i, p[1], p[2]), (r[0], r[1] + motion[1] * i, r[2]), w, h, spp)

    return osc, tex, cam_of, (w, h)


def _mse(a, conv):
    return float(np.mean((a[..., :3].astype(np.float64) - conv) ** 2))


CORRECTED = L.VMX_SAMPLING_CORRECTED


def _frame_guide(osc, cam, opts, w, h):
    raw, _ = osc.render(cam, opts)
    o, d = O.primary_rays(cam, opts, 0)
    rec = osc.raycast(o, d).reshape(h, w)
    return raw, rec


@pytest.fixture(scope="module")
def cornell_converged():
    """the textured Cornell set at 4096 spp, seed 1: computed once, never written to"""
    osc, _, cam_of, _ = _oracle_case("cornell8")
    conv, _ = osc.render(cam_of(4096), va.make_opts(seed=1, early_stop=False, sampling=CORRECTED))
    osc.close()
    conv = conv[..., :3].astype(np.float64)
    conv.setflags(write=False)
    return conv


def test_spec_quality_on_textured_cornell_frames(cornell_converged):
    """(a) cornell8 at 70x41 with the checker bound, 16-spp frames, corrected sampling, early stop off, seeds 3-6; guide
    and albedo from the frame's own seed.  Against the oracle's 4096-spp frame (seed 1):
    mse(demodulated, 16 albedo samples) <= 0.6 * mse(plain filter) (a prototype measured 0.36-0.44) and
    mse(demodulated, 4 albedo samples) <= 0.65 * mse(plain filter) (0.45-0.52).  Guards, not tuning targets."""
    osc, tex, cam_of, (w, h) = _oracle_case("cornell8")
    conv = cornell_converged
    for seed in (3, 4, 5, 6):
        opts = va.make_opts(seed=seed, early_stop=False, sampling=CORRECTED)
        cam = cam_of(16)
        raw, rec = _frame_guide(osc, cam, opts, w, h)
        n, z = FS.guide_of(rec)
        mse_raw, mse_plain = _mse(raw, conv), _mse(FS.filtered_frame(raw, n, z), conv)
        a16, a4 = DS.albedo_plane(osc, tex, cam, opts, 0, 16), DS.albedo_plane(osc, tex, cam, opts, 0, 4)
        d16, d4 = DS.demodulated_frame(raw, n, z, a16), DS.demodulated_frame(raw, n, z, a4)
        mse16, mse4 = _mse(d16, conv), _mse(d4, conv)
        print(f"cornell8 seed {seed}: of the raw error, plain {mse_plain / mse_raw:.4f} demodulated(16) "
              f"{mse16 / mse_raw:.4f} demodulated(4) {mse4 / mse_raw:.4f}; demodulated / plain: {mse16 / mse_plain:.4f} "
              f"(16), {mse4 / mse_plain:.4f} (4)")
        assert mse16 <= 0.6 * mse_plain, (seed, mse16 / mse_plain)
        assert mse4 <= 0.65 * mse_plain, (seed, mse4 / mse_plain)
        for out in (d16, d4):
            assert FS.same_bits(out[..., 3:], raw[..., 3:])
    osc.close()


def test_spec_quality_on_textured_lattice_frames():
    """(a) the lattice at 64x48 with the same texture, 16 albedo samples: thin bars with a minified texture, the known
    limit — a prototype measured 1.05-1.07 x the plain filter's error there (1.22 with 4 samples).  The cap,
    mse(demodulated) <= 1.15 * mse(plain), lets a regression show; resolved textures on surfaces wider than the
    filter's footprint are where demodulation pays."""
    osc, tex, cam_of, (w, h) = _oracle_case("lattice")
    conv, _ = osc.render(cam_of(4096), va.make_opts(seed=1, early_stop=False, sampling=CORRECTED))
    conv = conv[..., :3].astype(np.float64)
    for seed in (3, 4, 5, 6):
        opts = va.make_opts(seed=seed, early_stop=False, sampling=CORRECTED)
        cam = cam_of(16)
        raw, rec = _frame_guide(osc, cam, opts, w, h)
        n, z = FS.guide_of(rec)
        mse_plain = _mse(FS.filtered_frame(raw, n, z), conv)
        mse16 = _mse(DS.demodulated_frame(raw, n, z, DS.albedo_plane(osc, tex, cam, opts, 0, 16)), conv)
        print(f"lattice seed {seed}: demodulated(16) / plain {mse16 / mse_plain:.4f}")
        assert mse16 <= 1.15 * mse_plain, (seed, mse16 / mse_plain)
    osc.close()


def test_spec_on_accumulated_frames_prints_its_ratio():
    """(a) the composition with temporal accumulation, measured and printed, not asserted: 8 frames of 16 spp of the
    textured Cornell set under the "slow" camera motion of tests/test_temporal_abi.py (TS.step), the accumulated frame
    filtered both ways with the last camera's guide and 16-sample albedo, against 4096 spp at that camera."""
    osc, tex, cam_of, (w, h) = _oracle_case("cornell8")
    mv, frames, state = (6.0, 0.15), 8, None
    for i in range(frames):
        opts = va.make_opts(seed=3 + i, early_stop=False, sampling=CORRECTED)
        cam = cam_of(16, i, mv)
        raw, rec = _frame_guide(osc, cam, opts, w, h)
        acc, state, _ = TS.step(state, raw, rec, cam)
    conv, _ = osc.render(cam_of(4096, frames - 1, mv), va.make_opts(seed=1, early_stop=False, sampling=CORRECTED))
    conv = conv[..., :3].astype(np.float64)
    n, z = FS.guide_of(rec)
    albedo = DS.albedo_plane(osc, tex, cam, opts, 0, 16)
    mse_raw = _mse(raw, conv)
    mse_plain, mse_demod = _mse(FS.filtered_frame(acc, n, z), conv), _mse(DS.demodulated_frame(acc, n, z, albedo), conv)
    print(f"accumulated textured cornell8, slow: of the last raw frame's error, accumulated {_mse(acc, conv) / mse_raw:.4f} "
          f"plain filter {mse_plain / mse_raw:.4f} demodulated {mse_demod / mse_raw:.4f}; demodulated / plain "
          f"{mse_demod / mse_plain:.4f}")
    assert np.isfinite(mse_demod) and np.isfinite(mse_plain)
    osc.close()


def test_spec_untextured_scene_is_the_plain_filter():
    """(b) without a texture the plane is (1, 1, 1, m), m the share of the samples' rays with the material bit, and
    dividing and multiplying by 1 changes no bit: demodulated_frame is FS.filtered_frame"""
    osc, tex, cam_of, (w, h) = _oracle_case("cornell8", textured=False)
    opts = va.make_opts(seed=3, early_stop=False, sampling=CORRECTED)
    cam = cam_of(16)
    raw, rec = _frame_guide(osc, cam, opts, w, h)
    n, z = FS.guide_of(rec)
    plane = DS.albedo_plane(osc, None, cam, opts, 0, 4)
    assert np.array_equal(bits(plane[..., :3]), bits(np.ones((h, w, 3), np.float32)))
    m = np.zeros(w * h, np.float32)
    for k in range(4):
        m += (osc.raycast(*O.primary_rays(cam, opts, k))["flags"] & 2) != 0
    assert np.array_equal(plane[..., 3].ravel(), m / np.float32(4)) and 0 < plane[..., 3].mean() <= 1
    for prm in (None, FS.params_of(iterations=1), FS.params_of(iterations=3, normal_squarings=2)):
        assert np.array_equal(bits(DS.demodulated_frame(raw, n, z, plane, prm)), bits(FS.filtered_frame(raw, n, z, prm)))
    osc.close()


def exactly_demodulable(hh=9, ww=12):
    """a frame = constant irradiance x an exact checker albedo, on one normal at one depth"""
    y, x = np.mgrid[0:hh, 0:ww]
    chk = ((x + y) & 1).astype(bool)
    albedo = np.empty((hh, ww, 4), np.float32)
    albedo[..., 0] = np.where(chk, 0.25, 1.0)
    albedo[..., 1] = np.where(chk, 1.0, 0.5)
    albedo[..., 2] = 0.125
    albedo[..., 3] = 1.0
    frame = np.empty((hh, ww, 5), np.float32)
    frame[..., :3] = np.float32([0.75, 0.5, 0.375]) * albedo[..., :3]  # (powers of two: exact)
    frame[..., 3], frame[..., 4] = 1.0, 16.0
    n = np.zeros((hh, ww, 3), np.float32)
    n[..., 2] = 1
    z = np.full((hh, ww), 10, np.float32)
    return frame, albedo, n, z


@pytest.mark.parametrize("iterations", [1, 2, 5])
def test_spec_keeps_an_exactly_demodulable_frame(iterations):
    """(c) the demodulated result is within 2 ulp of the input (a prototype measured 0); the plain filter is off by more
    than 0.1 somewhere (0.27)"""
    frame, albedo, n, z = exactly_demodulable()
    prm = FS.params_of(iterations=iterations)
    out = DS.demodulated_frame(frame, n, z, albedo, prm)
    ulps = np.abs(out[..., :3].view(np.int32).astype(np.int64) - frame[..., :3].view(np.int32))
    plain = FS.filtered_frame(frame, n, z, prm)
    off = float(np.abs(plain[..., :3] - frame[..., :3]).max())
    print(f"iterations {iterations}: demodulated within {int(ulps.max())} ulp of the input; the plain filter off by {off:.4f}")
    assert ulps.max() <= 2
    assert off > 0.1


def test_spec_degenerate_albedo_takes_the_floor():
    """(d) 0, -1, NaN, +inf and 1e-9 all take the floor; -inf, -0, a denormal and the floor itself too; the output is
    finite for a finite frame"""
    rng = np.random.RandomState(11)
    hh, ww = 7, 11
    frame = rng.uniform(0, 1, (hh, ww, 5)).astype(np.float32)
    albedo = rng.uniform(0.2, 1, (hh, ww, 4)).astype(np.float32)
    odd = np.float32([0.0, -1.0, np.nan, np.inf, 1e-9, -np.inf, -0.0, 1e-42, 2.0 ** -10])
    albedo[1, :9, 0], albedo[3, :9, 1], albedo[5, :9, 2] = odd, odd, odd
    albedo[6, 4, :3] = np.nan
    am = DS.clamped_albedo(albedo)
    for row, ch in ((1, 0), (3, 1), (5, 2)):
        assert np.array_equal(bits(am[row, :9, ch]), bits(np.full(9, DS.ALBEDO_FLOOR, np.float32)))
    assert np.array_equal(bits(am[6, 4]), bits(np.full(3, DS.ALBEDO_FLOOR, np.float32)))
    keep = np.ones((hh, ww, 3), bool)
    keep[1, :9, 0] = keep[3, :9, 1] = keep[5, :9, 2] = False
    keep[6, 4] = False
    assert np.array_equal(bits(am[keep]), bits(albedo[..., :3][keep]))
    above = np.nextafter(DS.ALBEDO_FLOOR, np.float32(1))
    assert DS.clamped_albedo(np.full((1, 1, 4), above, np.float32))[0, 0, 0] == above  # the first value that is kept
    assert DS.clamped_albedo(np.full((1, 1, 4), DS.FLT_MAX, np.float32))[0, 0, 0] == DS.FLT_MAX
    n = np.zeros((hh, ww, 3), np.float32)
    n[..., 1] = 1
    z = rng.uniform(1, 2, (hh, ww)).astype(np.float32)
    for prm in (None, FS.params_of(iterations=1)):
        out = DS.demodulated_frame(frame, n, z, albedo, prm)
        assert np.isfinite(out).all()


def test_spec_passes_alpha_and_depth_through_bitwise():
    """(e) channels 3 and 4 leave exactly as they came, whatever they hold"""
    rng = np.random.RandomState(6)
    frame = rng.uniform(0, 1, (7, 11, 5)).astype(np.float32)
    odd = np.array([0x7FC12345, 0xFF800000, 0x80000000, 0x00000001, 0x7F7FFFFF], np.uint32).view(np.float32)
    frame[0, :5, 3] = odd
    frame[1, :5, 4] = odd
    albedo = rng.uniform(0.1, 1, (7, 11, 4)).astype(np.float32)
    n = np.zeros((7, 11, 3), np.float32)
    n[..., 1] = 1
    z = rng.uniform(1, 2, (7, 11)).astype(np.float32)
    z[3, 4:8] = -1
    out = DS.demodulated_frame(frame, n, z, albedo)
    assert np.array_equal(bits(out[..., 3:]), bits(frame[..., 3:]))
    assert not np.array_equal(out[..., :3], frame[..., :3])
    assert not np.array_equal(out[..., :3], FS.filtered_frame(frame, n, z)[..., :3])
