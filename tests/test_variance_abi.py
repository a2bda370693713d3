"""Variance-guided denoising (vmx_temporal_create_ex, vmx_temporal_accumulate_variance_device, vmx_variance_default_params,
vmx_filter_apply_variance_device) without a GPU: the symbols, the struct layout against the header, the defaults, the
argument checks that come before any device work, the Python layer's checks of its tensors — and the conditions the
restatement itself (tests/variance_spec.py, what the GPU tests compare with) is held to.  (The overlap checks and the
refusals by kind of handle need a handle, hence a device: tests/test_gpu_variance.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import demod_spec as DS
import filter_spec as FS
import oracle_lib as O
import test_demod_abi as TD
import test_temporal_abi as TT
import variance_spec as VS
import vermilion_amd as va
from vermilion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vermilion_hip.h")
ENTRIES = ("vmx_variance_default_params", "vmx_temporal_create_ex", "vmx_temporal_accumulate_variance_device",
           "vmx_filter_apply_variance_device")
F = np.float32
CORRECTED = L.VMX_SAMPLING_CORRECTED


def _err(lib):
    return lib.vmx_last_error().decode()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_variance_symbols_are_declared_and_bound(hip_lib):
    src = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, src), name
    # additive: no new ABI version
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src) and hip_lib.vmx_abi_version() == 2
    for name in ("make_variance_params", "VARIANCE_EPS", "SIGMA_LUMINANCE_DEFAULT"):
        assert name in va.__all__ and hasattr(va, name)
    # the constants are the header's, and the restatement's
    assert re.search(r"#define VMX_TEMPORAL_MOMENTS 1u\b", src) and L.VMX_TEMPORAL_MOMENTS == 1
    assert re.search(r"#define VMX_VARIANCE_EPS 1e-10f\b", src) and F(va.VARIANCE_EPS) == F(1e-10) == VS.EPS
    assert re.search(r"#define VMX_SIGMA_LUMINANCE_DEFAULT 4\.f\b", src)
    assert va.SIGMA_LUMINANCE_DEFAULT == 4.0 == VS.SIGMA_LUMINANCE


def test_variance_params_layout_matches_header(tmp_path):
    fields = [n for n, _ in L.VarianceParams._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vermilion_hip.h"\nint main(void){\n'
    prog += 'printf("size %zu\\n", sizeof(vmx_variance_params));\n'
    for n in fields:
        prog += f'printf("{n} %zu\\n", offsetof(vmx_variance_params, {n}));\n'
    prog += "return 0;}\n"
    src = tmp_path / "sz.c"
    src.write_text(prog)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(L.VarianceParams) == 32
    for n in fields:
        assert int(out[n]) == getattr(L.VarianceParams, n).offset, n
    assert [int(out[n]) for n in fields] == [0, 4, 8, 12]


def test_default_params(hip_lib):
    p = L.VarianceParams(9.0, 9, 9.0, (C.c_uint32 * 5)(1, 2, 3, 4, 5))
    assert hip_lib.vmx_variance_default_params(C.byref(p)) == L.VMX_OK
    assert (F(p.min_history), p.normal_squarings, F(p.sigma_depth)) == (F(4.0), 5, F(0.1))
    assert list(p.reserved) == [0, 0, 0, 0, 0]
    assert hip_lib.vmx_variance_default_params(None) == L.VMX_ERR_INVALID
    q = va.make_variance_params(min_history=2, sigma_depth=0.5)
    assert (q.min_history, q.normal_squarings, q.sigma_depth) == (2.0, 5, 0.5)
    # the restatement's defaults are the library's
    lib_defaults, spec_defaults = VS.params_of(va.make_variance_params()), VS.params_of()
    assert all(F(lib_defaults[k]) == F(spec_defaults[k]) for k in spec_defaults)


def test_create_ex_checks_do_not_need_a_gpu(hip_lib):
    h = C.c_void_p()
    create = hip_lib.vmx_temporal_create_ex
    # unknown flag bits, each alone and beside the known one
    for flags in (2, 4, 1 << 31, 3, 0xFFFFFFFF):
        assert create(0, 8, 8, flags, C.byref(h)) == L.VMX_ERR_INVALID, flags
        assert "unknown flags" in _err(hip_lib) and not h.value
    # every other refusal is vmx_temporal_create's, with either kind of handle
    for flags in (0, L.VMX_TEMPORAL_MOMENTS):
        for w, hh in ((0, 8), (8, 0)):
            assert create(0, w, hh, flags, C.byref(h)) == L.VMX_ERR_INVALID
            assert "resolution must be non-zero" in _err(hip_lib) and not h.value
        assert create(0, 1 << 16, 1 << 16, flags, C.byref(h)) == L.VMX_ERR_INVALID and "image too large" in _err(hip_lib)
        assert create(0, 8, 8, flags, None) == L.VMX_ERR_INVALID
        assert create(1 << 20, 8, 8, flags, C.byref(h)) == L.VMX_ERR_NO_DEVICE and not h.value
        if hip_lib.vmx_device_count() == 0:
            assert create(0, 8, 8, flags, C.byref(h)) == L.VMX_ERR_NO_DEVICE and "no CPU path" in _err(hip_lib)
    if hip_lib.vmx_device_count() == 0:
        with pytest.raises(va.VmxError) as e:
            va.Temporal(8, 8, moments=True)
        assert e.value.code == L.VMX_ERR_NO_DEVICE


def test_accumulate_variance_checks_do_not_need_a_gpu(hip_lib):
    """the motion call's checks in its order — the variance parameters right after the temporal ones, d_variance after
    d_in_rgbaz and its alignment after the other buffers' — each seen alone, the handle last"""
    acc = hip_lib.vmx_temporal_accumulate_variance_device
    buf = np.zeros(8 * 8 * 16 + 4, np.float32)
    ptr = (buf.ctypes.data + 15) & ~15
    cam = va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 16)

    def refused(args, what):
        assert acc(*args) == L.VMX_ERR_INVALID, what
        assert what in _err(hip_lib), (what, _err(hip_lib))

    cb = C.byref(cam)
    for mv in (None, ptr):
        refused((None, cb, ptr, mv, ptr, ptr, None, None, ptr, None, None, None), "NULL handle")
        # the variance counts as an output: no other one is needed
        refused((None, cb, ptr, mv, ptr, None, None, None, ptr, None, None, None), "NULL handle")
        refused((None, cb, ptr, mv, ptr, ptr, None, None, None, None, None, None), "NULL d_variance")
        refused((None, None, ptr, mv, ptr, ptr, None, None, ptr, None, None, None), "NULL camera")
        refused((None, cb, None, mv, ptr, ptr, None, None, ptr, None, None, None), "NULL d_rayhit")
        refused((None, cb, ptr, mv, None, ptr, None, None, ptr, None, None, None), "NULL d_in_rgbaz")
        refused((None, cb, ptr + 4, mv, ptr, ptr, None, None, ptr, None, None, None), "d_rayhit must be 16-byte")
        refused((None, cb, ptr, mv, ptr + 2, ptr, None, None, ptr, None, None, None), "4-byte")
        for off in (1, 2, 3):
            refused((None, cb, ptr, mv, ptr, ptr, None, None, ptr + off, None, None, None), "d_variance must be 4-byte aligned")
        bad_cam = va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 3)
        refused((None, C.byref(bad_cam), ptr, mv, ptr, ptr, None, None, ptr, None, None, None), "rays_per_pixel < 4")
    refused((None, cb, ptr, ptr + 8, ptr, ptr, None, None, ptr, None, None, None), "d_motion must be 16-byte aligned")
    # the temporal parameters first, then the variance parameters, both before every pointer
    tp = va.make_temporal_params(plane_tol=0.0)
    vp = va.make_variance_params(min_history=0.5)
    refused((None, None, None, None, None, None, None, None, None, C.byref(tp), C.byref(vp), None), "vmx_temporal_params")
    refused((None, None, None, None, None, None, None, None, None, None, C.byref(vp), None), "vmx_variance_params")
    bad = [dict(min_history=float("nan")), dict(min_history=float("inf")), dict(min_history=0.5), dict(min_history=-4.0),
           dict(normal_squarings=9), dict(normal_squarings=1 << 31),
           dict(sigma_depth=float("nan")), dict(sigma_depth=float("inf")), dict(sigma_depth=0.0), dict(sigma_depth=-0.1)]
    for kw in bad:
        p = va.make_variance_params(**kw)
        refused((None, cb, ptr, None, ptr, ptr, None, None, ptr, None, C.byref(p), None), "vmx_variance_params")
        assert list(kw)[0] in _err(hip_lib), (kw, _err(hip_lib))
    for i in range(5):
        p = va.make_variance_params()
        p.reserved[i] = 1
        refused((None, cb, ptr, None, ptr, ptr, None, None, ptr, None, C.byref(p), None), "reserved")
        assert "vmx_variance_params" in _err(hip_lib)
    # the ends of the ranges are inside them
    for kw in (dict(min_history=1.0), dict(normal_squarings=0), dict(normal_squarings=8)):
        p = va.make_variance_params(**kw)
        refused((None, cb, ptr, None, ptr, ptr, None, None, ptr, None, C.byref(p), None), "NULL handle")


def test_apply_variance_checks_do_not_need_a_gpu(hip_lib):
    """the demodulated call's checks in its order, sigma_luminance right after the parameters, d_variance after d_in_rgbaz
    and its alignment before the albedo's, each seen alone, the handle last"""
    app = hip_lib.vmx_filter_apply_variance_device
    buf = np.zeros(64, np.float32)
    ptr = (buf.ctypes.data + 15) & ~15

    def refused(args, what):
        assert app(*args) == L.VMX_ERR_INVALID, what
        assert what in _err(hip_lib), (what, _err(hip_lib))

    for alb in (None, ptr):
        refused((None, ptr, ptr, alb, ptr, None, None, 4.0, None), "NULL handle")
        refused((None, ptr, ptr, alb, None, ptr, None, 4.0, None), "NULL handle")
        for sl in (float("nan"), float("inf"), float("-inf"), 0.0, -0.0, -4.0):
            refused((None, ptr, ptr, alb, ptr, None, None, sl, None), "sigma_luminance must be finite and > 0")
        refused((None, None, ptr, alb, ptr, None, None, 4.0, None), "NULL d_in_rgbaz")
        refused((None, ptr, None, alb, ptr, None, None, 4.0, None), "NULL d_variance")
        refused((None, ptr, ptr, alb, None, None, None, 4.0, None), "no output")
        refused((None, ptr + 2, ptr, alb, ptr, None, None, 4.0, None), "must be 4-byte aligned")
        for off in (1, 2, 3):
            refused((None, ptr, ptr + off, alb, ptr, None, None, 4.0, None), "d_variance must be 4-byte aligned")
    for off in (4, 8, 12):
        refused((None, ptr, ptr, ptr + off, ptr, None, None, 4.0, None), "d_albedo must be 16-byte aligned")
    # the parameters come first, sigma_colour among them although the call does not use it
    for kw in (dict(iterations=0), dict(iterations=11), dict(normal_squarings=9), dict(sigma_colour=0.0),
               dict(sigma_colour=float("nan")), dict(sigma_depth=-1.0)):
        p = va.make_filter_params(**kw)
        refused((None, None, None, None, None, None, C.byref(p), float("nan"), None), "vmx_filter_params")
        assert list(kw)[0] in _err(hip_lib)
    p = va.make_filter_params()
    p.reserved[2] = 1
    refused((None, ptr, ptr, None, ptr, None, C.byref(p), 4.0, None), "reserved")
    # a tiny and a huge sigma_luminance are inside the range
    for sl in (1e-30, 3e38):
        refused((None, ptr, ptr, None, ptr, None, None, sl, None), "NULL handle")


def test_stand_alone_argument_checks_build_and_pass(tmp_path):
    """tests/cpp/variance_args.cpp, the program to run under the host sanitizers (against a library built with them), built
    plainly: the same checks through the C header, from C++"""
    exe = tmp_path / "variance_args"
    so_dir = os.path.join(ROOT, "vermilion_amd")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "variance_args.cpp"), os.path.join(so_dir, "libvermilion_hip.so"),
                    "-Wl,-rpath," + so_dir, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "clean" in run.stdout, run.stderr


class NoLib:  # any call into the library fails the test
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_layer_rejects_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")

    class OnDevice:  # a tensor that passes every check: the later arguments are reached
        def __init__(self, shape, dtype):
            self.shape, self.dtype, self.device = shape, dtype, torch.device("cuda", 0)

        def data_ptr(self):
            return 0

        def is_contiguous(self):
            return True

    OnDevice.__module__ = "torch"
    cam = va.make_camera((0, 0, 0), (0, 0, 0), 70, 41, 16)
    ok_raw, ok_frame = OnDevice((41, 70, 16), torch.float32), OnDevice((41, 70, 5), torch.float32)
    ok_var = OnDevice((41, 70), torch.float32)
    # Temporal.accumulate(variance=...): required on a moments handle, refused on any other, before anything else
    t = va.Temporal.__new__(va.Temporal)
    t._lib, t._h, t.device, t.shape, t.moments = NoLib(), None, 0, (41, 70), True
    with pytest.raises(ValueError, match="variance is required"):
        t.accumulate(cam, ok_raw, ok_frame)
    with pytest.raises(ValueError, match="variance must be a torch tensor"):
        t.accumulate(cam, ok_raw, ok_frame, variance=np.zeros((41, 70), np.float32))
    with pytest.raises(ValueError, match="variance must be torch.float32"):
        t.accumulate(cam, ok_raw, ok_frame, variance=torch.zeros((41, 70), dtype=torch.float64))
    with pytest.raises(ValueError, match=r"variance must be \[41, 70\]"):
        t.accumulate(cam, ok_raw, ok_frame, variance=torch.zeros((41, 70, 1)))
    with pytest.raises(ValueError, match="variance must be contiguous"):
        t.accumulate(cam, ok_raw, ok_frame, variance=torch.zeros((70, 41)).transpose(0, 1))
    with pytest.raises(ValueError, match="variance must be on cuda"):
        t.accumulate(cam, ok_raw, ok_frame, variance=torch.zeros((41, 70)))
    with pytest.raises(ValueError, match="raw must be on cuda"):  # (the other tensors are checked as ever)
        t.accumulate(cam, torch.zeros((41, 70, 16)), ok_frame, variance=ok_var)
    plain = va.Temporal.__new__(va.Temporal)
    plain._lib, plain._h, plain.device, plain.shape, plain.moments = NoLib(), None, 0, (41, 70), False
    with pytest.raises(ValueError, match="moments=True"):
        plain.accumulate(cam, ok_raw, ok_frame, variance=ok_var)
    with pytest.raises(ValueError, match="moments=True"):
        plain.accumulate(cam, ok_raw, ok_frame, variance_params=L.VarianceParams())
    # Filter.apply(variance=..., sigma_luminance=...)
    f = va.Filter.__new__(va.Filter)
    f._lib, f._h, f.device, f.shape = NoLib(), None, 0, (41, 70)
    with pytest.raises(ValueError, match="variance must be a torch tensor"):
        f.apply(ok_frame, variance=np.zeros((41, 70), np.float32))
    with pytest.raises(ValueError, match="variance must be torch.float32"):
        f.apply(ok_frame, variance=torch.zeros((41, 70), dtype=torch.float16))
    with pytest.raises(ValueError, match=r"variance must be \[41, 70\]"):
        f.apply(ok_frame, variance=torch.zeros((70, 41)))
    with pytest.raises(ValueError, match="variance must be contiguous"):
        f.apply(ok_frame, variance=torch.zeros((70, 41)).transpose(0, 1))
    with pytest.raises(ValueError, match="variance must be on cuda"):
        f.apply(ok_frame, variance=torch.zeros((41, 70)))
    for sl in (float("nan"), float("inf"), 0.0, -1.0):
        with pytest.raises(ValueError, match="sigma_luminance must be finite and > 0"):
            f.apply(ok_frame, variance=ok_var, sigma_luminance=sl)
    with pytest.raises(ValueError, match="albedo must be on cuda"):  # (it composes with the albedo, checked as ever)
        f.apply(ok_frame, variance=ok_var, albedo=torch.zeros((41, 70, 4)))


# ---- the restatement's own conditions ----------------------------------------------------------------------------------
def test_spec_static_camera_moments_are_running_means():
    """(a) a camera that does not move and one guide for every frame, 5 random frames: every hit pixel's m1 and m2 are the
    running means of l and l*l — within 4 ulp of the float64 means, as the colour is in tests/test_temporal_abi.py — and
    with min_history = 1 no pixel takes the window: the variance is vt, and differs from the float64 population variance
    of the five float32 luminances by at most 16 * 2^-24 * m2' (each mean carries under 2 ulp, squaring doubles that, the
    difference is taken once).  On the first frame vt is exactly 0 everywhere."""
    osc, cam_of, (w, h) = TT._oracle_case("cornell8")
    cam = cam_of(16)
    opts = va.make_opts(seed=3, early_stop=False)
    o, d = O.primary_rays(cam, opts, 0)
    rec = np.array(osc.raycast(o, d).reshape(h, w))
    osc.close()
    rec["flags"][5, 10:20] &= ~np.uint32(1)  # (a few misses, which the set's own camera does not see)
    rec["distance"][5, 10:20] = np.inf
    hit = (rec["flags"] & 1) != 0
    assert hit.any() and not hit.all()
    rng = np.random.RandomState(23)
    frames = [rng.uniform(0, 1, (h, w, 5)).astype(np.float32) for _ in range(5)]
    state, lums = None, []
    for k, f in enumerate(frames, 1):
        _, state, hist = VS.step(state, f, rec, cam)
        lums.append(VS.lum(f))
        var = VS.variance(state, dict(min_history=1.0))
        m1, m2 = state["m"][..., 0], state["m"][..., 1]
        vt = m2 - m1 * m1
        vt = np.where(vt > 0, vt, F(0))
        assert FS.same_bits(var, vt), k  # (no pixel takes the window)
        if k == 1:
            assert np.all(var == 0) and FS.same_bits(m1, lums[0]) and FS.same_bits(m2, lums[0] * lums[0])
        # a miss restarts every frame
        assert FS.same_bits(m1[~hit], lums[-1][~hit]) and np.all(var[~hit] == 0)
    l64 = np.stack(lums).astype(np.float64)
    mean1, mean2 = l64.mean(axis=0).astype(np.float32), (l64 * l64).mean(axis=0).astype(np.float32)
    ulps = lambda a, b: np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32))[hit]  # noqa: E731
    print("largest distance from the float64 means after 5 frames:", int(ulps(m1, mean1).max()), "and",
          int(ulps(m2, mean2).max()), "ulp")
    assert ulps(m1, mean1).max() <= 4 and ulps(m2, mean2).max() <= 4
    err = np.abs(var.astype(np.float64) - l64.var(axis=0))[hit]
    bound = 16 * 2.0 ** -24 * m2.astype(np.float64)[hit]
    print("variance against the float64 population variance: largest error / bound", float((err / bound).max()))
    assert np.all(err <= bound)
    # with the default min_history (4) the second frame's pixels do take the window, the fifth frame's hits do not
    _, s2, _ = VS.step(None, frames[0], rec, cam)
    _, s2, _ = VS.step(s2, frames[1], rec, cam)
    assert not FS.same_bits(VS.variance(s2), VS.variance(s2, dict(min_history=1.0)))
    assert FS.same_bits(VS.variance(state)[hit], var[hit])


@pytest.mark.parametrize("iterations", [1, 5])
def test_spec_infinite_variance_is_the_plain_filter(iterations):
    """(b) with d_variance = +inf everywhere (dl*dl)/den is 0, as e*isc2 vanishes beside 1.f for colours in [0, 1] with
    sigma_colour = 1e19: the variance call's colours are filter_spec.atrous bit for bit — its geometry weights, tap order
    and fallback are the yardstick's.  A cornell8 oracle frame, 70 x 41."""
    osc, cam_of, (w, h) = TT._oracle_case("cornell8")
    cam, opts = cam_of(16), va.make_opts(seed=3, early_stop=False, sampling=CORRECTED)
    raw, _ = osc.render(cam, opts)
    o, d = O.primary_rays(cam, opts, 0)
    n, z = FS.guide_of(osc.raycast(o, d).reshape(h, w))
    osc.close()
    assert raw[..., :3].min() >= 0 and raw[..., :3].max() <= 1
    got = VS.atrous(raw[..., :3], np.full((h, w), np.inf, np.float32), n, z, FS.params_of(iterations=iterations))
    want = FS.atrous(raw[..., :3], n, z, FS.params_of(iterations=iterations, sigma_colour=1e19))
    assert not np.isnan(got).any() and FS.same_bits(got, want)
    assert not FS.same_bits(got, FS.atrous(raw[..., :3], n, z, FS.params_of(iterations=iterations)))


def plane_records(w, h):
    """w x h records of a camera at the origin looking down -z at the plane z = -4, one world unit per pixel: one normal,
    one distance for every pixel"""
    cam = va.make_camera((0, 0, 0), (0, 0, 0), w, h, 16, back_distance=1.0, back_size=(w / 4.0, h / 4.0))
    rec = np.zeros((h, w, 16), np.float32)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rec[..., 0] = xs + 0.5 - w / 2
    rec[..., 1] = -(ys + 0.5 - h / 2)
    rec[..., 2] = -4.0
    rec[..., 3] = 4.0
    rec[..., 6] = 1.0
    rec.view(np.uint32)[..., 11] = 3
    return cam, rec


def adaptivity_frames():
    """(c)'s eight 64 x 24 frames: columns 0..31 are 0.5 plus independent uniform noise of +-0.35 per frame, columns
    32..63 a noise-free 2-pixel checker of 0.4 / 0.6, identical every frame; grey, alpha 1"""
    rng = np.random.RandomState(5)
    ys, xs = np.meshgrid(np.arange(24), np.arange(64), indexing="ij")
    checker = np.where(((xs // 2 + ys // 2) & 1) == 1, F(0.6), F(0.4)).astype(np.float32)
    frames = []
    for _ in range(8):
        v = np.array(checker)
        v[:, :32] = (0.5 + rng.uniform(-0.35, 0.35, (24, 32))).astype(np.float32)
        f = np.ones((24, 64, 5), np.float32)
        f[..., :3] = v[..., None]
        frames.append(f)
    return frames


def test_spec_adapts_to_the_variance():
    """(c) one plane, 8 static frames, half noise around 0.5 and half a noise-free checker of 0.4 / 0.6.  On the checker
    var == 0 exactly, and away from the noisy half (the 16 columns next to it left out) the variance call changes no
    pixel by more than 1e-6 — a tap of the other shade has (dl*dl)/den = 0.04/1e-10, its weight is below 3e-9 of its kernel
    weight — while the plain call at its defaults changes those pixels by more than 0.01 in the mean.  On the noisy half
    (the same margin left out) the variance call leaves at most 0.25 of the accumulated frame's squared error against
    0.5: with den ~ 16 var and dl^2 << den the weights are near the kernel's, whose first iteration alone leaves
    (sum h^2)^2 = 0.075."""
    cam, rec = plane_records(64, 24)
    state = None
    for f in adaptivity_frames():
        acc, state, hist = VS.step(state, f, rec, cam)
    assert np.all(hist == 8)
    var = VS.variance(state)
    assert np.all(var[:, 32:] == 0) and np.all(var[:, :32] > 0)
    n, z = FS.guide_of(rec)
    guided, plain = VS.filtered_frame(acc, var, n, z), FS.filtered_frame(acc, n, z)
    far = slice(48, 64)
    moved_guided = np.abs(guided[:, far, :3] - acc[:, far, :3])
    moved_plain = np.abs(plain[:, far, :3] - acc[:, far, :3])
    print("checker, away from the noise: the variance call moves a pixel by at most", float(moved_guided.max()),
          "the plain call by", float(moved_plain.mean()), "in the mean")
    assert moved_guided.max() <= 1e-6
    assert moved_plain.mean() > 0.01
    noisy = slice(0, 16)
    se = lambda a: float(np.sum((a[:, noisy, :3].astype(np.float64) - 0.5) ** 2))  # noqa: E731
    print("noise: the variance call leaves", se(guided) / se(acc), "of the accumulated frame's squared error, the plain call",
          se(plain) / se(acc))
    assert se(guided) <= 0.25 * se(acc)
    assert FS.same_bits(guided[..., 3:], acc[..., 3:])


# (d) prototype figures, as shares of the raw last frame's error against the 2048-spp frame: (variance-guided, plain)
QUALITY = {("cornell8", "static"): (0.0431, 0.0435), ("cornell8", "slow"): (0.0439, 0.0447),
           ("cornell8", "fast"): (0.0492, 0.0502), ("lattice", "static"): (0.0484, 0.0524),
           ("lattice", "slow"): (0.0436, 0.0459), ("lattice", "fast"): (0.0426, 0.0473)}


@pytest.mark.parametrize("motion", list(TT.MOTIONS))
@pytest.mark.parametrize("name", ["cornell8", "lattice"])
def test_spec_quality_on_oracle_frames(name, motion):
    """(d) the six cases of test_temporal_abi.test_spec_quality_cap_on_oracle_frames unchanged: 8 frames of 16 spp,
    accumulated with moments, the variance at the defaults, the accumulated frame filtered with sigma_luminance = 4 and,
    beside it, by the plain filter.  As shares of the raw last frame's error against the 2048-spp frame a prototype of this
    arithmetic measured (variance-guided, plain filter):
        cornell8 static 0.0431 0.0435    cornell8 slow 0.0439 0.0447    cornell8 fast 0.0492 0.0502
        lattice  static 0.0484 0.0524    lattice  slow 0.0436 0.0459    lattice  fast 0.0426 0.0473
    The oracle and the restatement are deterministic; the cap is the prototype's own figure x 1.25, so that it is no
    tuning target.  Variance guidance beats the plain filter in all six, by 1-2 % on the Cornell set and 5-10 % on the
    lattice: these frames hold little shading detail without a G-buffer edge behind it."""
    osc, cam_of, (w, h) = TT._oracle_case(name)
    mv, frames, state = TT.MOTIONS[motion], 8, None
    for i in range(frames):
        opts = va.make_opts(seed=3 + i, early_stop=False, sampling=CORRECTED)
        cam = cam_of(16, i, mv)
        raw, _ = osc.render(cam, opts)
        o, d = O.primary_rays(cam, opts, 0)
        rec = osc.raycast(o, d).reshape(h, w)
        acc, state, hist = VS.step(state, raw, rec, cam)
    conv, _ = osc.render(cam_of(2048, frames - 1, mv), va.make_opts(seed=1, early_stop=False, sampling=CORRECTED))
    osc.close()
    conv = conv[..., :3].astype(np.float64)
    n, z = FS.guide_of(rec)
    var = VS.variance(state)
    mse_raw = TT._mse(raw, conv)
    guided, plain = TT._mse(VS.filtered_frame(acc, var, n, z), conv), TT._mse(FS.filtered_frame(acc, n, z), conv)
    print(f"{name} {motion}: of the raw error, variance-guided {guided / mse_raw:.4f} plain {plain / mse_raw:.4f} "
          f"(accumulated {TT._mse(acc, conv) / mse_raw:.4f}); share of pixels in the window {np.mean(hist < 4):.3f}")
    assert guided / mse_raw <= 1.25 * QUALITY[name, motion][0], (name, motion, guided / mse_raw)
    assert np.isfinite(plain)


TEXTURED = (0.0160, 0.0167)  # the prototype's figures: (variance-guided with albedo, demodulated plain call)


def test_spec_quality_on_textured_frames_with_albedo():
    """(d) one more: the Cornell set with the checker texture bound (tests/test_demod_abi.py), "slow" camera motion, 8
    frames of 16 spp accumulated with moments, albedo from 16 samples at the last camera; the variance-guided call with
    d_albedo against the demodulated plain call, as shares of the raw last frame's error against the 2048-spp frame.
    A prototype measured 0.0160 against 0.0167 (and, without the albedo, 0.0577 against the plain filter's 0.0614); the
    cap is the variance-guided figure x 1.25."""
    osc, tex, cam_of, (w, h) = TD._oracle_case("cornell8")
    mv, frames, state = (6.0, 0.15), 8, None
    for i in range(frames):
        opts = va.make_opts(seed=3 + i, early_stop=False, sampling=CORRECTED)
        cam = cam_of(16, i, mv)
        raw, rec = TD._frame_guide(osc, cam, opts, w, h)
        acc, state, _ = VS.step(state, raw, rec, cam)
    conv, _ = osc.render(cam_of(2048, frames - 1, mv), va.make_opts(seed=1, early_stop=False, sampling=CORRECTED))
    conv = conv[..., :3].astype(np.float64)
    n, z = FS.guide_of(rec)
    albedo = DS.albedo_plane(osc, tex, cam, opts, 0, 16)
    osc.close()
    var = VS.variance(state)
    mse_raw = TT._mse(raw, conv)
    guided = TT._mse(VS.filtered_frame(acc, var, n, z, albedo=albedo), conv)
    demod = TT._mse(DS.demodulated_frame(acc, n, z, albedo), conv)
    print(f"textured cornell8, slow: of the raw error, variance-guided with albedo {guided / mse_raw:.4f} demodulated plain "
          f"{demod / mse_raw:.4f}; without albedo: variance-guided {TT._mse(VS.filtered_frame(acc, var, n, z), conv) / mse_raw:.4f} "
          f"plain {TT._mse(FS.filtered_frame(acc, n, z), conv) / mse_raw:.4f}")
    assert guided / mse_raw <= 1.25 * TEXTURED[0], guided / mse_raw
    assert np.isfinite(demod)
