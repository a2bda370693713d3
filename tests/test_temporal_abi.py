"""Temporal accumulation (vmx_temporal_*) without a GPU: the symbols, the struct layout against the header, the
defaults, the argument checks that come before any device work, the Python layer's checks of its tensors — and the
conditions the restatement itself (tests/temporal_spec.py, what the GPU tests compare with) is held to, on oracle data
and on synthetic cases, so that the yardstick cannot drift."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import filter_spec as FS
import oracle_lib as O
import temporal_spec as TS
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vermilion_hip.h")
ENTRIES = ("vmx_temporal_default_params", "vmx_temporal_create", "vmx_temporal_destroy", "vmx_temporal_reset",
           "vmx_temporal_frames", "vmx_temporal_accumulate_device")


def _err(lib):
    return lib.vmx_last_error().decode()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_temporal_symbols_are_declared_and_bound(hip_lib):
    src = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, src), name
    # additive: no new ABI version
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src) and hip_lib.vmx_abi_version() == 2
    for name in ("Temporal", "make_temporal_params"):
        assert name in va.__all__ and hasattr(va, name)


def test_temporal_params_layout_matches_header(tmp_path):
    fields = [n for n, _ in L.TemporalParams._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vermilion_hip.h"\nint main(void){\n'
    prog += 'printf("size %zu\\n", sizeof(vmx_temporal_params));\n'
    for n in fields:
        prog += f'printf("{n} %zu\\n", offsetof(vmx_temporal_params, {n}));\n'
    prog += "return 0;}\n"
    src = tmp_path / "sz.c"
    src.write_text(prog)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(L.TemporalParams) == 32
    for n in fields:
        assert int(out[n]) == getattr(L.TemporalParams, n).offset, n
    assert [int(out[n]) for n in fields] == [0, 4, 8, 12]


def test_default_params(hip_lib):
    p = L.TemporalParams(9.0, 9.0, 9.0, (C.c_uint32 * 5)(1, 2, 3, 4, 5))
    assert hip_lib.vmx_temporal_default_params(C.byref(p)) == L.VMX_OK
    assert (np.float32(p.normal_min), np.float32(p.plane_tol), np.float32(p.max_history)) == \
        (np.float32(0.9), np.float32(0.01), np.float32(32.0))
    assert list(p.reserved) == [0, 0, 0, 0, 0]
    assert hip_lib.vmx_temporal_default_params(None) == L.VMX_ERR_INVALID
    q = va.make_temporal_params(plane_tol=0.5, max_history=4)
    assert (np.float32(q.normal_min), q.plane_tol, q.max_history) == (np.float32(0.9), 0.5, 4.0)
    # the restatement's defaults are the library's
    lib_defaults, spec_defaults = TS.params_of(va.make_temporal_params()), TS.params_of()
    assert all(np.float32(lib_defaults[k]) == np.float32(spec_defaults[k]) for k in spec_defaults)


def test_create_and_null_handles_do_not_need_a_gpu(hip_lib):
    h = C.c_void_p()
    # a zero size is refused before the device is looked at
    for w, hh in ((0, 8), (8, 0), (0, 0)):
        assert hip_lib.vmx_temporal_create(0, w, hh, C.byref(h)) == L.VMX_ERR_INVALID
        assert "resolution must be non-zero" in _err(hip_lib) and not h.value
    assert hip_lib.vmx_temporal_create(0, 1 << 16, 1 << 16, C.byref(h)) == L.VMX_ERR_INVALID  # make_frame's size check
    assert "image too large" in _err(hip_lib)
    assert hip_lib.vmx_temporal_create(0, 8, 8, None) == L.VMX_ERR_INVALID
    # no such device: an ordinal no machine has; without any device, device 0 as well
    assert hip_lib.vmx_temporal_create(1 << 20, 8, 8, C.byref(h)) == L.VMX_ERR_NO_DEVICE and not h.value
    if hip_lib.vmx_device_count() == 0:
        assert hip_lib.vmx_temporal_create(0, 8, 8, C.byref(h)) == L.VMX_ERR_NO_DEVICE and not h.value
        assert "no CPU path" in _err(hip_lib)
        with pytest.raises(va.VmxError) as e:
            va.Temporal(8, 8)
        assert e.value.code == L.VMX_ERR_NO_DEVICE
    buf = np.zeros(8 * 8 * 16 + 4, np.float32)
    ptr = (buf.ctypes.data + 15) & ~15  # (d_rayhit must be 16-byte aligned)
    cam = va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 16)
    n = C.c_uint64(0)
    for fn, args in ((hip_lib.vmx_temporal_destroy, (None,)),
                     (hip_lib.vmx_temporal_reset, (None, None)),
                     (hip_lib.vmx_temporal_frames, (None, C.byref(n))),
                     (hip_lib.vmx_temporal_accumulate_device, (None, C.byref(cam), ptr, ptr, ptr, None, None, None, None))):
        assert fn(*args) == L.VMX_ERR_INVALID, fn
        assert "NULL handle" in _err(hip_lib), _err(hip_lib)
    # checks that come before the handle, so that each is seen alone: parameters, pointers, outputs, the camera
    acc = hip_lib.vmx_temporal_accumulate_device
    assert acc(None, C.byref(cam), ptr, ptr, None, None, None, None, None) == L.VMX_ERR_INVALID
    assert "no output" in _err(hip_lib)
    assert acc(None, C.byref(cam), ptr, ptr, None, None, ptr, None, None) == L.VMX_ERR_INVALID  # history alone is none
    assert "no output" in _err(hip_lib)
    assert acc(None, None, ptr, ptr, ptr, None, None, None, None) == L.VMX_ERR_INVALID and "NULL camera" in _err(hip_lib)
    assert acc(None, C.byref(cam), None, ptr, ptr, None, None, None, None) == L.VMX_ERR_INVALID and "NULL d_rayhit" in _err(hip_lib)
    assert acc(None, C.byref(cam), ptr, None, ptr, None, None, None, None) == L.VMX_ERR_INVALID and "NULL d_in_rgbaz" in _err(hip_lib)
    assert acc(None, C.byref(cam), ptr + 4, ptr, ptr, None, None, None, None) == L.VMX_ERR_INVALID and "16-byte" in _err(hip_lib)
    assert acc(None, C.byref(cam), ptr, ptr + 2, ptr, None, None, None, None) == L.VMX_ERR_INVALID and "4-byte" in _err(hip_lib)
    # the camera, as vmx_raycast_camera_device checks its own (make_frame)
    for bad_cam, what in ((va.make_camera((0, 0, 0), (0, 0, 0), 0, 8, 16), "resolution must be non-zero"),
                          (va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 3), "rays_per_pixel < 4"),
                          (va.make_camera((0, 0, 0), (0, 0, 0), 1 << 16, 1 << 16, 16), "image too large")):
        assert acc(None, C.byref(bad_cam), ptr, ptr, ptr, None, None, None, None) == L.VMX_ERR_INVALID
        assert what in _err(hip_lib), _err(hip_lib)
    units = va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 16)
    units.rotation_units = 2
    assert acc(None, C.byref(units), ptr, ptr, ptr, None, None, None, None) == L.VMX_ERR_INVALID
    assert "rotation_units" in _err(hip_lib)
    bad = [dict(normal_min=float("nan")), dict(normal_min=float("inf")), dict(normal_min=1.5), dict(normal_min=-1.5),
           dict(plane_tol=float("nan")), dict(plane_tol=float("inf")), dict(plane_tol=0.0), dict(plane_tol=-0.01),
           dict(max_history=float("nan")), dict(max_history=float("inf")), dict(max_history=0.5), dict(max_history=-3.0)]
    for kw in bad:
        p = va.make_temporal_params(**kw)
        assert acc(None, C.byref(cam), ptr, ptr, ptr, None, None, C.byref(p), None) == L.VMX_ERR_INVALID, kw
        assert "vmx_temporal_params" in _err(hip_lib) and list(kw)[0] in _err(hip_lib), (kw, _err(hip_lib))
    for i in range(5):
        p = va.make_temporal_params()
        p.reserved[i] = 1
        assert acc(None, C.byref(cam), ptr, ptr, ptr, None, None, C.byref(p), None) == L.VMX_ERR_INVALID
        assert "reserved" in _err(hip_lib)
    # the ends of the ranges are inside them
    for kw in (dict(normal_min=-1.0), dict(normal_min=1.0), dict(max_history=1.0)):
        p = va.make_temporal_params(**kw)
        assert acc(None, C.byref(cam), ptr, ptr, ptr, None, None, C.byref(p), None) == L.VMX_ERR_INVALID
        assert "NULL handle" in _err(hip_lib), (kw, _err(hip_lib))


class NoLib:  # any call into the library fails the test
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_layer_rejects_bad_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    t = va.Temporal.__new__(va.Temporal)
    t._lib, t._h, t.device, t.shape = NoLib(), None, 0, (41, 70)
    cam = va.make_camera((0, 0, 0), (0, 0, 0), 70, 41, 16)
    frame = torch.zeros((41, 70, 5), dtype=torch.float32)  # CPU tensors: not on the handle's device
    raw = torch.zeros((41, 70, 16), dtype=torch.float32)
    with pytest.raises(ValueError, match="raw must be a torch tensor"):
        t.accumulate(cam, np.zeros((41, 70, 16), np.float32), frame)
    with pytest.raises(ValueError, match="raw must be torch.float32"):
        t.accumulate(cam, raw.double(), frame)
    with pytest.raises(ValueError, match=r"raw must be \[41, 70, 16\]"):
        t.accumulate(cam, raw.reshape(-1, 16), frame)
    with pytest.raises(ValueError, match="raw must be contiguous"):
        t.accumulate(cam, torch.zeros((70, 41, 16)).transpose(0, 1), frame)
    with pytest.raises(ValueError, match="raw must be on cuda"):
        t.accumulate(cam, raw, frame)

    class OnDevice:  # a tensor that passes every check: the later arguments are reached
        def __init__(self, shape, dtype):
            self.shape, self.dtype, self.device = shape, dtype, torch.device("cuda", 0)

        def data_ptr(self):
            return 0

        def is_contiguous(self):
            return True

    OnDevice.__module__ = "torch"
    ok_raw = OnDevice((41, 70, 16), torch.float32)
    ok_frame = OnDevice((41, 70, 5), torch.float32)
    with pytest.raises(ValueError, match="rgbaz must be a torch tensor"):
        t.accumulate(cam, ok_raw, np.zeros((41, 70, 5), np.float32))
    with pytest.raises(ValueError, match="rgbaz must be torch.float32"):
        t.accumulate(cam, ok_raw, frame.double())
    with pytest.raises(ValueError, match=r"rgbaz must be \[41, 70, 5\]"):
        t.accumulate(cam, ok_raw, frame.reshape(-1, 5))
    with pytest.raises(ValueError, match="rgbaz must be contiguous"):
        t.accumulate(cam, ok_raw, torch.zeros((70, 41, 5)).transpose(0, 1))
    with pytest.raises(ValueError, match="rgbaz must be on cuda"):
        t.accumulate(cam, ok_raw, frame)
    with pytest.raises(ValueError, match="out must be on cuda"):
        t.accumulate(cam, ok_raw, ok_frame, out=frame)
    with pytest.raises(ValueError, match="rgba8 must be torch.uint8"):
        t.accumulate(cam, ok_raw, ok_frame, rgba8=torch.zeros((41, 70, 4)))
    with pytest.raises(ValueError, match=r"rgba8 must be \[41, 70, 4\]"):
        t.accumulate(cam, ok_raw, ok_frame, rgba8=torch.zeros((41, 70, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"history must be \[41, 70\]"):
        t.accumulate(cam, ok_raw, ok_frame, out=ok_frame, history=torch.zeros((41, 70, 1)))
    with pytest.raises(ValueError, match="history must be torch.float32"):
        t.accumulate(cam, ok_raw, ok_frame, out=ok_frame, history=torch.zeros((41, 70), dtype=torch.int32))
    with pytest.raises(ValueError, match="history must be on cuda"):
        t.accumulate(cam, ok_raw, ok_frame, out=ok_frame, history=torch.zeros((41, 70)))


# ---- the restatement's own conditions ----------------------------------------------------------------------------------
MOTIONS = {"static": (0.0, 0.0), "slow": (6.0, 0.15), "fast": (25.0, 0.6)}


def _oracle_case(name):
    if name == "cornell8":
        pos, nrm, uv = scenes.cornell8()
        c, (w, h) = scenes.cornell_camera(), (70, 41)
    else:
        pos, nrm, uv = scenes.lattice()
        c, (w, h) = scenes.lattice_camera(), (64, 48)

    def cam_of(spp, i=0, motion=(0.0, 0.0)):
        p, r = c["position"], c["rotation_deg"]
        return va.make_camera((p[0] + motion[0] * i, p[1], p[2]), (r[0], r[1] + motion[1] * i, r[2]), w, h, spp)

    return O.OracleScene(pos, nrm, uv), cam_of, (w, h)


def _mse(a, conv):
    return float(np.mean((a[..., :3].astype(np.float64) - conv) ** 2))


@pytest.mark.parametrize("motion", list(MOTIONS))
@pytest.mark.parametrize("name", ["cornell8", "lattice"])
def test_spec_quality_cap_on_oracle_frames(name, motion):
    """(a) 8 frames of 16 spp, corrected sampling, early stop off, frame i with seed 3 + i and the camera moved to
    x + dx*i, y-rotation + dr*i; the guide from the oracle's sample-0 camera rays.  Against the oracle's 2048-spp frame at
    the last camera (seed 1): mse(accumulated) / mse(raw last frame) <= 0.35, and the a-trous restatement of the
    accumulated frame beats that of the raw last frame.  A prototype of this arithmetic measured 0.106-0.233 for the
    first and 0.044-0.052 against 0.068-0.092 (as shares of the raw error) for the second.  The caps stop a broken
    reprojection passing; they are no tuning targets."""
    osc, cam_of, (w, h) = _oracle_case(name)
    corrected = L.VMX_SAMPLING_CORRECTED
    mv = MOTIONS[motion]
    frames = 8
    state = None
    for i in range(frames):
        opts = va.make_opts(seed=3 + i, early_stop=False, sampling=corrected)
        cam = cam_of(16, i, mv)
        raw, _ = osc.render(cam, opts)
        o, d = O.primary_rays(cam, opts, 0)
        rec = osc.raycast(o, d).reshape(h, w)
        acc, state, hist = TS.step(state, raw, rec, cam)
        assert FS.same_bits(acc[..., 3:], raw[..., 3:])
    conv, _ = osc.render(cam_of(2048, frames - 1, mv), va.make_opts(seed=1, early_stop=False, sampling=corrected))
    conv = conv[..., :3].astype(np.float64)
    n, z = FS.guide_of(rec)
    mse_raw, mse_acc = _mse(raw, conv), _mse(acc, conv)
    mse_fraw, mse_facc = _mse(FS.filtered_frame(raw, n, z), conv), _mse(FS.filtered_frame(acc, n, z), conv)
    print(f"{name} {motion}: mse raw {mse_raw:.6f} accumulated {mse_acc:.6f} ratio {mse_acc / mse_raw:.4f}; filtered: "
          f"accumulated {mse_facc / mse_raw:.4f} vs raw {mse_fraw / mse_raw:.4f} of the raw error; "
          f"mean history {hist.mean():.2f}")
    assert mse_acc / mse_raw <= 0.35, (name, motion, mse_acc / mse_raw)
    assert mse_facc < mse_fraw, (name, motion, mse_facc, mse_fraw)
    osc.close()


def test_spec_static_camera_is_the_running_mean():
    """(b) a camera that does not move and one guide record per pixel for every frame: gx = x and gy = y exactly, one tap
    of weight 1, so every hit pixel's history length is the frame count (up to max_history) and its colour the running
    mean.  Five frames: step k adds at most half an ulp of its result and keeps (k - 1) / k of the error before it
    (the rounding of 1.f / k and of the difference are second order), under 1.7 ulp after five steps, and the ulp halves
    where the mean falls into the binade below: 4 ulp holds with room.  With max_history = 4 the colours are the
    float32 recurrence h + (c - h) * (1.f / min(k, 4)) itself."""
    osc, cam_of, (w, h) = _oracle_case("cornell8")
    cam = cam_of(16)
    opts = va.make_opts(seed=3, early_stop=False)
    o, d = O.primary_rays(cam, opts, 0)
    rec = osc.raycast(o, d).reshape(h, w)
    osc.close()
    hit = (rec["flags"] & 1) != 0
    assert hit.any()
    rng = np.random.RandomState(11)
    frames = [rng.uniform(0, 1, (h, w, 5)).astype(np.float32) for _ in range(7)]
    state = None
    for k, f in enumerate(frames[:5], 1):
        out, state, hist = TS.step(state, f, rec, cam)
        assert np.all(hist[hit] == np.float32(k)) and np.all(hist[~hit] == 1)
        assert np.array_equal(bits(out[~hit]), bits(f[~hit]))
    mean = np.mean(np.stack(frames[:5]).astype(np.float64), axis=0)[..., :3].astype(np.float32)
    ulps = np.abs(out[..., :3].view(np.int32).astype(np.int64) - mean.view(np.int32))[hit]
    print("largest distance from the float64 mean after 5 frames:", int(ulps.max()), "ulp")
    assert ulps.max() <= 4
    # a history cap of 4: the recurrence, and the length stops at 4
    F = np.float32
    state, want = None, None
    for k, f in enumerate(frames, 1):
        out, state, hist = TS.step(state, f, rec, cam, dict(max_history=4.0))
        c = f[..., :3]
        want = np.array(c) if want is None else np.where(hit[..., None], want + (c - want) * (F(1) / F(min(k, 4))), c)
        assert want.dtype == np.float32
        assert np.all(hist[hit] == F(min(k, 4))) and np.all(hist[~hit] == 1)
        assert np.array_equal(bits(out[..., :3]), bits(want)), k


def _two_planes(pos_x):
    """12 x 9 records of a camera at (pos_x, 0, 0) looking down -z at the plane z = -4 (one world unit per pixel), the left
    half with normal +z and the right half with normal +x whatever the camera's position"""
    cam = va.make_camera((pos_x, 0, 0), (0, 0, 0), 12, 9, 16, back_distance=1.0, back_size=(3.0, 2.25))
    rec = np.zeros((9, 12, 16), np.float32)
    ys, xs = np.meshgrid(np.arange(9), np.arange(12), indexing="ij")
    rec[..., 0] = pos_x + (xs + 0.5 - 6.0)
    rec[..., 1] = -(ys + 0.5 - 4.5)
    rec[..., 2] = -4.0
    rec[..., 3] = np.sqrt((rec[..., 0] - pos_x) ** 2 + rec[..., 1] ** 2 + 16.0)
    rec[:, :6, 6] = 1.0
    rec[:, 6:, 4] = 1.0
    rec.view(np.uint32)[..., 11] = 3
    return cam, rec


def test_spec_rejects_history_across_a_normal_edge():
    """(c) two planes in a 12 x 9 image, the left half normal +z with history colour (0.8, 0, 0.1) and the right half
    normal +x with (0, 0.6, 0.1); the camera pans by one pixel, so pixel x lands on history pixel x + 1 and column 5 on
    the other plane's column 6.  Red is history of the left plane alone and green of the right alone, and the new frame
    has neither: no output pixel has both, and none carries the other plane's — column 5 restarts.  With normal_min = -1
    and a huge plane_tol column 5 does take the right plane's green."""
    cam1, rec1 = _two_planes(-1.0)
    cam2, rec2 = _two_planes(0.0)
    hist = np.zeros((9, 12, 5), np.float32)
    hist[:, :6, :3] = np.float32([0.8, 0, 0.1])
    hist[:, 6:, :3] = np.float32([0, 0.6, 0.1])
    new = np.zeros((9, 12, 5), np.float32)
    new[..., 2] = 0.5
    _, state, _ = TS.step(None, hist, rec1, cam1)
    # the pan is one pixel: a point seen at pixel x was seen at x + 1
    u_c, _, _ = TS.proj(rec2[..., 0:3], TS.camera_of(cam2), 12, 9)
    u_h, _, _ = TS.proj(rec2[..., 0:3], TS.camera_of(cam1), 12, 9)
    assert np.abs((u_h - u_c) - 1).max() < 1e-5
    out, _, n = TS.step(state, new, rec2, cam2)
    r, g = out[..., 0], out[..., 1]
    assert not np.any((r > 0) & (g > 0))
    assert np.all(g[:, :6] == 0) and np.all(r[:, 6:] == 0)
    assert np.all(r[:, :5] > 0) and np.all(n[:, :5] == 2)          # the left plane kept its history
    assert np.all(g[:, 6:11] > 0) and np.all(n[:, 6:11] == 2)      # ... and the right plane its own
    assert np.array_equal(bits(out[:, 5]), bits(new[:, 5])) and np.all(n[:, 5] == 1)    # the edge column restarts
    assert np.array_equal(bits(out[:, 11]), bits(new[:, 11])) and np.all(n[:, 11] == 1)  # history outside the image
    loose, _, n = TS.step(state, new, rec2, cam2, dict(normal_min=-1.0, plane_tol=1e18))
    assert np.all(loose[:, 5, 1] > 0) and np.all(n[:, 5] == 2)
    assert np.array_equal(bits(loose[:, :5]), bits(out[:, :5])) and np.array_equal(bits(loose[:, 6:]), bits(out[:, 6:]))


def test_spec_passes_alpha_and_depth_through_bitwise_and_leaves_misses():
    """(d) channels 3 and 4 leave exactly as they came, whatever they hold, on the first call and on later ones; a pixel
    whose ray missed leaves with its input colour and a history length of 1"""
    cam1, rec1 = _two_planes(-0.25)
    cam2, rec2 = _two_planes(0.0)
    rng = np.random.RandomState(6)
    odd = np.array([0x7FC12345, 0xFF800000, 0x80000000, 0x00000001, 0x7F7FFFFF, 0xFFC00001], np.uint32).view(np.float32)
    miss = np.zeros((9, 12), bool)
    miss[2, 3:9] = miss[6, ::2] = True
    state = None
    for cam, rec in ((cam1, rec1), (cam2, rec2), (cam2, rec2)):
        rec = np.array(rec)
        rec.view(np.uint32)[..., 11] = np.where(miss, 2, 3)
        rec[..., 3][miss] = np.inf
        frame = rng.uniform(0, 1, (9, 12, 5)).astype(np.float32)
        frame[0, :6, 3] = odd
        frame[1, :6, 4] = odd
        frame[2, 3:9, 3] = odd  # (on missed pixels too)
        out, state, n = TS.step(state, frame, rec, cam)
        assert np.array_equal(bits(out[..., 3:]), bits(frame[..., 3:]))
        assert np.array_equal(bits(out[miss]), bits(frame[miss])) and np.all(n[miss] == 1)
    assert n.max() == 3  # (three calls, the last with the camera where it was)
    assert not np.array_equal(out[..., :3], frame[..., :3])
