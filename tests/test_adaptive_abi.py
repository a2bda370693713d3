"""Adaptive temporal accumulation (vmx_adaptive_default_params, vmx_temporal_accumulate_adaptive_device) without a GPU: the
symbols, the struct layout against the header, the defaults, the argument checks that come before any device work, the
Python layer's checks of its tensors — and the conditions the restatement itself (tests/adaptive_spec.py, what the GPU
tests compare with) is held to: identity with the existing restatements when nothing is cut, synthetic steps, and
oracle sequences in which a light is switched.  (The refusals by kind of handle and the overlaps need a handle, hence a
device: tests/test_gpu_adaptive.py.)"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_spec as AS
import filter_spec as FS
import motion_spec as MS
import oracle_lib as O
import temporal_spec as TS
import test_temporal_abi as TT
import test_variance_abi as TV
import variance_spec as VS
import vermilion_amd as va
from vermilion_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vermilion_hip.h")
ENTRIES = ("vmx_adaptive_default_params", "vmx_temporal_accumulate_adaptive_device")
F = np.float32
CORRECTED = L.VMX_SAMPLING_CORRECTED


def _err(lib):
    return lib.vmx_last_error().decode()


def test_adaptive_symbols_are_declared_and_bound(hip_lib):
    src = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, src), name
    # additive: no new ABI version
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src) and hip_lib.vmx_abi_version() == 2
    for name in ("make_adaptive_params", "ADAPTIVE_EPS"):
        assert name in va.__all__ and hasattr(va, name)
    assert re.search(r"#define VMX_ADAPTIVE_EPS 1e-10f\b", src) and F(va.ADAPTIVE_EPS) == F(1e-10) == AS.EPS
    # the argument list is the header's: fourteen, d_change after d_variance, the three parameter structs, the stream
    decl = re.search(r"int vmx_temporal_accumulate_adaptive_device\((.*?)\);", src, re.S).group(1)
    names = [re.sub(r"/\*.*?\*/", "", a).split()[-1].lstrip("*") for a in decl.split(",")]
    assert names == ["t", "cam", "d_rayhit", "d_motion", "d_in_rgbaz", "d_out_rgbaz", "d_rgba8", "d_history_len", "d_variance",
                     "d_change", "tparams", "vparams", "aparams", "stream"]
    assert len(L.SYMBOLS["vmx_temporal_accumulate_adaptive_device"][1]) == 14


def test_adaptive_params_layout_matches_header(tmp_path):
    fields = [n for n, _ in L.AdaptiveParams._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vermilion_hip.h"\nint main(void){\n'
    prog += 'printf("size %zu\\n", sizeof(vmx_adaptive_params));\n'
    for n in fields:
        prog += f'printf("{n} %zu\\n", offsetof(vmx_adaptive_params, {n}));\n'
    prog += "return 0;}\n"
    src = tmp_path / "sz.c"
    src.write_text(prog)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(L.AdaptiveParams) == 32
    for n in fields:
        assert int(out[n]) == getattr(L.AdaptiveParams, n).offset, n
    assert [int(out[n]) for n in fields] == [0, 4, 8, 12, 16]


def test_default_params(hip_lib):
    p = L.AdaptiveParams(9.0, 9.0, 9, 9.0, (C.c_uint32 * 4)(1, 2, 3, 4))
    assert hip_lib.vmx_adaptive_default_params(C.byref(p)) == L.VMX_OK
    assert (F(p.gamma), F(p.min_support), p.normal_squarings, F(p.sigma_depth)) == (F(3.0), F(4.0), 5, F(0.1))
    assert list(p.reserved) == [0, 0, 0, 0]
    assert hip_lib.vmx_adaptive_default_params(None) == L.VMX_ERR_INVALID
    q = va.make_adaptive_params(gamma=2, sigma_depth=0.5)
    assert (q.gamma, q.min_support, q.normal_squarings, q.sigma_depth) == (2.0, 4.0, 5, 0.5)
    lib_defaults, spec_defaults = AS.params_of(va.make_adaptive_params()), AS.params_of()
    assert all(F(lib_defaults[k]) == F(spec_defaults[k]) for k in spec_defaults)


def test_accumulate_adaptive_checks_do_not_need_a_gpu(hip_lib):
    """the variance call's checks in its order — aparams right after vparams, d_change's alignment after d_variance's —
    each seen alone, the handle last.  Without a handle the call cannot know whether a variance is due: a missing one is
    then no refusal, and counts as no output."""
    acc = hip_lib.vmx_temporal_accumulate_adaptive_device
    buf = np.zeros(8 * 8 * 16 + 4, np.float32)
    ptr = (buf.ctypes.data + 15) & ~15
    cam = va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 16)

    def refused(args, what):
        assert acc(*args) == L.VMX_ERR_INVALID, what
        assert what in _err(hip_lib), (what, _err(hip_lib))

    cb = C.byref(cam)
    N = None
    for mv in (None, ptr):
        for var in (None, ptr):
            for chg in (None, ptr):
                refused((N, cb, ptr, mv, ptr, ptr, N, N, var, chg, N, N, N, N), "NULL handle")
                refused((N, cb, ptr, mv, ptr, N, ptr, N, var, chg, N, N, N, N), "NULL handle")
                refused((N, N, ptr, mv, ptr, ptr, N, N, var, chg, N, N, N, N), "NULL camera")
                refused((N, cb, N, mv, ptr, ptr, N, N, var, chg, N, N, N, N), "NULL d_rayhit")
                refused((N, cb, ptr, mv, N, ptr, N, N, var, chg, N, N, N, N), "NULL d_in_rgbaz")
                refused((N, cb, ptr + 4, mv, ptr, ptr, N, N, var, chg, N, N, N, N), "d_rayhit must be 16-byte")
                refused((N, cb, ptr, mv, ptr + 2, ptr, N, N, var, chg, N, N, N, N), "4-byte")
        # a variance counts as an output, the change plane and the history do not
        refused((N, cb, ptr, mv, ptr, N, N, N, ptr, N, N, N, N, N), "NULL handle")
        refused((N, cb, ptr, mv, ptr, N, N, ptr, N, ptr, N, N, N, N), "no output")
        for off in (1, 2, 3):
            refused((N, cb, ptr, mv, ptr, ptr, N, N, ptr + off, N, N, N, N, N), "d_variance must be 4-byte aligned")
            refused((N, cb, ptr, mv, ptr, ptr, N, N, ptr, ptr + off, N, N, N, N), "d_change must be 4-byte aligned")
            refused((N, cb, ptr, mv, ptr, ptr, N, N, N, ptr + off, N, N, N, N), "d_change must be 4-byte aligned")
        # d_variance's alignment comes before d_change's
        refused((N, cb, ptr, mv, ptr, ptr, N, N, ptr + 2, ptr + 2, N, N, N, N), "d_variance must be 4-byte aligned")
        bad_cam = va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 3)
        refused((N, C.byref(bad_cam), ptr, mv, ptr, ptr, N, N, N, N, N, N, N, N), "rays_per_pixel < 4")
    refused((N, cb, ptr, ptr + 8, ptr, ptr, N, N, N, N, N, N, N, N), "d_motion must be 16-byte aligned")
    # the temporal parameters first, then the variance parameters, then the adaptive ones, all before every pointer
    tp = va.make_temporal_params(plane_tol=0.0)
    vp = va.make_variance_params(min_history=0.5)
    ap = va.make_adaptive_params(gamma=0.0)
    refused((N, N, N, N, N, N, N, N, N, N, C.byref(tp), C.byref(vp), C.byref(ap), N), "vmx_temporal_params")
    refused((N, N, N, N, N, N, N, N, N, N, N, C.byref(vp), C.byref(ap), N), "vmx_variance_params")
    refused((N, N, N, N, N, N, N, N, N, N, N, N, C.byref(ap), N), "vmx_adaptive_params")
    refused((N, N, N, N, N, N, N, N, N, N, N, N, N, N), "NULL camera")
    bad = [dict(gamma=float("nan")), dict(gamma=float("inf")), dict(gamma=0.0), dict(gamma=-3.0),
           dict(min_support=float("nan")), dict(min_support=float("inf")), dict(min_support=0.5), dict(min_support=-4.0),
           dict(normal_squarings=9), dict(normal_squarings=1 << 31),
           dict(sigma_depth=float("nan")), dict(sigma_depth=float("inf")), dict(sigma_depth=0.0), dict(sigma_depth=-0.1)]
    for kw in bad:
        p = va.make_adaptive_params(**kw)
        refused((N, cb, ptr, N, ptr, ptr, N, N, N, N, N, N, C.byref(p), N), "vmx_adaptive_params")
        assert list(kw)[0] in _err(hip_lib), (kw, _err(hip_lib))
    for i in range(4):
        p = va.make_adaptive_params()
        p.reserved[i] = 1
        refused((N, cb, ptr, N, ptr, ptr, N, N, N, N, N, N, C.byref(p), N), "reserved")
        assert "vmx_adaptive_params" in _err(hip_lib)
    # the ends of the ranges are inside them
    for kw in (dict(min_support=1.0), dict(normal_squarings=0), dict(normal_squarings=8), dict(gamma=3e38), dict(gamma=1e-30)):
        p = va.make_adaptive_params(**kw)
        refused((N, cb, ptr, N, ptr, ptr, N, N, N, N, N, N, C.byref(p), N), "NULL handle")


def test_stand_alone_argument_checks_build_and_pass(tmp_path):
    """tests/cpp/adaptive_args.cpp, the program to run under the host sanitizers (against a library built with them), built
    plainly: the same checks through the C header, from C++"""
    exe = tmp_path / "adaptive_args"
    so_dir = os.path.join(ROOT, "vermilion_amd")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "adaptive_args.cpp"), os.path.join(so_dir, "libvermilion_hip.so"),
                    "-Wl,-rpath," + so_dir, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "clean" in run.stdout, run.stderr


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
    for moments in (False, True):
        t = va.Temporal.__new__(va.Temporal)
        t._lib, t._h, t.device, t.shape, t.moments = TV.NoLib(), None, 0, (41, 70), moments
        kw = dict(variance=ok_var) if moments else {}
        with pytest.raises(ValueError, match="adaptive must be None, True or make_adaptive_params"):
            t.accumulate(cam, ok_raw, ok_frame, adaptive=3.0, **kw)
        with pytest.raises(ValueError, match="adaptive must be None, True or make_adaptive_params"):
            t.accumulate(cam, ok_raw, ok_frame, adaptive=L.VarianceParams(), **kw)
        with pytest.raises(ValueError, match="change needs adaptive"):
            t.accumulate(cam, ok_raw, ok_frame, change=ok_var, **kw)
        with pytest.raises(ValueError, match="change needs adaptive"):
            t.accumulate(cam, ok_raw, ok_frame, change=ok_var, adaptive=False, **kw)
        for adaptive in (True, L.AdaptiveParams()):
            with pytest.raises(ValueError, match="change must be a torch tensor"):
                t.accumulate(cam, ok_raw, ok_frame, adaptive=adaptive, change=np.zeros((41, 70), np.float32), **kw)
            with pytest.raises(ValueError, match="change must be torch.float32"):
                t.accumulate(cam, ok_raw, ok_frame, adaptive=adaptive, change=torch.zeros((41, 70), dtype=torch.float64), **kw)
            with pytest.raises(ValueError, match=r"change must be \[41, 70\]"):
                t.accumulate(cam, ok_raw, ok_frame, adaptive=adaptive, change=torch.zeros((41, 70, 1)), **kw)
            with pytest.raises(ValueError, match="change must be contiguous"):
                t.accumulate(cam, ok_raw, ok_frame, adaptive=adaptive, change=torch.zeros((70, 41)).transpose(0, 1), **kw)
            with pytest.raises(ValueError, match="change must be on cuda"):
                t.accumulate(cam, ok_raw, ok_frame, adaptive=adaptive, change=torch.zeros((41, 70)), **kw)
            with pytest.raises(ValueError, match="raw must be on cuda"):  # (the other tensors are checked as ever)
                t.accumulate(cam, torch.zeros((41, 70, 16)), ok_frame, adaptive=adaptive, **kw)
    # the rules of the kind of handle are the existing calls'
    t.moments = True
    with pytest.raises(ValueError, match="variance is required"):
        t.accumulate(cam, ok_raw, ok_frame, adaptive=True)
    t.moments = False
    with pytest.raises(ValueError, match="moments=True"):
        t.accumulate(cam, ok_raw, ok_frame, adaptive=True, variance=ok_var)


# ---- identity with the existing restatements ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frame(name, motion, i, light):
    """(cam, raw [H, W, 5], rec [H, W]) of frame i of the sequences of tests/test_temporal_abi.py — 16 spp, corrected
    sampling, seed 3 + i, the camera at step i of MOTIONS[motion] — under the sphere table `light`"""
    osc, cam_of, (w, h) = _scene(name, light)
    opts = va.make_opts(seed=3 + i, early_stop=False, sampling=CORRECTED)
    cam = cam_of(16, i, TT.MOTIONS[motion])
    raw, _ = osc.render(cam, opts)
    o, d = O.primary_rays(cam, opts, 0)
    rec = np.array(osc.raycast(o, d).reshape(h, w))
    raw.setflags(write=False), rec.setflags(write=False)
    return cam, raw, rec


@functools.lru_cache(maxsize=None)
def _converged(name, motion, i, light):
    """the oracle's 1024-spp frame (seed 1) of frame i's camera under `light`, float64 [H, W, 3]"""
    osc, cam_of, _ = _scene(name, light)
    conv, _ = osc.render(cam_of(1024, i, TT.MOTIONS[motion]), va.make_opts(seed=1, early_stop=False, sampling=CORRECTED))
    return conv[..., :3].astype(np.float64)


LIGHTS = {"default": None, "dim": (3.8, 3.8, 3.8), "red": (15.2, 5.0, 1.5)}


@functools.lru_cache(maxsize=None)
def _scene(name, light):
    """the oracle scene of TT._oracle_case with the default sphere table, or with its big light (sphere 1) dimmed from
    15.2 to 3.8 ("dim") or recoloured to (15.2, 5.0, 1.5) ("red")"""
    from vermilion_amd import scenes
    if name == "cornell8":
        pos, nrm, uv = scenes.cornell8()
    else:
        pos, nrm, uv = scenes.lattice()
    _, cam_of, size = TT._oracle_case(name)
    spheres = va.default_spheres()
    assert spheres[1].flags & L.VMX_SPHERE_EMIT and tuple(F(v) for v in spheres[1].colour) == (F(15.2),) * 3
    if LIGHTS[light] is not None:
        spheres[1].colour[:] = LIGHTS[light]
    return O.OracleScene(pos, nrm, uv, spheres=spheres), cam_of, size


def test_spec_without_a_cut_is_the_existing_restatement():
    """gamma = 3e38: gamma*gamma is +inf, r is 0 or NaN and no history is cut.  Six frames of the Cornell set under the
    slow camera: adaptive_spec.step equals temporal_spec.step bit for bit — frame, state and history lengths — and its
    moments form equals variance_spec.step, moments and variance included; d_change is 0 or NaN everywhere.  With motion
    records (the block of tests/motion_spec.py, case D) it equals motion_spec.step."""
    sa = sm = st = sv = None
    for i in range(6):
        cam, raw, rec = _frame("cornell8", "slow", i, "default")
        want, st, want_n = TS.step(st, raw, rec, cam)
        got, sa, got_n, chg = AS.step(sa, raw, rec, cam, aparams=AS.OFF)
        assert FS.same_bits(got, want) and FS.same_bits(got_n, want_n), i
        assert all(FS.same_bits(sa[k], st[k]) for k in ("c", "n_h", "n", "z", "X")), i
        assert np.all((chg == 0) | np.isnan(chg))
        wantv, sv, wantv_n = VS.step(sv, raw, rec, cam)
        gotm, sm, gotm_n, _ = AS.step(sm, raw, rec, cam, aparams=AS.OFF, moments=True)
        assert FS.same_bits(gotm, wantv) and FS.same_bits(gotm_n, wantv_n) and FS.same_bits(sm["m"], sv["m"]), i
        assert FS.same_bits(VS.variance(sm), VS.variance(sv)), i
    assert want_n.max() >= 6 and 0 < np.mean(want_n < 6) < 1  # (history kept and history lost)
    # with the defaults the same sequence does differ somewhere (the detector is not inert), in few pixels
    sa, cuts = None, 0
    for i in range(6):
        cam, raw, rec = _frame("cornell8", "slow", i, "default")
        _, sa, _, chg = AS.step(sa, raw, rec, cam)
        cuts += int(np.sum(chg > 1))
    assert 0 < cuts < 0.03 * 6 * chg.size
    # motion records
    from vermilion_amd import scenes
    pos0, nrm0, uv = scenes.cornell8()
    shift, angle, cam_step = MS.CASES["D"]
    c, (w, h) = scenes.cornell_camera(), (70, 41)
    sa = sm = None
    prev = None
    for k in range(3):
        pos, nrm = MS.moved_block(pos0, nrm0, shift, angle, k)
        p, r = c["position"], c["rotation_deg"]
        cam = va.make_camera((p[0] + cam_step[0] * k, p[1], p[2]), (r[0], r[1] + cam_step[1] * k, r[2]), w, h, 16)
        opts = va.make_opts(seed=3 + k, early_stop=False, sampling=CORRECTED)
        osc = O.OracleScene(pos, nrm, uv)
        raw, _ = osc.render(cam, opts)
        o, d = O.primary_rays(cam, opts, 0)
        rec = np.array(osc.raycast(o, d).reshape(h, w))
        osc.close()
        mv = None if prev is None else MS.motion(rec, pos, prev[0], prev[1])
        want, sm, want_n = MS.step(sm, raw, rec, cam, mv)
        got, sa, got_n, _ = AS.step(sa, raw, rec, cam, mv, aparams=AS.OFF)
        assert FS.same_bits(got, want) and FS.same_bits(got_n, want_n), k
        prev = (pos, nrm)
    assert (mv.view(np.uint32)[..., 3] & 1).any()


# ---- synthetic ----------------------------------------------------------------------------------------------------------
def test_spec_cuts_a_step_on_a_flat_wall():
    """a constant grey frame sequence on one plane (tests/test_variance_abi.py's plane_records), 0.5 for four frames, 0.1
    from frame 4: the input has no variance, s2 is the floor and r is huge, so frame 4's history is cut to nothing —
    n' < 1.01 and the output within 1e-6 of 0.1 wherever the window has support (everywhere: the plane is flat) — while
    the plain call still shows (3*0.5 + ... ) 0.42"""
    cam, rec = TV.plane_records(40, 20)
    sa = st = None
    for i in range(6):
        f = np.ones((20, 40, 5), np.float32)
        f[..., :3] = F(0.5 if i < 4 else 0.1)
        out, sa, n, chg = AS.step(sa, f, rec, cam)
        plain, st, n_plain = TS.step(st, f, rec, cam)
        if i < 4:
            assert FS.same_bits(out, plain) and np.all(chg == 0) and np.all(n == i + 1)
        if i == 4:
            support = chg > 0
            assert support.all()
            print("frame 4: largest n'", float(n.max()), "largest distance from 0.1", float(np.abs(out[..., :3] - F(0.1)).max()),
                  "; the plain call shows", float(plain[0, 0, 0]))
            assert np.all(n[support] < 1.01)
            assert np.abs(out[..., :3] - F(0.1))[support].max() <= 1e-6
            assert abs(float(plain[0, 0, 0]) - 0.42) < 1e-6 and np.all(n_plain == 5)
        if i == 5:  # the cut history grows again
            assert np.all(chg < 1e-3) and np.all(n > 1.9) and np.all(n < 2.01)  # (r: the rounding of frame 4's blend)


def test_spec_never_cuts_without_support():
    """a bar one pixel wide at distance 1 in front of a wall at distance 40, in an image three rows high: a bar pixel's
    window holds three taps of its own surface, and with sigma_depth 0.1 the wall's weigh 1/(1 + 390^2) each — about three
    effective taps, fewer than min_support = 4.  The bar is never cut and d_change == 0 on it, although its colour steps
    like the wall's, which is cut.  With min_support = 1 the bar has support and is cut too."""
    w, h = 24, 3
    cam, rec = TV.plane_records(w, h)
    rec = np.array(rec)
    rec[..., 3] = 40.0
    rec[:, 11, 3] = 1.0
    wall = np.ones(w, bool)
    wall[11] = False
    for ap, bar_cut in ((None, False), (dict(min_support=1.0), True)):
        sa = None
        for i in range(4):
            f = np.ones((h, w, 5), np.float32)
            f[..., :3] = F(0.5 if i < 2 else 0.1)
            out, sa, n, chg = AS.step(sa, f, rec, cam, aparams=ap)
            if i == 2:
                assert np.all(chg[:, wall] > 1) and np.all(n[:, wall] < 1.01)
            if bar_cut:
                assert np.all(chg[:, 11] > 1) == (i == 2)
            else:
                assert np.all(chg[:, 11] == 0) and np.all(n[:, 11] == i + 1), i
        if not bar_cut:
            assert np.allclose(out[:, 11, :3], (0.5 + 0.5 + 0.1 + 0.1) / 4, atol=1e-6)


def test_spec_nan_colours_never_cut():
    """a NaN colour in a window makes K, r NaN (or leaves the finite channels' maximum, if it came later): `r > 1` is
    false for NaN, the pixel keeps its history length, and the NaN passes into the blend as in the existing call"""
    cam, rec = TV.plane_records(20, 12)
    f0 = np.full((12, 20, 5), 0.5, np.float32)
    f1 = np.array(f0)
    f1[5, 9, 0] = np.nan
    _, s, _, _ = AS.step(None, f0, rec, cam)
    out, s, n, chg = AS.step(s, f1, rec, cam)
    assert np.all(n == 2)
    assert np.isnan(out[5, 9, 0]) and np.isnan(out[..., :3]).sum() == 1
    assert np.isnan(chg[2:9, 6:13]).all() and np.all(chg[:, 13:] == 0)


# ---- oracle frames: a light is switched -------------------------------------------------------------------------------
def _run(name, motion, switch, frames=16):
    """the three accumulations of a sequence whose lighting changes to `switch` at frame 8 (None: never): per frame
    (mse plain, mse adaptive, mse of a handle reset at frame 8, raw mse, share of pixels with r > 1)"""
    sp = sa = sr = None
    rows = []
    for i in range(frames):
        light = switch if (switch and i >= 8) else "default"
        cam, raw, rec = _frame(name, motion, i, light)
        conv = _converged(name, motion, i, light) if i in (7, 8, 10, 15) else None
        plain, sp, _ = TS.step(sp, raw, rec, cam)
        adapt, sa, _, chg = AS.step(sa, raw, rec, cam)
        if i == 8:
            sr = None
        reset, sr, _ = TS.step(sr, raw, rec, cam)
        share = float(np.mean(chg > 1))
        if conv is None:
            rows.append((None, None, None, None, share))
        else:
            rows.append((TT._mse(plain, conv), TT._mse(adapt, conv), TT._mse(reset, conv), TT._mse(raw, conv), share))
    return rows


CASES = [("cornell8", "static"), ("cornell8", "slow"), ("lattice", "static"), ("lattice", "slow")]


@pytest.mark.parametrize("name,motion", CASES)
def test_spec_follows_a_dimmed_light(name, motion):
    """the big light (sphere 1) dimmed from 15.2 to 3.8 at frame 8; against the oracle's 1024-spp frame of each frame's own
    camera and lighting: at frame 10 mse(adaptive) <= 2.0 x mse(a handle reset at frame 8) and <= 0.5 x mse(plain); at
    frame 15 mse(adaptive) <= 1.6 x mse(reset).  A prototype measured 1.27-1.46 x reset and 0.22-0.30 x plain at frame 10
    and 1.10-1.27 x reset at frame 15.  The caps stop a broken detector passing; they are no tuning targets."""
    rows = _run(name, motion, "dim")
    for i in (8, 10, 15):
        p, a, r, raw, share = rows[i]
        print(f"{name} {motion} dim, frame {i}: of the raw error, plain {p / raw:.3f} adaptive {a / raw:.3f} reset {r / raw:.3f}; "
              f"adaptive / reset {a / r:.3f}, adaptive / plain {a / p:.3f}; r > 1 in {100 * share:.2f} % of pixels")
    p, a, r, _, _ = rows[10]
    assert a <= 2.0 * r, (name, motion, a / r)
    assert a <= 0.5 * p, (name, motion, a / p)
    p, a, r, _, _ = rows[15]
    assert a <= 1.6 * r, (name, motion, a / r)


@pytest.mark.parametrize("motion", ["static", "slow"])
def test_spec_follows_a_recoloured_light(motion):
    """the big light recoloured to (15.2, 5.0, 1.5) at frame 8, Cornell set: the luminance moves little, the per-channel
    statistic sees it — at frame 10 mse(adaptive) <= 0.85 x mse(plain); a prototype measured 0.68-0.72"""
    rows = _run("cornell8", motion, "red")
    for i in (8, 10, 15):
        p, a, r, raw, share = rows[i]
        print(f"cornell8 {motion} red, frame {i}: of the raw error, plain {p / raw:.3f} adaptive {a / raw:.3f} reset {r / raw:.3f}; "
              f"adaptive / plain {a / p:.3f}")
    p, a, _, _, _ = rows[10]
    assert a <= 0.85 * p, (motion, a / p)


@pytest.mark.parametrize("name,motion", CASES)
def test_spec_costs_little_under_unchanged_lighting(name, motion):
    """the same sequences with no switch: at frame 7 mse(adaptive) <= 1.10 x mse(plain), and in every frame at most 3 % of
    the pixels have r > 1.  A prototype measured 1.002-1.05 and at most 0.8 %."""
    rows = _run(name, motion, None)
    shares = [r[4] for r in rows]
    for i in (7, 15):
        p, a, _, _, _ = rows[i]
        print(f"{name} {motion}, unchanged lighting, frame {i}: adaptive / plain {a / p:.4f}")
    print(f"{name} {motion}: share of pixels with r > 1 per frame, largest {100 * max(shares):.2f} %")
    p, a, _, _, _ = rows[7]
    assert a <= 1.10 * p, (name, motion, a / p)
    assert max(shares) <= 0.03, (name, motion, shares)
