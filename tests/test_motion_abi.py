"""Motion records (vmx_motion_device, vmx_temporal_accumulate_motion_device) without a GPU: the symbols, the struct layout
against the header, the argument checks that come before any device work, the Python layer's checks of its tensors — and
the conditions the restatement itself (tests/motion_spec.py, what the GPU tests compare with) is held to, on oracle data
and on synthetic cases, so that the yardstick cannot drift."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import motion_spec as MS
import oracle_lib as O
import temporal_spec as TS
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vermilion_hip.h")
ENTRIES = ("vmx_motion_device", "vmx_temporal_accumulate_motion_device")


def _err(lib):
    return lib.vmx_last_error().decode()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_motion_symbols_are_declared_and_bound(hip_lib):
    src = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, src), name
    # additive: no new ABI version
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src) and hip_lib.vmx_abi_version() == 2
    assert re.search(r"#define VMX_MOTION_MOVED 1u\b", src) and MS.MOVED == 1
    for name in ("motion_vectors", "MOTION_DTYPE"):
        assert name in va.__all__ and hasattr(va, name)


def test_motion_layout_matches_header(tmp_path):
    fields = [n for n, _ in L.Motion._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vermilion_hip.h"\nint main(void){\n'
    prog += 'printf("size %zu\\n", sizeof(vmx_motion));\n'
    for n in fields:
        prog += f'printf("{n} %zu\\n", offsetof(vmx_motion, {n}));\n'
    prog += "return 0;}\n"
    src = tmp_path / "sz.c"
    src.write_text(prog)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(L.Motion) == va.MOTION_DTYPE.itemsize == 32
    for n in fields:
        assert int(out[n]) == getattr(L.Motion, n).offset == va.MOTION_DTYPE.fields[n][1], n
    assert [int(out[n]) for n in fields] == [0, 12, 16, 28]


def test_motion_device_checks_do_not_need_a_gpu(hip_lib):
    """every host check of vmx_motion_device, each seen alone, in the order the header gives them"""
    mot = hip_lib.vmx_motion_device
    buf = np.zeros(4096, np.float32)
    p = (buf.ctypes.data + 15) & ~15
    rec, out, now, prev, nrm = p, p + 64 * 8, p + 4096, p + 4096 + 36, p + 4096 + 72  # (8 records, one triangle)

    def refused(args, what):
        assert mot(*args) == L.VMX_ERR_INVALID, what
        assert what in _err(hip_lib), (what, _err(hip_lib))

    refused((None, 8, now, prev, nrm, 1, out, 0, None), "NULL d_rayhit")
    refused((rec, 8, None, prev, nrm, 1, out, 0, None), "NULL d_pos_now")
    refused((rec, 8, now, None, nrm, 1, out, 0, None), "NULL d_pos_prev")
    refused((rec, 8, now, prev, nrm, 1, None, 0, None), "NULL d_out")
    refused((rec, 8, now, prev, nrm, 0, out, 0, None), "ntris must be non-zero")
    refused((rec + 4, 8, now, prev, nrm, 1, out, 0, None), "16-byte aligned")
    refused((rec, 8, now, prev, nrm, 1, out + 8, 0, None), "16-byte aligned")
    refused((rec, 8, now + 2, prev, nrm, 1, out, 0, None), "4-byte aligned")
    refused((rec, 8, now, prev + 1, nrm, 1, out, 0, None), "4-byte aligned")
    refused((rec, 8, now, prev, nrm + 3, 1, out, 0, None), "4-byte aligned")
    refused((rec, 1 << 31, now, prev, nrm, 1, out, 0, None), "2^31 - 1")
    refused((rec, 0xFFFFFFFF, now, prev, nrm, 1, out, 0, None), "2^31 - 1")
    # d_out over each input: the records (in place, and their last 16 bytes), either position array, the normals
    refused((rec, 8, now, prev, nrm, 1, rec, 0, None), "d_out overlaps")
    refused((rec, 8, now, prev, nrm, 1, rec + 64 * 8 - 16, 0, None), "d_out overlaps")
    refused((rec, 8, now, prev, nrm, 1, now - 8 * 32 + 16, 0, None), "d_out overlaps")
    refused((rec, 8, now, prev, nrm, 1, p + 4144, 0, None), "d_out overlaps")  # (inside d_pos_prev alone)
    refused((rec, 8, now, prev, nrm, 1, p + 4176, 0, None), "d_out overlaps")  # (from inside d_nrm_prev on)
    assert mot(rec, 0, now, prev, None, 1, p + 4176, 0, None) == L.VMX_OK      # (no normals: nothing there to overlap)
    # nothing to do: no launch and no device needed, with or without normals
    assert mot(rec, 0, now, prev, nrm, 1, out, 0, None) == L.VMX_OK
    assert mot(rec, 0, now, prev, None, 1, out, 0, None) == L.VMX_OK
    assert mot(rec, 0, now, prev, None, 1, out, 1 << 20, None) == L.VMX_OK
    # a device no machine has; without any device, device 0 as well (host pointers never reach a kernel: with a device
    # they are refused as "not device memory")
    assert mot(rec, 8, now, prev, None, 1, out, 1 << 20, None) == L.VMX_ERR_NO_DEVICE
    assert mot(rec, 8, now, prev, None, 1, out, -1, None) == L.VMX_ERR_NO_DEVICE
    if hip_lib.vmx_device_count() == 0:
        assert mot(rec, 8, now, prev, nrm, 1, out, 0, None) == L.VMX_ERR_NO_DEVICE and "no CPU path" in _err(hip_lib)
    else:
        refused((rec, 8, now, prev, nrm, 1, out, 0, None), "not device memory")


def test_accumulate_motion_checks_do_not_need_a_gpu(hip_lib):
    """the new entry makes vmx_temporal_accumulate_device's checks in its order, d_motion's alignment beside d_rayhit's"""
    acc = hip_lib.vmx_temporal_accumulate_motion_device
    buf = np.zeros(8 * 8 * 16 + 4, np.float32)
    ptr = (buf.ctypes.data + 15) & ~15
    cam = va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 16)

    def refused(args, what):
        assert acc(*args) == L.VMX_ERR_INVALID, what
        assert what in _err(hip_lib), (what, _err(hip_lib))

    for mv in (None, ptr):
        refused((None, C.byref(cam), ptr, mv, ptr, ptr, None, None, None, None), "NULL handle")
        refused((None, C.byref(cam), ptr, mv, ptr, None, None, None, None, None), "no output")
        refused((None, C.byref(cam), ptr, mv, ptr, None, None, ptr, None, None), "no output")
        refused((None, None, ptr, mv, ptr, ptr, None, None, None, None), "NULL camera")
        refused((None, C.byref(cam), None, mv, ptr, ptr, None, None, None, None), "NULL d_rayhit")
        refused((None, C.byref(cam), ptr, mv, None, ptr, None, None, None, None), "NULL d_in_rgbaz")
        refused((None, C.byref(cam), ptr + 4, mv, ptr, ptr, None, None, None, None), "d_rayhit must be 16-byte")
        refused((None, C.byref(cam), ptr, mv, ptr + 2, ptr, None, None, None, None), "4-byte")
        p = va.make_temporal_params(plane_tol=0.0)
        refused((None, C.byref(cam), ptr, mv, ptr, ptr, None, None, C.byref(p), None), "plane_tol")
        bad_cam = va.make_camera((0, 0, 0), (0, 0, 0), 8, 8, 3)
        refused((None, C.byref(bad_cam), ptr, mv, ptr, ptr, None, None, None, None), "rays_per_pixel < 4")
    for off in (4, 8, 12):
        refused((None, C.byref(cam), ptr, ptr + off, ptr, ptr, None, None, None, None), "d_motion must be 16-byte aligned")


def test_stand_alone_argument_checks_build_and_pass(tmp_path):
    """tests/cpp/motion_args.cpp, the program tools/host_asan_args.sh runs under the host sanitizers, built plainly: the
    same checks through the C header, from C++"""
    exe = tmp_path / "motion_args"
    so_dir = os.path.join(ROOT, "vermilion_amd")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "motion_args.cpp"), os.path.join(so_dir, "libvermilion_hip.so"),
                    "-Wl,-rpath," + so_dir, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "clean" in run.stdout, run.stderr


class NoLib:  # any call into the library fails the test
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_layer_rejects_bad_tensors_before_the_library(monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(L, "lib", lambda: NoLib())

    class OnDevice:  # a tensor that passes every check: the later arguments are reached
        def __init__(self, shape, dtype):
            self.shape, self.dtype, self.device = shape, dtype, torch.device("cuda", 0)

        def data_ptr(self):
            return 0

        def is_contiguous(self):
            return True

    OnDevice.__module__ = "torch"
    cuda0 = re.escape("cuda:0")
    # Temporal.accumulate(motion=...)
    t = va.Temporal.__new__(va.Temporal)
    t._lib, t._h, t.device, t.shape = NoLib(), None, 0, (41, 70)
    cam = va.make_camera((0, 0, 0), (0, 0, 0), 70, 41, 16)
    ok_raw, ok_frame = OnDevice((41, 70, 16), torch.float32), OnDevice((41, 70, 5), torch.float32)
    with pytest.raises(ValueError, match="motion must be a torch tensor"):
        t.accumulate(cam, ok_raw, ok_frame, motion=np.zeros((41, 70, 8), np.float32))
    with pytest.raises(ValueError, match="motion must be torch.float32"):
        t.accumulate(cam, ok_raw, ok_frame, motion=torch.zeros((41, 70, 8), dtype=torch.int32))
    with pytest.raises(ValueError, match=r"motion must be \[41, 70, 8\]"):
        t.accumulate(cam, ok_raw, ok_frame, motion=torch.zeros((41 * 70, 8)))
    with pytest.raises(ValueError, match="motion must be contiguous"):
        t.accumulate(cam, ok_raw, ok_frame, motion=torch.zeros((70, 41, 8)).transpose(0, 1))
    with pytest.raises(ValueError, match="motion must be on " + cuda0):
        t.accumulate(cam, ok_raw, ok_frame, motion=torch.zeros((41, 70, 8)))
    # motion_vectors
    raw, pos = torch.zeros((41, 70, 16)), torch.zeros((8, 9))
    with pytest.raises(ValueError, match="raw must be a torch tensor"):
        va.motion_vectors(np.zeros((41, 70, 16), np.float32), pos, pos)
    with pytest.raises(ValueError, match="raw must be torch.float32"):
        va.motion_vectors(raw.double(), pos, pos)
    with pytest.raises(ValueError, match=r"raw must be \[..., 16\]"):
        va.motion_vectors(torch.zeros((41, 70, 8)), pos, pos)
    with pytest.raises(ValueError, match="raw must be contiguous"):
        va.motion_vectors(torch.zeros((70, 41, 16)).transpose(0, 1), pos, pos)
    with pytest.raises(ValueError, match="raw must be on cuda"):
        va.motion_vectors(raw, pos, pos)
    ok_pos = OnDevice((8, 9), torch.float32)
    with pytest.raises(ValueError, match="pos_now must be a torch tensor"):
        va.motion_vectors(ok_raw, np.zeros((8, 9), np.float32), ok_pos)
    with pytest.raises(ValueError, match=r"pos_now must be \[ntris, 9\]"):
        va.motion_vectors(ok_raw, torch.zeros(72), ok_pos)
    with pytest.raises(ValueError, match=r"pos_now must be \[ntris, 9\]"):
        va.motion_vectors(ok_raw, torch.zeros((0, 9)), ok_pos)
    with pytest.raises(ValueError, match=r"pos_now must be \[8, 9\]"):
        va.motion_vectors(ok_raw, torch.zeros((8, 6)), ok_pos)
    with pytest.raises(ValueError, match="pos_now must be torch.float32"):
        va.motion_vectors(ok_raw, pos.double(), ok_pos)
    with pytest.raises(ValueError, match="pos_now must be on " + cuda0):
        va.motion_vectors(ok_raw, pos, ok_pos)
    with pytest.raises(ValueError, match="pos_prev must be a torch tensor"):
        va.motion_vectors(ok_raw, ok_pos, np.zeros((8, 9), np.float32))
    with pytest.raises(ValueError, match=r"pos_prev must be \[8, 9\]"):
        va.motion_vectors(ok_raw, ok_pos, torch.zeros((7, 9)))
    with pytest.raises(ValueError, match="pos_prev must be contiguous"):
        va.motion_vectors(ok_raw, ok_pos, torch.zeros((9, 8)).transpose(0, 1))
    with pytest.raises(ValueError, match="pos_prev must be on " + cuda0):
        va.motion_vectors(ok_raw, ok_pos, pos)
    with pytest.raises(ValueError, match=r"nrm_prev must be \[8, 9\]"):
        va.motion_vectors(ok_raw, ok_pos, ok_pos, nrm_prev=torch.zeros((8, 3)))
    with pytest.raises(ValueError, match="nrm_prev must be on " + cuda0):
        va.motion_vectors(ok_raw, ok_pos, ok_pos, nrm_prev=pos)
    with pytest.raises(ValueError, match=r"out must be \[41, 70, 8\]"):
        va.motion_vectors(ok_raw, ok_pos, ok_pos, out=torch.zeros((41, 70, 16)))
    with pytest.raises(ValueError, match="out must be torch.float32"):
        va.motion_vectors(ok_raw, ok_pos, ok_pos, out=torch.zeros((41, 70, 8), dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be on " + cuda0):
        va.motion_vectors(ok_raw, ok_pos, ok_pos, out=torch.zeros((41, 70, 8)))


# ---- the restatement's own conditions ----------------------------------------------------------------------------------
W, H = 70, 41


def _camera(i, step, spp):
    c = scenes.cornell_camera()
    p, r = c["position"], c["rotation_deg"]
    return va.make_camera((p[0] + step[0] * i, p[1], p[2]), (r[0], r[1] + step[1] * i, r[2]), W, H, spp)


def _oracle_frame(pos, nrm, uv, cam, seed):
    """(frame, records [H, W]) of the oracle on this geometry: 16 spp as the cases state them, the guide from sample 0's
    camera rays"""
    opts = va.make_opts(seed=seed, early_stop=False, sampling=L.VMX_SAMPLING_CORRECTED)
    osc = O.OracleScene(pos, nrm, uv)
    raw, _ = osc.render(cam, opts)
    o, d = O.primary_rays(cam, opts, 0)
    rec = osc.raycast(o, d).reshape(H, W)
    osc.close()
    return raw, rec


def _interior(rec):
    """pixels whose whole 5 x 5 neighbourhood lies on their own face (tri_id // 2), on a triangle of the block"""
    tri = np.where((rec["flags"] & 1) != 0, rec["tri_id"], -1)
    on_block = (tri >= MS.BLOCK.start) & (tri < MS.BLOCK.stop) & (rec["distance"] == rec["tri_t"])
    face = np.where(tri >= 0, tri // 2, -1)
    same = np.ones((H, W), bool)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            sh = np.full((H, W), -2)
            sh[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)] = \
                face[max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)]
            same &= sh == face
    return on_block, on_block & same


def _mse(a, conv, mask=None):
    d = (a[..., :3].astype(np.float64) - conv) ** 2
    return float(np.mean(d if mask is None else d[mask]))


def test_spec_static_world_is_temporal_spec_bit_for_bit():
    """over a whole sequence of a moving camera: step(motion=None) is temporal_spec.step, and so is step with the records
    of an update that moved nothing (motion(rec, pos, pos, nrm): no flag set, every record passed through)"""
    pos, nrm, uv = scenes.cornell8()
    a = b = c = None
    for i in range(4):
        cam = _camera(i, (6.0, 0.15), 16)
        frame, rec = _oracle_frame(pos, nrm, uv, cam, 3 + i)
        mv = MS.motion(rec, pos, pos, nrm)
        assert not bits(mv)[..., 3].any() and not bits(mv)[..., 7].any()
        assert np.array_equal(bits(mv)[..., 0:3], bits(rec["location"])) and np.array_equal(bits(mv)[..., 4:7], bits(rec["normal"]))
        want, a, want_n = TS.step(a, frame, rec, cam)
        for got in (MS.step(b, frame, rec, cam), MS.step(c, frame, rec, cam, mv)):
            assert np.array_equal(bits(got[0]), bits(want)) and np.array_equal(bits(got[2]), bits(want_n)), i
            for k in ("c", "n_h", "n", "z", "X"):
                assert np.array_equal(bits(got[1][k]), bits(a[k])), (i, k)
        b, c = MS.step(b, frame, rec, cam)[1], MS.step(c, frame, rec, cam, mv)[1]
    assert want_n.max() == 4


@pytest.mark.parametrize("case", list(MS.CASES))
def test_spec_quality_cap_on_a_moving_block(case):
    """8 frames of 16 spp of scenes.cornell8() at 70 x 41, corrected sampling, early stop off, frame i with seed 3 + i; the
    block (triangles 4..7) moves each frame (motion_spec.CASES: A +30 x +40 z, camera at rest; B the same with the camera
    stepping +6 x, +0.15 deg y; D +20 x +30 z and 0.04 rad about y, that camera).  The converged frame is the oracle's
    2048 spp, seed 1, at the last frame.  Moved pixels: those whose record lies on a moved triangle in the last frame;
    interior: the whole 5 x 5 neighbourhood on the same face.  On interior pixels the history length is <= 1.5 without
    motion records (a prototype measured exactly 1) and >= 7.9 with them (7.985-7.998); the error on moved pixels with
    motion is <= 0.25 x the error without (0.08-0.09), and the whole frame's error is below that without.  The caps
    stop a broken reprojection passing; they are no tuning targets."""
    shift, angle, cam_step = MS.CASES[case]
    pos0, nrm0, uv = scenes.cornell8()
    frames = 8
    with_mv = without = None
    prev = None
    for i in range(frames):
        pos, nrm = MS.moved_block(pos0, nrm0, shift, angle, i)
        cam = _camera(i, cam_step, 16)
        raw, rec = _oracle_frame(pos, nrm, uv, cam, 3 + i)
        mv = None if prev is None else MS.motion(rec, pos, prev[0], prev[1])
        acc_mv, with_mv, hist_mv = MS.step(with_mv, raw, rec, cam, mv)
        acc_no, without, hist_no = MS.step(without, raw, rec, cam)
        prev = (pos, nrm)
    osc = O.OracleScene(pos, nrm, uv)
    conv, _ = osc.render(_camera(frames - 1, cam_step, 2048), va.make_opts(seed=1, early_stop=False, sampling=L.VMX_SAMPLING_CORRECTED))
    osc.close()
    conv = conv[..., :3].astype(np.float64)
    moved, interior = _interior(rec)
    assert interior.sum() > 50, interior.sum()
    flagged = (bits(mv)[..., 3] & 1) != 0
    assert np.array_equal(flagged, moved)  # exactly the records on the block carry the flag
    static = ~moved
    assert np.array_equal(bits(mv)[static][:, 0:3], bits(rec["location"])[static])
    mse = {k: (_mse(a, conv, moved), _mse(a, conv)) for k, a in (("raw", raw), ("without", acc_no), ("with", acc_mv))}
    print(f"case {case}: interior pixels {int(interior.sum())} of {int(moved.sum())} moved; history on interior without "
          f"{hist_no[interior].mean():.3f} (max {hist_no[interior].max():.3f}), with {hist_mv[interior].mean():.3f} "
          f"(min {hist_mv[interior].min():.3f}); mse on moved px raw / without / with "
          f"{mse['raw'][0]:.4f} / {mse['without'][0]:.4f} / {mse['with'][0]:.4f}; whole frame without / with "
          f"{mse['without'][1]:.4f} / {mse['with'][1]:.4f}")
    assert hist_no[interior].max() <= 1.5
    assert hist_mv[interior].min() >= 7.9
    assert mse["with"][0] <= 0.25 * mse["without"][0]
    assert mse["with"][1] < mse["without"][1]


def _sliding_quad(offset):
    """12 x 9 records of a camera at the origin looking down -z at a quad of two triangles in the plane z = -4 (one world
    unit per pixel, far wider than the image) that has slid by `offset` in x, within its own plane: (camera, records,
    positions [2, 9], normals [2, 9]).  The records are the same wherever the quad is: that is the point."""
    cam = va.make_camera((0, 0, 0), (0, 0, 0), 12, 9, 16, back_distance=1.0, back_size=(3.0, 2.25))
    pos, nrm, _ = scenes._finish(*scenes._quad((-20 + offset, -20, -4), (20 + offset, -20, -4), (20 + offset, 20, -4),
                                               (-20 + offset, 20, -4), (0, 0, -1)))  # (a record's normal is the negated interpolation)
    rec = np.zeros((9, 12, 16), np.float32)
    ys, xs = np.meshgrid(np.arange(9), np.arange(12), indexing="ij")
    rec[..., 0] = xs + 0.5 - 6.0
    rec[..., 1] = -(ys + 0.5 - 4.5)
    rec[..., 2] = -4.0
    rec[..., 3] = rec[..., 10] = np.sqrt(rec[..., 0] ** 2 + rec[..., 1] ** 2 + 16.0)
    rec[..., 6] = 1.0
    # triangle 0 is (p00, p10, p11), below the diagonal y - y0 = x - x0; triangle 1 the other half
    rec.view(np.uint32)[..., 7] = np.where(rec[..., 1] + 20 <= rec[..., 0] - (-20 + offset), 0, 1)
    rec.view(np.uint32)[..., 11] = 3
    return cam, rec, pos, nrm


def test_spec_in_plane_slide_takes_the_moved_history():
    """a face that slides within its own plane passes the normal and the plane test wherever it is looked up: without
    motion records column x keeps its own history, which belongs to the surface point one unit along; with them column x
    carries the history of column x - 1, where its surface point was (the quad moved +1 in x, one pixel), and column 0,
    whose point was outside the image, restarts.  The history colours are a ramp by column, the new frame is black: what
    is left of a pixel is half of the history it took."""
    cam, rec1, pos1, nrm1 = _sliding_quad(0.0)
    _, rec2, pos2, _ = _sliding_quad(1.0)
    ramp = (np.arange(12, dtype=np.float32) + 1) / 16
    hist = np.zeros((9, 12, 5), np.float32)
    hist[..., 0] = ramp
    new = np.zeros((9, 12, 5), np.float32)
    _, state, _ = MS.step(None, hist, rec1, cam)
    mv = MS.motion(rec2, pos2, pos1, nrm1)
    assert np.all(bits(mv)[..., 3] == 1)
    assert np.abs(mv[..., 0] - (rec2[..., 0] - 1)).max() < 1e-5 and np.abs(mv[..., 1:3] - rec2[..., 1:3]).max() < 1e-5
    assert np.abs(mv[..., 4:7] - rec2[..., 4:7]).max() < 1e-6
    out, _, n = MS.step(state, new, rec2, cam, mv)
    assert np.all(n[:, 1:] == 2) and np.all(n[:, 0] == 1)
    assert np.abs(out[:, 1:, 0] - ramp[:-1] / 2).max() < 1e-5
    assert np.array_equal(bits(out[:, 0]), bits(new[:, 0]))
    same, _, n = MS.step(state, new, rec2, cam)
    assert np.all(n == 2) and np.array_equal(bits(same[..., 0]), bits(np.broadcast_to(ramp / 2, (9, 12))))


@pytest.mark.parametrize("ntris", [1, 8])
def test_spec_motion_edge_cases(ntris):
    """every kind of record that is not on a moved, non-degenerate triangle of the arrays leaves with the flag clear and
    its location and normal bitwise; zero previous normals leave the flag set and the normal as the record's; a regular
    record's point is where float64 barycentrics put it, and its normal the negated, normalised interpolation"""
    rec, pos_now, pos_prev, nrm_prev, kind = MS.synthetic_records(1000, ntris, 5)
    rw = bits(rec)
    assert set(kind) >= {"regular", "miss", "no_triangle", "sphere_nearer", "id_ntris", "id_ntris_plus_1", "id_minus_2",
                         "nan_location"}
    if ntris >= 8:
        assert set(kind) >= {"unmoved", "degenerate", "zero_normals"}
    for nrm in (None, nrm_prev):
        w = bits(MS.motion(rec, pos_now, pos_prev, nrm))
        assert not w[..., 7].any()
        for k in sorted(set(kind)):
            m = kind == k
            if k in MS.FLAGGED:
                assert np.all(w[m, 3] == 1), k
            else:
                assert not w[m, 3].any(), k
                assert np.array_equal(w[m, 0:3], rw[m, 0:3]) and np.array_equal(w[m, 4:7], rw[m, 4:7]), k
        keep = (kind == "zero_normals") if nrm is not None else np.isin(kind, MS.FLAGGED)
        assert np.array_equal(w[keep, 4:7], rw[keep, 4:7])
        # against float64: the point with the same barycentrics in the previous triangle
        m = kind == "regular"
        tid = rw[m, 7].view(np.int32)
        a = pos_now[tid].astype(np.float64).reshape(-1, 3, 3)
        q = pos_prev[tid].astype(np.float64).reshape(-1, 3, 3)
        P = rec[m, 0:3].astype(np.float64)
        b12 = np.stack([np.linalg.lstsq(np.stack([a[i, 1] - a[i, 0], a[i, 2] - a[i, 0]], axis=1), P[i] - a[i, 0], rcond=None)[0]
                        for i in range(len(P))])
        want = q[:, 0] + b12[:, :1] * (q[:, 1] - q[:, 0]) + b12[:, 1:] * (q[:, 2] - q[:, 0])
        got = w[m, 0:3].view(np.float32)
        assert np.abs(got - want).max() < 1e-3, np.abs(got - want).max()
        if nrm is not None:
            nn = nrm_prev[tid].astype(np.float64).reshape(-1, 3, 3)
            mm = nn[:, 0] + b12[:, :1] * (nn[:, 1] - nn[:, 0]) + b12[:, 1:] * (nn[:, 2] - nn[:, 0])
            ok = np.linalg.norm(mm, axis=1) > 0.05  # (an interpolated normal near zero amplifies the rounding of b)
            want_n = -mm / np.linalg.norm(mm, axis=1, keepdims=True)
            assert ok.mean() > 0.9 and np.abs(w[m, 4:7].view(np.float32) - want_n)[ok].max() < 1e-3
    # an update that moved nothing sets no flag anywhere
    w = bits(MS.motion(rec, pos_now, pos_now, nrm_prev))
    assert not w[..., 3].any() and np.array_equal(w[..., 0:3], rw[..., 0:3]) and np.array_equal(w[..., 4:7], rw[..., 4:7])
