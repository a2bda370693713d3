"""Motion records on the device (vmx_motion_device, vmx_temporal_accumulate_motion_device): every output word — the motion
records, the accumulated frame, the history lengths, the rgba8 form — is compared with the float32 restatement
(tests/motion_spec.py) fed the same sequence of calls, as uint32 bits; NaN may appear only where the restatement has NaN.

Shapes: 1000 synthetic records (no multiple of a wave or a block) over 1 and 8 triangles; the 8-triangle Cornell set at
70x41 with its block moving and the lattice at 64x48 with every triangle moving, four frames of 16 spp each; 5x3, 1x1,
257x1 and 1x130 for images smaller than a block, one pixel wide or one pixel high."""
import ctypes as C

import numpy as np
import pytest

import filter_spec as FS
import motion_spec as MS
import oracle_lib as O
import temporal_spec as TS
import vermilion_amd as va
from test_gpu_temporal import PARAMS  # the three parameter sets of the accumulator's own tests
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
W, H = 70, 41


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared inputs are read-only)


def lib_params(p):
    return None if p is None else va.make_temporal_params(**p)


def inside_nan(a, pad):
    """a device copy of `a` that is a view `pad` words into a larger NaN-filled tensor: a kernel that read a triangle it
    should not have reads NaN, inside the allocation"""
    import torch
    big = torch.full((a.size + 2 * pad,), float("nan"), dtype=torch.float32, device="cuda")
    view = big[pad:pad + a.size].view(*a.shape)
    view.copy_(torch.from_numpy(np.array(a, order="C")))
    return view


@pytest.mark.parametrize("ntris", [1, 8])
def test_synthetic_records_are_the_restatement_bit_for_bit(ntris):
    """the records of test_motion_abi's edge cases, with and without previous normals; ids ntris, ntris + 1, -2 and -1,
    misses and records on a sphere must not read the arrays at all: around them is NaN"""
    import torch
    rec, pos_now, pos_prev, nrm_prev, kind = MS.synthetic_records(1000, ntris, 5)
    d_rec = dev(rec)
    # (37 and 1019 words: the arrays are 4-byte aligned and no more; ntris + 1 and -2 stay inside the padding)
    d_now, d_prev, d_nrm = inside_nan(pos_now, 37), inside_nan(pos_prev, 1019), inside_nan(nrm_prev, 37)
    assert d_now.data_ptr() % 16 and d_prev.data_ptr() % 16
    for nrm, d_n in ((None, None), (nrm_prev, d_nrm)):
        want = MS.motion(rec, pos_now, pos_prev, nrm)
        out = torch.full((1000 + 8, 8), float("nan"), dtype=torch.float32, device="cuda")
        got = va.motion_vectors(d_rec, d_now, d_prev, d_n, out=out[:1000])
        assert got.data_ptr() == out.data_ptr()
        assert FS.same_bits(got.cpu().numpy(), want), int((bits(got.cpu().numpy()) != bits(want)).any(axis=-1).sum())
        assert torch.isnan(out[1000:]).all()  # nothing written past record n - 1
        flagged = (bits(want)[:, 3] & 1) != 0
        assert np.array_equal(flagged, np.isin(kind, MS.FLAGGED))
    # a made output, other leading shapes, and n == 0
    got = va.motion_vectors(d_rec.view(10, 100, 16), d_now, d_prev, d_nrm)
    assert tuple(got.shape) == (10, 100, 8) and FS.same_bits(got.cpu().numpy().reshape(1000, 8), want)
    assert tuple(va.motion_vectors(d_rec[:0], d_now, d_prev).shape) == (0, 8)
    torch.cuda.synchronize()


def moved_camera(c, w, h, i=0, step=(0.0, 0.0), spp=16):
    p, r = c["position"], c["rotation_deg"]
    return va.make_camera((p[0] + step[0] * i, p[1], p[2]), (r[0], r[1] + step[1] * i, r[2]), w, h, spp)


def moving_sequence(tris, c, w, h, geometry, cam_step, frames=4):
    """[(cam, frame [H, W, 5], records [H, W, 16], motion [H, W, 8] or None, positions)] of a scene whose geometry of frame i
    is geometry(i) = (pos, nrm): Scene.update (device tensors, refit), raycast_camera, motion_vectors, render; frame i with
    seed 3 + i.  The motion records are the device's, checked here against the restatement; never written to."""
    pos0, nrm0, uv = tris
    out, prev = [], None
    with va.Scene(pos0, nrm0, uv) as sc:
        for i in range(frames):
            pos, nrm = geometry(i)
            d_pos, d_nrm = dev(pos), dev(nrm)
            if i:
                sc.update(pos=d_pos, nrm=d_nrm)
            cam = moved_camera(c, w, h, i, cam_step)
            opts = va.make_opts(seed=3 + i, early_stop=False, sampling=va.VMX_SAMPLING_CORRECTED)
            d_raw = sc.raycast_camera(cam, opts, 0)["raw"]
            mv = None
            if prev is not None:
                mv = va.motion_vectors(d_raw, d_pos, prev[0], prev[1]).cpu().numpy()
            img, _ = sc.render(cam, opts)
            raw = d_raw.cpu().numpy()
            if mv is not None:
                assert FS.same_bits(mv, MS.motion(raw, pos, prev[2], prev[3])), ("motion records", i)
                mv.setflags(write=False)
            img.setflags(write=False), raw.setflags(write=False)
            out.append((cam, img, raw, mv, pos))
            prev = (d_pos, d_nrm, pos, nrm)
    return out


@pytest.fixture(scope="module")
def sequences():
    """case -> four frames, computed once: the Cornell block of cases A and D, and the lattice with every triangle turned
    by 0.02 rad about y (through the origin) and moved by (15, 5, -10) per frame under a slowly stepping camera"""
    out = {}
    pos0, nrm0, uv = scenes.cornell8()
    for case in ("A", "D"):
        shift, angle, cam_step = MS.CASES[case]
        out[case] = moving_sequence((pos0, nrm0, uv), scenes.cornell_camera(), W, H,
                                    lambda i: MS.moved_block(pos0, nrm0, shift, angle, i), cam_step)
    lp, ln, luv = scenes.lattice()

    def lattice_at(i):
        P, N = np.array(lp, np.float64).reshape(-1, 3), np.array(ln, np.float64).reshape(-1, 3)
        c, s = np.cos(0.02 * i), np.sin(0.02 * i)
        R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
        return ((P @ R.T + i * np.array([15.0, 5.0, -10.0])).reshape(-1, 9).astype(np.float32),
                (N @ R.T).reshape(-1, 9).astype(np.float32))

    out["lattice"] = moving_sequence((lp, ln, luv), scenes.lattice_camera(), 64, 48, lattice_at, (6.0, 0.15))
    return out


class Pair:
    """a handle and the restatement, fed the same calls: `step` makes one on both and compares every output"""

    def __init__(self, w, h):
        self.t = va.Temporal(w, h)
        self.w, self.h = w, h
        self.state = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.t.close()

    def reset(self):
        self.t.reset()
        self.state = None

    def step(self, cam, frame, raw, mv, params=None, tag=None, in_place=False):
        import torch
        want, self.state, want_n = MS.step(self.state, frame, raw, cam, mv, params)
        hist = torch.empty((self.h, self.w), dtype=torch.float32, device="cuda")
        q = torch.empty((self.h, self.w, 4), dtype=torch.uint8, device="cuda")
        src = dev(frame)
        dst = src if in_place else torch.empty((self.h, self.w, 5), device="cuda")
        d_mv = None if mv is None else dev(mv)
        out, q = self.t.accumulate(cam, dev(raw), src, rgba8=q, out=dst, history=hist, params=lib_params(params), motion=d_mv)
        assert out is dst
        got = out.cpu().numpy()
        assert FS.same_bits(got, want), (tag, int((bits(got) != bits(want)).any(axis=-1).sum()), "pixels differ")
        assert FS.same_bits(hist.cpu().numpy(), want_n), (tag, "history lengths differ")
        # (the conversion to a byte is defined for finite values in 0..1 only: pixels outside are left out on purpose)
        ok = np.all(np.isfinite(want[..., :4]) & (want[..., :4] >= 0) & (want[..., :4] <= 1), axis=-1)
        assert np.array_equal(q.cpu().numpy()[ok], O.quantize(want)[0].reshape(self.h, self.w, 4)[ok]), (tag, "rgba8")
        if not in_place:
            assert np.array_equal(bits(src.cpu().numpy()), bits(frame))  # the input is left alone
        if d_mv is not None:
            assert np.array_equal(bits(d_mv.cpu().numpy()), bits(mv))  # the records are read only
        return want, want_n, ok


def interior_of(raw, moved_tris):
    """(moved, interior): pixels whose record lies on one of `moved_tris`, and those of them whose whole 5 x 5
    neighbourhood lies on the same face (tri_id // 2)"""
    w = bits(raw)
    h, wd = w.shape[:2]
    tri = np.where((w[..., 11] & 1) != 0, w[..., 7].view(np.int32), -1)
    moved = np.isin(tri, moved_tris) & (w[..., 3] == w[..., 10])
    face = np.where(tri >= 0, tri // 2, -1)
    same = np.ones((h, wd), bool)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            sh = np.full((h, wd), -2)
            sh[max(0, -dy):h - max(0, dy), max(0, -dx):wd - max(0, dx)] = \
                face[max(0, dy):h - max(0, -dy), max(0, dx):wd - max(0, -dx)]
            same &= sh == face
    return moved, moved & same


@pytest.mark.parametrize("in_place", [False, True], ids=["out of place", "in place"])
@pytest.mark.parametrize("case", ["A", "D"])
def test_moving_block_is_the_restatement_bit_for_bit(sequences, case, in_place):
    """four frames of the Cornell set with its block moving (cases A and D of test_motion_abi's quality caps), at the
    defaults and two further parameter sets; on interior pixels of the block the history after four frames is >= 3.9 with
    motion records and <= 1.5 without"""
    seq = sequences[case]
    with Pair(W, H) as p:
        for prm in PARAMS:
            p.reset()
            for i, (cam, frame, raw, mv, _) in enumerate(seq):
                want, n, ok = p.step(cam, frame, raw, mv, prm, (case, prm, i), in_place)
                assert ok.all()
                assert p.t.frames() == i + 1
            assert not np.array_equal(bits(want[..., :3]), bits(frame[..., :3]))
            if prm is None:
                moved, interior = interior_of(raw, np.arange(MS.BLOCK.start, MS.BLOCK.stop))
                assert interior.sum() > 50 and np.array_equal(moved, (bits(mv)[..., 3] & 1) != 0)
                print(f"case {case}: history on {int(interior.sum())} interior moved pixels with motion: min {n[interior].min():.3f}")
                assert n[interior].min() >= 3.9
                p.reset()
                for i, (cam, frame, raw, mv, _) in enumerate(seq):
                    _, n_without, _ = p.step(cam, frame, raw, None, None, (case, "without", i), in_place)
                print(f"case {case}: without: max {n_without[interior].max():.3f}")
                assert n_without[interior].max() <= 1.5


def test_every_triangle_moving(sequences):
    """the lattice at 64 x 48 turning and moving as a whole under a moving camera: every record on a triangle carries the
    flag (a tilted quad that moves less than the plane tolerance along its normal keeps some history without the records
    too: the lengths are printed, not compared)"""
    seq = sequences["lattice"]
    with Pair(64, 48) as p:
        for prm in (None, PARAMS[2]):
            p.reset()
            for i, (cam, frame, raw, mv, _) in enumerate(seq):
                want, n, ok = p.step(cam, frame, raw, mv, prm, ("lattice", prm, i))
                assert ok.all()
        hit, _ = interior_of(raw, np.arange(len(seq[0][4])))
        assert np.array_equal((bits(mv)[..., 3] & 1) != 0, hit) and hit.sum() > 100
        p.reset()
        for cam, frame, raw, mv, _ in seq:
            _, n_with, _ = p.step(cam, frame, raw, mv)
        p.reset()
        for cam, frame, raw, mv, _ in seq:
            _, n_without, _ = p.step(cam, frame, raw, None)
        print(f"lattice: mean history on {int(hit.sum())} pixels on triangles with motion {n_with[hit].mean():.3f}, without "
              f"{n_without[hit].mean():.3f}")


def quad_case(rng, w, h, cx, offset, miss_share=0.25):
    """a synthetic call: a camera at (cx, 0, 0) looking down -z at a quad of two triangles in the plane z = -4, one world
    unit per pixel, that has slid by `offset` in x: records of points of that plane near each pixel's centre with the id of
    the triangle they lie in, most normals +z and the rest random, some rays missing; a frame of uniform colours.
    Returns (cam, frame, records, positions [2, 9], normals [2, 9])."""
    cam = va.make_camera((cx, 0, 0), (0, 0, 0), w, h, 16, back_distance=1.0, back_size=(w / 4, h / 4))
    x0 = -300.0 + offset
    pos, nrm, _ = scenes._finish(*scenes._quad((x0, -300, -4), (x0 + 600, -300, -4), (x0 + 600, 300, -4), (x0, 300, -4),
                                               (0, 0, -1)))
    rec = np.zeros((h, w, 16), np.float32)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rec[..., 0] = cx + (xs + 0.5 - w / 2) + rng.uniform(-0.2, 0.2, (h, w))
    rec[..., 1] = -(ys + 0.5 - h / 2) + rng.uniform(-0.2, 0.2, (h, w))
    rec[..., 2] = -4.0
    rec[..., 3] = rec[..., 10] = np.sqrt((rec[..., 0] - cx) ** 2 + rec[..., 1] ** 2 + 16.0)
    n = rng.normal(size=(h, w, 3))
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    n[rng.uniform(size=(h, w)) < 0.8] = (0, 0, 1)
    rec[..., 4:7] = n
    rec.view(np.uint32)[..., 7] = np.where(rec[..., 1] + 300 <= rec[..., 0] - x0, 0, 1)
    hit = rng.uniform(size=(h, w)) >= miss_share
    rec[..., 3][~hit] = np.inf
    rec.view(np.uint32)[..., 11] = np.where(hit, 3, 2)
    frame = rng.uniform(0, 1, (h, w, 5)).astype(np.float32)
    return cam, frame, rec, pos, nrm


@pytest.mark.parametrize("w,h", [(5, 3), (1, 1), (257, 1), (1, 130)])
def test_degenerate_shapes(w, h):
    """synthetic frames and records of a quad that slides by whole and fractional pixels under a camera that steps too"""
    rng = np.random.RandomState(w * 1000 + h)
    with Pair(w, h) as p:
        for prm in (None, dict(normal_min=-1.0, plane_tol=10.0, max_history=3.0)):
            p.reset()
            taken, prev = 0, None
            for i, (cx, off) in enumerate(((0, 0), (0.3, 1.0), (0.3, 1.0), (1.3, 0.5), (-0.75, 0.5), (0.25, -1.25))):
                cam, frame, rec, pos, nrm = quad_case(rng, w, h, cx, off, 0.0 if w * h == 1 else 0.25)
                mv = None
                if prev is not None:
                    mv = va.motion_vectors(dev(rec), dev(pos), dev(prev[0]), dev(prev[1])).cpu().numpy()
                    assert FS.same_bits(mv, MS.motion(rec, pos, prev[0], prev[1])), (w, h, i)
                _, n, ok = p.step(cam, frame, rec, mv, prm, (w, h, prm, i))
                assert ok.all()
                taken += int((n > 1).sum())
                prev = (pos, nrm)
            assert taken > 0  # (some history was taken)


def test_without_records_and_with_clear_records_is_the_old_entry(sequences):
    """vmx_temporal_accumulate_motion_device with d_motion == NULL, and with the records of an update that moved nothing
    (every flag clear), writes what vmx_temporal_accumulate_device writes, bit for bit"""
    import torch
    seq = sequences["D"]
    P = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="cuda")  # noqa: E731
    with va.Temporal(W, H) as old, va.Temporal(W, H) as null, va.Temporal(W, H) as clear:
        lib = old._lib
        for i, (cam, frame, raw, _, pos) in enumerate(seq):
            d_raw, d_pos, d_frame = dev(raw), dev(pos), dev(frame)
            mv = va.motion_vectors(d_raw, d_pos, d_pos)
            assert not bits(mv.cpu().numpy())[..., 3].any()
            outs = []
            for t, how in ((old, "old"), (null, "null"), (clear, "clear")):
                out, q, hist = new(H, W, 5), new(H, W, 4, dtype=torch.uint8), new(H, W)
                if how == "old":
                    rc = lib.vmx_temporal_accumulate_device(t._h, C.byref(cam), P(d_raw), P(d_frame), P(out), P(q), P(hist),
                                                            None, None)
                else:
                    rc = lib.vmx_temporal_accumulate_motion_device(t._h, C.byref(cam), P(d_raw), P(mv if how == "clear" else None),
                                                                   P(d_frame), P(out), P(q), P(hist), None, None)
                assert rc == L.VMX_OK, lib.vmx_last_error().decode()
                torch.cuda.synchronize()
                outs.append((out.cpu().numpy(), q.cpu().numpy(), hist.cpu().numpy()))
            for other in outs[1:]:
                for a, b in zip(outs[0], other):
                    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), i
        assert outs[0][2].max() > 1
        want = None
        for cam, frame, raw, _, _ in seq:
            w_frame, want, w_n = TS.step(want, frame, raw, cam)
        assert FS.same_bits(outs[0][0], w_frame) and FS.same_bits(outs[0][2], w_n)


def test_refusals(sequences):
    import torch
    seq = sequences["A"]
    P = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
    with Pair(W, H) as p:
        t, lib = p.t, p.t._lib
        made = []

        def still_works():
            cam, frame, raw, mv, _ = seq[len(made) % len(seq)]
            p.step(cam, frame, raw, mv, None, "after a refusal")
            made.append(1)

        def refused(call, match):
            with pytest.raises(va.VmxError, match=match) as e:
                call()
            assert e.value.code == L.VMX_ERR_INVALID
            still_works()

        still_works()
        cam, frame, raw, mv, pos = seq[1]
        src, rec, out = dev(frame), dev(raw), torch.empty((H, W, 5), device="cuda")
        # the records inside a buffer the call writes: the frame, the bytes, the history lengths
        buf = torch.zeros(W * H * 8 + 8, dtype=torch.float32, device="cuda")
        inside = buf[:W * H * 8].view(H, W, 8)
        refused(lambda: t.accumulate(cam, rec, src, out=buf[4:4 + W * H * 5].view(H, W, 5), motion=inside), "overlap")
        refused(lambda: t.accumulate(cam, rec, src, rgba8=buf[8:8 + W * H].view(torch.uint8).view(H, W, 4), motion=inside), "overlap")
        refused(lambda: t.accumulate(cam, rec, src, out=out, history=buf[W * H * 7:W * H * 8].view(H, W), motion=inside), "overlap")
        # ... but they may be the input's neighbours, and overlap what is read
        t.accumulate(cam, rec, src, out=out, motion=rec.view(-1)[:W * H * 8].view(H, W, 8))
        p.reset()
        made.clear()
        still_works()
        # host pointers, straight through the C ABI
        host = np.zeros(W * H * 8 + 4, np.float32)
        hp = C.c_void_p((host.ctypes.data + 15) & ~15)
        assert lib.vmx_temporal_accumulate_motion_device(t._h, C.byref(cam), P(rec), hp, P(src), P(out), None, None, None,
                                                         None) == L.VMX_ERR_INVALID
        assert "d_motion is not device memory" in lib.vmx_last_error().decode()
        still_works()
        assert lib.vmx_temporal_accumulate_motion_device(t._h, C.byref(cam), P(rec), C.c_void_p(buf.data_ptr() + 4), P(src),
                                                         P(out), None, None, None, None) == L.VMX_ERR_INVALID
        assert "d_motion must be 16-byte aligned" in lib.vmx_last_error().decode()
        still_works()
        assert p.t.frames() == len(made)  # the refused calls did not count
        d_pos, d_out = dev(pos), torch.empty((H, W, 8), device="cuda")
        for args, what in (((hp, W * H, P(d_pos), P(d_pos), None, 8, P(d_out)), "d_rayhit is not device memory"),
                           ((P(rec), W * H, hp, P(d_pos), None, 8, P(d_out)), "d_pos_now is not device memory"),
                           ((P(rec), W * H, P(d_pos), hp, None, 8, P(d_out)), "d_pos_prev is not device memory"),
                           ((P(rec), W * H, P(d_pos), P(d_pos), hp, 8, P(d_out)), "d_nrm_prev is not device memory"),
                           ((P(rec), W * H, P(d_pos), P(d_pos), None, 8, hp), "d_out is not device memory"),
                           ((P(rec), W * H, P(d_pos), P(d_pos), None, 8, P(rec)), "d_out overlaps")):
            assert lib.vmx_motion_device(*args, 0, None) == L.VMX_ERR_INVALID
            assert what in lib.vmx_last_error().decode(), (what, lib.vmx_last_error().decode())
        assert lib.vmx_motion_device(P(rec), W * H, P(d_pos), P(d_pos), None, 8, P(d_out), 1 << 20, None) == L.VMX_ERR_NO_DEVICE
        with pytest.raises(va.VmxError, match="d_out overlaps"):
            va.motion_vectors(rec, d_pos, d_pos, out=rec.view(-1)[:W * H * 8].view(H, W, 8))
        torch.cuda.synchronize()
