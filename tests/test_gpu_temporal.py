"""Temporal accumulation on the device (vmx_temporal_*): every output — the accumulated frame, the history lengths, the
rgba8 form — is compared with the float32 restatement (tests/temporal_spec.py) fed the same sequence of calls, as uint32
bits, every pixel, after every frame; NaN may appear only where the restatement has NaN.

Shapes: the 8-triangle Cornell set at 70x41 (three blocks across, six down, the last of each partial) and the lattice
at 64x48, both at 16 spp; 5x3, 1x1, 257x1 and 1x130 for images smaller than a block, one pixel wide or one pixel high."""
import ctypes as C

import numpy as np
import pytest

import filter_spec as FS
import oracle_lib as O
import temporal_spec as TS
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
W, H = 70, 41
MOTIONS = {"static": (0.0, 0.0), "slow": (6.0, 0.15), "fast": (25.0, 0.6)}
PARAMS = (None, dict(normal_min=0.5, plane_tol=0.1, max_history=2.0), dict(normal_min=-1.0, plane_tol=1e-4, max_history=1000.0))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared inputs are read-only)


def lib_params(p):
    return None if p is None else va.make_temporal_params(**p)


def moved_camera(c, w, h, i=0, motion=(0.0, 0.0), spp=16):
    p, r = c["position"], c["rotation_deg"]
    return va.make_camera((p[0] + motion[0] * i, p[1], p[2]), (r[0], r[1] + motion[1] * i, r[2]), w, h, spp)


def light_spheres():
    """the two VMX_SPHERE_EMIT entries of the default table alone: about 30 % of the camera rays miss"""
    table = va.default_spheres()
    emit = [s for s in table if s.flags & L.VMX_SPHERE_EMIT]
    assert len(emit) == 2
    out = (L.Sphere * 2)()
    for i, s in enumerate(emit):
        C.memmove(C.byref(out[i]), C.byref(s), C.sizeof(L.Sphere))
    return out


def rendered(sc, cams, first_seed=3):
    """[(cam, frame [H, W, 5], records [H, W, 16])] through Scene.render and Scene.raycast_camera(k = 0), frame i with
    seed first_seed + i; never written to"""
    out = []
    for i, cam in enumerate(cams):
        opts = va.make_opts(seed=first_seed + i, early_stop=False, sampling=va.VMX_SAMPLING_CORRECTED)
        img, _ = sc.render(cam, opts)
        raw = sc.raycast_camera(cam, opts, 0)["raw"].cpu().numpy()
        img.setflags(write=False), raw.setflags(write=False)
        out.append((cam, img, raw))
    return out


@pytest.fixture(scope="module")
def sequences():
    """(scene, motion) -> four frames of 16 spp along the camera path, computed once"""
    out = {}
    for name, tris, c, (w, h) in (("cornell8", scenes.cornell8(), scenes.cornell_camera(), (W, H)),
                                  ("lattice", scenes.lattice(), scenes.lattice_camera(), (64, 48))):
        with va.Scene(*tris) as sc:
            for motion, mv in MOTIONS.items():
                out[name, motion] = rendered(sc, [moved_camera(c, w, h, i, mv) for i in range(4)])
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

    def check(self, want, want_n, out, q, hist, tag):
        if out is not None:
            got = out.cpu().numpy()
            assert FS.same_bits(got, want), (tag, int((bits(got) != bits(want)).any(axis=-1).sum()), "pixels differ")
        if hist is not None:
            assert FS.same_bits(hist.cpu().numpy(), want_n), (tag, "history lengths differ")
        if q is not None:
            # (the conversion to a byte is defined for finite values in 0..1 only: pixels outside are left out on purpose.
            # `ok` goes back to the caller: every pixel of a rendered or uniform frame, all but the seeded ones elsewhere)
            ok = np.all(np.isfinite(want[..., :4]) & (want[..., :4] >= 0) & (want[..., :4] <= 1), axis=-1)
            assert np.array_equal(q.cpu().numpy()[ok], O.quantize(want)[0].reshape(self.h, self.w, 4)[ok]), (tag, "rgba8")
            return ok
        return None

    def step(self, cam, frame, raw, params=None, tag=None):
        import torch
        want, self.state, want_n = TS.step(self.state, frame, raw, cam, params)
        hist = torch.empty((self.h, self.w), dtype=torch.float32, device="cuda")
        q = torch.empty((self.h, self.w, 4), dtype=torch.uint8, device="cuda")
        out, q = self.t.accumulate(cam, dev(raw), dev(frame), rgba8=q, out=torch.empty((self.h, self.w, 5), device="cuda"),
                                   history=hist, params=lib_params(params))
        ok = self.check(want, want_n, out, q, hist, tag)
        return want, want_n, ok


@pytest.mark.parametrize("motion", list(MOTIONS))
@pytest.mark.parametrize("name", ["cornell8", "lattice"])
def test_sequences_are_the_restatement_bit_for_bit(sequences, name, motion):
    """four frames along each camera path, at the defaults and two further parameter sets (a short history with loose
    tests; every normal accepted, a tight plane and no cap)"""
    seq = sequences[name, motion]
    h, w = seq[0][1].shape[:2]
    with Pair(w, h) as p:
        for prm in PARAMS:
            p.reset()
            for i, (cam, frame, raw) in enumerate(seq):
                want, n, ok = p.step(cam, frame, raw, prm, (name, motion, prm, i))
                assert ok.all()
                assert p.t.frames() == i + 1
            # it did accumulate: most pixels have a history, and the frame is no longer the last input
            assert (n > 1).mean() > 0.5, (n > 1).mean()
            assert not np.array_equal(bits(want[..., :3]), bits(frame[..., :3]))
            if motion == "static" and prm is None:
                # (each frame's guide ray has its own jitter: a pixel near an edge of the geometry may see another
                # surface and restart — the lattice is mostly edges; most pixels that were hit have all four frames)
                hit = (bits(raw)[..., 11] & 1) != 0
                assert (n[hit] == 4).mean() > 0.5 and n.max() == 4


def test_history_out_of_sight():
    """a pan wider than the image, and a camera turned by 180 degrees (the history lies behind it): no pixel has a valid
    history and the output is the input; a `lights_only` sphere table: hits and misses mixed along a path"""
    c = scenes.cornell_camera()
    far = dict(position=(c["position"][0] + 9000.0, c["position"][1], c["position"][2]), rotation_deg=c["rotation_deg"])
    back = dict(position=c["position"], rotation_deg=(0.0, 180.0, 0.0))
    with va.Scene(*scenes.cornell8()) as sc, Pair(W, H) as p:
        for other in (far, back):
            seq = rendered(sc, [moved_camera(c, W, H), moved_camera(other, W, H)])
            p.reset()
            for i, (cam, frame, raw) in enumerate(seq):
                want, n, ok = p.step(cam, frame, raw, None, (other, i))
                assert ok.all()
            assert np.all(n == 1) and np.array_equal(bits(want), bits(frame))
    with va.Scene(*scenes.cornell8(), spheres=light_spheres()) as sc, Pair(W, H) as p:
        seq = rendered(sc, [moved_camera(c, W, H, i, MOTIONS["slow"]) for i in range(3)])
        miss = (bits(seq[-1][2])[..., 11] & 1) == 0
        assert 0.15 < miss.mean() < 0.6, miss.mean()  # hits and misses are mixed
        for i, (cam, frame, raw) in enumerate(seq):
            want, n, ok = p.step(cam, frame, raw, None, ("lights_only", i))
        assert np.all(n[miss] == 1) and n.max() == 3
        assert np.array_equal(bits(want[miss]), bits(frame[miss]))


def plane_case(rng, w, h, cx, cy, miss_share=0.25):
    """a synthetic call: a camera at (cx, cy, 0) looking down -z at the plane z = -4, one world unit per pixel; records of
    points of that plane near each pixel's centre, most normals +z and the rest random, some rays missing; a frame of
    uniform colours"""
    cam = va.make_camera((cx, cy, 0), (0, 0, 0), w, h, 16, back_distance=1.0, back_size=(w / 4, h / 4))
    rec = np.zeros((h, w, 16), np.float32)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rec[..., 0] = cx + (xs + 0.5 - w / 2) + rng.uniform(-0.2, 0.2, (h, w))
    rec[..., 1] = cy - (ys + 0.5 - h / 2) + rng.uniform(-0.2, 0.2, (h, w))
    rec[..., 2] = -4.0
    rec[..., 3] = np.sqrt((rec[..., 0] - cx) ** 2 + (rec[..., 1] - cy) ** 2 + 16.0)
    nrm = rng.normal(size=(h, w, 3))
    nrm = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
    nrm[rng.uniform(size=(h, w)) < 0.8] = (0, 0, 1)
    rec[..., 4:7] = nrm
    hit = rng.uniform(size=(h, w)) >= miss_share
    rec[..., 3][~hit] = np.inf  # (a miss's record: distance INFINITY, a stale normal and location)
    rec.view(np.uint32)[..., 11] = np.where(hit, 3, 2)
    frame = rng.uniform(0, 1, (h, w, 5)).astype(np.float32)
    return cam, frame, rec


@pytest.mark.parametrize("w,h", [(5, 3), (1, 1), (257, 1), (1, 130)])
def test_degenerate_shapes(w, h):
    """synthetic frames and records along a path of whole and fractional pixel steps, back and forth"""
    rng = np.random.RandomState(w * 1000 + h)
    with Pair(w, h) as p:
        for prm in (None, dict(normal_min=-1.0, plane_tol=10.0, max_history=3.0)):
            p.reset()
            taken = 0
            for i, (cx, cy) in enumerate(((0, 0), (0.3, -0.6), (0.3, -0.6), (1.3, 0.4), (-0.75, 0.25), (0.25, 0.25))):
                cam, frame, rec = plane_case(rng, w, h, cx, cy, 0.0 if w * h == 1 else 0.25)
                _, n, ok = p.step(cam, frame, rec, prm, (w, h, prm, i))
                assert ok.all()
                taken += int((n > 1).sum())
            assert taken > 0  # (some history was taken)


def test_synthetic_records_over_two_calls():
    """Records a renderer would not write, in both calls of a 24 x 12 image whose camera moves by a fraction of a pixel.
    Rows: zero normals, NaN normals, NaN and inf locations, z of 1e-38 (its square is 0), 1e30 (its square is inf) and
    exactly 0, alternating hit and miss; a row whose history colours are 1e-38 and whose new colours are 0 (every weighted
    colour, their sum, the quotient and the output are denormal); a NaN and an inf colour, which spread to the pixels that take them as taps (an inf
    history blends to inf + -inf, a NaN).
    (A denormal tap WEIGHT cannot arise: u and w are W or H times a multiple of 2^-25, so a fraction fx, 1 - fx is 0
    or at least 2^-25 and a product of two at least 2^-50.)"""
    rng = np.random.RandomState(77)
    h, w = 12, 24
    calls = []
    for cx, cy in ((0.0, 0.0), (0.4, 0.0)):  # (no step in y: row 7 takes history from row 7 alone)
        cam, frame, rec = plane_case(rng, w, h, cx, cy, 0.0)
        rec[:, :, 4:7] = (0, 0, 1)
        rec[0, :, 4:7] = 0.0
        rec[1, :, 4:7] = np.nan
        rec[2, 0::3, 0] = np.nan
        rec[2, 1::3, 1] = np.inf
        rec[2, 2::3, 2] = -np.inf
        rec[3, :, 3] = np.float32(1e-38)
        rec[4, :, 3] = np.float32(1e30)
        rec[5, :, 3] = 0.0
        rec.view(np.uint32)[6, 0::2, 11] = 2
        calls.append((cam, frame, rec))
    calls[0][1][7, :, :3] = np.float32(1e-38)
    calls[1][1][7, :, :3] = 0  # (the second frame's own colours in row 7: what is left of a pixel is its history's share)
    calls[0][1][9, 3, 1] = np.nan
    calls[0][1][10, 17, 0] = np.inf
    for prm in (None, dict(normal_min=-1.0, plane_tol=1e18, max_history=8.0)):
        with Pair(w, h) as p:
            for i, (cam, frame, rec) in enumerate(calls):
                want, n, ok = p.step(cam, frame, rec, prm, (prm, i))
            # the denormal case cannot silently vanish: row 7 took history, and what the device was compared with there
            # is denormal — out = h + (0 - h) * a of a denormal h, wrong in every bit if a product, a sum or the quotient
            # had been flushed to 0
            tiny = np.finfo(np.float32).tiny
            assert np.all(n[7, 1:-1] == 2) and np.all((want[7, 1:-1, :3] > 0) & (want[7, 1:-1, :3] < tiny))
            assert np.isnan(want[9, 3, 1]) and np.isnan(want[10, 17, 0]) and 2 <= int(np.isnan(want).sum()) <= 4
            assert np.all(n[6, 0::2] == 1)
            assert (~ok).sum() <= 4  # (rgba8 was compared everywhere but at the pixels the NaN and the inf reached)


def test_a_tap_of_weight_zero_does_not_leak():
    """a camera that does not move: gx = x, gy = y exactly, three of the four taps have weight exactly 0 — the NaN and the
    inf history colour beside them stay where they are (0 * NaN would be NaN)"""
    rng = np.random.RandomState(78)
    h, w = 12, 24
    cam, frame1, rec = plane_case(rng, w, h, 0.0, 0.0)
    rec[..., 4:7] = (0, 0, 1)
    rec.view(np.uint32)[..., 11] = 3
    rec[..., 3] = 5.0
    frame1[9, 3, 1] = np.nan
    frame1[10, 17, 0] = np.inf
    frame2 = rng.uniform(0, 1, (h, w, 5)).astype(np.float32)
    with Pair(w, h) as p:
        p.step(cam, frame1, rec, None, 0)
        want, n, _ = p.step(cam, frame2, rec, None, 1)
        assert np.all(n == 2)
        # (the inf history itself blends to inf + -inf, a NaN: two pixels that are not finite, each where it was)
        assert np.isnan(want[9, 3, 1]) and np.isnan(want[10, 17, 0]) and int((~np.isfinite(want)).sum()) == 2
        want, n, _ = p.step(cam, frame1, rec, dict(max_history=1.0), 2)  # a history of one frame: the input alone
        assert np.all(n == 1)


def test_in_place_outputs_reset_frames_and_streams(sequences):
    import torch
    seq = sequences["cornell8", "slow"]
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="cuda")  # noqa: E731
    # the restatement's outputs for the sequence, once
    state, wants = None, []
    for cam, frame, raw in seq:
        want, state, n = TS.step(state, frame, raw, cam)
        wants.append((want, n))
    with va.Temporal(W, H) as t, va.Temporal(W, H) as fresh:
        assert t.frames() == 0
        for variant in ("both", "rgbaz", "rgba8", "in place", "after reset"):
            if variant == "after reset":
                handle = fresh
            else:
                handle = t
                handle.reset()
                assert handle.frames() == 0
            for i, (cam, frame, raw) in enumerate(seq):
                src, hist = dev(frame), new(H, W)
                if variant == "rgbaz":
                    out, q = handle.accumulate(cam, dev(raw), src, history=hist)
                    assert q is None
                elif variant == "rgba8":
                    out, q = handle.accumulate(cam, dev(raw), src, rgba8=new(H, W, 4, dtype=torch.uint8), history=hist)
                    assert out is None
                elif variant == "in place":
                    out, q = handle.accumulate(cam, dev(raw), src, out=src)
                    assert out is src
                    hist = None
                else:
                    out, q = handle.accumulate(cam, dev(raw), src, out=new(H, W, 5), rgba8=new(H, W, 4, dtype=torch.uint8),
                                               history=hist)
                want, n = wants[i]
                if out is not None:
                    assert FS.same_bits(out.cpu().numpy(), want), (variant, i)
                if q is not None:
                    assert np.array_equal(q.cpu().numpy().reshape(-1, 4), O.quantize(want)[0]), (variant, i)
                if hist is not None:
                    assert FS.same_bits(hist.cpu().numpy(), n), (variant, i)
                if variant != "in place":
                    assert np.array_equal(bits(src.cpu().numpy()), bits(frame))  # the input is left alone
                assert handle.frames() == i + 1
        # six calls alternate on two streams: ordered by enqueue on the handle, each result its own call's
        six = (seq + seq[::-1])[:6]
        state, want6 = None, []
        for cam, frame, raw in six:
            want, state, n = TS.step(state, frame, raw, cam)
            want6.append((want, n))
        ins = [(cam, dev(raw), dev(frame)) for cam, frame, raw in six]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        t.reset()
        torch.cuda.synchronize()
        outs = []
        for i, (cam, raw, frame) in enumerate(ins):
            hist = new(H, W)
            o, _ = t.accumulate(cam, raw, frame, out=new(H, W, 5), history=hist, stream=s2 if i % 2 else s1)
            outs.append((o, hist))
        torch.cuda.synchronize()
        for i, (o, hist) in enumerate(outs):
            assert FS.same_bits(o.cpu().numpy(), want6[i][0]), i
            assert FS.same_bits(hist.cpu().numpy(), want6[i][1]), i
        assert t.frames() == 6


def test_composition_with_the_filter(sequences):
    """Filter.apply on the accumulated frame, guided by the last frame's records, is filter_spec of the restatement's
    accumulated frame"""
    seq = sequences["lattice", "fast"]
    h, w = seq[0][1].shape[:2]
    with Pair(w, h) as p, va.Filter(w, h) as f:
        for i, (cam, frame, raw) in enumerate(seq):
            want, _, _ = p.step(cam, frame, raw, None, i)
        f.set_guide(dev(raw))
        got, _ = f.apply(dev(want))
        assert FS.same_bits(got.cpu().numpy(), FS.filtered_frame(want, *FS.guide_of(raw)))


def test_history_restarts_on_geometry_that_moved():
    """Scene.update moves the block (triangles 4-7: its front and its top) by 60 up and 60 towards the camera between two
    frames of a camera at rest: on the moved faces the plane test fails and the history restarts at 1, elsewhere (where
    the same surface is seen) it goes on — per the restatement, which the device matches"""
    pos, nrm, uv = scenes.cornell8()
    c = scenes.cornell_camera()
    cam = moved_camera(c, W, H)
    moved = np.array(pos).reshape(-1, 3, 3)
    moved[4:8] += np.float32([0, 60, 60])
    with va.Scene(pos, nrm, uv) as sc, Pair(W, H) as p:
        for i in range(2):
            (_, frame, raw), = rendered(sc, [cam], first_seed=3 + i)
            want, n, ok = p.step(cam, frame, raw, None, ("before", i))
        assert n.max() == 2
        sc.update(pos=moved.reshape(-1, 9))
        (_, frame, raw), = rendered(sc, [cam], first_seed=5)
        want, n, ok = p.step(cam, frame, raw, None, "after")
        tri = bits(raw)[..., 7].view(np.int32)
        on_block = (tri >= 4) & (tri < 8)
        assert on_block.sum() > 20 and np.all(n[on_block] == 1)
        assert np.array_equal(bits(want[on_block]), bits(frame[on_block]))
        assert (n[~on_block] == 3).mean() > 0.8


def test_refusals(sequences):
    import torch
    seq = sequences["cornell8", "fast"]
    P = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    with Pair(W, H) as p:
        t, lib = p.t, p.t._lib
        made = []

        def still_works():
            cam, frame, raw = seq[len(made) % len(seq)]
            p.step(cam, frame, raw, None, "after a refusal")
            made.append(1)

        def refused(call, match):
            with pytest.raises(va.VmxError, match=match) as e:
                call()
            assert e.value.code == L.VMX_ERR_INVALID
            still_works()

        still_works()
        cam, frame, raw = seq[1]
        src, rec, out = dev(frame), dev(raw), torch.empty((H, W, 5), device="cuda")
        bad = [dict(normal_min=float("nan")), dict(normal_min=1.5), dict(normal_min=-2.0), dict(plane_tol=0.0),
               dict(plane_tol=float("inf")), dict(plane_tol=float("nan")), dict(max_history=0.0),
               dict(max_history=float("inf")), dict(max_history=float("nan"))]
        for kw in bad:
            refused(lambda: t.accumulate(cam, rec, src, params=va.make_temporal_params(**kw)), "vmx_temporal_params")
        prm = va.make_temporal_params()
        prm.reserved[4] = 7
        refused(lambda: t.accumulate(cam, rec, src, params=prm), "reserved")
        # a camera of another size, straight through the C ABI (the Python layer takes the size from the handle)
        for other in (moved_camera(scenes.cornell_camera(), W + 1, H), moved_camera(scenes.cornell_camera(), H, W)):
            assert lib.vmx_temporal_accumulate_device(t._h, C.byref(other), P(rec), P(src), P(out), None, None, None,
                                                      None) == L.VMX_ERR_INVALID
            assert "the handle's frames are 70 x 41" in lib.vmx_last_error().decode()
            still_works()
        # host pointers
        host5, host16 = np.array(frame), np.array(raw)
        hp5, hp16 = C.c_void_p(host5.ctypes.data), C.c_void_p((host16.ctypes.data + 15) & ~15)
        for args in ((hp16, P(src), P(out), None, None), (P(rec), hp5, P(out), None, None), (P(rec), P(src), hp5, None, None),
                     (P(rec), P(src), None, hp5, None), (P(rec), P(src), P(out), None, hp5)):
            assert lib.vmx_temporal_accumulate_device(t._h, C.byref(cam), *args, None, None) == L.VMX_ERR_INVALID
            assert "not device memory" in lib.vmx_last_error().decode()
            still_works()
        assert lib.vmx_temporal_accumulate_device(t._h, C.byref(cam), P(rec), P(src), None, None, None, None,
                                                  None) == L.VMX_ERR_INVALID
        assert "no output" in lib.vmx_last_error().decode()
        still_works()
        # a partially overlapping in and out; rgba8 and the history lengths inside the input; an output over the records
        buf = torch.zeros(W * H * 5 + 5, dtype=torch.float32, device="cuda")
        a, b = buf[:W * H * 5].view(H, W, 5), buf[5:].view(H, W, 5)
        a.copy_(src)
        refused(lambda: t.accumulate(cam, rec, a, out=b), "overlap")
        refused(lambda: t.accumulate(cam, rec, a, rgba8=buf[8:8 + W * H].view(torch.uint8).view(H, W, 4)), "overlap")
        refused(lambda: t.accumulate(cam, rec, a, out=out, history=buf[8:8 + W * H].view(H, W)), "overlap")
        refused(lambda: t.accumulate(cam, rec, src, out=rec.view(-1)[16:16 + W * H * 5].view(H, W, 5)), "overlap")
        assert p.t.frames() == len(made)  # the refused calls did not count
