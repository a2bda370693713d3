"""The G-buffer-guided a-trous filter on the device (vmx_filter_*, vmx_progressive_preview_filtered*): every output is
compared as uint32 bits with the float32 restatement (tests/filter_spec.py), every pixel; NaN may appear only where
the restatement has NaN, which happens only through its pass-through rule.

Shapes: the 8-triangle Cornell set at 70x41 (three blocks across, six down, the last of each partial) and the lattice
at 64x48, both at 16 spp; 5x3, 1x1, 257x1 and 1x130 for images smaller than a block, one pixel wide or one pixel high."""
import ctypes as C

import numpy as np
import pytest

import filter_spec as FS
import oracle_lib as O
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
W, H = 70, 41


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cornell_cam(spp, w=W, h=H):
    c = scenes.cornell_camera()
    return va.make_camera(c["position"], c["rotation_deg"], w, h, spp)


def light_spheres():
    """the two VMX_SPHERE_EMIT entries of the default table alone: about 30 % of the camera rays miss"""
    table = va.default_spheres()
    emit = [s for s in table if s.flags & L.VMX_SPHERE_EMIT]
    assert len(emit) == 2
    out = (L.Sphere * 2)()
    for i, s in enumerate(emit):
        C.memmove(C.byref(out[i]), C.byref(s), C.sizeof(L.Sphere))
    return out


@pytest.fixture(scope="module")
def frames():
    """name -> (frame [H, W, 5], guide records [H, W, 16]) from Scene.render and Scene.raycast_camera(k=0): computed
    once and never written to"""
    out = {}
    lc = scenes.lattice_camera()
    cases = (("cornell_parity", scenes.cornell8(), None, cornell_cam(16), va.VMX_SAMPLING_PARITY),
             ("cornell_corrected", scenes.cornell8(), None, cornell_cam(16), va.VMX_SAMPLING_CORRECTED),
             ("lattice", scenes.lattice(), None, va.make_camera(lc["position"], lc["rotation_deg"], 64, 48, 16),
              va.VMX_SAMPLING_CORRECTED),
             ("lights_only", scenes.cornell8(), light_spheres(), cornell_cam(16), va.VMX_SAMPLING_CORRECTED))
    for name, (pos, nrm, uv), spheres, cam, sampling in cases:
        opts = va.make_opts(seed=3, early_stop=False, sampling=sampling)
        with va.Scene(pos, nrm, uv, spheres=spheres) as sc:
            img, _ = sc.render(cam, opts)
            raw = sc.raycast_camera(cam, opts, 0)["raw"].cpu().numpy()
        img.setflags(write=False), raw.setflags(write=False)
        out[name] = (img, raw)
    miss = (bits(out["lights_only"][1])[..., 11] & 1) == 0
    assert 0.15 < miss.mean() < 0.6, miss.mean()  # hits and misses are mixed
    return out


def apply_np(f, frame, params=None, **kw):
    out, _ = f.apply(dev(frame), params=params, **kw)
    return out.cpu().numpy()


def check(f, frame, raw, params=None, tag=None):
    n, z = FS.guide_of(raw)
    want = FS.filtered_frame(frame, n, z, params)
    got = apply_np(f, frame, params)
    assert FS.same_bits(got, want), (tag, int((bits(got) != bits(want)).any(axis=-1).sum()), "pixels differ")
    return got


PARAMS = ([dict(iterations=i) for i in (1, 2, 5, 7)] + [dict(normal_squarings=0), dict(normal_squarings=8)] +
          [dict(sigma_colour=0.5, sigma_depth=0.02), dict(sigma_colour=8.0, sigma_depth=1.0)])


@pytest.mark.parametrize("name", ["cornell_parity", "cornell_corrected", "lattice", "lights_only"])
def test_apply_is_the_restatement_bit_for_bit(frames, name):
    """iterations 1, 2, 5 and 7 (step 64: most taps fall outside the image), normal_squarings 0 and 8 (the kernel's
    general form; 5 is its constant form), two further sigma pairs"""
    frame, raw = frames[name]
    h, w = frame.shape[:2]
    with va.Filter(w, h) as f:
        f.set_guide(dev(raw))
        for kw in PARAMS:
            got = check(f, frame, raw, va.make_filter_params(**kw), (name, kw))
            assert not np.array_equal(bits(got[..., :3]), bits(frame[..., :3]))  # (it did filter)
        check(f, frame, raw, None, (name, "defaults"))


def synthetic(rng, h, w):
    """a frame and guide records from a seeded RandomState: random unit normals, a third of the pixels misses"""
    frame = rng.uniform(0, 1, (h, w, 5)).astype(np.float32)
    raw = np.zeros((h, w, 16), np.float32)
    nrm = rng.normal(size=(h, w, 3))
    raw[..., 4:7] = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    raw[..., 3] = rng.uniform(5, 6, (h, w)).astype(np.float32)
    hit = rng.uniform(size=(h, w)) < 0.67
    raw[..., 3][~hit] = np.inf  # (a miss's record: distance INFINITY, a stale normal)
    raw.view(np.uint32)[..., 11] = np.where(hit, 3, 2)
    return frame, raw


@pytest.mark.parametrize("w,h", [(5, 3), (1, 1), (257, 1), (1, 130)])
def test_degenerate_shapes(w, h):
    frame, raw = synthetic(np.random.RandomState(w * 1000 + h), h, w)
    with va.Filter(w, h) as f:
        f.set_guide(dev(raw))
        for kw in (dict(), dict(iterations=1), dict(iterations=7, normal_squarings=2)):
            check(f, frame, raw, va.make_filter_params(**kw), (w, h, kw))


def test_synthetic_guide_records():
    """Guide records a renderer would not write.  Rows of a 24 x 12 image: zero normals, NaN normals, normals of length
    1e3 (dot^32 overflows: the weight is not finite), z of 1e-38 (isz overflows), 1e30 and exactly 0, alternating hit
    and miss, and a pixel whose taps to its neighbours all have a denormal dot^32.  Colours in [0, 1], one NaN pixel and
    one +inf pixel."""
    rng = np.random.RandomState(77)
    h, w = 12, 24
    frame, raw = synthetic(rng, h, w)
    flags = raw.view(np.uint32)[..., 11]
    flags[:8] = 1
    raw[:8, :, 3] = 5.0
    raw[0, :, 4:7] = 0.0
    raw[1, :, 4:7] = np.nan
    raw[2, :, 4:7] *= np.float32(1e3)
    raw[3, :, 3] = np.float32(1e-38)
    raw[4, :, 3] = np.float32(1e30)
    raw[5, :, 3] = 0.0
    flags[6, 0::2] = 0
    # row 7: normals (1, 0, 0) at one depth, but pixel 11's is (0.0562, 0, 0): its own tap has dot^32 = 0.0562^64 = 0 and
    # every tap to a row-7 neighbour has dot^32 = 0.0562^32 ~ 1e-40, so all of its weights and their sum are denormal
    cos = np.float32(0.0562)
    raw[7, :, 4:7] = np.float32([1, 0, 0])
    raw[7, 11, 4:7] = [cos, 0, 0]
    frame[9, 3, 1] = np.nan
    frame[10, 17, 0] = np.inf
    n, z = FS.guide_of(raw)
    # the denormal case cannot silently vanish: the restatement's weight of tap (7, 11) -> (7, 10) at step 1
    prm = FS.params_of()
    wt = FS.tap_weight(FS.H5[2] * FS.H5[1], n[7, 11], z[7, 11], n[7, 10], z[7, 10], frame[7, 11, :3], frame[7, 10, :3],
                       prm["normal_squarings"], FS.F(1) / (FS.F(prm["sigma_colour"]) * FS.F(prm["sigma_colour"])),
                       FS.F(prm["sigma_depth"]) * FS.F(1))
    assert 0 < wt < np.finfo(np.float32).tiny, wt
    # ... and it decides the pixel: with the denormals flushed no tap of (7, 11) would count and it would keep its colour
    one = FS.atrous(frame[..., :3], n, z, FS.params_of(iterations=1))
    assert not np.array_equal(bits(one[7, 11]), bits(frame[7, 11, :3]))
    with va.Filter(w, h) as f:
        f.set_guide(dev(raw))
        for kw in (dict(), dict(iterations=1), dict(iterations=3, normal_squarings=8), dict(normal_squarings=0)):
            got = check(f, frame, raw, va.make_filter_params(**kw), kw)
            assert np.isnan(got[9, 3, 1]) and int(np.isnan(got).sum()) == 1
            assert got[10, 17, 0] == np.inf


def test_in_place_outputs_repeats_and_streams(frames):
    import torch
    frame, raw = frames["cornell_corrected"]
    n, z = FS.guide_of(raw)
    with va.Filter(W, H) as f:
        f.set_guide(dev(raw))
        for prm in (None, va.make_filter_params(iterations=1), va.make_filter_params(iterations=2)):
            want = FS.filtered_frame(frame, n, z, prm)
            src = dev(frame)
            out, q = f.apply(src, out=torch.empty_like(src), rgba8=torch.empty((H, W, 4), dtype=torch.uint8, device="cuda"),
                             params=prm)
            assert FS.same_bits(out.cpu().numpy(), want)
            assert np.array_equal(q.cpu().numpy().reshape(-1, 4), O.quantize(want)[0])
            assert np.array_equal(bits(src.cpu().numpy()), bits(frame))  # the input is left alone
            only5, none4 = f.apply(src, params=prm)
            none5, only4 = f.apply(src, rgba8=torch.empty_like(q), params=prm)
            assert none4 is None and none5 is None
            assert torch.equal(only5, out) and torch.equal(only4, q)
            again, _ = f.apply(src, params=prm)
            assert torch.equal(again.view(torch.int32), out.view(torch.int32))
            same, _ = f.apply(src, out=src, params=prm)  # in place
            assert same is src and torch.equal(src.view(torch.int32), out.view(torch.int32))
        # calls on two streams alternate: ordered by enqueue on the handle, each result its own call's
        pa, pb = va.make_filter_params(iterations=3), va.make_filter_params(iterations=4, sigma_colour=1.0)
        want_a, want_b = FS.filtered_frame(frame, n, z, pa), FS.filtered_frame(frame, n, z, pb)
        src = dev(frame)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        outs = []
        for i in range(6):
            o, _ = f.apply(src, out=torch.empty_like(src), params=pb if i % 2 else pa, stream=s2 if i % 2 else s1)
            outs.append(o)
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            assert FS.same_bits(o.cpu().numpy(), want_b if i % 2 else want_a), i


@pytest.mark.parametrize("early_stop", [0, 1])
def test_progressive_filtered_previews(early_stop):
    """70x41x64 spp in steps of 3 samples: every filtered preview — before the first sample, after each step, of the
    complete frame — is Filter.apply(preview(), guide of raycast_camera k = 0) and the restatement; it changes nothing,
    and the final frame is still Scene.render's."""
    import torch
    cam = cornell_cam(64)
    opts = va.make_opts(seed=9, early_stop=bool(early_stop))
    with va.Scene(*scenes.cornell8()) as sc, va.Filter(W, H) as f:
        ref, _ = sc.render(cam, opts)
        raw = sc.raycast_camera(cam, opts, 0)["raw"]
        f.set_guide(raw)
        n, z = FS.guide_of(raw.cpu().numpy())
        short = va.make_filter_params(iterations=2, normal_squarings=3)
        with sc.progressive(cam, opts) as p:
            for step in range(64):
                plain, info = p.preview(), p.info()
                got, q = p.preview_filtered(rgba8=True)
                via_apply = apply_np(f, plain)
                assert np.array_equal(bits(got), bits(via_apply)), step
                assert FS.same_bits(got, FS.filtered_frame(plain, n, z)), step
                assert np.array_equal(q.reshape(-1, 4), O.quantize(got)[0]), step
                assert np.array_equal(bits(p.preview()), bits(plain)) and p.info() == info  # nothing changed
                if step in (0, 2):
                    assert FS.same_bits(p.preview_filtered(params=short), FS.filtered_frame(plain, n, z, short))
                    d5 = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
                    d4 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
                    e5, e4 = torch.empty_like(d5), torch.empty_like(d4)
                    torch.cuda.synchronize()
                    p.preview_filtered_device(d5, d4)
                    p.preview_filtered_device(rgbaz=e5)
                    p.preview_filtered_device(rgba8=e4)
                    p.preview()  # (the host entry synchronises the handle's stream)
                    for t5 in (d5, e5):
                        assert np.array_equal(bits(t5.cpu().numpy()), bits(got))
                    for t4 in (d4, e4):
                        assert np.array_equal(t4.cpu().numpy(), q)
                if info["pixels_active"] == 0:
                    break
                p.step(3)
            assert p.info()["pixels_active"] == 0 and step > 0
            assert np.array_equal(bits(p.preview()), bits(ref))


def test_refusals(frames):
    import torch
    frame, raw = frames["cornell_parity"]
    n, z = FS.guide_of(raw)
    want = FS.filtered_frame(frame, n, z)
    src = dev(frame)

    def refused(call, match):
        with pytest.raises(va.VmxError, match=match) as e:
            call()
        assert e.value.code == L.VMX_ERR_INVALID

    with va.Filter(W, H) as f:
        refused(lambda: f.apply(src), "no guide")
        f.set_guide(dev(raw))

        def still_works():
            assert FS.same_bits(f.apply(src)[0].cpu().numpy(), want)

        still_works()
        bad = [dict(iterations=0), dict(iterations=11), dict(normal_squarings=9), dict(sigma_colour=0.0),
               dict(sigma_depth=0.0), dict(sigma_colour=float("nan")), dict(sigma_depth=float("nan")),
               dict(sigma_colour=float("inf")), dict(sigma_depth=float("inf"))]
        for kw in bad:
            refused(lambda: f.apply(src, params=va.make_filter_params(**kw)), "vmx_filter_params")
            still_works()
        prm = va.make_filter_params()
        prm.reserved[3] = 7
        refused(lambda: f.apply(src, params=prm), "reserved")
        still_works()
        # host pointers, straight through the C ABI (the Python layer would refuse them itself)
        host = np.array(frame)
        out = torch.empty_like(src)
        P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        lib = f._lib
        for args in ((C.c_void_p(host.ctypes.data), P(out), None), (P(src), C.c_void_p(host.ctypes.data), None),
                     (P(src), None, C.c_void_p(host.ctypes.data))):
            assert lib.vmx_filter_apply_device(f._h, *args, None, None) == L.VMX_ERR_INVALID
            assert "not device memory" in lib.vmx_last_error().decode()
            still_works()
        assert lib.vmx_filter_set_guide_device(f._h, C.c_void_p(np.array(raw).ctypes.data), None) == L.VMX_ERR_INVALID
        assert "not device memory" in lib.vmx_last_error().decode()
        still_works()
        assert lib.vmx_filter_apply_device(f._h, P(src), None, None, None, None) == L.VMX_ERR_INVALID
        assert "no output" in lib.vmx_last_error().decode()
        # a partially overlapping in and out; rgba8 inside the input
        buf = torch.zeros(W * H * 5 + 5, dtype=torch.float32, device="cuda")
        a, b = buf[:W * H * 5].view(H, W, 5), buf[5:].view(H, W, 5)
        a.copy_(src)
        refused(lambda: f.apply(a, out=b), "overlap")
        refused(lambda: f.apply(a, rgba8=buf[8:8 + W * H].view(torch.uint8).view(H, W, 4)), "overlap")
        still_works()
        assert FS.same_bits(f.apply(a, out=a)[0].cpu().numpy(), want)  # in place is the overlap that is allowed

    cam = cornell_cam(16)
    pos, nrm, uv = scenes.cornell8()
    with va.Scene(pos, nrm, uv) as s:
        with s.progressive(cam, va.make_opts(seed=2, world=3, rank=1, stripe_rows=4)) as p:
            p.step(2)
            plain = p.preview()
            refused(lambda: p.preview_filtered(), "whole images only")
            assert np.array_equal(bits(p.preview()), bits(plain))
        opts = va.make_opts(seed=2)
        with s.progressive(cam, opts) as early, s.progressive(cam, opts) as late:
            early.step(2), late.step(2)
            before = early.preview_filtered()  # builds this handle's guide
            refused(lambda: early.preview_filtered(params=va.make_filter_params(iterations=0)), "vmx_filter_params")
            s.update(pos=pos)  # a refit to the same positions is still an update
            refused(lambda: late.preview_filtered(), "scene updated since vmx_progressive_begin")
            refused(lambda: late.preview_filtered(), "scene updated since vmx_progressive_begin")
            assert np.array_equal(bits(late.preview()), bits(early.preview()))
            # a guide built before the update keeps working
            assert np.array_equal(bits(early.preview_filtered()), bits(before))
            g = s.raycast_camera(cam, opts, 0)["raw"].cpu().numpy()
            assert FS.same_bits(before, FS.filtered_frame(early.preview(), *FS.guide_of(g)))
