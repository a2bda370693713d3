"""Albedo-demodulated denoising on the device (vmx_albedo_camera_device, vmx_filter_apply_demodulated_device,
vmx_progressive_preview_demodulated*): every output is compared as uint32 bits with the float32 restatement
(tests/demod_spec.py), every pixel.

Shapes: the 8-triangle Cornell set at 70x41 (three filter blocks across, six down, the last of each partial; twelve
blocks of the albedo finish, the last partial) and the lattice at 64x48, both at 16 spp; 5x3, 1x1, 257x1 and 1x130 for
images smaller than a block, one pixel wide or one pixel high."""
import ctypes as C

import numpy as np
import pytest

import demod_spec as DS
import filter_spec as FS
import oracle_lib as O
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
W, H = 70, 41
CORRECTED = va.VMX_SAMPLING_CORRECTED
SMALL = [(5, 3), (1, 1), (257, 1), (1, 130)]
DEGENERATE = np.float32([0.0, -1.0, np.nan, np.inf, 1e-9])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_plane(got, want):
    return np.array_equal(bits(got), bits(want))


def texture(h, w, c, seed=0):
    """values in [0.05, 1), every channel its own; the 32 x 32 x 3 one is the checker of tests/test_demod_abi.py"""
    if (h, w, c) == (32, 32, 3):
        y, x = np.mgrid[0:32, 0:32]
        chk = ((x // 4 + y // 4) & 1).astype(np.float32)
        return np.ascontiguousarray(np.stack([0.25 + 0.7 * chk, 0.9 - 0.6 * chk, 0.3 + 0.5 * ((x // 2) & 1)], axis=-1), np.float32)
    t = np.random.RandomState(100 * h + 10 * w + c + seed).uniform(0.05, 1, (h, w, c)).astype(np.float32)
    return t[..., 0] if c == 1 else t


def case(name, w=None, h=None, spp=16):
    if name == "cornell8":
        geo, c, size = scenes.cornell8(), scenes.cornell_camera(), (W, H)
    else:
        geo, c, size = scenes.lattice(), scenes.lattice_camera(), (64, 48)
    w, h = (w or size[0]), (h or size[1])
    return geo, va.make_camera(c["position"], c["rotation_deg"], w, h, spp)


def light_spheres():
    """the two VMX_SPHERE_EMIT entries of the default table alone: about 30 % of the camera rays miss"""
    emit = [s for s in va.default_spheres() if s.flags & L.VMX_SPHERE_EMIT]
    out = (L.Sphere * 2)()
    for i, s in enumerate(emit):
        C.memmove(C.byref(out[i]), C.byref(s), C.sizeof(L.Sphere))
    return out


def big_light():
    """the default table with its first sphere, the small light in front of the block, at radius 120: triangle hits of
    many pixels sit behind it"""
    table = va.default_spheres()
    table[0].radius = 120.0
    return table


def both(geo, tex=None, spheres=None):
    """the scene on the device and in the oracle, the same texture bound to both"""
    pos, nrm, uv = geo
    sc, osc = va.Scene(pos, nrm, uv, spheres=spheres), O.OracleScene(pos, nrm, uv, spheres=spheres)
    if tex is not None:
        sc.bind_texture(tex), osc.bind_texture(tex)
    return sc, osc


def plane_np(sc, cam, opts, n, first=0):
    return sc.albedo_camera(cam, opts, samples=n, first=first).cpu().numpy()


# ---- the albedo plane ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell8", "lattice"])
def test_albedo_plane_scenes_and_textures(name):
    """textures of 1, 2, 3 and 4 channels, 32x32 and 5x3, and no texture at all; default spheres"""
    geo, cam = case(name)
    opts = va.make_opts(seed=3, sampling=CORRECTED)
    texs = [None] + [texture(th, tw, c) for th, tw in ((32, 32), (3, 5)) for c in (1, 2, 3, 4)]
    for tex in texs:
        sc, osc = both(geo, tex)
        with sc:
            got = plane_np(sc, cam, opts, 4)
        want = DS.albedo_plane(osc, tex, cam, opts, 0, 4)
        osc.close()
        tag = (name, None if tex is None else tex.shape)
        assert same_plane(got, want), (tag, int((bits(got) != bits(want)).any(axis=-1).sum()), "pixels differ")
        if tex is None:
            assert np.array_equal(got[..., :3], np.ones_like(got[..., :3]))
        else:
            assert got[..., :3].std() > 0.01, tag  # (the texture shows)
        assert 0 < got[..., 3].mean() <= 1


def test_albedo_plane_sample_ranges_and_out():
    import torch
    geo, cam = case("cornell8")
    opts = va.make_opts(seed=5, sampling=CORRECTED)
    tex = texture(32, 32, 3)
    sc, osc = both(geo, tex)
    with sc:
        for first, n in ((0, 1), (0, 4), (0, 16), (4, 8), (15, 1)):
            want = DS.albedo_plane(osc, tex, cam, opts, first, n)
            assert same_plane(plane_np(sc, cam, opts, n, first), want), (first, n)
        # into a caller's tensor, on a stream of the caller's; the call before it on the scene's workspace is not disturbed
        out = torch.full((H, W, 4), 7.0, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        a = sc.albedo_camera(cam, opts, samples=16)
        b = sc.albedo_camera(cam, opts, samples=4, first=4, out=out, stream=s)
        torch.cuda.synchronize()
        assert b is out
        assert same_plane(a.cpu().numpy(), DS.albedo_plane(osc, tex, cam, opts, 0, 16))
        assert same_plane(out.cpu().numpy(), DS.albedo_plane(osc, tex, cam, opts, 4, 4))
        # a G-buffer between two planes: the raycast's records and the plane's scratch do not meet
        raw = sc.raycast_camera(cam, opts, 2)["raw"].cpu().numpy()
        want = osc.raycast(*O.primary_rays(cam, opts, 2))
        assert np.array_equal(bits(raw.reshape(-1, 16)[:, 8:10]), bits(want["uv"]))
        for first, n, what in ((0, 17, "sample range"), (16, 1, "sample range"), (13, 4, "sample range")):
            with pytest.raises(va.VmxError, match=what) as e:
                sc.albedo_camera(cam, opts, samples=n, first=first)
            assert e.value.code == L.VMX_ERR_INVALID
        host = np.zeros((H, W, 4), np.float32)
        assert sc._lib.vmx_albedo_camera_device(sc._h, C.byref(cam), C.byref(opts), 0, 4, C.c_void_p(host.ctypes.data),
                                                None) == L.VMX_ERR_INVALID
        assert "not device memory" in sc._lib.vmx_last_error().decode()
        assert same_plane(plane_np(sc, cam, opts, 4), DS.albedo_plane(osc, tex, cam, opts, 0, 4))
    osc.close()


def test_albedo_plane_ray_cases():
    """uvs scaled by 2.5 and negated (the wrap); the default sphere table, and the same with a large sphere in front of
    the block, where material hits sit behind a nearer sphere and their stale uv is still what is sampled; the two light
    spheres alone, where about 30 % of the rays miss"""
    (pos, nrm, uv), cam = case("cornell8")
    opts = va.make_opts(seed=4, sampling=CORRECTED)
    tex = texture(32, 32, 3)
    for tag, uvs, spheres in (("wrap", np.asarray(uv, np.float32) * np.float32(-2.5), None), ("default spheres", uv, None),
                              ("big light", uv, big_light()), ("lights only", uv, light_spheres())):
        sc, osc = both((pos, nrm, uvs), tex, spheres)
        with sc:
            got = plane_np(sc, cam, opts, 4)
            rec = sc.raycast_camera(cam, opts, 0)
            flags, dist, tri_t = (rec[k].cpu().numpy() for k in ("flags", "distance", "tri_t"))
        assert same_plane(got, DS.albedo_plane(osc, tex, cam, opts, 0, 4)), tag
        hidden = ((flags & 2) != 0) & (dist < tri_t)  # a material hit behind a nearer sphere
        miss = (flags & 1) == 0
        if tag == "big light":
            assert hidden.sum() > 20, int(hidden.sum())
        if tag == "lights only":
            assert 0.15 < miss.mean() < 0.6, miss.mean()
            assert np.all(got[got[..., 3] == 0][:, :3] == 1)  # no sample hit the mesh: every sample was (1, 1, 1)
        osc.close()


@pytest.mark.parametrize("w,h", SMALL)
def test_albedo_plane_image_shapes(w, h):
    geo, cam = case("cornell8", w, h)
    opts = va.make_opts(seed=6, sampling=CORRECTED)
    tex = texture(3, 5, 4)
    sc, osc = both(geo, tex)
    with sc:
        for first, n in ((0, 3), (5, 1)):
            assert same_plane(plane_np(sc, cam, opts, n, first), DS.albedo_plane(osc, tex, cam, opts, first, n)), (w, h, first, n)
    osc.close()


def test_albedo_plane_follows_a_refit():
    """a plane built after Scene.update (a refit) is the restatement on the updated geometry"""
    (pos, nrm, uv), cam = case("cornell8")
    opts = va.make_opts(seed=8, sampling=CORRECTED)
    tex = texture(32, 32, 3)
    pos = np.asarray(pos, np.float32).reshape(-1, 9)
    moved = pos.copy()
    moved[: len(moved) // 2, 0::3] += np.float32(150.0)  # half of the triangles, along x
    sc, osc = both((pos, nrm, uv), tex)
    with sc:
        before = plane_np(sc, cam, opts, 4)
        assert same_plane(before, DS.albedo_plane(osc, tex, cam, opts, 0, 4))
        sc.update(pos=moved)
        after = plane_np(sc, cam, opts, 4)  # enqueued behind the update, whatever its stream
        osc2 = O.OracleScene(moved, nrm, uv, tree=sc.bvh())
        osc2.bind_texture(tex)
        assert same_plane(after, DS.albedo_plane(osc2, tex, cam, opts, 0, 4))
        assert not same_plane(after, before)
        osc2.close()
    osc.close()


# ---- the demodulated apply -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    """name -> (frame [H, W, 5], guide records [H, W, 16], albedo plane [H, W, 4]) of the textured scenes from
    Scene.render, Scene.raycast_camera(k = 0) and Scene.albedo_camera(4 samples); "plain": the Cornell set without a
    texture.  Computed once and never written to"""
    out = {}
    for name, scene_name, tex in (("cornell8", "cornell8", texture(32, 32, 3)), ("lattice", "lattice", texture(32, 32, 3)),
                                  ("plain", "cornell8", None)):
        geo, cam = case(scene_name)
        opts = va.make_opts(seed=3, early_stop=False, sampling=CORRECTED)
        with va.Scene(*geo) as sc:
            if tex is not None:
                sc.bind_texture(tex)
            img, _ = sc.render(cam, opts)
            raw = sc.raycast_camera(cam, opts, 0)["raw"].cpu().numpy()
            alb = plane_np(sc, cam, opts, 4)
        for a in (img, raw, alb):
            a.setflags(write=False)
        out[name] = (img, raw, alb)
    return out


def check(f, frame, raw, albedo, params=None, tag=None):
    n, z = FS.guide_of(raw)
    want = DS.demodulated_frame(frame, n, z, albedo, params)
    got = f.apply(dev(frame), albedo=dev(albedo), params=params)[0].cpu().numpy()
    assert FS.same_bits(got, want), (tag, int((bits(got) != bits(want)).any(axis=-1).sum()), "pixels differ")
    return got


PARAMS = ([dict(iterations=i) for i in (1, 2, 5)] + [dict(normal_squarings=0), dict(normal_squarings=8, iterations=1),
                                                     dict(normal_squarings=3, iterations=2)])


@pytest.mark.parametrize("name", ["cornell8", "lattice"])
def test_demodulated_apply_is_the_restatement_bit_for_bit(frames, name):
    """iterations 1 (one launch divides and multiplies), 2 and 5; normal_squarings 0, 3 and 8 (the kernel's general
    form; 5 is its constant form)"""
    frame, raw, alb = frames[name]
    h, w = frame.shape[:2]
    n, z = FS.guide_of(raw)
    with va.Filter(w, h) as f:
        f.set_guide(dev(raw))
        for kw in PARAMS:
            prm = va.make_filter_params(**kw)
            got = check(f, frame, raw, alb, prm, (name, kw))
            assert not FS.same_bits(got, FS.filtered_frame(frame, n, z, prm))  # (demodulation did something)
        check(f, frame, raw, alb, None, (name, "defaults"))


def test_demodulated_apply_in_place_outputs_and_the_plain_call(frames):
    import torch
    frame, raw, alb = frames["cornell8"]
    n, z = FS.guide_of(raw)
    with va.Filter(W, H) as f:
        f.set_guide(dev(raw))
        d_alb = dev(alb)
        for prm in (None, va.make_filter_params(iterations=1), va.make_filter_params(iterations=2)):
            want = DS.demodulated_frame(frame, n, z, alb, prm)
            plain_want = FS.filtered_frame(frame, n, z, prm)
            src = dev(frame)
            plain_before = f.apply(src, params=prm)[0]
            assert FS.same_bits(plain_before.cpu().numpy(), plain_want)
            out, q = f.apply(src, out=torch.empty_like(src), rgba8=torch.empty((H, W, 4), dtype=torch.uint8, device="cuda"),
                             params=prm, albedo=d_alb)
            assert FS.same_bits(out.cpu().numpy(), want)
            assert np.array_equal(q.cpu().numpy().reshape(-1, 4), O.quantize(want)[0])  # rgba8 of the multiplied result
            assert np.array_equal(bits(src.cpu().numpy()), bits(frame))  # the input and the plane are left alone
            assert np.array_equal(bits(d_alb.cpu().numpy()), bits(alb))
            none5, only4 = f.apply(src, rgba8=torch.empty_like(q), params=prm, albedo=d_alb)
            assert none5 is None and torch.equal(only4, q)
            # a plain apply after a demodulated one on the same handle gives the bits it gave before
            plain_after = f.apply(src, params=prm)[0]
            assert torch.equal(plain_after.view(torch.int32), plain_before.view(torch.int32))
            same, _ = f.apply(src, out=src, params=prm, albedo=d_alb)  # in place
            assert same is src and torch.equal(src.view(torch.int32), out.view(torch.int32))


def test_demodulated_apply_untextured_is_the_plain_apply(frames):
    import torch
    frame, raw, alb = frames["plain"]
    assert np.array_equal(alb[..., :3], np.ones_like(alb[..., :3]))
    with va.Filter(W, H) as f:
        f.set_guide(dev(raw))
        for prm in (None, va.make_filter_params(iterations=1), va.make_filter_params(iterations=3, normal_squarings=2)):
            src = dev(frame)
            plain, demod = f.apply(src, params=prm)[0], f.apply(src, params=prm, albedo=dev(alb))[0]
            assert torch.equal(plain.view(torch.int32), demod.view(torch.int32))


def test_demodulated_apply_degenerate_albedo(frames):
    """0, -1, NaN, +inf and 1e-9 take the floor, in any channel; the output is finite"""
    frame, raw, alb = frames["cornell8"]
    alb = np.array(alb)
    alb[3, 10:15, 0], alb[9, 20:25, 1], alb[30, 40:45, 2] = DEGENERATE, DEGENERATE, DEGENERATE
    alb[20, 33, :3] = np.nan
    alb[..., 3] = np.nan  # (.w is not read)
    with va.Filter(W, H) as f:
        f.set_guide(dev(raw))
        for kw in (dict(), dict(iterations=1), dict(iterations=2, normal_squarings=1)):
            got = check(f, frame, raw, alb, va.make_filter_params(**kw), kw)
            assert np.isfinite(got).all()


def synthetic(rng, h, w):
    """a frame, guide records and an albedo plane from a seeded RandomState: random unit normals, a third of the pixels
    misses, a few degenerate albedo values"""
    frame = rng.uniform(0, 1, (h, w, 5)).astype(np.float32)
    raw = np.zeros((h, w, 16), np.float32)
    nrm = rng.normal(size=(h, w, 3))
    raw[..., 4:7] = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    raw[..., 3] = rng.uniform(5, 6, (h, w)).astype(np.float32)
    hit = rng.uniform(size=(h, w)) < 0.67
    raw[..., 3][~hit] = np.inf
    raw.view(np.uint32)[..., 11] = np.where(hit, 3, 2)
    alb = rng.uniform(0.05, 1, (h, w, 4)).astype(np.float32)
    flat = alb.reshape(-1, 4)
    for i in range(0, flat.shape[0], 7):
        flat[i, i % 3] = DEGENERATE[(i // 7) % 5]
    return frame, raw, alb


@pytest.mark.parametrize("w,h", SMALL)
def test_demodulated_apply_image_shapes(w, h):
    frame, raw, alb = synthetic(np.random.RandomState(w * 1000 + h), h, w)
    with va.Filter(w, h) as f:
        f.set_guide(dev(raw))
        for kw in (dict(), dict(iterations=1), dict(iterations=7, normal_squarings=2)):
            check(f, frame, raw, alb, va.make_filter_params(**kw), (w, h, kw))


def test_demodulated_apply_streams_and_refusals(frames):
    import torch
    frame, raw, alb = frames["cornell8"]
    n, z = FS.guide_of(raw)
    src, d_alb = dev(frame), dev(alb)
    with va.Filter(W, H) as f:
        with pytest.raises(va.VmxError, match="no guide"):
            f.apply(src, albedo=d_alb)
        f.set_guide(dev(raw))
        # calls on two streams alternate: ordered by enqueue on the handle, each result its own call's
        pa, pb = va.make_filter_params(iterations=3), va.make_filter_params(iterations=4, sigma_colour=1.0)
        want_a, want_b = DS.demodulated_frame(frame, n, z, alb, pa), DS.demodulated_frame(frame, n, z, alb, pb)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        outs = []
        for i in range(6):
            o, _ = f.apply(src, out=torch.empty_like(src), params=pb if i % 2 else pa, stream=s2 if i % 2 else s1, albedo=d_alb)
            outs.append(o)
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            assert FS.same_bits(o.cpu().numpy(), want_b if i % 2 else want_a), i

        def refused(call, match):
            with pytest.raises(va.VmxError, match=match) as e:
                call()
            assert e.value.code == L.VMX_ERR_INVALID

        # the plane may meet no written buffer: the frame written in place, an rgba8 inside the plane
        big = torch.zeros(W * H * 5 + 8, dtype=torch.float32, device="cuda")
        inplace = big[:W * H * 5].view(H, W, 5)
        inplace.copy_(src)
        refused(lambda: f.apply(inplace, out=inplace, albedo=big[4:4 + W * H * 4].view(H, W, 4)), "d_albedo overlaps")
        plane = torch.ones(W * H * 4, dtype=torch.float32, device="cuda")
        refused(lambda: f.apply(src, rgba8=plane[4:4 + W * H].view(torch.uint8).view(H, W, 4), albedo=plane.view(H, W, 4)),
                "d_albedo overlaps")
        refused(lambda: f.apply(src, out=big[5:5 + W * H * 5].view(H, W, 5), albedo=d_alb,
                                rgba8=big[8:8 + W * H].view(torch.uint8).view(H, W, 4)), "overlap")
        # reading the frame as the plane is no overlap of a written buffer when the output is elsewhere: it runs
        f.apply(src, albedo=big[:W * H * 4].view(H, W, 4))
        host = np.array(alb)
        P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        out = torch.empty_like(src)
        assert f._lib.vmx_filter_apply_demodulated_device(f._h, P(src), C.c_void_p(host.ctypes.data), P(out), None, None,
                                                          None) == L.VMX_ERR_INVALID
        assert "d_albedo is not device memory" in f._lib.vmx_last_error().decode()
        refused(lambda: f.apply(src, albedo=d_alb, params=va.make_filter_params(iterations=0)), "vmx_filter_params")
        assert FS.same_bits(f.apply(src, albedo=d_alb, params=pa)[0].cpu().numpy(), want_a)  # the handle still works


# ---- progressive previews --------------------------------------------------------------------------------------------
def test_progressive_demodulated_previews():
    """70x41x16 spp with the checker bound: the demodulated preview is demodulated_frame(preview, guide of k = 0,
    albedo_plane(samples)) before the first sample, mid-frame and of the complete frame; previews change neither the
    step results nor the final frame; another albedo_samples builds the plane again"""
    import torch
    geo, cam = case("cornell8")
    opts = va.make_opts(seed=9, early_stop=False, sampling=CORRECTED)
    tex = texture(32, 32, 3)
    sc, osc = both(geo, tex)
    with sc:
        ref, _ = sc.render(cam, opts)
        n, z = FS.guide_of(sc.raycast_camera(cam, opts, 0)["raw"].cpu().numpy())
        planes = {k: DS.albedo_plane(osc, tex, cam, opts, 0, k) for k in (4, 16, 1)}
        short = va.make_filter_params(iterations=1)
        with sc.progressive(cam, opts) as quiet:  # the same steps without any preview
            quiet_mid = (quiet.step(5), quiet.preview())[1]
        with sc.progressive(cam, opts) as p:
            for point in ("no sample yet", "mid-frame", "complete"):
                plain, info = p.preview(), p.info()
                got, q = p.preview_filtered(rgba8=True, albedo_samples=4)
                assert FS.same_bits(got, DS.demodulated_frame(plain, n, z, planes[4])), point
                assert np.array_equal(q.reshape(-1, 4), O.quantize(got)[0]), point
                assert FS.same_bits(p.preview_filtered(params=short, albedo_samples=4),
                                    DS.demodulated_frame(plain, n, z, planes[4], short)), point
                # another number of samples: the plane is built again, and again on the way back
                assert FS.same_bits(p.preview_filtered(albedo_samples=16), DS.demodulated_frame(plain, n, z, planes[16])), point
                assert FS.same_bits(p.preview_filtered(albedo_samples=1), DS.demodulated_frame(plain, n, z, planes[1])), point
                d5 = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
                d4 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                p.preview_filtered_device(d5, d4, albedo_samples=4)
                p.preview()  # (the host entry synchronises the handle's stream)
                assert np.array_equal(bits(d5.cpu().numpy()), bits(got)) and np.array_equal(d4.cpu().numpy(), q)
                # the plain filtered preview is the one it was
                assert FS.same_bits(p.preview_filtered(), FS.filtered_frame(plain, n, z)), point
                assert np.array_equal(bits(p.preview()), bits(plain)) and p.info() == info  # nothing changed
                if point == "no sample yet":
                    p.step(5)
                    assert np.array_equal(bits(p.preview()), bits(quiet_mid))
                elif point == "mid-frame":
                    p.step(0)
            assert p.info()["pixels_active"] == 0
            assert np.array_equal(bits(p.preview()), bits(ref))
            for bad in (17, 1 << 20):
                with pytest.raises(va.VmxError, match="albedo_samples") as e:
                    p.preview_filtered(albedo_samples=bad)
                assert e.value.code == L.VMX_ERR_INVALID
            assert sc._lib.vmx_progressive_preview_demodulated(p._h, C.c_void_p(np.zeros(W * H * 5, np.float32).ctypes.data),
                                                               None, None, 0) == L.VMX_ERR_INVALID
            assert "albedo_samples" in sc._lib.vmx_last_error().decode()
    osc.close()


def test_progressive_demodulated_refusals():
    geo, cam = case("cornell8")
    pos, nrm, uv = geo

    def refused(call, match):
        with pytest.raises(va.VmxError, match=match) as e:
            call()
        assert e.value.code == L.VMX_ERR_INVALID

    with va.Scene(pos, nrm, uv) as s:
        s.bind_texture(texture(32, 32, 3))
        with s.progressive(cam, va.make_opts(seed=2, world=3, rank=1, stripe_rows=4)) as p:
            p.step(2)
            plain = p.preview()
            refused(lambda: p.preview_filtered(albedo_samples=4), "whole images only")
            assert np.array_equal(bits(p.preview()), bits(plain))
        opts = va.make_opts(seed=2)
        with s.progressive(cam, opts) as early, s.progressive(cam, opts) as late, s.progressive(cam, opts) as guided:
            early.step(2), late.step(2), guided.step(2)
            before = early.preview_filtered(albedo_samples=4)  # builds this handle's guide and plane
            guided.preview_filtered()  # the guide alone
            s.update(pos=pos)  # a refit to the same positions is still an update
            refused(lambda: late.preview_filtered(albedo_samples=4), "scene updated since vmx_progressive_begin")
            refused(lambda: guided.preview_filtered(albedo_samples=4), "scene updated since vmx_progressive_begin")
            refused(lambda: early.preview_filtered(albedo_samples=8), "scene updated since vmx_progressive_begin")
            # a plane built before the update keeps working
            assert np.array_equal(bits(early.preview_filtered(albedo_samples=4)), bits(before))
            assert np.array_equal(bits(late.preview()), bits(early.preview()))
