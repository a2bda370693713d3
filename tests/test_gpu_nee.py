"""Light sampling on the device (vmx_radiance_nee, vmx_render_nee*, k_nee) against its definition tests/nee_spec.py, bit for
bit: explicit rays and frames, every sphere table and scene state the entry must follow, the ray counts."""
import functools

import numpy as np
import pytest

import nee_cases as K
import nee_spec as N
import oracle_lib as O
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
LIBM = L.VMX_SAMPLING_LIBM_DOUBLE


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, what):
    diff = bits(got) != bits(want)
    assert not diff.any(), "%s: %d of %d values differ, first at %s" % (what, int(diff.sum()), diff.size,
                                                                         np.argwhere(diff)[0].tolist())


def camera(scene, W, H, spp):
    c = scenes.cornell_camera() if scene == "cornell8" else scenes.lattice_camera()
    return va.make_camera(c["position"], c["rotation_deg"], W, H, spp)


@functools.lru_cache(maxsize=None)
def spec_radiance(scene, table, channels, sampling, seed):
    """the spec's answer for the golden camera rays of the scene, computed once and shared"""
    pos, nrm, uv, o, d, _ = K.golden(scene)
    tb = K.table(table)
    tex = K.texture(channels) if channels else None
    osc = O.OracleScene(pos, nrm, uv, spheres=tb)
    if tex is not None:
        osc.bind_texture(tex)
    out, st = N.radiance(osc, o, d, seed, tb, sampling, True, tex)
    osc.close()
    out.setflags(write=False)
    return out, st


def device_scene(scene, table, channels, builder=L.VMX_BVH_REFERENCE):
    pos, nrm, uv, _, _, _ = K.golden(scene)
    sc = va.Scene(pos, nrm, uv, spheres=K.table(table), builder=builder)
    if channels:
        sc.bind_texture(K.texture(channels))
    return sc


RADIANCE = [("cornell8", "default", 0, K.CORRECTED), ("lattice", "default", 0, K.CORRECTED), ("cornell8", "overlap", 0, K.CORRECTED),
            ("cornell8", "three", 0, K.CORRECTED), ("cornell8", "single", 3, K.CORRECTED), ("lattice", "default", 4, K.CORRECTED),
            ("lattice", "overlap", 1, K.CORRECTED | LIBM), ("cornell8", "default", 0, K.CORRECTED | LIBM)]


@pytest.mark.parametrize("scene,table,channels,sampling", RADIANCE)
def test_radiance_nee_matches_the_spec(scene, table, channels, sampling):
    """the golden camera rays (1536 of cornell8, 960 of the lattice): accumColour and the ray counts"""
    _, _, _, o, d, _ = K.golden(scene)
    want, wst = spec_radiance(scene, table, channels, sampling, 7)
    with device_scene(scene, table, channels) as sc:
        got, st = sc.radiance_nee(o, d, K.opts(7, sampling))
    same(got, want, "radiance")
    assert st["rays_primary"] == wst["rays_primary"] == len(o)
    assert st["rays_secondary"] == wst["rays_secondary"] and st["samples"] == len(o)
    assert wst["rays_shadow"] > 0


@pytest.mark.parametrize("scene", ["cornell8", "lattice"])
def test_radiance_nee_without_emitters_is_corrected_radiance(scene):
    _, _, _, o, d, _ = K.golden(scene)
    want, wst = spec_radiance(scene, "none", 0, K.CORRECTED, 9)
    with device_scene(scene, "none", 0) as sc:
        got, st = sc.radiance_nee(o, d, K.opts(9))
        plain, pst = sc.radiance(o, d, K.opts(9))
    same(got, want, "against the spec")
    same(got, plain, "against Scene.radiance")
    assert st["rays_secondary"] == pst["rays_secondary"] == wst["rays_secondary"] and wst["rays_shadow"] == 0


def test_radiance_nee_of_rays_that_start_inside_an_emitter():
    tb, o, d = K.inside_rays(64)
    pos, nrm, uv, _, _, _ = K.golden("cornell8")
    osc = O.OracleScene(pos, nrm, uv, spheres=tb)
    want, wst = N.radiance(osc, o, d, 41, tb, K.CORRECTED, True)
    with va.Scene(pos, nrm, uv, spheres=tb) as sc:
        got, st = sc.radiance_nee(o, d, K.opts(41))
    same(got, want, "inside rays")
    assert st["rays_secondary"] == wst["rays_secondary"]


@pytest.mark.parametrize("n", [1, 63, 65])
def test_radiance_nee_of_a_few_rays(n):
    """ray i runs on stream (seed, i, 0) whatever n is: the first n rows of the whole batch's answer"""
    _, _, _, o, d, _ = K.golden("cornell8")
    want, _ = spec_radiance("cornell8", "default", 0, K.CORRECTED, 7)
    with device_scene("cornell8", "default", 0) as sc:
        got, st = sc.radiance_nee(o[:n], d[:n], K.opts(7))
        none, _ = sc.radiance_nee(o[:0], d[:0], K.opts(7))
    same(got, want[:n], "n = %d" % n)
    assert st["samples"] == n and none.shape == (0, 4)


# ---- frames ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spec_frame(scene, table, channels, W, H, spp, seed, tree=False):
    pos, nrm, uv, _, _, _ = K.golden(scene)
    tb = K.table(table)
    tex = K.texture(channels) if channels else None
    t = None
    if tree:
        with device_scene(scene, table, 0, builder=L.VMX_BVH_LBVH) as sc:
            t = sc.bvh()
    osc = O.OracleScene(pos, nrm, uv, spheres=tb, tree=t)
    if tex is not None:
        osc.bind_texture(tex)
    out, st = N.frame(osc, camera(scene, W, H, spp), K.opts(seed), tb, tex)
    osc.close()
    out.setflags(write=False)
    return out, st


FRAMES = [("cornell8", 48, 32, 8, 0), ("lattice", 40, 24, 4, 0), ("cornell8", 37, 5, 4, 0), ("cornell8", 37, 5, 4, 1)]


@pytest.mark.parametrize("scene,W,H,spp,batch", FRAMES)
def test_render_nee_matches_the_spec(scene, W, H, spp, batch):
    """frames, the ray counts and the sample count; 37 x 5: a width that is no multiple of 64; samples_per_batch = 1: a pass
    per sample, the same frame"""
    want, wst = spec_frame(scene, "default", 0, W, H, spp, 5)
    with device_scene(scene, "default", 0) as sc:
        got, st = sc.render_nee(camera(scene, W, H, spp), K.opts(5, samples_per_batch=batch))
        again, _ = sc.render_nee(camera(scene, W, H, spp), K.opts(5, samples_per_batch=batch))
    same(got, want, "frame")
    assert got.tobytes() == again.tobytes()  # two identical calls, identical bytes
    assert (got[..., 3] == 1).all() and (got[..., 4] == spp).all()
    assert st["samples"] == wst["samples"] == W * H * spp
    assert st["rays_primary"] == wst["rays_primary"] and st["rays_secondary"] == wst["rays_secondary"]
    if batch:
        assert st["passes"] == spp


def test_render_nee_follows_the_scenes_state():
    """after set_spheres with another emitter count, after update and after bind_texture the frame is that of a scene created
    in that state — and that of the spec"""
    pos, nrm, uv, _, _, _ = K.golden("cornell8")
    cam, opts = camera("cornell8", 37, 5, 4), K.opts(5)
    moved = pos.copy().reshape(-1, 3, 3)
    moved[4:] += np.float32([64.0, 32.0, -16.0])  # the block
    moved = moved.reshape(-1, 9)
    tex = K.texture(3)
    with va.Scene(pos, nrm, uv) as sc:
        first, _ = sc.render_nee(cam, opts)
        same(first, spec_frame("cornell8", "default", 0, 37, 5, 4, 5)[0], "default table")
        sc.set_spheres(K.table("three"))
        got, _ = sc.render_nee(cam, opts)
        with va.Scene(pos, nrm, uv, spheres=K.table("three")) as fresh:
            want, _ = fresh.render_nee(cam, opts)
        same(got, want, "after set_spheres")
        same(got, spec_frame("cornell8", "three", 0, 37, 5, 4, 5)[0], "after set_spheres, against the spec")
        assert not np.array_equal(bits(got), bits(first))
        sc.bind_texture(tex)
        got_t, _ = sc.render_nee(cam, opts)
        same(got_t, spec_frame("cornell8", "three", 3, 37, 5, 4, 5)[0], "after bind_texture, against the spec")
        sc.update(pos=moved)
        got_u, _ = sc.render_nee(cam, opts)
        with va.Scene(moved, nrm, uv, spheres=K.table("three")) as fresh:
            fresh.bind_texture(tex)
            want_u, _ = fresh.render_nee(cam, opts)
        same(got_u, want_u, "after update")
        assert not np.array_equal(bits(got_u), bits(got_t))


def test_render_nee_on_a_device_built_tree():
    """an LBVH scene: the frame of the spec fed the exported tree"""
    want, wst = spec_frame("lattice", "default", 0, 40, 24, 4, 5, tree=True)
    with device_scene("lattice", "default", 0, builder=L.VMX_BVH_LBVH) as sc:
        got, st = sc.render_nee(camera("lattice", 40, 24, 4), K.opts(5))
    same(got, want, "LBVH frame")
    assert st["rays_secondary"] == wst["rays_secondary"]


def test_render_nee_device_on_a_callers_stream():
    import torch
    cam, opts = camera("cornell8", 48, 32, 8), K.opts(5)
    with device_scene("cornell8", "default", 0) as sc:
        want, wst = sc.render_nee(cam, opts)
        out = torch.full((32, 48, 5), -7.0, dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        st = sc.render_nee_device(cam, opts, out.data_ptr(), side.cuda_stream)
        side.synchronize()
        got = out.cpu().numpy()
        out2 = torch.full((32, 48, 5), -7.0, dtype=torch.float32, device="cuda")
        sc.render_nee_device(cam, opts, out2.data_ptr())
        torch.cuda.synchronize()
    same(got, want, "on a stream")
    same(out2.cpu().numpy(), want, "on the scene's stream")
    assert st["rays_secondary"] == wst["rays_secondary"]
