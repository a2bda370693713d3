"""Whole frames through k_shade<0> (vmx_render_device), bit-identical to the oracle's, for the cases the per-pixel
sphere bounds (vmx_kernels.hip: pixel_sphere_bound, cast_finish<.., BOUNDS>) and the pixel-per-wave loop of the dense
camera form have to get right and the other tests do not aim at: a triangle lying on a wall sphere's surface, light
spheres smaller than a pixel, across pixel borders and behind the camera, custom tables with the camera outside every
sphere and a thousandth of a unit off a surface, 64 / 128 / 256 and a ragged number of samples, strided cursors,
a sharded rank, a bound texture — each in the default, the headline (0x100) and the two-phase (0x200) form, as the
library routes them (small passes go to the fused kernel) and with every pass forced through the split kernels."""
import numpy as np
import pytest
import torch

import oracle_lib as O
import vermilion_amd as va
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu

FORMS = (0, 0x100, 0x200, 4, 4 | 0x100, 4 | 0x200)
WALLS = [dict(centre=(0, -5e7, 0), radius=5e7), dict(centre=(0, 5e7 + 1000, 0), radius=5e7),
         dict(centre=(-5e7 + 2000, 0, 0), radius=5e7, normal_sign=-1), dict(centre=(5e7 - 2000, 0, 0), radius=5e7, normal_sign=-1),
         dict(centre=(0, 0, -5e7 + 2000), radius=5e7, normal_sign=-1), dict(centre=(0, 0, 5e7 - 2000), radius=5e7)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cornell_cam(W, H, spp):
    c = scenes.cornell_camera()
    return va.make_camera(c["position"], c["rotation_deg"], W, H, spp, back_size=(3.6, 3.6 * H / W))


def with_quad(geom, a, b, c, d, n):
    """the scene plus the quad a b c d (two triangles, normal n)"""
    pos, nrm, uv = geom
    q = np.array([a + b + c, a + c + d], np.float32)
    qn = np.array([list(n) * 3] * 2, np.float32)
    quv = np.array([[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]], np.float32)
    return (np.concatenate([np.asarray(pos, np.float32).reshape(-1, 9), q]),
            np.concatenate([np.asarray(nrm, np.float32).reshape(-1, 9), qn]),
            np.concatenate([np.asarray(uv, np.float32).reshape(-1, 6), quv]))


def check_forms(geom, cam, spheres=None, tex=None, forms=FORMS, **opt):
    pos, nrm, uv = geom
    W = cam.image_res[0]
    osc = O.OracleScene(pos, nrm, uv, spheres=spheres)
    if tex is not None:
        osc.bind_texture(tex)
    ref, rst = osc.render(cam, va.make_opts(**opt))
    osc.close()
    with va.Scene(pos, nrm, uv, spheres=spheres) as sc:
        if tex is not None:
            sc.bind_texture(tex)
        for form in forms:
            out = torch.full((ref.shape[0], W, 5), -7.0, dtype=torch.float32, device="cuda")
            st = sc.render_device(cam, va.make_opts(pipeline=form, **opt), out.data_ptr())
            torch.cuda.synchronize()
            img = out.cpu().numpy()
            same = bits(img) == bits(ref)
            assert np.all(same), "form %#x %r: %d of %d values differ" % (form, opt, int((~same).sum()), same.size)
            assert st["samples"] == rst["samples"], (form, opt)
    return ref


@pytest.mark.parametrize("spp", [64, 128, 256, 100])
def test_reference_room_sample_counts(spp):
    check_forms(scenes.cornell8(), cornell_cam(48, 32, spp), seed=31 + spp, early_stop=False)


def test_floor_on_a_wall_spheres_surface():
    """a quad at y = 0, the surface of the room's floor sphere under the camera: the triangle distance and the sphere's
    root agree to the last digits, on either side of one another"""
    geom = with_quad(scenes.cornell8(), [-1900.0, 0.0, -1900.0], [1900.0, 0.0, -1900.0], [1900.0, 0.0, 1900.0],
                     [-1900.0, 0.0, 1900.0], (0.0, 1.0, 0.0))
    c = scenes.cornell_camera()
    cam = va.make_camera(c["position"], (-25.0, 10.0, 0.0), 48, 32, 64, back_size=(3.6, 2.4))
    for es in (False, True):
        check_forms(geom, cam, seed=41, early_stop=es)


def test_small_straddling_and_hidden_lights():
    c = scenes.cornell_camera()
    cam = cornell_cam(48, 32, 64)
    _, d = O.primary_rays(cam, va.make_opts(seed=1), 0)
    pos = np.array(c["position"], np.float64)
    px = 3.6 / 48 / 6.0  # a pixel's angle
    a, b = d[10 * 48 + 30].astype(np.float64), d[12 * 48 + 9].astype(np.float64)
    lights = [dict(centre=tuple(pos + 900.0 * a), radius=900.0 * px * 0.2, colour=(40.0, 30.0, 20.0), emit=True),   # a fraction of a pixel
              dict(centre=tuple(pos + 700.0 * b), radius=700.0 * px * 1.7, colour=(3.0, 4.0, 5.0), emit=True),     # across pixel borders
              dict(centre=tuple(pos - 500.0 * a), radius=120.0, colour=(9.0, 9.0, 9.0), emit=True)]                # behind the camera
    ref = check_forms(scenes.cornell8(), cam, spheres=va.spheres_array(lights + WALLS), seed=43, early_stop=False)
    assert ref[:, :, :3].max() > 0.5  # a light is seen


def test_custom_tables_camera_outside_and_on_a_surface():
    c = scenes.cornell_camera()
    cam = cornell_cam(48, 32, 64)
    pos = np.array(c["position"], np.float64)
    r = np.random.RandomState(44)
    outside = [dict(centre=tuple(r.uniform((-400, 50, -500), (400, 800, 1200))), radius=float(r.uniform(20, 250)),
                    colour=tuple(r.uniform(0, 5, 3)), emit=bool(i % 2 == 0), normal_sign=-1.0 if i % 3 == 0 else 1.0) for i in range(9)]
    assert all(np.linalg.norm(np.array(s["centre"]) - pos) > s["radius"] + 50 for s in outside)
    check_forms(scenes.cornell8(), cam, spheres=va.spheres_array(outside), seed=44, early_stop=False)
    u = np.array([0.3, -0.2, -0.933])
    u /= np.linalg.norm(u)
    near = [dict(centre=tuple(pos + (800.0 - 1e-3) * u), radius=800.0, colour=(0.5, 0.7, 0.9), emit=True, normal_sign=-1),  # 1e-3 inside
            dict(centre=tuple(pos - (300.0 + 1e-3) * u), radius=300.0, colour=(2.0, 1.0, 0.5), emit=True),                # 1e-3 outside
            dict(centre=tuple(pos + np.array([0.0, 1e-3, 0.0])), radius=2500.0, normal_sign=-1)]                          # at the centre
    for es in (False, True):
        check_forms(scenes.cornell8(), cam, spheres=va.spheres_array(near + WALLS), seed=45, early_stop=es)


def test_strided_cursors_in_the_dense_form():
    """early stop with floor(sqrt(spp)) + 4 = 64 samples in a pass: the dense form with a lead and, after the first pass,
    strided cursors"""
    cam = cornell_cam(16, 8, 3600)
    check_forms(scenes.cornell8(), cam, forms=(0, 4 | 0x100, 4 | 0x200), seed=46, early_stop=True)


def test_sharded_rank_and_bound_texture():
    geom = scenes.cornell8()
    cam = cornell_cam(48, 32, 64)
    for rank in (0, 1):
        check_forms(geom, cam, seed=47, early_stop=False, rank=rank, world=2, stripe_rows=4)
    tex = np.random.RandomState(48).uniform(0.1, 1.0, size=(8, 8, 3)).astype(np.float32)
    pos, nrm, uv = geom
    check_forms((pos, nrm, uv * np.float32(3.7) - np.float32(1.2)), cam, tex=tex, seed=48, early_stop=False)
    check_forms((pos, nrm, uv * np.float32(3.7) - np.float32(1.2)), cornell_cam(48, 32, 128), tex=tex, seed=49, early_stop=True)
