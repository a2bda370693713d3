"""Emissive triangles on the device (vmx_scene_set_emitters, k_emitter_table, k_nee_mesh) against their definition
tests/nee_mesh_spec.py, bit for bit: the derived table, explicit rays, frames through every entry that reaches the
light-sampled pass routine, updates with every builder, and one case at VMX_CU_LIMIT = 1."""
import functools

import numpy as np
import pytest

import nee_cases as K
import nee_mesh_cases as MC
import nee_mesh_spec as M
import nee_spec as N
import oracle_lib as O
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import dist as vdist

pytestmark = pytest.mark.gpu
LIBM = L.VMX_SAMPLING_LIBM_DOUBLE
SEED = 7
BUILDERS = [L.VMX_BVH_REFERENCE, L.VMX_BVH_SAH, L.VMX_BVH_LBVH, L.VMX_BVH_PLOC]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, what):
    diff = bits(got) != bits(want)
    assert not diff.any(), "%s: %d of %d values differ, first at %s" % (what, int(diff.sum()), diff.size,
                                                                         np.argwhere(diff)[0].tolist())


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def case(name):
    return MC.case(name)


@functools.lru_cache(maxsize=None)
def spec_table(name):
    c = case(name)
    return M.table(MC.current(c), c["ids"], c["radiance"])


def oracle_scene(c, channels=0):
    osc = O.OracleScene(MC.current(c), c["nrm"], c["uv"], spheres=K.table(c["spheres"]))
    tex = K.texture(channels) if channels else None
    if tex is not None:
        osc.bind_texture(tex)
    return osc, tex


@functools.lru_cache(maxsize=None)
def spec_radiance(name, channels=0, sampling=K.CORRECTED, seed=SEED):
    """the spec's answer for the case's rays, computed once and shared"""
    c = case(name)
    osc, tex = oracle_scene(c, channels)
    out, st = M.radiance(osc, c["o"], c["d"], seed, K.table(c["spheres"]), sampling, True, tex, emitters=spec_table(name))
    osc.close()
    out.setflags(write=False)
    return out, st


def camera(c, W, H, spp):
    return va.make_camera(c["camera"]["position"], c["camera"]["rotation_deg"], W, H, spp)


@functools.lru_cache(maxsize=None)
def spec_frame(name, W, H, spp, seed=SEED):
    c = case(name)
    osc, _ = oracle_scene(c)
    out, st = M.frame(osc, camera(c, W, H, spp), K.opts(seed), K.table(c["spheres"]), None, spec_table(name))
    osc.close()
    out.setflags(write=False)
    return out, st


def device_scene(name, channels=0, builder=L.VMX_BVH_REFERENCE, table_first=True):
    """the case on the device: created on its first positions, the table set, then the refit where the case has one (the
    table follows the update); table_first=False sets the table last"""
    c = case(name)
    sc = va.Scene(c["pos"], c["nrm"], c["uv"], spheres=K.table(c["spheres"]), builder=builder)
    if channels:
        sc.bind_texture(K.texture(channels))
    if table_first:
        sc.set_emitters(c["ids"], c["radiance"])
    if c["moved"] is not None:
        sc.update(pos=c["moved"])
    if not table_first:
        sc.set_emitters(c["ids"], c["radiance"])
    return sc


def check_table(got, want, what):
    assert len(got) == want["n"], what
    assert np.array_equal(got["tri_id"], want["ids"]), what
    same(got["radiance"], want["radiance"], what + ": radiance")
    for key in ("area", "weight", "cdf"):
        assert np.array_equal(got[key].view(np.uint64), want[key].view(np.uint64)), (what, key, got[key][:4], want[key][:4])


# ---- the table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.ALL)
def test_the_derived_table_is_the_specs(name):
    with device_scene(name) as sc:
        check_table(sc.emitters(), spec_table(name), name)


# ---- batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.ALL)
def test_radiance_nee_matches_the_spec(name):
    c = case(name)
    want, wst = spec_radiance(name)
    with device_scene(name, table_first=name != "lattice_63") as sc:
        got, st = sc.radiance_nee(c["o"], c["d"], K.opts(SEED))
    same(got, want, name)
    assert st["rays_primary"] == wst["rays_primary"] == len(c["o"])
    assert st["rays_secondary"] == wst["rays_secondary"] and wst["rays_shadow"] > 0


VARIANTS = [("quad_single", 3, K.CORRECTED), ("lattice_65", 4, K.CORRECTED), ("quad_overlap", 1, K.CORRECTED | LIBM),
            ("block_top", 0, K.CORRECTED | LIBM)]


@pytest.mark.parametrize("name,channels,sampling", VARIANTS)
def test_radiance_nee_with_textures_and_libm_double(name, channels, sampling):
    c = case(name)
    want, wst = spec_radiance(name, channels, sampling)
    with device_scene(name, channels) as sc:
        got, st = sc.radiance_nee(c["o"], c["d"], K.opts(SEED, sampling))
    same(got, want, name)
    assert st["rays_secondary"] == wst["rays_secondary"]
    if channels or sampling != K.CORRECTED:
        assert (bits(want) != bits(spec_radiance(name)[0])).any(), "the variant changes nothing: it tests nothing"


@pytest.mark.parametrize("n", [1, 63, 65])
def test_radiance_nee_of_a_few_rays_on_the_device(n):
    """ray i runs on stream (seed, i, 0) whatever n is; radiance_nee_device on device arrays"""
    import torch
    c = case("quad_single")
    want, _ = spec_radiance("quad_single")
    with device_scene("quad_single") as sc:
        got, st = sc.radiance_nee(c["o"][:n], c["d"][:n], K.opts(SEED))
        d_o, d_d = dev(c["o"][:n]), dev(c["d"][:n])
        out = torch.full((n + 1, 4), -7.0, dtype=torch.float32, device="cuda")
        sc.radiance_nee_device(d_o.data_ptr(), d_d.data_ptr(), n, K.opts(SEED), out.data_ptr())
        torch.cuda.synchronize()
    same(got, want[:n], "n = %d" % n)
    same(out[:n].cpu().numpy(), want[:n], "device arrays, n = %d" % n)
    assert (out[n].cpu().numpy() == -7.0).all() and st["samples"] == n


# ---- frames ----------------------------------------------------------------------------------------------------------------
FRAMES = [(48, 32, 8), (37, 5, 4)]


@pytest.mark.parametrize("batch", [0, 1])
@pytest.mark.parametrize("W,H,spp", FRAMES)
def test_frames_from_one_call_and_from_handles(W, H, spp, batch):
    name = "quad_overlap"
    c = case(name)
    want, wst = spec_frame(name, W, H, spp)
    cam, opts = camera(c, W, H, spp), K.opts(SEED, samples_per_batch=batch)
    with device_scene(name) as sc:
        one, st = sc.render_nee(cam, opts)
        same(one, want, "render_nee")
        assert st["rays_secondary"] == wst["rays_secondary"] and st["samples"] == W * H * spp
        for step in (1, 3):
            with sc.progressive_nee(cam, opts) as p:
                while p.info()["pixels_active"]:
                    p.step(step)
                same(p.preview(), want, "handle in steps of %d" % step)
        yy, xx = np.mgrid[0:H, 0:W]
        with sc.progressive_nee(cam, opts) as p:  # one selected and one budgeted step, then the rest
            p.step(1)
            _, nsel = p.step_selected(2, dev(((xx + yy) % 3 == 0).astype(np.uint8)))
            assert nsel == int(((xx + yy) % 3 == 0).sum())
            _, nbud = p.step_budget(dev(((xx * 7 + yy) % 4).astype(np.int32)))
            assert nbud > 0
            while p.info()["pixels_active"]:
                p.step(3)
            same(p.preview(), want, "handle after a selected and a budgeted step")


@pytest.mark.parametrize("W,H,spp", FRAMES)
def test_frames_from_two_ranks_and_from_a_device_list(W, H, spp):
    name = "quad_overlap"
    c = case(name)
    want, _ = spec_frame(name, W, H, spp)
    cam, stripe = camera(c, W, H, spp), 2
    with device_scene(name) as sc:
        parts = [vdist.render_nee_local(sc, cam, K.opts(SEED, rank=r, world=2, stripe_rows=stripe))[0].cpu().numpy() for r in range(2)]
    same(vdist.assemble_host(parts, W, H, stripe, 2), want, "two ranks assembled")
    with va.MultiScene(c["pos"], c["nrm"], c["uv"], spheres=K.table(c["spheres"]), devices=[0, 0]) as multi:
        multi.set_emitters(c["ids"], c["radiance"])
        got, _ = multi.render_nee(cam, K.opts(SEED))
        same(got, want, "a repeated-device list")
        multi.set_emitters(None)
        dark, _ = multi.render_nee(cam, K.opts(SEED))
    assert (bits(dark) != bits(want)).any()


# ---- updates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
def test_the_table_and_the_frames_follow_updates(builder):
    """a refit, a rebuild with the scene's builder and a new sphere table, each against a FRESH scene of the same builder on
    the same arrays; the table against the spec as well"""
    name = "lattice_65"
    c = case(name)
    cam, opts = camera(c, 40, 24, 4), K.opts(SEED)
    moved = c["moved"]
    other = K.table("overlap")

    def fresh(pos, spheres):
        with va.Scene(pos, c["nrm"], c["uv"], spheres=spheres, builder=builder) as f:
            f.set_emitters(c["ids"], c["radiance"])
            return f.emitters(), f.render_nee(cam, opts)[0], f.radiance_nee(c["o"], c["d"], opts)[0]

    with va.Scene(c["pos"], c["nrm"], c["uv"], spheres=K.table(c["spheres"]), builder=builder) as sc:
        sc.set_emitters(c["ids"], c["radiance"])
        before = sc.emitters()
        check_table(before, M.table(c["pos"], c["ids"], c["radiance"]), "before any update")
        for what, change, pos, spheres in (("refit", lambda: sc.update(pos=moved), moved, K.table(c["spheres"])),
                                           ("rebuild", lambda: sc.update(pos=c["pos"], rebuild=True), c["pos"], K.table(c["spheres"])),
                                           ("rebuild moved", lambda: sc.update(pos=moved, rebuild=True), moved, K.table(c["spheres"])),
                                           ("set_spheres", lambda: sc.set_spheres(other), moved, other)):
            change()
            ftable, fframe, frad = fresh(pos, spheres)
            table = sc.emitters()
            check_table(table, M.table(pos, c["ids"], c["radiance"]), what)
            assert table.tobytes() == ftable.tobytes(), what
            same(sc.render_nee(cam, opts)[0], fframe, what + ": frame")
            same(sc.radiance_nee(c["o"], c["d"], opts)[0], frad, what + ": rays")
        assert (before["area"] != table["area"]).any(), "the refit changed no area: the case tests nothing"
    if builder == L.VMX_BVH_REFERENCE:
        same(frad, M.radiance(*_oracle_args(c, moved, other), emitters=M.table(moved, c["ids"], c["radiance"]))[0], "the last state against the spec")


def _oracle_args(c, pos, spheres):
    return O.OracleScene(pos, c["nrm"], c["uv"], spheres=spheres), c["o"], c["d"], SEED, spheres


def test_a_cleared_table_and_a_live_handle():
    name = "quad_single"
    c = case(name)
    opts = K.opts(SEED)
    with va.Scene(c["pos"], c["nrm"], c["uv"], spheres=K.table(c["spheres"])) as never:
        plain, pst = never.radiance_nee(c["o"], c["d"], opts)
        assert len(never.emitters()) == 0
    with device_scene(name) as sc:
        lit, _ = sc.radiance_nee(c["o"], c["d"], opts)
        sc.set_emitters(None)
        assert len(sc.emitters()) == 0
        got, st = sc.radiance_nee(c["o"], c["d"], opts)
        assert got.tobytes() == plain.tobytes() and st["rays_secondary"] == pst["rays_secondary"]
        assert (bits(lit) != bits(plain)).any()
        osc = O.OracleScene(c["pos"], c["nrm"], c["uv"], spheres=K.table(c["spheres"]))
        same(got, N.radiance(osc, c["o"], c["d"], SEED, K.table(c["spheres"]))[0], "nee_spec without a table")
        # a live handle is refused after set_emitters, as after set_spheres
        cam = camera(c, 16, 8, 4)
        with sc.progressive_nee(cam, opts) as p:
            p.step(1)
            sc.set_emitters(c["ids"], c["radiance"])
            with pytest.raises(L.VmxError, match="scene updated since vmx_progressive_begin"):
                p.step(1)
        # what vmx_scene_set_emitters refuses on a real scene: the scene is as it was
        for ids, rad in (([10], [1, 1, 1]), ([3, 3], [1, 1, 1]), ([3], [1, -1, 1]), ([3], [np.inf, 1, 1]), (list(range(11)), [1, 1, 1])):
            with pytest.raises(L.VmxError):
                sc.set_emitters(ids, rad)
        same(sc.radiance_nee(c["o"], c["d"], opts)[0], lit, "after the refused tables")


# ---- small work loops ------------------------------------------------------------------------------------------------------
def test_render_nee_with_a_table_under_the_cu_limit(monkeypatch):
    """created as tests/test_gpu_cu_limit.py creates its scenes: the persistent loop and the refill run at test size"""
    name, W, H, spp = "quad_overlap", 48, 32, 8
    c = case(name)
    monkeypatch.setenv("VMX_CU_LIMIT", "1")
    sc = device_scene(name)
    monkeypatch.delenv("VMX_CU_LIMIT")
    with sc:
        assert sc.compute_units == 1, "VMX_CU_LIMIT was ignored"
        items = W * H * spp
        print("load: k_nee_mesh items=%d compute_units=1 reservations_per_wave=%.1f" % (items, items / (64.0 * 32)))
        assert items >= 4 * 64 * 32
        got, st = sc.render_nee(camera(c, W, H, spp), K.opts(SEED))
    want, wst = spec_frame(name, W, H, spp)
    same(got, want, "frame under VMX_CU_LIMIT = 1")
    assert st["rays_secondary"] == wst["rays_secondary"]
