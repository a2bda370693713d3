"""Changing lights on the GPU: a scene whose sphere table was replaced (vmx_scene_set_spheres / vmx_multi_set_spheres)
is, bit for bit, a scene created with that table — frames of every pipeline form, ray counts, G-buffers, radiance,
progressive renders, BruteForceTracer — through changes of count, refits and device-built trees; what the call does to
handles and work in flight; and k_motion_spheres against its numpy restatement (sphere_motion_spec.py), every record."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as O
import sphere_motion_spec as SS
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
RAY_COUNTS = ("rays_primary", "rays_secondary", "samples", "samples_discarded")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- tables -----------------------------------------------------------------------------------------------------------
def table_a():
    return va.default_spheres()


def dimmed():
    """the big light at a quarter"""
    t = va.default_spheres()
    t[1].colour[:] = [c * 0.25 for c in t[1].colour]
    return t


def light_moved():
    """the small light 40 units along: which rays have a light in reach changes"""
    t = va.default_spheres()
    t[0].centre[:] = [t[0].centre[0] + 40.0, t[0].centre[1], t[0].centre[2]]
    return t


def emitter_last():
    """the small light in the last slot, the only emitter left (the big one no longer emits): the emitter prefix, 2 in
    A, is 8 — a scene that kept A's would not see the light at all"""
    a = va.default_spheres()
    t = (L.Sphere * 8)()
    for dst, src in enumerate([1, 2, 3, 4, 5, 6, 7, 0]):
        C.memmove(C.byref(t[dst]), C.byref(a[src]), C.sizeof(L.Sphere))
    t[0].flags = 0
    return t


def no_emitter():
    t = va.default_spheres()
    t[0].flags = t[1].flags = 0
    return t


TABLES = {"dimmed": dimmed, "light_moved": light_moved, "emitter_last": emitter_last, "no_emitter": no_emitter}


def cornell():
    c = scenes.cornell_camera()
    return scenes.cornell8(), va.make_camera(c["position"], c["rotation_deg"], 48, 32, 16)


def lattice():
    c = scenes.lattice_camera()
    return scenes.lattice(), va.make_camera(c["position"], c["rotation_deg"], 40, 24, 16)


SCENES = {"cornell": cornell, "lattice": lattice}
# (pipeline form, sampling, early stop): forms 0, 1 and 4; corrected sampling; dead-path elision; early stop on and off
FORMS = [(0, L.VMX_SAMPLING_PARITY, True), (1, L.VMX_SAMPLING_PARITY, True), (4, L.VMX_SAMPLING_PARITY, True),
         (0, L.VMX_SAMPLING_PARITY, False), (4, L.VMX_SAMPLING_PARITY, False), (0, L.VMX_SAMPLING_CORRECTED, True),
         (4, L.VMX_SAMPLING_CORRECTED, False), (0, L.VMX_SAMPLING_ELIDE_DEAD, True), (4, L.VMX_SAMPLING_ELIDE_DEAD, False)]


def everything(sc, cam, forms=FORMS, extras=True):
    """what a scene answers, as words: {name: uint32 array}"""
    out = {}
    for form, sampling, early in forms:
        img, st = sc.render(cam, va.make_opts(seed=5, early_stop=early, sampling=sampling, pipeline=form))
        out[f"frame {form} {sampling:#x} {early}"] = bits(img)
        out[f"rays {form} {sampling:#x} {early}"] = np.array([st[k] for k in RAY_COUNTS], np.uint64)
    opts = va.make_opts(seed=5)
    out["gbuffer"] = bits(sc.raycast_camera(cam, opts, 0)["raw"].cpu().numpy())
    if extras:
        o, d = O.primary_rays(cam, opts, 1)
        out["radiance"] = bits(sc.radiance(o, d, opts)[0])
        with sc.progressive(cam, opts) as p:
            p.step(4)
            p.step(0)
            out["progressive"] = bits(p.preview())
        out["bruteforce"] = bits(sc.render_bruteforce(cam, opts)[0])
    return out


def assert_same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


def differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in a)


# ---- set_spheres equals a fresh scene ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("scene", list(SCENES))
def test_set_spheres_equals_a_fresh_scene(scene, table):
    (pos, nrm, uv), cam = SCENES[scene]()
    b = TABLES[table]()
    with va.Scene(pos, nrm, uv, spheres=b) as fresh:
        want = everything(fresh, cam)
    with va.Scene(pos, nrm, uv, spheres=table_a()) as sc:
        before = everything(sc, cam)
        assert differs(before, want)  # (the table matters to what is compared)
        sc.set_spheres(b)
        assert sc.describe()["nspheres"] == len(b)
        assert_same(everything(sc, cam), want, "after set")
        sc.set_spheres(table_a())
        assert_same(everything(sc, cam), before, "set back")
        sc.set_spheres(None)  # (NULL, 0: the reference's table, which A is)
        short = everything(sc, cam, FORMS[:3], False)
        assert_same(short, {k: before[k] for k in short}, "NULL")


def test_the_count_may_change_between_calls():
    """8 -> 3 -> 16 -> 0 -> NULL, 0 on one scene: after each the scene is a fresh scene of that table"""
    (pos, nrm, uv), cam = cornell()
    base = va.default_spheres()
    sixteen = SS.moved_tables(base, 16, scenes.cornell_camera()["position"])[0]
    forms = [FORMS[0], FORMS[2], FORMS[8]]
    with va.Scene(pos, nrm, uv, spheres=table_a()) as sc:
        last = None
        for name, t in (("3", SS.copy_table(base, 3)), ("16", sixteen), ("0", (L.Sphere * 0)()), ("NULL", None), ("3 again", SS.copy_table(base, 3))):
            with va.Scene(pos, nrm, uv, spheres=t) as fresh:
                want = everything(fresh, cam, forms)
                n = fresh.describe()["nspheres"]
            sc.set_spheres(t)
            assert sc.describe()["nspheres"] == n == (8 if t is None else len(t))
            got = everything(sc, cam, forms)
            assert_same(got, want, name)
            assert last is None or differs(got, last), name
            last = got


@pytest.mark.parametrize("builder", ["lbvh", "ploc", "sah"])
def test_other_builders(builder):
    (pos, nrm, uv), cam = lattice()
    b = light_moved()
    kind = {"lbvh": L.VMX_BVH_LBVH, "ploc": L.VMX_BVH_PLOC, "sah": L.VMX_BVH_SAH}[builder]
    with va.Scene(pos, nrm, uv, spheres=b, builder=kind) as fresh:
        want = everything(fresh, cam)
    with va.Scene(pos, nrm, uv, spheres=table_a(), builder=kind) as sc:
        sc.set_spheres(b)
        assert_same(everything(sc, cam), want, builder)


@pytest.mark.parametrize("rebuild", [False, True])
def test_geometry_updates_and_table_updates_do_not_disturb_each_other(rebuild):
    (pos, nrm, uv), cam = lattice()
    moved = np.array(pos, np.float32).reshape(-1, 9).copy()
    moved[::3, 1::3] += np.float32(35.0)
    b = dimmed()
    forms = FORMS[:5]
    with va.Scene(pos, nrm, uv, spheres=b) as fresh:
        fresh.update(moved, rebuild=rebuild)
        want = everything(fresh, cam, forms)
    with va.Scene(pos, nrm, uv, spheres=table_a()) as sc:  # the table first, then the geometry
        sc.set_spheres(b)
        sc.update(moved, rebuild=rebuild)
        assert_same(everything(sc, cam, forms), want, "table, geometry")
    with va.Scene(pos, nrm, uv, spheres=table_a()) as sc:  # the geometry first
        sc.update(moved, rebuild=rebuild)
        sc.set_spheres(b)
        assert_same(everything(sc, cam, forms), want, "geometry, table")
        sc.update(np.array(pos, np.float32).reshape(-1, 9), rebuild=rebuild)
        sc.set_spheres(table_a())
        sc.update(moved, rebuild=rebuild)
        sc.set_spheres(b)
        assert_same(everything(sc, cam, forms), want, "there and back")


# ---- lifecycle --------------------------------------------------------------------------------------------------------------
def test_progressive_handles_end_at_the_call():
    (pos, nrm, uv), cam = cornell()
    opts = va.make_opts(seed=5)
    b = dimmed()
    with va.Scene(pos, nrm, uv, spheres=b) as fresh:
        want = bits(fresh.render(cam, opts)[0])
    with va.Scene(pos, nrm, uv, spheres=table_a()) as sc:
        with sc.progressive(cam, opts) as p:
            p.step(4)
            sc.set_spheres(b)
            with pytest.raises(L.VmxError, match="scene updated since vmx_progressive_begin") as e:
                p.step(4)
            assert e.value.code == L.VMX_ERR_INVALID
        with sc.progressive(cam, opts) as p:
            p.step(4)
            p.step(0)
            assert np.array_equal(bits(p.preview()), want)


def test_a_refused_call_leaves_the_scene_as_it_was():
    (pos, nrm, uv), cam = cornell()
    opts = va.make_opts(seed=5)
    with va.Scene(pos, nrm, uv, spheres=table_a()) as sc:
        before = everything(sc, cam, FORMS[:3])
        big = (L.Sphere * 17)()
        some = dimmed()
        with sc.progressive(cam, opts) as p:
            p.step(4)
            assert sc._lib.vmx_scene_set_spheres(sc._h, C.addressof(big), 17) == L.VMX_ERR_INVALID
            assert sc._lib.vmx_scene_set_spheres(sc._h, None, 3) == L.VMX_ERR_INVALID
            assert sc._lib.vmx_scene_set_spheres(None, C.addressof(some), 8) == L.VMX_ERR_INVALID
            p.step(0)  # (no generation went by)
            assert np.array_equal(bits(p.preview()), before["frame 0 0x0 True"])
        assert sc.describe()["nspheres"] == 8
        assert_same(everything(sc, cam, FORMS[:3]), before, "refused")


def test_the_write_waits_for_a_query_in_flight():
    """a device raycast on a side stream, then set_spheres with no host synchronisation between: the records are A's"""
    (pos, nrm, uv), cam = lattice()
    n = 1 << 18
    rng = np.random.RandomState(9)
    c = np.array(scenes.lattice_camera()["position"], np.float32)
    o = torch.from_numpy(np.tile(c, (n, 1))).to(DEV)
    d = rng.normal(size=(n, 3))
    d = torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)).to(DEV)
    b = no_emitter()
    b[0].centre[:] = [b[0].centre[0], b[0].centre[1] + 300.0, b[0].centre[2]]
    b[2].centre[:] = [0.0, b[2].centre[1] - 64.0, 0.0]  # (the floor goes down: most records change)
    side = torch.cuda.Stream(DEV)
    with va.Scene(pos, nrm, uv, spheres=b) as fresh:
        want_b = bits(fresh.raycast(o, d)["raw"].cpu().numpy())
    with va.Scene(pos, nrm, uv, spheres=table_a()) as sc:
        want_a = bits(sc.raycast(o, d)["raw"].cpu().numpy())
        assert (want_a != want_b).any(axis=1).mean() > 0.2
        torch.cuda.synchronize(DEV)
        got = sc.raycast(o, d, stream=side)["raw"]
        sc.set_spheres(b)
        after = sc.raycast(o, d, stream=side)["raw"]
        torch.cuda.synchronize(DEV)
        assert np.array_equal(bits(got.cpu().numpy()), want_a)
        assert np.array_equal(bits(after.cpu().numpy()), want_b)


def test_multi_set_spheres_on_a_repeated_device():
    (pos, nrm, uv), cam = lattice()
    opts = va.make_opts(seed=5, stripe_rows=5)
    b = light_moved()
    with va.Scene(pos, nrm, uv, spheres=b) as one:
        want, wst = one.render(cam, opts)
        want_bf, _ = one.render_bruteforce(cam, opts)
    with va.MultiScene(pos, nrm, uv, devices=[0, 0], spheres=table_a()) as multi:
        first, _ = multi.render(cam, opts)
        assert not np.array_equal(bits(first), bits(want))
        multi.set_spheres(b)
        img, st = multi.render(cam, opts)
        assert np.array_equal(bits(img), bits(want)) and st["samples"] == wst["samples"]
        assert np.array_equal(bits(multi.render_bruteforce(cam, opts)[0]), bits(want_bf))
        assert L.lib().vmx_multi_set_spheres(multi._h, None, 2) == L.VMX_ERR_INVALID
        assert np.array_equal(bits(multi.render(cam, opts)[0]), bits(want))
        multi.set_spheres(None)
        assert np.array_equal(bits(multi.render(cam, opts)[0]), bits(first))


# ---- k_motion_spheres is the restatement, bit for bit -----------------------------------------------------------------
def _same_words(got, want, kind=None):
    g, w = bits(got), bits(want)
    bad = (g != w).any(axis=-1)
    assert not bad.any(), (int(bad.sum()), None if kind is None else sorted(set(kind[bad.reshape(-1)])))


@pytest.mark.parametrize("nspheres", [0, 1, 8, 16])
def test_kernel_is_the_restatement_on_synthetic_records(nspheres):
    """n = 1, 255, 256, 257 and 70 x 41 records of every kind; without d_motion_in, with it, and in place.  NaN appears only
    where the restatement has it (the words are compared), and the input buffers are left alone."""
    base = va.default_spheres()
    now, prev = SS.moved_tables(base, nspheres)
    rng = np.random.RandomState(21)
    for n in (1, 255, 256, 257, 70 * 41):
        rec, kind = SS.synthetic_records(n, now, SS.ORIGIN, 100 + n)
        if n == 1:  # (one record: let it be one the rule rewrites, where the table has such a sphere)
            rec, kind = (a[4:5] for a in SS.synthetic_records(8, now, SS.ORIGIN, 3))
        mv = rng.randint(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32).view(np.float32)
        d_rec = torch.from_numpy(np.array(rec)).to(DEV)
        d_mv = torch.from_numpy(mv).to(DEV)
        want_alone = SS.motion(rec, SS.ORIGIN, now, prev)
        want_after = SS.motion(rec, SS.ORIGIN, now, prev, mv)
        got = va.sphere_motion_vectors(d_rec, SS.ORIGIN, now, prev)
        _same_words(got.cpu().numpy(), want_alone, kind)
        out = torch.full((n, 8), float("nan"), dtype=torch.float32, device=DEV)
        assert va.sphere_motion_vectors(d_rec, SS.ORIGIN, now, prev, motion=d_mv, out=out) is out
        _same_words(out.cpu().numpy(), want_after, kind)
        assert np.array_equal(bits(d_mv.cpu().numpy()), bits(mv)) and np.array_equal(bits(d_rec.cpu().numpy()), bits(rec))
        va.sphere_motion_vectors(d_rec, SS.ORIGIN, now, prev, motion=d_mv, out=d_mv)  # in place
        _same_words(d_mv.cpu().numpy(), want_after, kind)
        assert np.array_equal(bits(d_rec.cpu().numpy()), bits(rec))
        if nspheres >= 1 and n >= 255:
            assert (bits(want_alone)[:, 3] & 1).sum() >= n // 16  # (the comparison is of records that do get rewritten)


def test_kernel_is_the_restatement_on_a_real_gbuffer():
    """the G-buffer of the Cornell set at 70 x 41 before and after set_spheres moves an emitter; the records compose after
    vmx_motion_device's (here: records of an update that moved nothing)"""
    pos, nrm, uv = scenes.cornell8()
    c = scenes.cornell_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], 70, 41, 16)
    opts = va.make_opts(seed=3)
    base = va.default_spheres()
    prev, now = SS.emitter_table(base, 6), SS.emitter_table(base, 7)
    with va.Scene(pos, nrm, uv, spheres=prev) as sc, va.Scene(pos, nrm, uv, spheres=now) as fresh:
        raw_prev = sc.raycast_camera(cam, opts, 0)["raw"]
        sc.set_spheres(now)
        raw = sc.raycast_camera(cam, opts, 0)["raw"]
        want_raw = fresh.raycast_camera(cam, opts, 0)["raw"]
        torch.cuda.synchronize(DEV)
        assert np.array_equal(bits(raw.cpu().numpy()), bits(want_raw.cpu().numpy()))
        assert not np.array_equal(bits(raw.cpu().numpy()), bits(raw_prev.cpu().numpy()))
        rec = raw.cpu().numpy()
        got = va.sphere_motion_vectors(raw, c["position"], now, prev)
        want = SS.motion(rec, c["position"], now, prev)
        _same_words(got.cpu().numpy(), want)
        flagged = (bits(want)[..., 3] & 1) != 0
        assert flagged.sum() > 100 and flagged.sum() < 70 * 41 // 4
        d_pos = torch.from_numpy(np.ascontiguousarray(pos, np.float32).reshape(-1, 9)).to(DEV)
        tri = va.motion_vectors(raw, d_pos, d_pos)
        both = va.sphere_motion_vectors(raw, c["position"], now, prev, motion=tri, out=tri)
        _same_words(both.cpu().numpy(), want)
