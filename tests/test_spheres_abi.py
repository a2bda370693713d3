"""Changing lights (vmx_scene_set_spheres, vmx_multi_set_spheres) and the motion records of moved spheres
(vmx_motion_spheres_device): what needs no GPU — the ABI surface, every argument check, and conditions on the numpy
restatement (sphere_motion_spec.py) the kernel is then held to bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import sphere_motion_spec as SS
import temporal_spec as TS
import motion_spec as MS
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vermilion_hip.h")
ENTRIES = ("vmx_scene_set_spheres", "vmx_multi_set_spheres", "vmx_motion_spheres_device")
F, D = np.float32, np.float64


def _err(lib):
    return lib.vmx_last_error().decode()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_symbols_are_declared_bound_and_exported(hip_lib):
    src = open(HEADER).read()
    for name in ENTRIES:
        assert hasattr(hip_lib, name), name
        assert name in L.SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, src), name
    # additive: no new ABI version
    assert re.search(r"#define VMX_ABI_VERSION 2\b", src) and hip_lib.vmx_abi_version() == 2
    assert "sphere_motion_vectors" in va.__all__ and callable(va.sphere_motion_vectors)
    assert callable(va.Scene.set_spheres) and callable(va.MultiScene.set_spheres)


@pytest.mark.parametrize("entry", ["vmx_scene_set_spheres", "vmx_multi_set_spheres"])
def test_set_spheres_checks_do_not_need_a_gpu(hip_lib, entry):
    """the (spheres, nspheres) pair as vmx_scene_create_ex checks it, then the NULL handle: each seen alone, in that order"""
    call = getattr(hip_lib, entry)
    table = va.default_spheres()
    big = (L.Sphere * 17)()
    p = C.addressof(table)

    def refused(args, what):
        assert call(*args) == L.VMX_ERR_INVALID, what
        assert what in _err(hip_lib), (what, _err(hip_lib))

    # a live-looking handle that is never reached: the table is refused first
    room = (C.c_char * 64)()
    handle = C.addressof(room)
    for h in (None, handle):
        refused((h, None, 1), "spheres is NULL but nspheres > 0")
        refused((h, None, 17), "spheres is NULL but nspheres > 0")
        refused((h, C.addressof(big), 17), "more than 16 spheres")
        refused((h, p, 0xFFFFFFFF), "more than 16 spheres")
    for args in ((None, None, 0), (None, p, 8), (None, p, 0), (None, C.addressof(big), 16)):
        refused(args, "NULL")


def test_motion_spheres_checks_do_not_need_a_gpu(hip_lib):
    """every host check of vmx_motion_spheres_device, each seen alone, in the order the header gives them"""
    mot = hip_lib.vmx_motion_spheres_device
    buf = np.zeros(4096, np.float32)
    p = (buf.ctypes.data + 15) & ~15
    rec, out, mv = p, p + 64 * 8, p + 64 * 8 + 32 * 8  # (8 records)
    org = (C.c_float * 3)(0, 0, 0)
    now, prev = va.default_spheres(), va.default_spheres()
    a, b = C.addressof(now), C.addressof(prev)
    o = C.addressof(org)

    def refused(args, what):
        assert mot(*args) == L.VMX_ERR_INVALID, what
        assert what in _err(hip_lib), (what, _err(hip_lib))

    refused((None, 8, o, a, b, 8, mv, out, None), "NULL d_rayhit")
    refused((rec, 8, None, a, b, 8, mv, out, None), "NULL origin")
    refused((rec, 8, o, None, b, 8, mv, out, None), "NULL spheres_now")
    refused((rec, 8, o, a, None, 8, mv, out, None), "NULL spheres_prev")
    refused((rec, 8, o, a, b, 8, mv, None, None), "NULL d_out")
    refused((rec, 8, o, a, b, 17, mv, out, None), "more than 16 spheres")
    refused((rec + 4, 8, o, a, b, 8, mv, out, None), "16-byte aligned")
    refused((rec, 8, o, a, b, 8, mv + 8, out, None), "16-byte aligned")
    refused((rec, 8, o, a, b, 8, mv, out + 12, None), "16-byte aligned")
    refused((rec, 1 << 31, o, a, b, 8, None, out, None), "2^31 - 1")
    refused((rec, 0xFFFFFFFF, o, a, b, 8, None, out, None), "2^31 - 1")
    # d_out over the records (in place, and their last 16 bytes); over d_motion_in other than exactly
    refused((rec, 8, o, a, b, 8, None, rec, None), "d_out overlaps")
    refused((rec, 8, o, a, b, 8, None, rec + 64 * 8 - 16, None), "d_out overlaps")
    refused((rec, 8, o, a, b, 8, mv, mv + 16, None), "d_out overlaps")
    refused((rec, 8, o, a, b, 8, mv, mv - 32 * 8 + 16, None), "d_out overlaps")
    refused((rec, 0x7FFFFFFF, o, a, b, 8, None, out, None), "d_out overlaps")  # (the products do not wrap)
    # nothing to do: no launch and no device needed; the tables may be NULL with no spheres; in place is no overlap
    assert mot(rec, 0, o, a, b, 8, mv, out, None) == L.VMX_OK
    assert mot(rec, 0, o, None, None, 0, None, out, None) == L.VMX_OK
    assert mot(rec, 0, o, a, b, 8, mv, mv, None) == L.VMX_OK
    # host pointers never reach a kernel: without a device there is none to run on, with one they are no device memory
    if hip_lib.vmx_device_count() == 0:
        assert mot(rec, 8, o, a, b, 8, mv, mv, None) == L.VMX_ERR_NO_DEVICE and "no CPU path" in _err(hip_lib)
        assert mot(rec, 8, o, None, None, 0, None, out, None) == L.VMX_ERR_NO_DEVICE
    else:
        refused((rec, 8, o, a, b, 8, mv, mv, None), "not device memory")


class NoLib:  # any call into the library fails the test
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_layer_rejects_bad_arguments_before_the_library(monkeypatch):
    torch = pytest.importorskip("torch")
    table = va.default_spheres()  # (before the library goes)
    monkeypatch.setattr(L, "lib", lambda: NoLib())

    class OnDevice:  # a tensor that passes every check: the later arguments are reached
        def __init__(self, shape, dtype):
            self.shape, self.dtype, self.device = shape, dtype, torch.device("cuda", 0)

        def data_ptr(self):
            return 0

        def is_contiguous(self):
            return True

    OnDevice.__module__ = "torch"
    raw, org = OnDevice((41, 70, 16), torch.float32), (0.0, 1.0, 2.0)
    with pytest.raises(ValueError, match="raw must be a torch tensor"):
        va.sphere_motion_vectors(np.zeros((4, 16), np.float32), org, table, table)
    with pytest.raises(ValueError, match=r"raw must be \[..., 16\]"):
        va.sphere_motion_vectors(torch.zeros((4, 8)), org, table, table)
    with pytest.raises(ValueError, match="raw must be on cuda"):
        va.sphere_motion_vectors(torch.zeros((4, 16)), org, table, table)
    with pytest.raises(ValueError, match="origin must be three floats"):
        va.sphere_motion_vectors(raw, (0.0, 1.0), table, table)
    with pytest.raises(ValueError, match="spheres_now must be None or a ctypes array of vmx_sphere"):
        va.sphere_motion_vectors(raw, org, [dict(centre=(0, 0, 0), radius=1)], table)
    with pytest.raises(ValueError, match="one length"):
        va.sphere_motion_vectors(raw, org, table, (L.Sphere * 3)())
    with pytest.raises(ValueError, match=r"motion must be \[41, 70, 8\]"):
        va.sphere_motion_vectors(raw, org, table, table, motion=torch.zeros((41, 70, 16)))
    with pytest.raises(ValueError, match="out must be on"):
        va.sphere_motion_vectors(raw, org, table, table, out=torch.zeros((41, 70, 8)))
    sc = va.Scene.__new__(va.Scene)
    sc._lib, sc._h = NoLib(), None
    with pytest.raises(ValueError, match="spheres must be None or a ctypes array of vmx_sphere"):
        sc.set_spheres([1, 2, 3])
    ms = va.MultiScene.__new__(va.MultiScene)
    ms._h = None
    with pytest.raises(ValueError, match="spheres must be None or a ctypes array of vmx_sphere"):
        ms.set_spheres(np.zeros(12))


# ---- conditions on the restatement itself -----------------------------------------------------------------------------
def _dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _raycast_spheres(tb, origin, d):
    """MeshEngine::RayCast's sphere loop for the rays (origin, d [n, 3] float32), written apart from the restatement:
    (sphere [n] or -1, location [n, 3] = o + d * (float)t, near [n]).  near: the ray passes within 1e-3 relative of the
    silhouette of ANOTHER sphere than the one it ends on.  Per sphere: for the lights, the distance of the ray's line from
    the centre is within 1e-3 of the radius, | sqrt(C - B*B) - r | <= 1e-3 r.  For the radius-5e7 walls that measure says
    nothing — the whole room is 1e-5 of that radius across, every ray would be near every wall — so theirs is on the
    discriminant det = B*B - (C - R2), relative to the terms it is the difference of: |det| <= 1e-3 (B*B + |C - R2|)."""
    o = np.asarray(origin, F)
    n = d.shape[0]
    op = (tb["centre"][None] - o[None, None]).astype(F)
    B = _dot32(op, d[:, None, :]).astype(D)
    Cc = _dot32(op, op).astype(D)
    R2 = (tb["radius"] * tb["radius"]).astype(D)
    det = (B * B - Cc) + R2
    q = np.sqrt(np.maximum(det, 0))
    t0, t1 = B - q, B + q
    th = np.where(det < 0, 0, np.where(t0 > 1e-4, t0.astype(F), np.where(t1 > 1e-4, t1.astype(F), 0))).astype(F)
    nearest = np.full(n, np.inf, F)
    which = np.full(n, -1)
    for i in range(len(tb["radius"])):
        acc = (th[:, i] > 0) & (th[:, i] < nearest)
        nearest = np.where(acc, th[:, i], nearest)
        which = np.where(acc, i, which)
    r = tb["radius"].astype(D)
    wall = r > 1e6
    graze_light = np.abs(np.sqrt(np.maximum(Cc - B * B, 0)) - r) <= 1e-3 * r
    graze_wall = np.abs(det) <= 1e-3 * (B * B + np.abs(Cc - R2))
    graze = np.where(wall[None, :], graze_wall, graze_light)
    graze[np.arange(n), which] = False  # (another sphere's silhouette, not its own)
    return which, (o + d * nearest[:, None]).astype(F), graze.any(axis=1)


def _unit32(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def _choice_batches():
    """[(origin, directions)]: from the Cornell camera, 6000 directions over the whole sphere (the walls, their edges and
    corners); from a point 44 units from the small light, 2000 over the whole sphere and 2000 aimed into the light's ball"""
    tb = SS.table_of(va.default_spheres())
    rng = np.random.RandomState(1)
    cam = np.array(scenes.cornell_camera()["position"], F)
    close = np.array([40.0, 150.0, 60.0], F)
    u = rng.normal(size=(2000, 3))
    u = u / np.linalg.norm(u, axis=1, keepdims=True) * (tb["radius"][0] * rng.uniform(0, 1, (2000, 1)) ** (1 / 3))
    aimed = _unit32(tb["centre"][0].astype(D) + u - close.astype(D))
    return tb, [(cam, _unit32(rng.normal(size=(6000, 3)))), (close, np.concatenate([aimed, _unit32(rng.normal(size=(2000, 3)))]))]


def test_spec_picks_the_sphere_the_ray_was_cast_on():
    """(a) records made as RayCast makes them on the reference's table — float32 dots, float64 roots, location = o + d *
    (float)t — from two points in the room.  The restatement sees only (location, origin) and must name the same sphere
    for every record whose ray does not pass within 1e-3 relative of another sphere's silhouette (_raycast_spheres says
    how that is measured per sphere); a ray at the rim of its own sphere is not exempt.  At least 95 % of the records are
    of that kind, rays at the small light among them.  The rays at the light start 44 units from it: from the Cornell
    camera, 1900 units away, RayCast's own float32 dots carry an error of about 1 in a discriminant that is at most r*r =
    12.25, so which rim rays hit the light is RayCast's rounding, not geometry.
    (Restatement only: this test reads no library code and passes with or without the feature.)"""
    tb, batches = _choice_batches()
    n_ok = n_all = n_light = 0
    for origin, d in batches:
        truth, P, near = _raycast_spheres(tb, origin, d)
        assert (truth >= 0).all()  # (the room is closed)
        got = SS.choose(P, origin, tb)
        ok = ~near
        print(f"origin {origin}: {int(ok.sum())} of {len(ok)} records are outside the exemption; spheres {np.bincount(truth, minlength=8)}; "
              f"differences among them {int((got != truth)[ok].sum())}, among the rest {int((got != truth)[near].sum())}")
        assert np.array_equal(got[ok], truth[ok])
        n_ok, n_all, n_light = n_ok + int(ok.sum()), n_all + len(ok), n_light + int(((truth == 0) & ok).sum())
    print(f"share {n_ok / n_all:.4f}, on the small light {n_light}")
    assert n_ok >= 0.95 * n_all
    assert n_light >= 1000


def _emitter_table(centre, radius=3.5):
    t = va.default_spheres()
    t[0].centre[:] = [float(v) for v in centre]
    t[0].normal_centre[:] = [float(v) for v in centre]
    t[0].normal_sign = 1.0
    t[0].radius = radius
    return t


def test_spec_pure_translation():
    """(b) an emitter translated with its radius unchanged: x_prev = c_prev + (location - c_now) * 1 is three single-rounded
    operations, so it is within 4 float32 ulps — of the largest coordinate magnitude among c_prev, c_now and location — of
    the float64 evaluation; n_prev is unit to 1e-6
    (Restatement only: this test reads no library code and passes with or without the feature.)"""
    origin = np.array([40.0, 150.0, 60.0], F)
    c_now, c_prev = (15.0, 140.0, 25.0), (3.25, 147.5, 31.125)
    now, prev = _emitter_table(c_now), _emitter_table(c_prev)
    tb = SS.table_of(now)
    rng = np.random.RandomState(2)
    u = rng.normal(size=(3000, 3))
    u = u / np.linalg.norm(u, axis=1, keepdims=True) * (3.5 * rng.uniform(0, 0.95, (3000, 1)))
    truth, P, near = _raycast_spheres(tb, origin, _unit32(np.array(c_now, D) + u - origin.astype(D)))
    rec = np.zeros((3000, 16), F)
    rec[:, 0:3], rec[:, 3], rec[:, 10] = P, 1.0, 999999999.0
    rec[:, 4:7] = _unit32(rng.normal(size=(3000, 3)))
    bits(rec)[:, 7], bits(rec)[:, 11] = 0xFFFFFFFF, 3
    out = SS.motion(rec, origin, now, prev)
    flagged = (bits(out)[:, 3] & 1) != 0
    assert np.array_equal(flagged, SS.choose(P, origin, tb) == 0) and flagged.sum() >= 2500
    want = np.array(c_prev, D) + (P.astype(D) - np.array(c_now, D)) * 1.0
    scale = max(np.abs(P).max(), max(abs(v) for v in c_now + c_prev))
    err = np.abs(out[flagged][:, 0:3].astype(D) - want[flagged]).max()
    print(f"{int(flagged.sum())} records; largest |x_prev - float64| {err:.3g}, bound {4 * np.spacing(F(scale)):.3g}")
    assert err <= 4 * np.spacing(F(scale))
    assert np.abs(np.linalg.norm(out[flagged][:, 4:7].astype(D), axis=1) - 1.0).max() <= 1e-6
    # the previous normal points from the previous centre to the previous location
    nrm = (want - np.array(c_prev, D)) / 3.5
    assert np.abs(out[flagged][:, 4:7] - nrm[flagged]).max() < 1e-4
    assert np.array_equal(bits(out)[~flagged][:, 0:3], bits(rec)[~flagged][:, 0:3])


def test_spec_passes_through_what_did_not_move():
    """(c) an unmoved table passes d_motion_in's bits through everywhere, records on the radius-5e7 walls included; so does
    a table without spheres, and so do misses whatever the table
    (Restatement only: this test reads no library code and passes with or without the feature.)"""
    tb, batches = _choice_batches()
    base = va.default_spheres()
    rng = np.random.RandomState(3)
    for origin, d in batches:
        truth, P, _ = _raycast_spheres(tb, origin, d)
        n = len(d)
        rec = np.zeros((n, 16), F)
        rec[:, 0:3], rec[:, 3], rec[:, 10] = P, 1.0, 999999999.0
        rec[:, 4:7] = _unit32(rng.normal(size=(n, 3)))
        bits(rec)[:, 7], bits(rec)[:, 11] = 0xFFFFFFFF, 3
        assert SS.sphere_records(rec).all() and (truth >= 2).sum() > 1000
        mv = rng.randint(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)
        plain = np.zeros((n, 8), np.uint32)
        plain[:, 0:3], plain[:, 4:7] = bits(rec)[:, 0:3], bits(rec)[:, 4:7]
        # nothing moved: a dimmed, recoloured light is no motion
        dimmed = va.default_spheres()
        dimmed[1].colour[:] = [3.8, 3.8, 3.8]
        dimmed[0].flags = 0
        for now in (base, dimmed):
            assert np.array_equal(bits(SS.motion(rec, origin, now, base, mv)), mv)
            assert np.array_equal(bits(SS.motion(rec, origin, now, base)), plain)
        # no spheres
        assert np.array_equal(bits(SS.motion(rec, origin, [], [], mv)), mv)
        assert np.array_equal(bits(SS.motion(rec, origin, [], [])), plain)
        # misses only, under tables that did move
        now, prev = SS.moved_tables(base, 8, origin)
        miss = np.array(rec)
        bits(miss)[:, 11] = 2
        assert np.array_equal(bits(SS.motion(miss, origin, now, prev, mv)), mv)
        # ... under which the records on the moved spheres (0 and 2) do change, and only those
        got = bits(SS.motion(rec, origin, now, prev, mv))
        changed = (got != mv).any(axis=1)
        which = SS.choose(P, origin, SS.table_of(now))
        assert changed.sum() > 100 and np.array_equal(changed, (which == 0) | (which == 2))


def test_spec_synthetic_records_cover_every_rule():
    """the records the device test compares on: every kind is there and takes the path it is named after
    (Restatement only: this test reads no library code and passes with or without the feature.)"""
    base = va.default_spheres()
    now, prev = SS.moved_tables(base, 16)
    rec, kind = SS.synthetic_records(70 * 41, now, SS.ORIGIN, 11)
    assert set(kind) == set(SS.KINDS)
    out = SS.motion(rec, SS.ORIGIN, now, prev)
    w, r = bits(out), bits(rec)
    flagged = (w[:, 3] & 1) != 0
    which = SS.choose(np.array(rec[:, 0:3]), SS.ORIGIN, SS.table_of(now))
    for k, sphere, flag in (("miss", None, False), ("triangle", None, False), ("unmoved_sphere", 1, False),
                            ("unmoved_small", 11, False), ("moved_emitter", 0, True), ("wall", 2, True),
                            ("sphere_nearer", 0, True), ("at_origin", -1, False), ("nan_location", -1, False),
                            ("inf_location", -1, False), ("zero_radius", 8, False), ("normal_centre", 9, True),
                            ("flipped_sign", 10, True)):
        m = kind == k
        assert m.sum() >= 100, k
        if sphere is not None:
            assert (which[m] == sphere).all(), (k, np.bincount(which[m] + 1))
        assert (flagged[m] == flag).all(), k
        if not flag:
            assert np.array_equal(w[m][:, 0:3], r[m][:, 0:3]) and np.array_equal(w[m][:, 4:7], r[m][:, 4:7]), k
    # normal_centre == x_prev: the record's own normal stands in
    m = kind == "normal_centre"
    assert np.array_equal(w[m][:, 4:7], r[m][:, 4:7])
    # a flipped sign alone turns the previous normal round
    m = kind == "flipped_sign"
    c = np.array(list(now[10].centre), D)
    n_now = (rec[m][:, 0:3].astype(D) - c) / now[10].radius
    assert np.abs(out[m][:, 4:7] + n_now).max() < 1e-4
    # NaN only where the restatement has it: a NaN location passed through
    assert np.array_equal(np.isnan(out).any(axis=1), kind == "nan_location")


# ---- (d) keeping history: a moving emitter under temporal_spec ------------------------------------------------------------
W, H = 70, 41
FRAMES = 8


def _camera(spp=16):
    c = scenes.cornell_camera()
    return va.make_camera(c["position"], c["rotation_deg"], W, H, spp)


def _oracle_frame(pos, nrm, uv, table, cam, seed):
    opts = va.make_opts(seed=seed, early_stop=False, sampling=L.VMX_SAMPLING_CORRECTED)
    osc = O.OracleScene(pos, nrm, uv, spheres=table)
    raw, _ = osc.render(cam, opts)
    o, d = O.primary_rays(cam, opts, 0)
    rec = osc.raycast(o, d).reshape(H, W)
    osc.close()
    return raw, rec


def _on_emitter(rec, table, origin):
    on = SS.sphere_records(rec) & (SS.choose(np.array(rec["location"], F), origin, SS.table_of(table)) == 0)
    core = np.zeros_like(on)
    core[1:-1, 1:-1] = np.logical_and.reduce([on[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    return on, core


def test_spec_keeps_history_on_a_moving_emitter():
    """(d) 8 oracle frames of 16 spp of scenes.cornell8() at 70 x 41, corrected sampling, early stop off, frame i with seed
    3 + i, under a table whose emitter (radius 120) moves +25 x, +40 z a frame.  Accumulated by temporal_spec's rule with
    the sphere motion records, without them, and in a run where the emitter stands still at its last position.  Interior
    pixels: the whole 3 x 3 neighbourhood lies on the emitter in the last frame and in the one before.  The yardstick is
    the static run: with motion the mean interior history is at least 0.9 of its, without at most half.
    Measured: static 8.000, with motion 7.999, without 1.030, on 135 interior pixels of 218 on the emitter.
    (Restatement only: this test reads no library code and passes with or without the feature.)"""
    pos, nrm, uv = scenes.cornell8()
    base = va.default_spheres()
    cam = _camera()
    origin = np.array(cam.position[:], F)
    with_mv = without = static = None
    prev_table = prev_core = None
    for i in range(FRAMES):
        table = SS.emitter_table(base, i)
        raw, rec = _oracle_frame(pos, nrm, uv, table, cam, 3 + i)
        mv = None if prev_table is None else SS.motion(rec, origin, table, prev_table)
        _, with_mv, hist_mv = MS.step(with_mv, raw, rec, cam, mv)
        _, without, hist_no = MS.step(without, raw, rec, cam)
        raw_s, rec_s = _oracle_frame(pos, nrm, uv, SS.emitter_table(base, FRAMES - 1), cam, 3 + i)
        _, static, hist_st = TS.step(static, raw_s, rec_s, cam)
        on, core = _on_emitter(rec, table, origin)
        if i == FRAMES - 1:
            interior = core & prev_core
            # pixels that are not on the moved sphere are bit for bit what they were
            plain = np.zeros((H, W, 8), np.uint32)
            plain[..., 0:3], plain[..., 4:7] = bits(rec["location"]), bits(rec["normal"])
            flagged = (bits(mv)[..., 3] & 1) != 0
            assert np.array_equal(flagged, on)
            assert np.array_equal(bits(mv)[~on], plain[~on])
            assert np.array_equal(bits(hist_mv)[~on], bits(hist_no)[~on])
        prev_table, prev_core = table, core
    assert np.array_equal(bits(rec_s), bits(rec))  # (the static run's last frame is the moving run's)
    m_st, m_mv, m_no = (float(h[interior].mean()) for h in (hist_st, hist_mv, hist_no))
    print(f"interior pixels {int(interior.sum())} of {int(on.sum())} on the emitter; mean history static {m_st:.3f}, "
          f"with sphere motion {m_mv:.3f}, without {m_no:.3f}")
    assert interior.sum() >= 50
    assert m_mv >= 0.9 * m_st
    assert m_no <= 0.5 * m_st
