"""In-place geometry updates (vmx_scene_update / vmx_scene_update_device / vmx_multi_update) on the GPU: refit parity
against the CPU oracle run over the old topology with boxes recomputed here, attribute-only updates, stream ordering,
repeated updates, in-place rebuilds (bit-identical to a fresh create, deeper trees, the depth limit), failures that
leave the scene as it was, a single-leaf tree and the multi-device replicas."""

import numpy as np
import pytest
import torch

import oracle_lib as O
from shared_inputs import numpy_boxes
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
BIG = np.float32(999999999.0)  # bvh.cpp:48
EPS = np.float32(1e-3)
BUILDERS = {"reference": L.VMX_BVH_REFERENCE, "sah": L.VMX_BVH_SAH, "lbvh": L.VMX_BVH_LBVH, "ploc": L.VMX_BVH_PLOC}
TOPO = ("start", "nprims", "right_offset", "prim_order")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_f32(x, y):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    return (bits(x) == bits(y)) | (np.isnan(x) & np.isnan(y))


def rand_rays(n, seed, lo, hi):
    r = np.random.RandomState(seed)
    o = r.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = r.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


def scene_rays(pos, n=20000, seed=5):
    v = pos.reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    pad = 0.1 * (hi - lo)
    return rand_rays(n, seed, lo - pad, hi + pad)


def deform(pos, amp=0.02, phase=0.0):
    """deterministic per-vertex displacement of about `amp` of the scene's extent"""
    v = np.asarray(pos, np.float64).reshape(-1, 3)
    ext = float((v.max(axis=0) - v.min(axis=0)).max())
    k = 12.0 / ext
    d = np.stack([np.sin(k * v[:, 1] + phase), np.cos(k * v[:, 2] + 2 * phase), np.sin(k * v[:, 0] - phase)], axis=1)
    return (v + amp * ext * d).astype(np.float32).reshape(-1, 9)


def move_half(pos):
    v = np.asarray(pos, np.float32).reshape(-1, 9).copy()
    ext = float(np.ptp(v.reshape(-1, 3), axis=0).max())
    v[::2, 0::3] += np.float32(4 * ext)
    v[::2, 1::3] += np.float32(ext)
    return v


def camera(camf, W=96, H=64, spp=16):
    c = camf()
    return va.make_camera(c["position"], c["rotation_deg"], W, H, spp)


def assert_raycast_equal(a, b):
    for f in a.dtype.names:
        if f == "pad":
            continue
        x, y = a[f], b[f]
        same = same_f32(x, y) if x.dtype == np.float32 else (x == y)
        assert np.all(same), f"raycast field {f}: {int((~same).sum())} mismatches"


def check_queries(sc, o, d, otri, ot):
    tri, t, hit = sc.query(o, d, mode="nearest")
    assert np.array_equal(tri, otri) and np.all(same_f32(t, np.where(otri >= 0, ot, BIG)))
    inside = (otri >= 0) & (ot < BIG)
    assert np.array_equal(hit, inside)
    assert np.array_equal(sc.query(o, d, mode="any"), inside)
    ctri, ct, chit = sc.query(o, d, mode="collision")
    assert np.array_equal(ctri, tri) and np.array_equal(chit, inside & (t >= EPS))


def check_against_oracle(sc, osc, camf, pos, full=True):
    o, d = scene_rays(pos)
    tri, t = sc.trace(o, d)
    otri, ot = osc.trace(o, d)
    assert np.array_equal(tri, otri) and np.array_equal(bits(t), bits(ot))
    if not full:
        return
    assert_raycast_equal(sc.raycast(o[:4000], d[:4000]), osc.raycast(o[:4000], d[:4000]))
    check_queries(sc, o, d, otri, ot)
    cam = camera(camf)
    for early in (True, False):
        ref, _ = osc.render(cam, va.make_opts(seed=3, early_stop=early))
        for form in (0, 0x100):  # default routing, the headline form (reserved[0] bit 8)
            img, _ = sc.render(cam, va.make_opts(seed=3, early_stop=early, pipeline=form))
            assert np.array_equal(bits(img), bits(ref)), (early, form)
        img, _ = sc.render(cam, va.make_opts(seed=3, early_stop=early, sampling=L.VMX_SAMPLING_ELIDE_DEAD))
        assert np.array_equal(bits(img), bits(ref)), (early, "elided")
    bf, _ = sc.render_bruteforce(cam, va.make_opts(seed=3))
    obf, _ = osc.render_bruteforce(cam, va.make_opts(seed=3))
    assert np.array_equal(bits(bf), bits(obf))


def assert_same_tree(a, b, boxes_by_value=False):
    for k in TOPO:
        assert np.array_equal(a[k], b[k]), k
    if boxes_by_value:
        assert np.array_equal(a["bbox"], b["bbox"])
    else:
        assert np.array_equal(bits(a["bbox"]), bits(b["bbox"]))


# ---- 1. round trip: an update with the scene's own arrays changes nothing -------------------------------------
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_round_trip(builder):
    gen, camf = scenes.SCENES["bunny70k"]
    pos, nrm, uv = gen()
    with va.Scene(pos, nrm, uv, builder=BUILDERS[builder]) as sc:
        before = sc.bvh()
        o, d = scene_rays(pos)
        tri0, t0 = sc.trace(o, d)
        cam = camera(camf)
        img0, _ = sc.render(cam, va.make_opts(seed=3))
        sc.update(pos, nrm, uv)
        assert_same_tree(sc.bvh(), before, boxes_by_value=True)
        tri, t = sc.trace(o, d)
        assert np.array_equal(tri, tri0) and np.array_equal(bits(t), bits(t0))
        img, _ = sc.render(cam, va.make_opts(seed=3))
        assert np.array_equal(bits(img), bits(img0))


# ---- 2. refit parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice", "bunny70k", "sponza260k"])
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_refit_parity(name, builder):
    gen, camf = scenes.SCENES[name]
    pos, nrm, uv = gen()
    with va.Scene(pos, nrm, uv, builder=BUILDERS[builder]) as sc:
        before = sc.bvh()
        for case, new in (("deform", deform(pos)), ("half far away", move_half(pos))):
            sc.update(pos=new)
            after = sc.bvh()
            for k in TOPO:
                assert np.array_equal(after[k], before[k]), (case, k)
            boxes = numpy_boxes(before, new)
            assert np.array_equal(after["bbox"], boxes), case
            tree = {k: before[k] for k in TOPO}
            tree["bbox"] = boxes  # never the exported boxes: the oracle trusts the boxes it is given
            osc = O.OracleScene(new, nrm, uv, tree=tree)
            check_against_oracle(sc, osc, camf, new, full=(case == "deform" or name == "lattice"))
            osc.close()


# ---- 3. attribute-only updates ----------------------------------------------------------------------------------
def test_attribute_only_updates():
    gen, camf = scenes.SCENES["bunny70k"]
    pos, nrm, uv = gen()
    cam = camera(camf)
    opts = va.make_opts(seed=3)
    with va.Scene(pos, nrm, uv) as sc:
        o, d = scene_rays(pos)
        tri0, t0 = sc.trace(o, d)
        nrm2 = (-nrm).astype(np.float32)
        sc.update(nrm=nrm2)
        tri, t = sc.trace(o, d)
        assert np.array_equal(tri, tri0) and np.array_equal(bits(t), bits(t0))
        img, _ = sc.render(cam, opts)
        ref, _ = O.OracleScene(pos, nrm2, uv).render(cam, opts)
        assert np.array_equal(bits(img), bits(ref))
    tex = np.random.RandomState(2).uniform(0.1, 1.0, size=(32, 48, 3)).astype(np.float32)
    with va.Scene(pos, nrm, uv) as sc:
        sc.bind_texture(tex)
        uv2 = np.ascontiguousarray(uv[:, ::-1] * np.float32(3.0) + np.float32(0.25), np.float32)
        sc.update(uv=uv2)
        tri, t = sc.trace(o, d)
        assert np.array_equal(tri, tri0) and np.array_equal(bits(t), bits(t0))
        img, _ = sc.render(cam, opts)
        osc = O.OracleScene(pos, nrm, uv2)
        osc.bind_texture(tex)
        ref, _ = osc.render(cam, opts)
        assert np.array_equal(bits(img), bits(ref))


# ---- 4. stream ordering -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["reference", "lbvh"])
def test_device_update_stream_ordering(builder):
    gen, camf = scenes.SCENES["sponza260k"]
    pos, nrm, uv = gen()
    new = deform(pos, amp=0.03)
    o, d = scene_rays(pos, n=100000)
    cam = camera(camf)
    with va.Scene(pos, nrm, uv, builder=BUILDERS[builder]) as a, va.Scene(pos, nrm, uv, builder=BUILDERS[builder]) as b:
        dev = torch.device("cuda", 0)
        d_new, d_o, d_d = (torch.from_numpy(x).to(dev) for x in (new, o, d))
        torch.cuda.synchronize()
        a.query(d_o, d_d)  # a query in flight before the update: the update waits for it
        side, other = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        a.update(pos=d_new, stream=side)
        img_a, _ = a.render(cam, va.make_opts(seed=3))  # no host sync in between: the render waits on the update
        with torch.cuda.stream(other):
            tri_a, t_a, hit_a = a.query(d_o, d_d, stream=other)
        torch.cuda.synchronize()
        b.update(pos=new)
        img_b, _ = b.render(cam, va.make_opts(seed=3))
        tri_b, t_b, hit_b = b.query(o, d)
        assert np.array_equal(bits(img_a), bits(img_b))
        assert np.array_equal(tri_a.cpu().numpy(), tri_b) and np.array_equal(bits(t_a.cpu().numpy()), bits(t_b))
        assert_same_tree(a.bvh(), b.bvh())


# ---- 5. repeated updates ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["reference", "lbvh"])
def test_repeated_updates_alternate(builder):
    pos, nrm, uv = scenes.bunny70k()
    geo = [deform(pos, amp=0.05, phase=0.0), deform(pos, amp=0.05, phase=1.3)]
    dev = torch.device("cuda", 0)
    d_geo = [torch.from_numpy(g).to(dev) for g in geo]
    with va.Scene(pos, nrm, uv, builder=BUILDERS[builder]) as sc:
        tree = sc.bvh()
        expect = [numpy_boxes(tree, g) for g in geo]
        for i in range(16):
            sc.update(pos=d_geo[i % 2])  # device entry, current stream, no sync
            got = sc.bvh()
            assert np.array_equal(got["bbox"], expect[i % 2]), i
            for k in TOPO:
                assert np.array_equal(got[k], tree[k]), (i, k)


# ---- 6. rebuild ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_rebuild_equals_fresh_create(builder):
    gen, camf = scenes.SCENES["bunny70k"]
    pos, nrm, uv = gen()
    new = deform(pos, amp=0.08)
    nrm2 = np.ascontiguousarray(nrm[:, ::-1], np.float32)
    cam = camera(camf)
    opts = va.make_opts(seed=3)
    with va.Scene(new, nrm2, uv, builder=BUILDERS[builder]) as fresh:
        ref_tree = fresh.bvh()
        ref_img, _ = fresh.render(cam, opts)
        variants = ["host", "host keeps nrm"] + (["device"] if builder in ("lbvh", "ploc") else [])
        for v in variants:
            with va.Scene(pos, nrm, uv, builder=BUILDERS[builder]) as sc:
                if v == "host":
                    sc.update(pos=new, nrm=nrm2, rebuild=True)
                elif v == "host keeps nrm":
                    sc.update(nrm=nrm2)
                    sc.update(pos=new, rebuild=True)
                else:
                    sc.update(pos=torch.from_numpy(new).cuda(), nrm=torch.from_numpy(nrm2).cuda(), rebuild=True)
                assert_same_tree(sc.bvh(), ref_tree)
                assert sc.describe() == fresh.describe(), v
                img, _ = sc.render(cam, opts)
                assert np.array_equal(bits(img), bits(ref_img)), v


BASE = 2.2  # > 2: the midpoint of the centroid bounds lies above the second-farthest centroid even in float


def peel_scene(n, deep):
    """n triangles in the plane z = 0.  deep: triangle k at x = 2.2^k, scaled with its distance, so that the reference
    builder's midpoint split on x (bbox.cpp:41-46: z is never wider) peels one triangle off per level (at x = 2^k the
    midpoint rounds onto the second-farthest centroid, and two go right)"""
    pos = np.zeros((n, 9), np.float32)
    for k in range(n):
        if deep:
            s = np.float32(BASE ** k)
            x0, y0 = s, np.float32(0)
        else:
            s = np.float32(1.0)
            x0, y0 = np.float32(3 * (k % 8)), np.float32(3 * (k // 8))
        pos[k] = [x0, y0, 0, x0 + 0.8 * s, y0, 0, x0 + 0.4 * s, y0 + 0.6 * s, 0]
    nrm = np.tile(np.array([0, 0, 1] * 3, np.float32), (n, 1))
    return pos, nrm


def test_rebuild_deeper_tree_query_and_render():
    pos, nrm = peel_scene(40, deep=False)
    deep, _ = peel_scene(40, deep=True)
    cam = va.make_camera((BASE ** 20, BASE ** 18, BASE ** 40), (0, 0, 0), 64, 48, 8)
    opts = va.make_opts(seed=3)
    o = np.tile(np.array([[0, 0, 10]], np.float32), (4096, 1))
    r = np.random.RandomState(3)
    tx = (BASE ** r.randint(0, 40, size=4096)).astype(np.float32)
    o[:, 0] = tx * np.float32(1.4)
    o[:, 1] = tx * np.float32(0.2)
    o[:, 2] = tx
    d = np.tile(np.array([[0, 0, -1]], np.float32), (4096, 1))
    with va.Scene(pos, nrm) as sc, va.Scene(deep, nrm) as fresh:
        shallow = sc.describe()["stack_entries"]
        sc.query(o, d)  # the query workspace now exists at the shallow depth
        sc.update(pos=deep, rebuild=True)
        assert sc.describe()["stack_entries"] == fresh.describe()["stack_entries"] > shallow + 30
        assert_same_tree(sc.bvh(), fresh.bvh())
        for mode in ("nearest", "collision"):
            got, ref = sc.query(o, d, mode=mode), fresh.query(o, d, mode=mode)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(bits(got[1]), bits(ref[1])), mode
        assert np.array_equal(sc.query(o, d, mode="any"), fresh.query(o, d, mode="any"))
        assert (sc.query(o, d)[0] >= 0).mean() > 0.5
        img, _ = sc.render(cam, opts)
        ref, _ = fresh.render(cam, opts)
        assert np.array_equal(bits(img), bits(ref))


def test_rebuild_past_the_stack_fails_and_keeps_the_scene():
    pos, nrm = peel_scene(80, deep=False)
    deep, _ = peel_scene(80, deep=True)
    cam = va.make_camera((12.0, 30.0, 60.0), (-20, 0, 0), 64, 48, 8)
    opts = va.make_opts(seed=3)
    with va.Scene(pos, nrm) as sc:
        before, img0 = sc.bvh(), sc.render(cam, opts)[0]
        with pytest.raises(L.VmxError) as e:
            sc.update(pos=deep, rebuild=True)
        assert e.value.code == L.VMX_ERR_DEPTH
        assert_same_tree(sc.bvh(), before)
        assert np.array_equal(bits(sc.render(cam, opts)[0]), bits(img0))


# ---- 7. failures leave the scene unchanged ------------------------------------------------------------------------
def test_failed_updates_leave_the_scene_unchanged():
    gen, camf = scenes.SCENES["bunny70k"]
    pos, nrm, uv = gen()
    cam = camera(camf)
    opts = va.make_opts(seed=3)
    with va.Scene(pos, nrm, uv) as sc:
        img0, _ = sc.render(cam, opts)
        tree0 = sc.bvh()
        bad = deform(pos)
        bad[7, 4] = np.nan
        with pytest.raises(L.VmxError, match="non-finite"):
            sc.update(pos=bad)
        new = deform(pos)
        rc = sc._lib.vmx_scene_update(sc._h, new.ctypes.data, None, None, sc.ntris - 1, L.VMX_UPDATE_REFIT)
        assert rc == L.VMX_ERR_INVALID and b"triangle count" in sc._lib.vmx_last_error()
        with pytest.raises(L.VmxError, match="vmx_scene_update"):
            sc.update(pos=torch.from_numpy(new).cuda(), rebuild=True)
        with pytest.raises(ValueError):
            sc.update(pos=torch.from_numpy(new).cuda().double())
        img, _ = sc.render(cam, opts)
        assert np.array_equal(bits(img), bits(img0))
        assert_same_tree(sc.bvh(), tree0)


# ---- 8. single leaf -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_single_leaf_tree(builder):
    pos, nrm, uv = scenes.cornell8()
    pos, nrm, uv = pos[:3].copy(), nrm[:3].copy(), uv[:3].copy()
    with va.Scene(pos, nrm, uv, builder=BUILDERS[builder]) as sc:
        before = sc.bvh()
        assert len(before["start"]) == 1
        new = deform(pos, amp=0.2)
        sc.update(pos=new)
        after = sc.bvh()
        assert np.array_equal(after["bbox"], numpy_boxes(before, new))
        tree = {k: before[k] for k in TOPO}
        tree["bbox"] = numpy_boxes(before, new)
        osc = O.OracleScene(new, nrm, uv, tree=tree)
        o, d = scene_rays(new, n=5000)
        tri, t = sc.trace(o, d)
        otri, ot = osc.trace(o, d)
        assert np.array_equal(tri, otri) and np.array_equal(bits(t), bits(ot)) and (tri >= 0).any()


# ---- 9. multi-device replicas -------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["reference", "ploc"])
def test_multi_update_equals_single_scene(builder):
    gen, camf = scenes.SCENES["bunny70k"]
    pos, nrm, uv = gen()
    new = deform(pos, amp=0.04)
    cam = camera(camf)
    opts = va.make_opts(seed=3)
    for rebuild in (False, True):
        with va.MultiScene(pos, nrm, uv, devices=[0, 0], builder=BUILDERS[builder]) as m, \
                va.Scene(pos, nrm, uv, builder=BUILDERS[builder]) as sc:
            m.update(pos=new, rebuild=rebuild)
            sc.update(pos=new, rebuild=rebuild)
            img_m, _ = m.render(cam, opts)
            img_s, _ = sc.render(cam, opts)
            assert np.array_equal(bits(img_m), bits(img_s)), rebuild
