"""MeshEngine::RayCast of device batches (vmx_raycast_device, vmx_raycast_camera_device; k_query<3 / 4> +
k_raycast_finish) on the GPU: every record word against the host parity hook vmx_raycast (first-generation k_raycast),
vmx_primary_ids and the CPU oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle_lib as O
import vermilion_amd as va
from vermilion_amd import _lib as L
from vermilion_amd import scenes
from test_gpu_query import rand_rays, same_f32, special_rays

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INT_WORDS = (7, 11, 15)  # tri_id, flags, pad
FLOAT_WORDS = tuple(i for i in range(16) if i not in INT_WORDS)
BUILDERS = (L.VMX_BVH_REFERENCE, L.VMX_BVH_SAH, L.VMX_BVH_LBVH, L.VMX_BVH_PLOC)


def words(rec):
    """[n, 16] uint32 view of vmx_rayhit records: a RAYHIT_DTYPE array, a [.., 16] tensor or a [.., 16] array"""
    if isinstance(rec, torch.Tensor):
        rec = rec.detach().cpu().numpy()
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 16)


def same_records(a, b, pad=True):
    """bit-exact, NaN compared as NaN in the float words; the oracle's pad word is not part of the record"""
    a, b = words(a), words(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    fa, fb = a[:, FLOAT_WORDS].view(np.float32), b[:, FLOAT_WORDS].view(np.float32)
    ok = same_f32(fa, fb).all(axis=1)
    cols = INT_WORDS if pad else INT_WORDS[:2]
    ok &= (a[:, cols] == b[:, cols]).all(axis=1)
    return ok


def check(a, b, tag="", pad=True):
    ok = same_records(a, b, pad)
    assert ok.all(), (tag, int((~ok).sum()), np.flatnonzero(~ok)[:5])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")


def device_cast(sc, o, d, per_lane=False):
    h = sc.raycast(dev(o), dev(d), per_lane_fetch=per_lane)
    torch.cuda.synchronize()
    return h["raw"]


def check_both_fetches(sc, o, d, ref=None, tag=""):
    """vmx_raycast_device == vmx_raycast (all 16 words) for both fetch forms; returns the host records"""
    host = sc.raycast(o, d) if ref is None else ref
    for per_lane in (False, True):
        check(device_cast(sc, o, d, per_lane), host, (tag, per_lane))
    return host


def cornell_rays(n, seed):
    """inside the box (toward walls, lights and the sphere walls) and from far outside it"""
    a = rand_rays(n // 2, seed, lo=(-500, 5, -700), hi=(500, 890, 1500))
    b = rand_rays(n - n // 2, seed + 1, lo=(-3e7, -3e7, -3e7), hi=(3e7, 3e7, 3e7))
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])


# ---- explicit rays against vmx_raycast and the oracle ----------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell8", "lattice", "sponza260k"])
def test_device_raycast_equals_host_and_oracle(name):
    gen, _ = scenes.SCENES[name]
    pos, nrm, uv = gen()
    o, d = cornell_rays(60000, 31) if name == "cornell8" else rand_rays(200000, 32)
    with va.Scene(pos, nrm, uv) as sc:
        host = check_both_fetches(sc, o, d, tag=name)
    osc = O.OracleScene(pos, nrm, uv)
    check(host, osc.raycast(o, d), name, pad=False)
    osc.close()
    h = host
    if name == "cornell8":
        # the reference's spheres: hits on spheres alone, and spheres in front of a triangle hit
        assert ((h["tri_id"] < 0) & ((h["flags"] & 1) != 0)).any()
        assert ((h["tri_id"] >= 0) & (h["distance"] < h["tri_t"])).any()
        assert (h["colour"] != 0).any()


def test_special_rays_and_golden():
    o, d = special_rays()
    for name in ("cornell8", "lattice"):
        g = np.load(os.path.join(GOLD, name + ".npz"))
        with va.Scene(g["pos"], g["nrm"], g["uv"]) as sc:
            host = check_both_fetches(sc, o, d, tag=(name, "special"))
            osc = O.OracleScene(g["pos"], g["nrm"], g["uv"])
            check(host, osc.raycast(o, d), (name, "special oracle"), pad=False)
            osc.close()
            gold = np.ascontiguousarray(g["raycast"]).reshape(-1, 16)
            check(device_cast(sc, g["ray_o"], g["ray_d"]), gold, (name, "golden"), pad=False)
            check(device_cast(sc, g["ray_o"], g["ray_d"], True), gold, (name, "golden per-lane"), pad=False)


@pytest.mark.parametrize("count", [0, 1, 16])
def test_custom_sphere_tables(count):
    pos, nrm, uv = scenes.cornell8()
    r = np.random.RandomState(33 + count)
    sph = [{"centre": r.uniform((-400, 50, -500), (400, 800, 1200)), "radius": float(r.uniform(20, 300)),
            "colour": r.uniform(0, 5, 3), "emit": bool(i % 2 == 0), "normal_sign": -1.0 if i % 3 == 0 else 1.0}
           for i in range(count)]
    arr = va.scene.spheres_array(sph)
    o, d = cornell_rays(60000, 34)
    with va.Scene(pos, nrm, uv, spheres=arr) as sc:
        host = check_both_fetches(sc, o, d, tag=count)
    osc = O.OracleScene(pos, nrm, uv, spheres=arr)
    check(host, osc.raycast(o, d), count, pad=False)
    osc.close()
    if count:
        assert ((host["tri_id"] >= 0) & (host["distance"] < host["tri_t"])).any()


@pytest.mark.parametrize("builder", BUILDERS)
def test_all_builders_against_the_oracle_over_the_same_tree(builder):
    pos, nrm, uv = scenes.sponza260k()
    o, d = rand_rays(150000, 35)
    with va.Scene(pos, nrm, uv, builder=builder) as sc:
        host = check_both_fetches(sc, o, d, tag=builder)
        tree = sc.bvh() if builder != L.VMX_BVH_REFERENCE else None
        if builder == L.VMX_BVH_REFERENCE:
            assert sc.describe()["stack_entries"] > 12  # deeper than the 9 LDS levels: the overflow slab is used
    osc = O.OracleScene(pos, nrm, uv, tree=tree)
    check(host, osc.raycast(o, d), builder, pad=False)
    osc.close()


# ---- camera rays -------------------------------------------------------------------------------------------------
def camera_case(name, W, H, spp, radians=False):
    gen, camf = scenes.SCENES[name]
    c = camf()
    if radians:
        rad = [-c["rotation_deg"][0] * 3.1415926535 / 180, -c["rotation_deg"][1] * 3.1415926535 / 180,
               c["rotation_deg"][2] * 3.1415926535 / 180]
        cam = va.make_camera(c["position"], None, W, H, spp, rotation_rad=rad)
    else:
        cam = va.make_camera(c["position"], c["rotation_deg"], W, H, spp)
    return gen(), cam


@pytest.mark.parametrize("name", ["cornell8", "sponza260k"])
def test_camera_gbuffer(name):
    W, H, spp = 100, 37, 16  # not a multiple of 64 pixels
    (pos, nrm, uv), cam = camera_case(name, W, H, spp)
    _, cam_rad = camera_case(name, W, H, spp, radians=True)
    kmax = 4 * (spp // 4)
    osc = O.OracleScene(pos, nrm, uv)
    with va.Scene(pos, nrm, uv) as sc:
        for seed in (3, 11):
            opts = va.make_opts(seed=seed)
            for k in (0, 1, spp // 4, kmax - 1):
                for c in (cam, cam_rad):
                    for per_lane in (False, True):
                        g = sc.raycast_camera(c, opts, k, per_lane_fetch=per_lane)
                        torch.cuda.synchronize()
                        assert g["raw"].shape == (H, W, 16) and g["normal"].shape == (H, W, 3)
                        tri, t = sc.primary_ids(c, opts, k)
                        assert np.array_equal(g["tri_id"].cpu().numpy().reshape(-1), tri), (seed, k)
                        assert np.all(same_f32(g["tri_t"].cpu().numpy().reshape(-1), t)), (seed, k)
                        o, d = O.primary_rays(c, opts, k)
                        host = sc.raycast(o, d)
                        check(g["raw"], host, (name, seed, k, per_lane))
                        if k == 1 and not per_lane:
                            check(host, osc.raycast(o, d), (name, seed, k, "oracle"), pad=False)
        # rejected: world > 1, k >= kmax, spp < 4
        out = torch.zeros((H, W, 16), dtype=torch.float32, device="cuda:0")
        for c, opts, k in ((cam, va.make_opts(seed=3, world=2), 0), (cam, va.make_opts(seed=3), kmax),
                           (va.make_camera((0, 0, 0), (0, 0, 0), W, H, 3), va.make_opts(), 0)):
            rc = sc._lib.vmx_raycast_camera_device(sc._h, C.byref(c), C.byref(opts), k, C.c_void_p(out.data_ptr()), 0,
                                                   None)
            assert rc == L.VMX_ERR_INVALID
        torch.cuda.synchronize()
        assert not out.any()
    osc.close()


# ---- updates ------------------------------------------------------------------------------------------------------
def test_raycast_after_updates():
    pos, nrm, uv = scenes.sponza260k()
    o, d = rand_rays(100000, 36)
    r = np.random.RandomState(37)
    nrm2 = (nrm + r.normal(0, 0.3, nrm.shape)).astype(np.float32)
    uv2 = r.uniform(-2, 2, uv.shape).astype(np.float32)
    with va.Scene(pos, nrm, uv) as sc:
        device_cast(sc, o, d)
        sc.update(nrm=nrm2)
        with va.Scene(pos, nrm2, uv) as fresh:
            check(device_cast(sc, o, d), fresh.raycast(o, d), "nrm")
        sc.update(uv=uv2)
        with va.Scene(pos, nrm2, uv2) as fresh:
            check(device_cast(sc, o, d, True), fresh.raycast(o, d), "uv")
        v = pos.reshape(-1, 3).astype(np.float64)
        moved = (v + 20.0 * np.sin(v[:, [1, 2, 0]] / 200.0)).astype(np.float32).reshape(pos.shape)
        sc.update(pos=moved)  # REFIT: the old topology over the new positions
        check(device_cast(sc, o, d), sc.raycast(o, d), "refit")
        sc.update(pos=moved, rebuild=True)
        with va.Scene(moved, nrm2, uv2) as fresh:
            check(device_cast(sc, o, d), fresh.raycast(o, d), "rebuild")


def test_update_on_another_stream_is_seen():
    pos, nrm, uv = scenes.sponza260k()
    r = np.random.RandomState(38)
    nrm2 = (nrm + r.normal(0, 0.3, nrm.shape)).astype(np.float32).reshape(-1, 9)
    o, d = rand_rays(200000, 39)
    with va.Scene(pos, nrm, uv, builder=L.VMX_BVH_PLOC) as sc:
        O_, D_ = dev(o), dev(d)
        n2 = dev(nrm2)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        s1.wait_stream(torch.cuda.current_stream())
        s2.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s1):
            sc.update(nrm=n2)
        with torch.cuda.stream(s2):
            h = sc.raycast(O_, D_)
        torch.cuda.synchronize()
        with va.Scene(pos, nrm2, uv, builder=L.VMX_BVH_PLOC) as fresh:
            check(h["raw"], fresh.raycast(o, d), "update then raycast")


# ---- sizes, streams, pointers ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_small_sizes(n):
    pos, nrm, uv = scenes.cornell8()
    o, d = cornell_rays(max(n, 2), 40 + n)
    o, d = o[:n], d[:n]
    with va.Scene(pos, nrm, uv) as sc:
        h = sc.raycast(dev(o).reshape(n, 3), dev(d).reshape(n, 3))
        torch.cuda.synchronize()
        assert h["raw"].shape == (n, 16)
        if n:
            check(h["raw"], sc.raycast(o, d), n)


def test_large_batch_stays_on_the_device():
    n = (1 << 22) + 33
    pos, nrm, uv = scenes.cornell8()
    with va.Scene(pos, nrm, uv) as sc:
        g = torch.Generator(device="cuda:0")
        g.manual_seed(41)
        lo = torch.tensor([-500.0, 5.0, -700.0], device="cuda:0")
        hi = torch.tensor([500.0, 890.0, 1500.0], device="cuda:0")
        o = (lo + (hi - lo) * torch.rand((n, 3), generator=g, device="cuda:0")).contiguous()
        d = torch.randn((n, 3), generator=g, device="cuda:0")
        d = (d / d.norm(dim=1, keepdim=True)).contiguous()
        h = sc.raycast(o, d)
        torch.cuda.synchronize()
        check(h["raw"], sc.raycast(o.cpu().numpy(), d.cpu().numpy()), "4M")


def test_interleaved_with_queries_on_two_streams():
    pos, nrm, uv = scenes.bunny70k()
    a_o, a_d = rand_rays(300000, 42)
    b_o, b_d = rand_rays(250000, 43)
    with va.Scene(pos, nrm, uv) as sc:
        a_ref = sc.raycast(a_o, a_d)
        b_ref = sc.trace(b_o, b_d)
        A, B = (dev(a_o), dev(a_d)), (dev(b_o), dev(b_d))
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        s1.wait_stream(torch.cuda.current_stream())
        s2.wait_stream(torch.cuda.current_stream())
        outs = []
        for rep in range(3):
            with torch.cuda.stream(s1):
                x = sc.raycast(*A, per_lane_fetch=rep == 1)
            with torch.cuda.stream(s2):
                y = sc.query(*B)
            outs.append((x, y))
        torch.cuda.synchronize()
        for x, y in outs:
            check(x["raw"], a_ref, "stream raycast")
            assert np.array_equal(y[0].cpu().numpy(), b_ref[0])
            assert np.array_equal(y[1].cpu().numpy().view(np.uint32), b_ref[1].view(np.uint32))


def test_bad_pointers_launch_nothing():
    pos, nrm, uv = scenes.cornell8()
    n = 100
    o, d = cornell_rays(n, 44)
    with va.Scene(pos, nrm, uv) as sc:
        lib = sc._lib
        O_, D_ = dev(o), dev(d)
        out = torch.zeros(n * 16 + 4, dtype=torch.float32, device="cuda:0")
        P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
        host_out = np.zeros(n * 16, np.float32)
        both = torch.zeros((2 * n, 3), dtype=torch.float32, device="cuda:0")
        cases = [
            ((P(O_), P(D_), n, C.c_void_p(host_out.ctypes.data)), "not device memory"),
            ((C.c_void_p(o.ctypes.data), P(D_), n, P(out)), "not device memory"),
            ((P(O_), P(D_), n, P(out, 4)), "16-byte aligned"),
            ((P(both), P(D_), n, P(both)), "overlaps the rays"),
        ]
        for args, msg in cases:
            assert lib.vmx_raycast_device(sc._h, *args, 0, None) == L.VMX_ERR_INVALID
            assert msg in lib.vmx_last_error().decode()
        torch.cuda.synchronize()
        assert not out.any() and not both.any() and not host_out.any()
        # the same arrays, valid, give the records
        assert lib.vmx_raycast_device(sc._h, P(O_), P(D_), n, P(out), 0, None) == L.VMX_OK
        torch.cuda.synchronize()
        check(out[:n * 16].reshape(n, 16), sc.raycast(o, d), "valid")


# ---- Python layer ---------------------------------------------------------------------------------------------------
def test_python_tensors_equal_numpy_and_meshengine():
    pos, nrm, uv = scenes.cornell8()
    m = va.MeshEngine()
    m.loadTriangles(pos, nrm, uv)
    o, d = cornell_rays(5000, 45)
    host = m.sceneAccelerator.raycast(o, d)
    h = m.sceneAccelerator.raycast(dev(o), dev(d))
    torch.cuda.synchronize()
    for f in ("location", "distance", "normal", "tri_id", "uv", "tri_t", "flags", "colour"):
        x, y = host[f], h[f].cpu().numpy()
        assert x.shape == y.shape, f
        ok = same_f32(x, y) if x.dtype == np.float32 else (x.view(np.int32) == y)
        assert np.all(ok), f
    a = m.RayCast(o, d)
    b = m.RayCast(dev(o), dev(d))
    torch.cuda.synchronize()
    assert b[0].dtype == torch.bool and b[1].dtype == torch.bool
    for x, y in zip(a, b):
        y = y.cpu().numpy()
        assert x.shape == y.shape
        assert np.all(same_f32(x, y) if x.dtype == np.float32 else x == y)
    with pytest.raises(ValueError, match="mix"):
        m.RayCast(dev(o), d)
