"""Device ray queries (vmx_query_device / vmx_query, k_query) on the GPU: NEAREST with and without a bound, ANY and
COLLISION against the identities of include/vermilion_hip.h, checked against today's vmx_trace and the CPU oracle."""
import os

import numpy as np
import pytest
import torch

import oracle_lib as O
import vermilion_amd as va
from shared_inputs import special_rays
from vermilion_amd import scenes

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BIG = np.float32(999999999.0)  # bvh.cpp:48
EPS = np.float32(1e-3)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_f32(x, y):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    return (bits(x) == bits(y)) | (np.isnan(x) & np.isnan(y))


def rand_rays(n, seed, lo=(-1500, 5, -900), hi=(1500, 950, 900)):
    r = np.random.RandomState(seed)
    o = r.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = r.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


def expected(id_ref, t_ref, tmax=None):
    """(tri, t, hit) of NEAREST, hit of ANY, hit of COLLISION from the unbounded result (vmx_trace)"""
    n = id_ref.shape[0]
    if tmax is None:
        tmax = np.full(n, np.inf, np.float32)
    tmax = np.asarray(tmax, np.float32)
    with np.errstate(invalid="ignore"):
        bad = ~(tmax > 0)
        lim = np.where(bad, tmax, np.minimum(tmax, BIG)).astype(np.float32)
        inside = ~bad & (id_ref >= 0) & (t_ref < lim)
    tri = np.where(inside, id_ref, -1).astype(np.int32)
    t = np.where(inside, t_ref, lim).astype(np.float32)
    hit = tri >= 0
    return tri, t, hit, hit.copy(), hit & (t >= EPS)


def check_window(sc, o, d, tmax, ref, tag):
    """Bounds a few ulps above t_ref: a box's slab `near` can lie those ulps above the Moeller-Trumbore t of a
    triangle inside it, and the bounded traversal then prunes that box (`near > best`, bvh.cpp:69) where the unbounded
    one, with a larger running `best`, did not.  What holds exactly: a NEAREST hit is the unbounded hit; every NEAREST
    hit is an ANY hit and every ANY hit an unbounded hit below L; COLLISION judges the NEAREST result."""
    id_ref, t_ref = ref
    etri, et, ehit, eany, ecoll = expected(id_ref, t_ref, tmax)
    tri, t, hit = sc.query(o, d, tmax, mode="nearest")
    lim = np.minimum(tmax, BIG)
    assert np.all((tri == etri) | ((tri == -1) & same_f32(t, lim))), tag
    assert np.all(same_f32(t[tri >= 0], et[tri >= 0])) and np.array_equal(hit, tri >= 0), tag
    any_hit = sc.query(o, d, tmax, mode="any")
    assert np.all(~hit | any_hit) and np.all(~any_hit | eany), tag
    ctri, ct, chit = sc.query(o, d, tmax, mode="collision")
    assert np.array_equal(ctri, tri) and np.all(same_f32(ct, t)) and np.array_equal(chit, hit & (t >= EPS)), tag
    return int((tri != etri).sum())


def check_all_modes(sc, o, d, tmax=None, ref=None, tag=""):
    """every mode through the host entry against the identities; returns the NEAREST result"""
    id_ref, t_ref = ref if ref is not None else sc.trace(o, d)
    etri, et, ehit, eany, ecoll = expected(id_ref, t_ref, tmax)
    tri, t, hit = sc.query(o, d, tmax, mode="nearest")
    assert np.array_equal(tri, etri), (tag, int((tri != etri).sum()))
    assert np.all(same_f32(t, et)), (tag, int((~same_f32(t, et)).sum()))
    assert np.array_equal(hit, ehit), tag
    any_hit = sc.query(o, d, tmax, mode="any")
    assert np.array_equal(any_hit, eany), (tag, int((any_hit != eany).sum()))
    ctri, ct, chit = sc.query(o, d, tmax, mode="collision")
    assert np.array_equal(ctri, etri) and np.all(same_f32(ct, et)), tag
    assert np.array_equal(chit, ecoll), (tag, int((chit != ecoll).sum()))
    return tri, t


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class Pair:
    def __init__(self, pos, nrm, uv=None, spheres=None, builder=va._lib.VMX_BVH_REFERENCE):
        self.gpu = va.Scene(pos, nrm, uv, spheres=spheres, builder=builder)
        tree = self.gpu.bvh() if builder != va._lib.VMX_BVH_REFERENCE else None
        self.cpu = O.OracleScene(pos, nrm, uv, spheres=spheres, tree=tree)

    def close(self):
        self.gpu.close()
        self.cpu.close()


@pytest.fixture(scope="module", params=["cornell8", "lattice", "bunny70k", "sponza260k"])
def pair(request):
    gen, camf = scenes.SCENES[request.param]
    p = Pair(*gen())
    p.name, p.camf = request.param, camf
    yield p
    p.close()


def primary(pair, W=160, H=96):
    c = pair.camf()
    cam = va.make_camera(c["position"], c["rotation_deg"], W, H, 4)
    return O.primary_rays(cam, va.make_opts(seed=3), 1)


# ---- NEAREST without a bound == vmx_trace == the oracle, host and device entries ----------------------------
def test_nearest_unbounded_bit_exact(pair):
    for o, d in (rand_rays(200000 if pair.name != "cornell8" else 60000, 11), primary(pair)):
        id_ref, t_ref = pair.gpu.trace(o, d)
        otri, ot = pair.cpu.trace(o, d)
        assert np.array_equal(id_ref, otri) and np.array_equal(bits(t_ref), bits(ot))
        tri, t, hit = pair.gpu.query(o, d)
        assert np.array_equal(tri, otri) and np.array_equal(bits(t), bits(ot))
        assert np.array_equal(hit, otri >= 0)
        for per_lane in (False, True):
            dtri, dt, dhit = pair.gpu.query(dev(o), dev(d), per_lane_fetch=per_lane)
            torch.cuda.synchronize()
            assert dtri.dtype == torch.int32 and dt.dtype == torch.float32 and dhit.dtype == torch.bool
            assert np.array_equal(dtri.cpu().numpy(), otri) and np.array_equal(bits(dt.cpu().numpy()), bits(ot))
            assert np.array_equal(dhit.cpu().numpy(), otri >= 0)
        check_all_modes(pair.gpu, o, d, ref=(id_ref, t_ref), tag=pair.name)


@pytest.mark.parametrize("builder", [va._lib.VMX_BVH_SAH, va._lib.VMX_BVH_LBVH, va._lib.VMX_BVH_PLOC])
def test_nearest_on_other_trees(builder):
    """SAH / LBVH / PLOC trees: the query follows that tree's order exactly as vmx_trace and the oracle do over it"""
    o, d = rand_rays(200000, 12)
    for gen in (scenes.bunny70k, scenes.sponza260k):
        p = Pair(*gen(), builder=builder)
        id_ref, t_ref = p.gpu.trace(o, d)
        otri, ot = p.cpu.trace(o, d)
        assert np.array_equal(id_ref, otri) and np.array_equal(bits(t_ref), bits(ot))
        tri, t = check_all_modes(p.gpu, o, d, ref=(id_ref, t_ref), tag=builder)
        assert np.array_equal(tri, otri) and np.array_equal(bits(t), bits(ot))
        r = np.random.RandomState(builder)
        tmax = np.where(r.rand(len(o)) < 0.5, t_ref, r.uniform(1, 2500, len(o))).astype(np.float32)
        check_all_modes(p.gpu, o, d, tmax, ref=(id_ref, t_ref), tag=(builder, "tmax"))
        p.close()


# ---- special rays, deep trees ---------------------------------------------------------------------------------
def test_special_rays_nan_slabs_ties_and_degenerates():
    o, d = special_rays()
    for gen in (scenes.cornell8, scenes.lattice):
        p = Pair(*gen())
        id_ref, t_ref = p.gpu.trace(o, d)
        otri, ot = p.cpu.trace(o, d)
        assert np.array_equal(id_ref, otri) and np.array_equal(bits(t_ref), bits(ot))
        tri, t = check_all_modes(p.gpu, o, d, ref=(id_ref, t_ref))
        assert np.array_equal(tri, otri) and np.array_equal(bits(t), bits(ot))
        tmax = np.where(np.arange(len(o)) % 2 == 0, t_ref, np.float32(500)).astype(np.float32)
        check_all_modes(p.gpu, o, d, tmax, ref=(id_ref, t_ref))
        p.close()


def test_deep_tree_uses_the_overflow_slab():
    """the bench scene's reference tree is deeper than the 9 stack levels k_query keeps in LDS: deep rays spill to
    the per-wave HBM slab and must still come out exact"""
    p = Pair(*scenes.sponza260k())
    assert p.gpu.describe()["stack_entries"] > 12
    o, d = rand_rays(300000, 13)
    otri, ot = p.cpu.trace(o, d)
    tri, t = check_all_modes(p.gpu, o, d)
    assert np.array_equal(tri, otri) and np.array_equal(bits(t), bits(ot))
    p.close()


# ---- bounds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell8", "sponza260k"])
def test_tmax_sweep(name):
    gen, camf = scenes.SCENES[name]
    with va.Scene(*gen()) as sc:
        o, d = rand_rays(100000, 14)
        id_ref, t_ref = sc.trace(o, d)
        n = len(o)
        inf32 = np.float32(np.inf)
        # one ulp above t_ref: the window of check_window (measured: 0.3 % of the rays report a miss on cornell8,
        # 1.2 % on sponza260k, whose walls and beams put many hits on box faces)
        above = np.nextafter(t_ref, inf32)
        missed = check_window(sc, o, d, above, (id_ref, t_ref), "above")
        assert missed < 0.05 * n, missed
        sweeps = {
            "t_ref": t_ref,
            "above_1e-3": (t_ref * np.float32(1.001)).astype(np.float32),
            "below": np.nextafter(t_ref, np.float32(0)),
            "zero": np.zeros(n, np.float32),
            "minus1": np.full(n, -1, np.float32),
            "nan": np.full(n, np.nan, np.float32),
            "inf": np.full(n, inf32),
            "1e30": np.full(n, 1e30, np.float32),
            "big": np.full(n, BIG),
            "below_big": np.full(n, np.nextafter(BIG, np.float32(0))),
            "mixed": np.where(np.arange(n) % 3 == 0, np.nan,
                              np.where(np.arange(n) % 3 == 1, t_ref * np.float32(0.5), np.float32(-0.0))).astype(np.float32),
        }
        for tag, tm in sweeps.items():
            tm = np.ascontiguousarray(tm, np.float32)
            tri, t = check_all_modes(sc, o, d, tm, ref=(id_ref, t_ref), tag=tag)
            if tag == "t_ref":
                assert np.all(tri == -1)  # strict: a hit at exactly t_ref is not below the bound
            if tag in ("above_1e-3", "inf", "1e30", "big"):
                assert np.array_equal(tri, id_ref)
            if tag in ("zero", "minus1", "nan"):
                assert np.all(tri == -1) and np.all(same_f32(t, tm))


def test_any_hit_shadow_rays():
    """shadow rays from RayCast hit points toward the emitting spheres' centres, bounded at distance - radius"""
    pos, nrm, uv = scenes.sponza260k()
    with va.Scene(pos, nrm, uv) as sc:
        o, d = rand_rays(200000, 15)
        h = sc.raycast(o, d)
        keep = h["tri_id"] >= 0
        p = h["location"][keep].astype(np.float32)
        sph = va.default_spheres()
        so, sd, st = [], [], []
        for s in sph:
            if not (s.flags & va._lib.VMX_SPHERE_EMIT):
                continue
            c = np.float32(list(s.centre))
            v = (c[None, :] - p).astype(np.float32)
            dist = np.linalg.norm(v.astype(np.float64), axis=1).astype(np.float32)
            so.append(p), sd.append((v / dist[:, None]).astype(np.float32)), st.append((dist - np.float32(s.radius)).astype(np.float32))
        so, sd, st = np.concatenate(so), np.concatenate(sd), np.concatenate(st)
        id_ref, t_ref = sc.trace(so, sd)
        check_all_modes(sc, so, sd, st, ref=(id_ref, t_ref), tag="shadow")
        occluded = sc.query(so, sd, st, mode="any")
        assert occluded.any() and not occluded.all()  # both outcomes occur
        # the device entry gives the same
        dh = sc.query(dev(so), dev(sd), dev(st), mode="any")
        assert np.array_equal(dh.cpu().numpy(), occluded)


def test_collision_near_the_threshold():
    """origins just off a triangle along the ray, so that the nearest t lies in [0, 2e-3]: RayCastCollision's
    `t > 1e-3` is decided in float as t >= 1e-3f"""
    pos, nrm, uv = scenes.cornell8()
    with va.Scene(pos, nrm, uv) as sc:
        o, d = rand_rays(200000, 16, lo=(-500, 5, -700), hi=(500, 890, 1500))
        tri, t = sc.trace(o, d)
        keep = (tri >= 0) & (t > 1.0)
        o, d, t = o[keep], d[keep], t[keep]
        r = np.random.RandomState(17)
        back = r.uniform(0, 2e-3, len(t)).astype(np.float32)
        o2 = (o + d * (t - back)[:, None]).astype(np.float32)
        id_ref, t_ref = sc.trace(o2, d)
        near = (id_ref >= 0) & (t_ref <= 2e-3)
        assert near.sum() > 1000 and (t_ref[near] >= EPS).any() and (t_ref[near] < EPS).any()
        check_all_modes(sc, o2, d, ref=(id_ref, t_ref), tag="collision")
        _, _, ch = sc.query(o2, d, mode="collision")
        assert np.array_equal(ch, (id_ref >= 0) & (t_ref.astype(np.float64) > 1e-3))  # the reference's double compare


# ---- sizes, workspace, streams ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_small_sizes(n):
    pos, nrm, uv = scenes.lattice()
    with va.Scene(pos, nrm, uv) as sc:
        o, d = rand_rays(max(n, 1), 18 + n)
        o, d = o[:n], d[:n]
        tri, t, hit = sc.query(o, d)
        assert tri.shape == (n,) and t.shape == (n,) and hit.shape == (n,)
        if n:
            check_all_modes(sc, o, d)
        dtri, dt, dhit = sc.query(dev(o).reshape(n, 3), dev(d).reshape(n, 3))
        torch.cuda.synchronize()
        assert np.array_equal(dtri.cpu().numpy(), tri) and np.array_equal(bits(dt.cpu().numpy()), bits(t))


def test_large_batch_on_the_device():
    """2^24 + 17 rays generated on the device, compared with vmx_trace of the same rays"""
    n = (1 << 24) + 17
    pos, nrm, uv = scenes.cornell8()
    with va.Scene(pos, nrm, uv) as sc:
        g = torch.Generator(device="cuda:0")
        g.manual_seed(19)
        lo = torch.tensor([-500.0, 5.0, -700.0], device="cuda:0")
        hi = torch.tensor([500.0, 890.0, 1500.0], device="cuda:0")
        o = (lo + (hi - lo) * torch.rand((n, 3), generator=g, device="cuda:0")).contiguous()
        d = torch.randn((n, 3), generator=g, device="cuda:0")
        d = (d / d.norm(dim=1, keepdim=True)).contiguous()
        tm = (torch.rand(n, generator=g, device="cuda:0") * 2000.0).contiguous()
        tri, t, hit = sc.query(o, d)
        ahit = sc.query(o, d, tm, mode="any")
        torch.cuda.synchronize()
        on, dn, tmn = o.cpu().numpy(), d.cpu().numpy(), tm.cpu().numpy()
        id_ref, t_ref = sc.trace(on, dn)
        assert np.array_equal(tri.cpu().numpy(), id_ref) and np.array_equal(bits(t.cpu().numpy()), bits(t_ref))
        assert np.array_equal(hit.cpu().numpy(), id_ref >= 0)
        assert np.array_equal(ahit.cpu().numpy(), expected(id_ref, t_ref, tmn)[3])


def test_workspace_reuse_and_two_streams():
    pos, nrm, uv = scenes.bunny70k()
    with va.Scene(pos, nrm, uv) as sc:
        a_o, a_d = rand_rays(300000, 20)
        b_o, b_d = rand_rays(250000, 21)
        a_ref, b_ref = sc.trace(a_o, a_d), sc.trace(b_o, b_d)
        A = (dev(a_o), dev(a_d))
        B = (dev(b_o), dev(b_d))
        torch.cuda.synchronize()
        # back to back on one stream, different batches and modes
        r1 = sc.query(*A)
        r2 = sc.query(*B, mode="collision")
        r3 = sc.query(*A, mode="any")
        torch.cuda.synchronize()
        assert np.array_equal(r1[0].cpu().numpy(), a_ref[0]) and np.array_equal(bits(r1[1].cpu().numpy()), bits(a_ref[1]))
        assert np.array_equal(r2[0].cpu().numpy(), b_ref[0]) and np.array_equal(bits(r2[1].cpu().numpy()), bits(b_ref[1]))
        assert np.array_equal(r2[2].cpu().numpy(), expected(*b_ref)[4])
        assert np.array_equal(r3.cpu().numpy(), a_ref[0] >= 0)
        # two torch streams, no synchronisation between the calls
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        s1.wait_stream(torch.cuda.current_stream())
        s2.wait_stream(torch.cuda.current_stream())
        outs = []
        for rep in range(3):
            with torch.cuda.stream(s1):
                x = sc.query(*A)
            with torch.cuda.stream(s2):
                y = sc.query(*B)
            outs.append((x, y))
        torch.cuda.synchronize()
        for x, y in outs:
            assert np.array_equal(x[0].cpu().numpy(), a_ref[0]) and np.array_equal(bits(x[1].cpu().numpy()), bits(a_ref[1]))
            assert np.array_equal(y[0].cpu().numpy(), b_ref[0]) and np.array_equal(bits(y[1].cpu().numpy()), bits(b_ref[1]))


# ---- Python layer ---------------------------------------------------------------------------------------------
def test_python_layer_numpy_torch_and_meshengine():
    pos, nrm, uv = scenes.cornell8()
    m = va.MeshEngine()
    m.loadTriangles(pos, nrm, uv)
    sc = m.sceneAccelerator
    o, d = rand_rays(5000, 22, lo=(-500, 5, -700), hi=(500, 890, 1500))
    tm = np.random.RandomState(23).uniform(-10, 1500, len(o)).astype(np.float32)
    for mode in ("nearest", "collision", "any"):
        a = sc.query(o, d, tm, mode=mode)
        b = sc.query(dev(o), dev(d), dev(tm), mode=mode)
        torch.cuda.synchronize()
        a, b = (a, b) if mode != "any" else ((a,), (b,))
        for x, y in zip(a, b):
            y = y.cpu().numpy()
            assert x.dtype == y.dtype and np.all(same_f32(x, y) if x.dtype == np.float32 else x == y), mode
    batch = m.RayCastCollision(o, d)
    _, _, ch = sc.query(o, d, mode="collision")
    assert batch.dtype == np.bool_ and np.array_equal(batch, ch)
    for i in range(0, 5000, 397):
        one = m.RayCastCollision(o[i], d[i])
        assert isinstance(one, bool) and one == bool(batch[i])
    # device inputs are taken as they are or refused: never copied through the host
    O3, D3 = dev(o), dev(d)
    with pytest.raises(ValueError, match="float32"):
        sc.query(O3.double(), D3.double())
    with pytest.raises(ValueError, match="contiguous"):
        sc.query(O3.t().contiguous().t(), D3)
    with pytest.raises(ValueError, match="cuda"):
        sc.query(torch.from_numpy(o), torch.from_numpy(d))
    with pytest.raises(ValueError, match="mix"):
        sc.query(O3, d)
    with pytest.raises(ValueError, match=r"\[n\]"):
        sc.query(O3, D3, dev(tm[:10]))
