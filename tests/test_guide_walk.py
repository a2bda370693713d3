"""The guide walk and the per-ray rule of vermilion_amd/csrc/guide_walk.h (CPU only).

The header's walk and rule run in the stand-alone host program tests/cpp/guide_walk_test.cpp over the guide a scene
builds (the binned-SAH tree with padded boxes) beside the reference tree.  Every ray the rule settles must carry the
oracle's triangle and the bits of its t over the REFERENCE tree, every settled miss must be the oracle's miss: wrong
rays are 0 everywhere.  A rule that settles nothing is sound and useless: on sponza260k and cornell8 it must settle at
least three quarters of the hit rays.

Measured (this file's prints, copied to profiles/guide_tree.txt):
  see profiles/guide_tree.txt section 2 for the settled shares, the reasons for fallback and the visits per ray."""
import os

import numpy as np
import pytest

import guide_spec as G

HERE = os.path.dirname(os.path.abspath(__file__))


def _normals(pos):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    e1, e2 = pos[:, 3:6] - pos[:, 0:3], pos[:, 6:9] - pos[:, 0:3]
    nr = np.cross(e1, e2)
    ln = np.linalg.norm(nr, axis=1, keepdims=True)
    nr = np.where(ln > 0, nr / np.maximum(ln, 1e-30), np.float32([0, 1, 0])).astype(np.float32)
    return np.repeat(nr[:, None, :], 3, axis=1).reshape(-1, 9)


def _run(name, osc, tree, pos, o, d, sanitize=False):
    res = G.host_guide(pos, tree, o, d, sanitize=sanitize)
    bad, hits, misses = G.verdict(osc, tree, o, d, res)
    tri, _ = osc.trace(np.asarray(o, np.float32), np.asarray(d, np.float32))
    share = G.report(name, res, tri)
    return bad, hits, misses, share, res, tri


@pytest.mark.parametrize("name,size", [("cornell8", (96, 64)), ("sponza260k", (160, 90)), ("bunny70k", (160, 90)),
                                       ("lattice", (96, 64))])
def test_settled_rays_are_the_oracles(name, size):
    import oracle_lib as O
    import vermilion_amd as va
    from vermilion_amd import scenes
    pos, nrm, uv = getattr(scenes, name)()
    c = {"cornell8": scenes.cornell_camera, "bunny70k": scenes.bunny_camera, "sponza260k": scenes.sponza_camera,
         "lattice": scenes.lattice_camera}[name]()
    cam = va.make_camera(c["position"], c["rotation_deg"], size[0], size[1], 64)
    osc = O.OracleScene(pos, nrm, uv)
    tree = osc.bvh()
    os_, ds_, kinds = [], [], []
    for k, kind in enumerate(("parity", "corrected", "uniform")):
        o, d = G.bounce_rays(osc, cam, 5 + k, kind)
        os_.append(o), ds_.append(d), kinds.append(np.full(len(o), k))
    o, d, kinds = np.concatenate(os_), np.concatenate(ds_), np.concatenate(kinds)
    bad, hits, misses, share, res, tri = _run("%s %dx%d" % (name, size[0], size[1]), osc, tree, pos, o, d)
    assert bad == 0
    assert hits > 0
    # the reference's sampling draws r2 = 10 U: a direction with sqrt(1 - r2) = NaN never walks the guide
    nan = ~np.isfinite(d).all(axis=1)
    assert np.all(res["verdict"][nan] == G.INPUT)
    if name in ("sponza260k", "cornell8"):
        assert share >= 0.75
        for k in (1, 2):  # each finite sampling on its own as well
            m = (kinds == k) & (tri >= 0)
            assert np.sum(res["verdict"][m] == G.SETTLED) >= 0.75 * m.sum()


def test_soup_settles_no_duplicated_triangle():
    """tests/golden/ref_soup_duplicates.npz: every hit on a duplicated triangle is a tie that the reference resolves by
    test order: second = best there, and the rule must leave those rays to the reference tree"""
    import oracle_lib as O
    import vermilion_amd as va
    g = np.load(os.path.join(HERE, "golden", "ref_soup_duplicates.npz"))
    pos, nrm = g["pos"].reshape(-1, 9), g["nrm"].reshape(-1, 9)
    tree = {k: g["bvh_" + k] for k in ("start", "nprims", "right_offset", "bbox", "prim_order")}
    cpos, crot = g["cam"][:3], g["cam"][3:6]
    _, inverse, counts = np.unique(pos, axis=0, return_inverse=True, return_counts=True)
    dup = counts[inverse.reshape(-1)] > 1
    osc = O.OracleScene(pos, nrm, None, tree=tree)
    cam = va.make_camera(cpos, crot, 96, 64, 64)
    o0, d0 = O.primary_rays(cam, va.make_opts(seed=3), 0)
    o1, d1 = G.bounce_rays(osc, cam, 3, "uniform")
    o, d = np.concatenate([o0, o1]), np.concatenate([d0, d1])
    bad, hits, misses, share, res, tri = _run("soup 96x64", osc, tree, pos, o, d)
    assert bad == 0
    on_dup = (tri >= 0) & dup[np.maximum(tri, 0)]
    assert on_dup.any()
    assert not np.any(res["verdict"][on_dup] == G.SETTLED)


def _scene(pos):
    import oracle_lib as O
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    osc = O.OracleScene(pos, _normals(pos), None)
    return pos, osc, osc.bvh()


def _dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _towards(rng, o, target, spread, n):
    """n rays from o (one origin or [n, 3]) towards points within `spread` of target"""
    o = np.broadcast_to(np.asarray(o, np.float64), (n, 3))
    p = np.asarray(target, np.float64) + rng.uniform(-spread, spread, (n, 3))
    v = p - o
    return o.astype(np.float32), (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def test_adversarial_scenes():
    """The constructions of tests/test_claim_lists.py (its _tri and fan_scene, imported; the coplanar pair, the T-junction
    and the two planes a few floats apart built as it builds them) under free origins, and the cases a free origin adds:
    rays that start on a triangle or on a shared edge, grazing rays, a zero direction component, origins outside the
    scene's bounds."""
    from test_claim_lists import _tri, fan_scene
    rng = np.random.default_rng(17)
    settled, rays = {}, {}

    def run(kind, pos, o, d):
        pos, osc, tree = _scene(pos)
        bad, hits, misses, share, res, tri = _run(kind, osc, tree, pos, o, d)
        assert bad == 0, (kind, bad)
        settled[kind] = settled.get(kind, 0) + hits
        rays[kind] = rays.get(kind, 0) + int(np.sum(tri >= 0))
        return res, tri

    r, u, f = np.array([1.0, 0.2, 0.1]), np.array([-0.1, 1.0, 0.3]), np.array([0.2, -0.3, 1.0])
    r, u, f = r / np.linalg.norm(r), u / np.linalg.norm(u), f / np.linalg.norm(f)
    # the shared edge of a coplanar pair, rays aimed at and around the edge
    c = np.array([3.0, 2.0, 51.0])
    a, b = c - 40 * u, c + 40 * u
    pair = np.concatenate([_tri(a, b, c - 60 * r), _tri(b, a, c + 60 * r)])
    o, d = _towards(rng, (3.0, 2.0, 1.0), c, 0.01, 4000)
    o2, d2 = _towards(rng, (3.0, 2.0, 1.0), c, 30.0, 2000)
    run("coplanar pair", pair, np.concatenate([o, o2]), np.concatenate([d, d2]))
    # ... and rays that hit the edge itself: points of the edge from the float vertices, t near 50
    k = rng.uniform(-0.9, 0.9, (2000, 1))
    edge = (np.float32(c) + k * np.float32(40 * u)).astype(np.float64)
    o = np.broadcast_to(np.array([3.0, 2.0, 1.0]), edge.shape)
    v = edge - o
    run("coplanar pair, edge points", pair, o.astype(np.float32), (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32))
    # a T-junction
    a, b = c - 50 * r, c + 50 * r
    tj = np.concatenate([_tri(a, b, c - 60 * u), _tri(a, c, c + 60 * u), _tri(c, b, c + 60 * u)])
    o, d = _towards(rng, (3.0, 2.0, 1.0), c, 0.02, 3000)
    o2, d2 = _towards(rng, (3.0, 2.0, 1.0), c, 30.0, 1000)
    run("T-junction", tj, np.concatenate([o, o2]), np.concatenate([d, d2]))
    # two parallel planes 1, 4 and 64 floats apart: every ray that hits both is a tie within 2^-16
    for steps in (1, 4, 64):
        big = _tri(c - 25 * r - 25 * u, c + 50 * r - 25 * u, c - 25 * r + 50 * u).astype(np.float32)
        other = (big.view(np.int32) + np.int32(steps) * np.sign(big).astype(np.int32)).view(np.float32)
        o, d = _towards(rng, (3.0, 2.0, 1.0), c, 8.0, 2000)
        res, tri = run("close planes", np.concatenate([big, other]).astype(np.float64), o, d)
    assert settled["close planes"] == 0 and rays["close planes"] > 0
    # sliver fans in a coordinate plane, coordinates of magnitude 3, 1000 and 4096, every plane
    for width, axis, x0 in ((0.1, 1, 0.0), (0.02, 1, 0.0), (0.5, 1, 0.0), (0.1, 0, 0.0), (0.1, 2, 0.0), (0.1, 1, 1000.0),
                            (0.1, 1, -4096.0), (0.5, 2, 1000.0)):
        eye = np.array([x0 + 3.0, 2.0, 1.0]) + rng.uniform(-1, 1, 3)
        dd = np.array([0.5, 0.6, 0.62])
        dd /= np.linalg.norm(dd)
        fan = fan_scene(eye, dd, 100.0, width, 141.0, axis)
        hitp = eye + 100.0 * dd
        o, d = _towards(rng, eye, hitp, 4 * width, 3000)
        o2, d2 = _towards(rng, eye, hitp, 150.0, 1000)
        run("sliver fan in a coordinate plane", fan, np.concatenate([o, o2]), np.concatenate([d, d2]))
    assert 0 < settled["sliver fan in a coordinate plane"] < rays["sliver fan in a coordinate plane"]

    # ---- free origins
    # rays that start ON a triangle or on the shared edge of the pair (t near 0), into the half space of a second wall
    wall = _tri(c + 30 * f - 200 * r - 200 * u, c + 30 * f + 400 * r - 200 * u, c + 30 * f - 200 * r + 400 * u)
    room = np.concatenate([pair, wall])
    k = rng.uniform(-0.9, 0.9, (1500, 1))
    on_edge = (np.float32(c) + k * np.float32(40 * u)).astype(np.float32)
    on_face = (np.float32(c) + k * np.float32(30 * u) + rng.uniform(-20, 20, (1500, 1)) * np.float32(r)).astype(np.float32)
    o = np.concatenate([on_edge, on_face])
    run("origins on a triangle", room, o, _dirs(rng, len(o)))
    # grazing rays: within 1e-4 of the plane of the pair, from beside it
    side = c - 70 * r + rng.uniform(-1e-4, 1e-4, (3000, 1)) * np.cross(r, u)
    tgt = c + 70 * r + rng.uniform(-30, 30, (3000, 1)) * u + rng.uniform(-1e-4, 1e-4, (3000, 1)) * np.cross(r, u)
    v = tgt - side
    run("grazing rays", room, side.astype(np.float32), (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32))
    # a direction with a zero component must fall back (its reciprocal is infinite)
    o, d = _towards(rng, (3.0, 2.0, 1.0), c, 20.0, 600)
    d = d.copy()
    d[:200, 0], d[200:400, 1], d[400:, 2] = 0.0, 0.0, -0.0
    res, tri = run("zero direction component", room, o, d)
    assert np.all(res["verdict"] == G.INPUT)
    # origins outside the scene's bounds: beyond M = four times the largest |coordinate| (about 450 here) the rule falls
    # back; inside it, it may settle
    o, d = _towards(rng, (9000.0, -7000.0, 8000.0), c, 30.0, 1000)
    res, tri = run("origins outside the bounds", room, o, d)
    assert np.all(res["verdict"] == G.INPUT)
    o, d = _towards(rng, (-900.0, 700.0, -800.0), c, 30.0, 1000)  # outside the vertex box, within M
    res, tri = run("origins outside the vertex box", room, o, d)
    for kind in sorted(rays):
        print("%-36s settled %d of %d hit rays" % (kind, settled[kind], rays[kind]))
    for kind in ("coplanar pair", "T-junction", "origins on a triangle", "origins outside the vertex box"):
        assert settled[kind] > 0, kind


def test_host_program_under_sanitizers():
    """the stand-alone program built with -fsanitize=address,undefined, on cornell8"""
    import oracle_lib as O
    import vermilion_amd as va
    from vermilion_amd import scenes
    pos, nrm, uv = scenes.cornell8()
    c = scenes.cornell_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], 32, 24, 64)
    osc = O.OracleScene(pos, nrm, uv)
    tree = osc.bvh()
    o, d = G.bounce_rays(osc, cam, 9, "uniform")
    bad, hits, misses, share, res, tri = _run("cornell8 32x24 (sanitizers)", osc, tree, pos, o, d, sanitize=True)
    assert bad == 0 and hits > 0
