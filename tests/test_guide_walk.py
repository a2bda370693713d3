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
    osc = O.OracleScene(pos, G.flat_normals(pos), None)
    return pos, osc, osc.bvh()


def test_adversarial_scenes():
    """The scenes and rays of guide_spec.adversarial_cases (one seeded generator, shared with the device's test): the
    constructions of tests/test_claim_lists.py under free origins, and the cases a free origin adds: rays that start on a
    triangle or on a shared edge, grazing rays, a zero direction component, origins outside the scene's bounds."""
    settled, rays = {}, {}
    for kind, pos, o, d in G.adversarial_cases():
        pos, osc, tree = _scene(pos)
        bad, hits, misses, share, res, tri = _run(kind, osc, tree, pos, o, d)
        assert bad == 0, (kind, bad)
        settled[kind] = settled.get(kind, 0) + hits
        rays[kind] = rays.get(kind, 0) + int(np.sum(tri >= 0))
        # a direction with a zero component must fall back (its reciprocal is infinite); so must an origin beyond M = four
        # times the largest |coordinate| (about 450 here)
        if kind in ("zero direction component", "origins outside the bounds"):
            assert np.all(res["verdict"] == G.INPUT)
        if kind == "tie across subtrees":  # the patch is triangles 0-15: each of its hits ties with the pair behind it
            on_patch = (tri >= 0) & (tri < 16)
            assert on_patch.sum() > 1000 and np.all(res["verdict"][on_patch] == G.TIE)
    assert settled["close planes"] == 0 and rays["close planes"] > 0
    assert 0 < settled["sliver fan in a coordinate plane"] < rays["sliver fan in a coordinate plane"]
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
