"""The guide walk's skip of boxes that end behind the ray's origin (guide_walk.h, premise (B)), CPU only.

The stand-alone host program tests/cpp/guide_cull_test.cpp walks every ray over the guide twice or more: never
skipping (the marks of a copy of the records cleared), with the marks make_guide_records leaves (kGwShapeMax), and for
the sweep with other limits up to "inf", the plain cull that skips every such box.  Held here:

  * 0 wrong rays against the oracle's trace — the four scenes of test_guide_walk.py, the duplicate soup, every case of
    guide_cull_spec.cull_cases at 200,000 rays per shape (more than 2 M in all), the existing adversarial cases;
  * the generator bites: the plain cull settles rays wrongly on every fan whose shape is beyond 1,000;
  * the limit: the smallest shape at which the plain cull fails is at least four times kGwShapeMax, and beyond 32;
  * the settled share of sponza260k and cornell8 is no lower than without the skip, no ray of any case gets more visits,
    and the corrected bounce rays of sponza260k take at most 0.75 x the steps.

Measured (this file's prints, copied to profiles/guide_cull.txt):
  see profiles/guide_cull.txt sections 1 and 2 for the sweep's table and the visits per ray."""
import os

import numpy as np
import pytest

import guide_cull_spec as S
import guide_spec as G

HERE = os.path.dirname(os.path.abspath(__file__))
RAYS_PER_SHAPE = 200_000


def _scene(pos):
    import oracle_lib as O
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    osc = O.OracleScene(pos, G.flat_normals(pos), None)
    return pos, osc, osc.bvh()


def _both(name, osc, tree, pos, o, d, sanitize=False):
    """(never skipping, the library's marks) for the rays, checked: 0 wrong either way, no ray with more visits"""
    o, d = np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d, np.float32).reshape(-1, 3)
    plain, cull = S.host_cull(pos, tree, o, d, sanitize=sanitize)
    tri, rt = osc.trace(o, d)
    bad = [int(S.wrong(tri, rt, tree, r).sum()) for r in (plain, cull)]
    walk = plain["verdict"] != G.INPUT
    w = max(int(walk.sum()), 1)
    print("%s: %d rays (%d walk), wrong %d / %d, settled %d / %d, visits per walking ray %.1f + %.1f / %.1f + %.1f, "
          "%d of %d triangles beyond the limit, %d of %d child boxes unmarked"
          % (name, len(o), int(walk.sum()), bad[0], bad[1], int(np.isin(plain["verdict"], (G.SETTLED, G.MISS)).sum()),
             int(np.isin(cull["verdict"], (G.SETTLED, G.MISS)).sum()), plain["inner"].sum() / w, plain["tris"].sum() / w,
             cull["inner"].sum() / w, cull["tris"].sum() / w, cull["flagged"], len(pos), cull["unmarked"], cull["children"]))
    assert bad == [0, 0], name
    assert np.all(cull["inner"] <= plain["inner"]) and np.all(cull["tris"] <= plain["tris"]), name
    assert np.array_equal(plain["verdict"] == G.INPUT, cull["verdict"] == G.INPUT)
    return plain, cull, tri


@pytest.mark.parametrize("name,size", [("cornell8", (96, 64)), ("sponza260k", (160, 90)), ("bunny70k", (160, 90)),
                                       ("lattice", (96, 64))])
def test_scenes(name, size):
    import oracle_lib as O
    import vermilion_amd as va
    from vermilion_amd import scenes
    pos, nrm, uv = getattr(scenes, name)()
    c = {"cornell8": scenes.cornell_camera, "bunny70k": scenes.bunny_camera, "sponza260k": scenes.sponza_camera,
         "lattice": scenes.lattice_camera}[name]()
    cam = va.make_camera(c["position"], c["rotation_deg"], size[0], size[1], 64)
    osc = O.OracleScene(pos, nrm, uv)
    tree = osc.bvh()
    rays = [G.bounce_rays(osc, cam, 5 + k, kind) for k, kind in enumerate(("parity", "corrected", "uniform"))]
    o, d = np.concatenate([r[0] for r in rays]), np.concatenate([r[1] for r in rays])
    kinds = np.concatenate([np.full(len(r[0]), k) for k, r in enumerate(rays)])
    plain, cull, tri = _both("%s %dx%d" % (name, size[0], size[1]), osc, tree, pos, o, d)
    if name in ("sponza260k", "cornell8"):
        hits = tri >= 0
        assert np.sum((cull["verdict"] == G.SETTLED) & hits) >= np.sum((plain["verdict"] == G.SETTLED) & hits)
        assert np.sum(cull["verdict"] == G.MISS) >= np.sum(plain["verdict"] == G.MISS)
    if name == "sponza260k":
        m = kinds == 1
        steps = [int(r["inner"][m].sum()) + int(r["tris"][m].sum()) for r in (plain, cull)]
        print("sponza260k corrected rays: %d steps without the skip, %d with it: %.3f x" % (steps[0], steps[1], steps[1] / steps[0]))
        assert steps[1] <= 0.75 * steps[0]


def test_soup():
    import oracle_lib as O
    import vermilion_amd as va
    g = np.load(os.path.join(HERE, "golden", "ref_soup_duplicates.npz"))
    pos, nrm = g["pos"].reshape(-1, 9), g["nrm"].reshape(-1, 9)
    tree = {k: g["bvh_" + k] for k in ("start", "nprims", "right_offset", "bbox", "prim_order")}
    osc = O.OracleScene(pos, nrm, None, tree=tree)
    cam = va.make_camera(g["cam"][:3], g["cam"][3:6], 96, 64, 64)
    o0, d0 = O.primary_rays(cam, va.make_opts(seed=3), 0)
    o1, d1 = G.bounce_rays(osc, cam, 3, "uniform")
    _both("soup 96x64", osc, tree, pos, np.concatenate([o0, o1]), np.concatenate([d0, d1]))


def test_existing_adversarial_cases():
    for kind, pos, o, d in G.adversarial_cases():
        pos, osc, tree = _scene(pos)
        _both(kind, osc, tree, pos, o, d)


LIMITS = (4, 8, 32, 128, "inf")


def test_generator_and_sweep():
    """Every case of the generator, 200,000 rays per shape: never skipping, the limits of the sweep and the plain cull.
    Wrong rays: 0 without the skip and at every limit up to kGwShapeMax; the plain cull must fail on the shapes beyond
    1,000 (the generator bites), and the smallest shape at which it fails fixes the limit: kGwShapeMax is at most a quarter
    of it, and no shape up to 32 fails."""
    total, rows, failing, biting, shape_max = 0, [], [], {}, None
    for kind, K, pos, o, d in S.cull_cases(RAYS_PER_SHAPE):
        pos, osc, tree = _scene(pos)
        sets = S.host_cull(pos, tree, o, d, limits=LIMITS)
        tri, rt = osc.trace(o, d)
        shape_max = sets[0]["shape_max"]  # kGwShapeMax as guide_walk.h has it
        assert len(o) >= RAYS_PER_SHAPE, kind
        bad = [int(S.wrong(tri, rt, tree, r).sum()) for r in sets]
        visits = [float(np.mean(r["inner"].astype(np.float64) + r["tris"])) for r in sets]
        total += len(o)
        rows.append((kind, K, len(o), bad, visits))
        print("%-46s shape %-9s %7d rays  wrong: none %d | %s  visits: none %.2f | %s"
              % (kind, "%.1f" % K if K else "-", len(o), bad[0], " ".join("%s %d" % (l, b) for l, b in zip(LIMITS, bad[1:])),
                 visits[0], " ".join("%s %.2f" % (l, v) for l, v in zip(LIMITS, visits[1:]))), flush=True)
        for r in sets[1:]:
            assert np.all(r["inner"] <= sets[0]["inner"]) and np.all(r["tris"] <= sets[0]["tris"]), kind
        assert bad[0] == 0, (kind, "wrong without any skip", bad)
        for l, b in zip(LIMITS, bad[1:]):
            if l != "inf" and l <= shape_max:
                assert b == 0, (kind, l, b)
        if K is not None:
            if bad[-1]:
                failing.append(K)
            # the fans are what (B) is about: origins PAST a sliver.  The walls' rays start 0.001 above the wall, within
            # a pad of it (the bounce ray's own situation): the wall's boxes contain the origin and are never skipped, so
            # a wall need not bite — it must stay right
            if K >= 1000 and kind.startswith("fan"):
                biting[kind] = bad[-1]
    assert total >= 2_000_000
    assert len(biting) == 4 and all(b > 0 for b in biting.values()), biting
    assert shape_max in LIMITS
    assert min(failing) > 32 and shape_max <= min(failing) / 4, sorted(failing)
    print("smallest failing shape under the plain cull: %.1f; limit %.1f" % (min(failing), shape_max))


def test_host_program_under_sanitizers():
    """the stand-alone program built with -fsanitize=address,undefined, on cornell8 32x24"""
    import oracle_lib as O
    import vermilion_amd as va
    from vermilion_amd import scenes
    pos, nrm, uv = scenes.cornell8()
    c = scenes.cornell_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], 32, 24, 64)
    osc = O.OracleScene(pos, nrm, uv)
    tree = osc.bvh()
    o, d = G.bounce_rays(osc, cam, 9, "uniform")
    plain, cull, tri = _both("cornell8 32x24 (sanitizers)", osc, tree, pos, o, d, sanitize=True)
    assert np.any(cull["verdict"] == G.SETTLED)
