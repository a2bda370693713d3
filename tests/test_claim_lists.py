"""List claims of vermilion_amd/csrc/pixel_claim.h (CPU only): for a pixel without a single claim, a list of up to four
triangles; a camera ray of the pixel is settled by its own test on the members alone where pc_list_settle says so.

The header's procedure and rule run in the stand-alone host program tests/cpp/pixel_claim_list_test.cpp over the exported
flat tree.  The oracle traces all 64 samples and the nine footprint points of every pixel; every ray the rule settles
must carry the oracle's triangle and the bits of its t.  A rule that settles nothing is sound and useless: single claims
and lists together must cover at least half of the pixels that the oracle finds to see at most two triangles (or
nothing), and on sponza260k and cornell8 the rule must settle at least half of the rays of the pixels with a list.

Measured (this file's prints, copied to profiles/claim_lists.txt section 2; shares of all pixels):
  cornell8 96x64      claims 86.1 %, lists 11.2 %, oracle at most two ids 99.3 %, settled 74.8 % of the list pixels' rays
  bunny70k 160x90     claims 73.8 %, lists  6.1 %, oracle at most two ids 81.4 %, settled 75.0 %
  sponza260k 160x90   claims 19.6 %, lists  8.4 %, oracle at most two ids 25.2 %, settled 97.5 %
  lattice 96x64       claims 56.8 %, lists 28.8 %, oracle at most two ids 99.2 %, settled 37.5 %
All four scenes are held to the pixel share."""
import os

import numpy as np
import pytest

import claim_list_spec as LS

HERE = os.path.dirname(os.path.abspath(__file__))


def check(osc, tree, pos, cam, seed=3, spp=64, sanitize=False):
    """Runs procedure and rule over every pixel's samples and footprint points.  Returns (wrongly settled rays, settled
    rays, rays of pixels with a list, claims, lists, pix, settled slot)"""
    W, H = cam.image_res[0], cam.image_res[1]
    pix, dirs = LS.sample_rays(cam, np.arange(W * H, dtype=np.uint32), spp, seed)
    claims, lists, slot, t = LS.host_lists(pos, tree, [cam], rays=[(pix, dirs)], sanitize=sanitize)[0]
    n = LS.list_lengths(lists)
    assert not np.any((n > 0) & (claims.reshape(-1) != LS.NONE)), "a pixel with a single claim carries a list"
    assert not np.any((slot != LS.NONE) & (n[pix] == 0)), "a ray of a pixel without a list was settled"
    rec = lists.reshape(-1, LS.WORDS)
    pad = rec == LS.NONE
    assert np.all(pad[:, 1:] >= pad[:, :-1]), "padding precedes a member"
    bad, settled = LS.verdict(osc, tree, cam, pix, dirs, slot, t)
    return bad, settled, int(np.sum(n[pix] > 0)), claims, lists, pix, slot


def oracle_two_share(osc, cam, spp=64, seed=3):
    """share of pixels whose samples return at most two triangle ids (misses aside), or nothing"""
    import oracle_lib as O
    import vermilion_amd as va
    W, H = cam.image_res[0], cam.image_res[1]
    opts = va.make_opts(seed=seed)
    tris = np.empty((spp, W * H), np.int64)
    for k in range(spp):
        o, d = O.primary_rays(cam, opts, k)
        tris[k] = osc.trace(o, d)[0]
    tris.sort(axis=0)
    distinct = 1 + np.sum(tris[1:] != tris[:-1], axis=0) - (tris[0] < 0)  # ids >= 0
    return float(np.mean(distinct <= 2))


@pytest.mark.parametrize("name,size", [("cornell8", (96, 64)), ("bunny70k", (160, 90)), ("sponza260k", (160, 90)),
                                       ("lattice", (96, 64))])
def test_settled_rays_are_the_oracles(name, size):
    import oracle_lib as O
    import vermilion_amd as va
    from vermilion_amd import scenes
    pos, nrm, uv = getattr(scenes, name)()
    c = {"cornell8": scenes.cornell_camera, "bunny70k": scenes.bunny_camera, "sponza260k": scenes.sponza_camera,
         "lattice": scenes.lattice_camera}[name]()
    W, H = size
    cam = va.make_camera(c["position"], c["rotation_deg"], W, H, 64)
    osc = O.OracleScene(pos, nrm, uv)
    tree = osc.bvh()
    bad, settled, list_rays, claims, lists, _, _ = check(osc, tree, pos, cam)
    single = float(np.mean(claims != LS.NONE))
    listed = float(np.mean(LS.list_lengths(lists) > 0))
    two = oracle_two_share(osc, cam)
    rate = settled / max(list_rays, 1)
    hist = np.bincount(LS.list_lengths(lists), minlength=5) / float(W * H)
    print("%s %dx%d: single claims %.1f %%, list pixels %.1f %% (lengths 1-4: %s), oracle at most two ids %.1f %%, settled %.1f %% of "
          "the list pixels' rays" % (name, W, H, 100 * single, 100 * listed, " ".join("%.1f" % (100 * h) for h in hist[1:]),
                                     100 * two, 100 * rate))
    assert bad == 0
    assert listed > 0 and settled > 0
    assert single + listed >= 0.5 * two
    if name in ("sponza260k", "cornell8"):
        assert rate >= 0.5


def test_soup_settles_no_duplicated_triangle():
    """tests/golden/ref_soup_duplicates.npz: every hit on a duplicated triangle is a tie that the reference resolves by
    test order — the tie band of the rule must leave those rays to the walk"""
    import oracle_lib as O
    import vermilion_amd as va
    g = np.load(os.path.join(HERE, "golden", "ref_soup_duplicates.npz"))
    pos, nrm = g["pos"].reshape(-1, 9), g["nrm"].reshape(-1, 9)
    tree = {k: g["bvh_" + k] for k in ("start", "nprims", "right_offset", "bbox", "prim_order")}
    cpos, crot = g["cam"][:3], g["cam"][3:6]
    _, inverse, counts = np.unique(pos, axis=0, return_inverse=True, return_counts=True)
    dup = counts[inverse.reshape(-1)] > 1
    osc = O.OracleScene(pos, nrm, None, tree=tree)
    for W, H in ((96, 64), (33, 17)):
        cam = va.make_camera(cpos, crot, W, H, 64)
        bad, settled, list_rays, claims, lists, pix, slot = check(osc, tree, pos, cam)
        ids = tree["prim_order"][slot[slot != LS.NONE]]
        print("soup %dx%d: list pixels %.1f %%, settled %d of %d rays" % (W, H, 100 * np.mean(LS.list_lengths(lists) > 0), settled, list_rays))
        assert bad == 0
        assert not np.any(dup[ids])


def test_random_cameras_inside_sponza():
    """the forty cameras of test_pixel_claims.py: random rotations, axis-aligned ones, cameras 1e-3 ... 10 units from the
    floor or a wall"""
    import oracle_lib as O
    import vermilion_amd as va
    from vermilion_amd import scenes
    pos, nrm, uv = scenes.sponza260k()
    osc = O.OracleScene(pos, nrm, uv)
    tree = osc.bvh()
    rng = np.random.default_rng(21)
    cams = []
    for trial in range(40):
        W, H = (160, 90) if trial in (0, 21) else ((64, 40) if trial % 5 == 3 else (33, 17))
        p = rng.uniform(-1300, 1300, 3) * np.array([1.0, 0.0, 0.3]) + np.array([0.0, rng.uniform(50, 900), 0.0])
        rot = rng.uniform(-180, 180, 3) * np.array([0.3, 1.0, 0.1])
        if trial % 4 == 1:  # axis-aligned
            rot = np.array([0.0, 90.0 * rng.integers(0, 4), 0.0])
        if trial % 4 == 2:  # close to the floor / a side wall
            dist = np.exp(rng.uniform(np.log(1e-3), np.log(10.0)))
            if rng.integers(0, 2):
                p[1] = dist
            else:
                p[0] = -1500.0 + dist
        cams.append(va.make_camera(p, rot, W, H, 64, back_size=(3.6, 3.6 * H / W)))
    bad = settled = rays = 0
    for i, cam in enumerate(cams):
        b, s, r, _, lists, _, _ = check(osc, tree, pos, cam, seed=i)
        bad, settled, rays = bad + b, settled + s, rays + r
        if i % 4 == 1:  # a cone on a coordinate plane: the pixel column and row that contain one have no list
            n = LS.list_lengths(lists).reshape(lists.shape[:2])
            assert np.any(np.all(n == 0, axis=0)) and np.any(np.all(n == 0, axis=1))
    print("40 cameras: settled %d of %d rays of list pixels" % (settled, rays))
    assert bad == 0 and settled > 0


def _tri(*v):
    return np.array(v, np.float64).reshape(1, 9)


def fan_scene(o, d, D, width, length, axis=1):
    """Eight triangles `width` x `length` in the coordinate plane (axis = const) that the ray o + t d meets at t = D, their
    short edges side by side on a line of constant z (x for axis 2) through that point and their far end a common apex
    off to the side (first vertex: both edges run along the diagonal, so the terms of det and cd cancel by
    length / width), and one large triangle in the same plane beyond the line: thin triangles whose own box has no extent
    on one axis and whose float t is off by far more than the slab slack"""
    a, b = [(1, 2), (2, 0), (0, 1)][axis]  # b: the axis the slivers run along
    c = o + D * d
    e_a, e_b = np.zeros(3), np.zeros(3)
    e_a[a], e_b[b] = 1.0, 1.0
    apex = c - (length / np.sqrt(2.0)) * (e_a + e_b)
    tris = [_tri(apex, c + (i * width) * e_a, c + ((i + 1) * width) * e_a) for i in range(-4, 4)]
    tris.append(_tri(c - 200 * e_a, c + 200 * e_a, c + 300 * e_b))
    return np.concatenate(tris)


def test_adversarial_single_pixel_scenes():
    """scenes of a few triangles built around one pixel of a 33x17 frame; every pixel of the frame is checked"""
    import oracle_lib as O
    import vermilion_amd as va
    from test_pixel_claims import _basis
    W, H = 33, 17
    rng = np.random.default_rng(11)
    made = []

    def setup(origin=(3.0, 2.0, 1.0), rot=None, back=3.6):
        rot = rng.uniform(-180, 180, 3) * np.array([0.3, 1.0, 0.1]) if rot is None else np.array(rot, np.float64)
        cam = va.make_camera(np.array(origin) + rng.uniform(-1, 1, 3), rot, W, H, 64, back_size=(back, back * H / W))
        p = int(rng.integers(W + 1, W * (H - 1) - 1))
        o = np.array(list(cam.position), np.float64)
        d, r, u = _basis(cam, p)
        pix = cam.back_size[0] / W / cam.back_distance
        return cam, o, d, r, u, pix

    # the shared edge of a coplanar pair through the pixel, at several offsets and slopes
    for off in (0.0, 0.2, -0.4):
        for slope in (0.0, 0.7):
            cam, o, d, r, u, pix = setup()
            D = 50.0
            c = o + D * d + off * pix * D * r
            a, b = c - 40 * (u + slope * r), c + 40 * (u + slope * r)
            made.append(("coplanar pair", cam, np.concatenate([_tri(a, b, c - 60 * r), _tri(b, a, c + 60 * r)])))
    # a T-junction: the long edge of one triangle against two triangles that meet in the pixel
    for off in (0.0, 0.3):
        cam, o, d, r, u, pix = setup()
        D = 40.0
        c = o + D * d + off * pix * D * u
        a, b = c - 50 * r, c + 50 * r
        made.append(("T-junction", cam, np.concatenate([_tri(a, b, c - 60 * u), _tri(a, c, c + 60 * u), _tri(c, b, c + 60 * u)])))
    # a silhouette over a back wall, the wall 2 ... 2000 units behind
    for gap in (2.0, 20.0, 2000.0):
        cam, o, d, r, u, pix = setup()
        D = 30.0
        c = o + D * d + 0.1 * pix * D * r
        wall = o + (D + gap) * d
        s = 10.0 * (D + gap)
        made.append(("silhouette", cam, np.concatenate([_tri(c - 40 * u, c + 40 * u, c - 60 * r),
                                                        _tri(wall - s * r - s * u, wall + 2 * s * r - s * u, wall - s * r + 2 * s * u)])))
    # a wall in a plane z = const whose triangles meet in an edge along y: the edge lies on a face of either triangle's own
    # box, so the rays next to it are inside the containment band and walk, the others are settled; coordinates of
    # magnitude 3, 1000 and 4096 (the band grows with them)
    for x0 in (0.0, 1000.0, -4096.0):
        for off in (0.0, 0.3):
            cam, o, d, r, u, pix = setup(origin=(x0 + 3.0, 2.0, 1.0))
            D = 25.0
            c = o + D * d
            x = c[0] + off * pix * D
            made.append(("wall edge on a box face", cam, np.concatenate([
                _tri((x, c[1] - 30, c[2]), (x + 40, c[1] - 30, c[2]), (x, c[1] + 50, c[2])),
                _tri((x - 40, c[1] - 30, c[2]), (x, c[1] - 30, c[2]), (x, c[1] + 50, c[2]))])))
    # two parallel planes closer than 2^-16 relative (1, 4, 64 floats apart at distance 60)
    for steps in (1, 4, 64):
        cam, o, d, r, u, pix = setup()
        c = o + 60.0 * d
        big = _tri(c - 25 * r - 25 * u, c + 50 * r - 25 * u, c - 25 * r + 50 * u).astype(np.float32)
        move = steps * np.sign(np.tile(d, 3)).reshape(1, 9) * np.sign(big)
        other = (big.view(np.int32) + move.astype(np.int32)).view(np.float32)
        shifted = other.astype(np.float64) + np.tile(0.3 * pix * 60.0 * r, 3).reshape(1, 9)  # ... and its edge through the pixel
        made.append(("close planes", cam, np.concatenate([big.astype(np.float64), other.astype(np.float64)])))
        made.append(("close planes, shifted", cam, np.concatenate([big.astype(np.float64), shifted])))
    # a sliver whose det changes sign inside the cone, in front of a covering pair
    for tilt in (0.0, 1e-8, 1e-6):
        cam, o, d, r, u, pix = setup()
        c = o + 90.0 * d
        back = np.concatenate([_tri(c - 40 * u, c + 40 * u, c - 60 * r), _tri(c + 40 * u, c - 40 * u, c + 60 * r)])
        n = r + tilt * d
        n /= np.linalg.norm(n)
        a = np.cross(n, u)
        e = o + 30.0 * d + 0.2 * pix * 30.0 * r
        made.append(("sliver", cam, np.concatenate([back, _tri(e - 10 * a, e + 10 * a, e + 8 * u)])))
    # slivers in a coordinate plane (fan_scene), seen through a narrow camera (a pixel is 0.01 units wide at the hit):
    # the old skip of the axis without extent settled rays of these with the sliver's t where the reference prunes its
    # leaf; widths 0.02 ... 0.5 of 141 units, every coordinate plane, coordinates of magnitude 3, 1000 and 4096
    for width, axis, x0 in ((0.1, 1, 0.0), (0.1, 1, 0.0), (0.1, 1, 0.0), (0.1, 1, 0.0), (0.02, 1, 0.0), (0.5, 1, 0.0),
                            (0.1, 0, 0.0), (0.1, 2, 0.0), (0.1, 1, 1000.0), (0.1, 1, -4096.0), (0.5, 2, 1000.0)):
        cam, o, d, r, u, pix = setup(origin=(x0 + 3.0, 2.0, 1.0), back=0.02)
        if abs(d[axis]) < 0.05:  # (a view along the plane: the next scene has another camera)
            continue
        made.append(("sliver fan in a coordinate plane", cam, fan_scene(o, d, 100.0, width, 141.0, axis)))
    # cones on a coordinate plane: an axis-aligned camera in front of an edge
    for yaw in (0.0, 90.0):
        cam, o, d, r, u, pix = setup(rot=(0.0, yaw, 0.0))
        c = o + 20.0 * d
        made.append(("cone on a coordinate plane", cam, np.concatenate([_tri(c - 40 * u, c + 40 * u, c - 60 * r), _tri(c + 40 * u, c - 40 * u, c + 60 * r)])))

    settled_by_kind = {}
    for i, (kind, cam, pos) in enumerate(made):
        pos = np.ascontiguousarray(pos, np.float32)
        e1, e2 = pos[:, 3:6] - pos[:, 0:3], pos[:, 6:9] - pos[:, 0:3]
        nr = np.cross(e1, e2)
        ln = np.linalg.norm(nr, axis=1, keepdims=True)
        nr = np.where(ln > 0, nr / np.maximum(ln, 1e-30), np.float32([0, 1, 0])).astype(np.float32)
        nrm = np.repeat(nr[:, None, :], 3, axis=1).reshape(-1, 9)
        osc = O.OracleScene(pos, nrm, None)
        tree = osc.bvh()
        bad, settled, rays, _, _, _, _ = check(osc, tree, pos, cam, seed=i)
        assert bad == 0, (i, kind, bad)
        s = settled_by_kind.setdefault(kind, [0, 0])
        s[0] += settled
        s[1] += rays
    for kind, (s, r) in settled_by_kind.items():
        print("%-28s settled %d of %d rays of list pixels" % (kind, s, r))
    # the kinds a list is made for do settle rays
    for kind in ("coplanar pair", "T-junction", "silhouette", "wall edge on a box face", "sliver fan in a coordinate plane"):
        assert settled_by_kind[kind][0] > 0, kind
    # the wall's edge lies on its triangles' box faces: the rays next to it are inside the containment band and walk
    assert settled_by_kind["wall edge on a box face"][0] < settled_by_kind["wall edge on a box face"][1]
    # two planes a few floats apart that both cover the pixel: every ray is a tie within 2^-16, none is settled
    assert settled_by_kind["close planes"][0] == 0 and settled_by_kind["close planes"][1] > 0
    # ... and the slivers' own rays walk: their t is not the slab distance
    assert settled_by_kind["sliver fan in a coordinate plane"][0] < settled_by_kind["sliver fan in a coordinate plane"][1]


def test_host_program_under_sanitizers():
    """the stand-alone program built with -fsanitize=address,undefined, on cornell8 32x24 with 8 samples per pixel"""
    import oracle_lib as O
    import vermilion_amd as va
    from vermilion_amd import scenes
    pos, nrm, uv = scenes.cornell8()
    c = scenes.cornell_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], 32, 24, 64)
    osc = O.OracleScene(pos, nrm, uv)
    tree = osc.bvh()
    bad, settled, _, _, _, _, _ = check(osc, tree, pos, cam, spp=8, sanitize=True)
    assert bad == 0 and settled > 0
