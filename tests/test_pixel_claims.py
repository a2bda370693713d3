"""vermilion_amd/csrc/pixel_claim.h: the per-pixel claim "every camera ray of this pixel hits triangle T" / "hits
nothing" that lets k_trace_w<0> replace a camera ray's BVH walk by one triangle test (CPU only).

The header's procedure runs in the stand-alone host program tests/cpp/pixel_claim_test.cpp over the exported flat tree;
the oracle then traces the pixel's samples (O.primary_rays) and the nine points of its sample footprint, and every
ray of a pixel with a slot claim must return that triangle, every ray of a MISS pixel nothing.  The share of claimed
pixels must be at least half of what the oracle itself finds (pixels whose samples all return one id, or all miss):
a procedure that claims nothing is conservative and useless."""
import os

import numpy as np
import pytest

import pixel_claim_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))


def shares(cl):
    flat = cl.reshape(-1)
    return float(np.mean(flat < S.MISS)), float(np.mean(flat == S.MISS)), float(np.mean(flat == S.NONE))


@pytest.mark.parametrize("name,size", [("cornell8", (96, 64)), ("bunny70k", (160, 90)), ("sponza260k", (160, 90)),
                                       ("lattice", (96, 64))])
def test_claims_hold_for_every_sample(name, size):
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
    cl = S.host_claims(pos, tree, [cam])[0]
    slot, miss, none = shares(cl)
    bad_slot, bad_miss, one, allmiss = S.oracle_verdict(osc, tree, cam, cl, spp=64)
    print("%s %dx%d: slot claims %.1f %% (oracle: one triangle %.1f %%), MISS %.1f %% (oracle: all miss %.1f %%), none %.1f %%"
          % (name, W, H, 100 * slot, 100 * one, 100 * miss, 100 * allmiss, 100 * none))
    assert bad_slot == 0 and bad_miss == 0
    assert slot + miss >= 0.5 * (one + allmiss)
    assert none > 0


def test_duplicated_triangles_are_never_claimed():
    """tests/golden/ref_soup_duplicates.npz: every triangle several times, every hit a tie that the reference resolves
    by test order — no pixel a duplicated pair covers may carry a slot claim"""
    import oracle_lib as O
    import vermilion_amd as va
    g = np.load(os.path.join(HERE, "golden", "ref_soup_duplicates.npz"))
    pos, nrm = g["pos"].reshape(-1, 9), g["nrm"].reshape(-1, 9)
    tree = {k: g["bvh_" + k] for k in ("start", "nprims", "right_offset", "bbox", "prim_order")}
    cpos, crot = g["cam"][:3], g["cam"][3:6]
    _, inverse, counts = np.unique(pos, axis=0, return_inverse=True, return_counts=True)
    dup = counts[inverse.reshape(-1)] > 1
    assert dup.sum() > 100
    osc = O.OracleScene(pos, nrm, None, tree=tree)
    total = np.zeros(3)
    for W, H in ((96, 64), (33, 17)):
        cam = va.make_camera(cpos, crot, W, H, 64)
        cl = S.host_claims(pos, tree, [cam])[0]
        flat = cl.reshape(-1)
        ids = tree["prim_order"][flat[flat < S.MISS]]
        assert not np.any(dup[ids])
        bad_slot, bad_miss, one, allmiss = S.oracle_verdict(osc, tree, cam, cl, spp=64)
        assert bad_slot == 0 and bad_miss == 0
        total += shares(cl)
    print("soup: slot %.1f %%, MISS %.1f %%, none %.1f %% (mean of two sizes)" % tuple(50 * total))
    assert total[1] > 0 and total[2] > 0


def test_random_cameras_inside_sponza():
    """forty cameras in the Sponza stand-in, 33x17 ... 160x90: random rotations, axis-aligned ones (a cone on a
    coordinate plane gives no claim) and cameras 1e-3 ... 10 units from the floor or a wall; all 64 samples and the
    nine footprint points of every claimed pixel"""
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
    tables = S.host_claims(pos, tree, cams)
    bad = 0
    tot = np.zeros(3)
    axis_none = []
    for i, (cam, cl) in enumerate(zip(cams, tables)):
        bs, bm, _, _ = S.oracle_verdict(osc, tree, cam, cl, spp=64, seed=i, only_claimed=True)
        bad += bs + bm
        tot += shares(cl)
        if i % 4 == 1:
            # the pixel column and the pixel row whose cones contain a coordinate plane: no claim
            axis_none.append(np.any(np.all(cl == S.NONE, axis=0)) and np.any(np.all(cl == S.NONE, axis=1)))
    print("40 cameras: slot %.1f %%, MISS %.1f %%, none %.1f %%" % tuple(100 * tot / len(cams)))
    assert bad == 0
    assert tot[0] > 0 and tot[2] > 0
    assert all(axis_none)


def _basis(cam, p):
    """centre direction of pixel p's footprint and two unit vectors across it (camera right and up), float64"""
    import oracle_lib as O
    d = S.footprint_directions(cam, np.array([p]))[4][0].astype(np.float64)
    M = O.camera_matrix(cam).T.astype(np.float64)
    right, up = M[:, 0], M[:, 1]
    right = right - d * (right @ d)
    right /= np.linalg.norm(right)
    up = np.cross(d, right)
    return d, right, up


def _tri(*v):
    return np.array(v, np.float64).reshape(1, 9)


def test_adversarial_single_pixel_scenes():
    """scenes of a few triangles built around one pixel of a 33x17 frame, every pixel of the frame checked with all 64
    samples and the footprint points"""
    import oracle_lib as O
    import vermilion_amd as va
    W, H = 33, 17
    rng = np.random.default_rng(5)
    scenes_ = []

    def camera(origin=(3.0, 2.0, 1.0)):
        rot = rng.uniform(-180, 180, 3) * np.array([0.3, 1.0, 0.1])
        return va.make_camera(np.array(origin) + rng.uniform(-1, 1, 3), rot, W, H, 64, back_size=(3.6, 3.6 * H / W))

    def setup(origin=(3.0, 2.0, 1.0)):
        cam = camera(origin)
        p = int(rng.integers(W + 1, W * (H - 1) - 1))
        o = np.array(list(cam.position), np.float64)
        d, r, u = _basis(cam, p)
        pix = cam.back_size[0] / W / cam.back_distance  # angular size of a pixel at the image centre (about, elsewhere)
        return cam, o, d, r, u, pix

    def cover(o, d, r, u, D, size):  # a triangle across the whole view of the pixel at distance D
        c = o + D * d
        return _tri(c - size * r - size * u, c + 2 * size * r - size * u, c - size * r + 2 * size * u)

    # a triangle edge +-0.01 ... +-2 pixels from the footprint's boundary
    for off in (0.01, 0.1, 0.5, 1.0, 2.0):
        for sign in (-1.0, 1.0):
            cam, o, d, r, u, pix = setup()
            D = 50.0
            e = (0.5 + sign * off) * pix * D  # the edge's distance from the footprint centre along r
            c = o + D * d
            scenes_.append((cam, _tri(c + e * r - 40 * u, c + e * r + 40 * u, c - 60 * r)))
    # an occluder a tenth of a pixel wide in front of a covering triangle
    for place in (0.0, 0.3, -0.45):
        cam, o, d, r, u, pix = setup()
        big = cover(o, d, r, u, 80.0, 30.0)
        c = o + 20.0 * d + place * pix * 20.0 * r
        w = 0.05 * pix * 20.0
        scenes_.append((cam, np.concatenate([big, _tri(c - w * r - 5 * u, c + w * r - 5 * u, c + 5 * u)])))
    # a second triangle nextafter distances behind and in front of T
    for steps in (1, 2, 16, 1024, 1 << 16):
        for sign in (-1, 1):
            cam, o, d, r, u, pix = setup()
            big = cover(o, d, r, u, 60.0, 25.0).astype(np.float32)
            # every coordinate `steps` floats along (sign = 1) or against the view direction
            move = sign * steps * np.sign(np.tile(d, 3)).reshape(1, 9) * np.sign(big)
            other = (big.view(np.int32) + move.astype(np.int32)).view(np.float32)
            scenes_.append((cam, np.concatenate([big, other]).astype(np.float64)))
    # an edge-on triangle (|det| from 1e-9 to 1e-5 of |e1||e2|) crossing the cone, in front of a covering triangle
    for tilt in (1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 0.0):
        cam, o, d, r, u, pix = setup()
        big = cover(o, d, r, u, 90.0, 40.0)
        n = r + tilt * d  # the plane through the camera's ray, tilted by `tilt`
        n /= np.linalg.norm(n)
        a = np.cross(n, u)
        c = o + 30.0 * d + 0.2 * pix * 30.0 * r
        scenes_.append((cam, np.concatenate([big, _tri(c - 10 * a, c + 10 * a, c + 8 * u)])))
    # vertex coordinates of magnitude 1e4 with millimetre extents
    for D in (0.02, 0.1, 1.0):
        cam, o, d, r, u, pix = setup(origin=(1e4, -1e4, 1e4))
        c = o + D * d
        s = 1e-3
        tris = [_tri(c + i * s * r + j * s * u, c + (i + 1) * s * r + j * s * u, c + i * s * r + (j + 1) * s * u)
                for i in range(-3, 3) for j in range(-3, 3)]
        scenes_.append((cam, np.concatenate(tris)))

    bad = 0
    tot = np.zeros(3)
    for i, (cam, pos) in enumerate(scenes_):
        pos = np.ascontiguousarray(pos, np.float32)
        e1, e2 = pos[:, 3:6] - pos[:, 0:3], pos[:, 6:9] - pos[:, 0:3]
        nr = np.cross(e1, e2)
        ln = np.linalg.norm(nr, axis=1, keepdims=True)
        nr = np.where(ln > 0, nr / np.maximum(ln, 1e-30), np.float32([0, 1, 0])).astype(np.float32)
        nrm = np.repeat(nr[:, None, :], 3, axis=1).reshape(-1, 9)
        osc = O.OracleScene(pos, nrm, None)
        tree = osc.bvh()
        cl = S.host_claims(pos, tree, [cam])[0]
        bs, bm, _, _ = S.oracle_verdict(osc, tree, cam, cl, spp=64, seed=i)
        assert bs == 0 and bm == 0, (i, bs, bm)
        bad += bs + bm
        tot += shares(cl)
    print("%d adversarial scenes: slot %.1f %%, MISS %.1f %%, none %.1f %%" % ((len(scenes_),) + tuple(100 * tot / len(scenes_))))
    assert bad == 0
    assert tot[0] > 0 and tot[1] > 0 and tot[2] > 0
