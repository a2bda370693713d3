"""vmx_kernels.hip: pixel_sphere_bound — k_shade<0>'s per-pixel answer to "below which nearest distance can sphere s
not matter to ANY camera ray of this pixel?" (CPU only).

The bound is restated here in numpy float32 exactly as the kernel computes it and checked against the reference's own
arithmetic (sphereIntersect, meshEngine.cpp:182-194: float dots, double discriminant): for every ray the kernels can
generate for the pixel and every limit <= lmax, the reference's result must be 0 or >= limit, so that cast_finish's
`th > 0 && th < nearest` is false and the sphere may be passed over for that ray."""
import numpy as np

from test_kernel_shortcuts import SPHERES, dot3, exact_and_shortcuts

f32 = np.float32
K_MARGIN_B = f32(2.0 ** -10)
K_INSIDE_REL = f32(2.0 ** -18)
K_SHRINK = f32(1.0) - f32(2.0 ** -13)
K_ROOT_REL = f32(2.0 ** -20)
INF = f32(np.inf)
REFERENCE_TABLE = SPHERES[:8]  # two lights, six walls (meshEngine.cpp's room)


def pixel_cone(M, sensor, film_dist, W, H, p):
    """PixelCone of the pixels p (array), float32 operation by operation as pixel_cone() in the kernels; M[row][col]"""
    fw, fh = f32(W), f32(H)
    hx = ((p % W).astype(f32) - f32(0.25)) / fw - f32(0.5)
    hy = ((p // W).astype(f32) - f32(0.25)) / fh - f32(0.5)
    gx, gy, gz = hx * f32(sensor[0]), -(hy * f32(sensor[1])), -f32(film_dist)
    M = M.astype(f32)
    a = np.stack([(M[r, 0] * gx + M[r, 1] * gy) + M[r, 2] * gz for r in range(3)], axis=1).astype(f32)
    alen = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    px_, py_ = f32(sensor[0]) / fw, f32(sensor[1]) / fh
    with np.errstate(divide="ignore", invalid="ignore"):
        sphi = np.minimum(f32(0.505) * np.sqrt(px_ * px_ + py_ * py_) / alen, f32(1))
    cphi = np.sqrt(np.maximum(f32(1) - sphi * sphi, f32(0)))
    assert a.dtype == f32 and alen.dtype == f32 and sphi.dtype == f32 and cphi.dtype == f32
    return a, alen, sphi, cphi


def pixel_sphere_bound(cone, pos, centre, radius):
    """lmax of every pixel of the cone for one sphere, as pixel_sphere_bound() in the kernels"""
    a, alen, sphi, cphi = cone
    op = (np.array(centre, dtype=f32) - np.array(pos, dtype=f32)).astype(f32)
    C = f32(f32(op[0] * op[0] + op[1] * op[1]) + op[2] * op[2])
    R2 = f32(f32(radius) * f32(radius))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ln = np.sqrt(C)
        norm = ln * alen
        ct = ((op[0] * a[:, 0] + op[1] * a[:, 1]) + op[2] * a[:, 2]) / norm
        kx = op[1] * a[:, 2] - a[:, 1] * op[2]
        ky = op[2] * a[:, 0] - a[:, 2] * op[0]
        kz = op[0] * a[:, 1] - a[:, 0] * op[1]
        st = np.sqrt((kx * kx + ky * ky) + kz * kz) / norm
        cone_ok = (alen > 0) & (sphi <= f32(0.5))
        m = np.where(ct >= cphi, f32(1), np.fmax(ct * cphi + st * sphi, f32(0)))
        clear = f32(1) - R2 / C
        never = cone_ok & (m * m * f32(1.0001) + f32(1e-3) < clear)
        cmin = np.where(ct <= -cphi, f32(-1), np.fmax(ct * cphi - st * sphi, f32(-1)))
        blo = ln * cmin - K_MARGIN_B * ln
        D = f32(R2 - C)
        inside = cone_ok & (D > K_INSIDE_REL * f32(C + R2))
        s = np.sqrt(blo * blo + D)
        T = np.where(blo < 0, D / (s - blo), blo + s) * K_SHRINK
        X = f32(C - R2)
        outside = cone_ok & (X > K_INSIDE_REL * f32(C + R2))
        bhi = np.fmax(ln * m + K_MARGIN_B * ln, np.sqrt(X))
        s_up = np.sqrt(np.fmax(bhi * bhi * (f32(1) + K_ROOT_REL) - X * (f32(1) - K_ROOT_REL), f32(0)))
        E = X / (bhi + s_up) * K_SHRINK
        lm = np.where(inside, T, E)
    assert lm.dtype == f32 and ct.dtype == f32 and st.dtype == f32 and E.dtype == f32
    return np.where(never, INF, np.where((inside | outside) & (lm > 0) & (lm < INF), lm, f32(0))).astype(f32)


def reference_hit(o, d, centre, radius):
    """sphereIntersect of the reference for the rays (o, d): its float result, 0 for "no hit" """
    return exact_and_shortcuts(o, d, centre, radius, np.full(o.shape[0], np.inf, f32))[0]


def footprint_directions(M, pos, sensor, film_dist, W, H, q):
    """corners and edge midpoints (and the centre) of the sample footprint of the pixels q: offsets [-0.75, 0.25]"""
    out = []
    for ex in (-0.75, -0.25, 0.25):
        for ey in (-0.75, -0.25, 0.25):
            hx = ((q % W) + ex) / W - 0.5
            hy = ((q // W) + ey) / H - 0.5
            g = np.stack([hx * sensor[0], -hy * sensor[1], np.full(q.shape, -film_dist)], axis=1)
            dd = g @ M.astype(np.float64).T
            dd /= np.linalg.norm(dd, axis=1, keepdims=True)
            out.append(dd.astype(f32))
    return out


def violations_of(lmax, o, dirs, centre, radius, rng):
    """number of (ray, limit) cases with limit <= lmax whose reference result lies in (0, limit)"""
    bad = 0
    n = lmax.shape[0]
    for d in dirs:
        th = reference_hit(o, d, centre, radius)
        delta = np.exp(rng.uniform(np.log(1e-8), np.log(1e-1), n))
        base = np.where(np.isfinite(lmax) & (lmax > 0), lmax, f32(1000))
        root = np.where(th > 0, th, f32(1000))
        limits = [lmax, (base * (1 - delta)).astype(f32), (base * (1 + delta)).astype(f32), (root * (1 - delta)).astype(f32),
                  (root * (1 + delta)).astype(f32), np.full(n, np.inf, f32)]
        for lim in limits:
            bad += int(np.sum((lim <= lmax) & (th > 0) & (th < lim)))
    return bad


def test_pixel_sphere_bound_is_conservative():
    import oracle_lib as O
    import vermilion_amd as va
    from vermilion_amd import scenes
    rng = np.random.default_rng(12)
    pairs = claims = none = bad = 0
    cams = []
    for trial in range(40):
        W, H = int(rng.choice([33, 64, 160])), int(rng.choice([17, 40, 90]))
        pos = rng.uniform(-1500, 1500, 3) * np.array([1.0, 0.3, 1.0]) + np.array([0.0, 500.0, 0.0])  # inside the room
        rot = rng.uniform(-180, 180, 3) * np.array([0.4, 1.0, 0.2])
        cams.append((pos, va.make_camera(pos, rot, W, H, 64, back_size=(3.6, 3.6 * H / W)), trial))
    for camf, (W, H) in ((scenes.sponza_camera, (160, 90)), (scenes.cornell_camera, (96, 64))):
        c = camf()
        cams.append((np.array(c["position"], dtype=np.float64), va.make_camera(c["position"], c["rotation_deg"], W, H, 64), 100))
    for pos, cam, seed in cams:
        W, H = cam.image_res[0], cam.image_res[1]
        sensor, film = (cam.back_size[0], cam.back_size[1]), cam.back_distance
        M = O.camera_matrix(cam).T  # [row][col]
        rays = [O.primary_rays(cam, va.make_opts(seed=seed), k) for k in (0, 9, 17, 25, 33, 41, 50, 63)]
        d0 = rays[0][1]
        table = [(c, r, None) for c, r in REFERENCE_TABLE]
        for _ in range(16):
            p = int(rng.integers(0, W * H))
            axis = d0[p].astype(np.float64)
            kind = rng.integers(0, 4)
            if kind == 0:    # camera outside, the pixel's cone grazes the sphere: a small one nearby, or the horizon of a large one
                if rng.integers(0, 2):
                    dist = np.exp(rng.uniform(np.log(5), np.log(5000)))
                    rad = dist * np.exp(rng.uniform(np.log(1e-3), np.log(0.5)))
                else:
                    rad = np.exp(rng.uniform(np.log(10), np.log(5e7)))
                    dist = rad + np.exp(rng.uniform(np.log(1e-3), np.log(1e4)))
                t = np.cross(axis, rng.normal(size=3))
                t /= np.linalg.norm(t)
                # the tangent direction +- a few degrees, or +- a few pixels
                off = rng.uniform(-0.05, 0.08) if rng.integers(0, 2) else rng.uniform(-4, 4) * cam.back_size[0] / W / cam.back_distance
                ang = np.arcsin(min(rad / dist, 1.0)) + off
                centre = pos + dist * (np.cos(ang) * axis + np.sin(ang) * t)
            else:            # camera 1e-3 ... 1e4 units inside (kind 1, 2) or outside (kind 3) the surface, any direction
                rad = np.exp(rng.uniform(np.log(10), np.log(5e7)))
                depth = np.exp(rng.uniform(np.log(1e-3), np.log(min(1e4, 0.9 * rad))))
                u = rng.normal(size=3) if rng.integers(0, 2) else axis * rng.choice([-1, 1]) + 0.01 * rng.normal(size=3)
                u /= np.linalg.norm(u)
                centre = pos + (rad - depth if kind != 3 else rad + depth) * u
            table.append((tuple(centre), rad, p))
        for centre, rad, p in table:
            q = rng.integers(0, W * H, 48)
            if p is not None:
                q = np.concatenate([q, np.clip(np.array([p, p - 1, p + 1, p - W, p + W]), 0, W * H - 1)])
            q = np.unique(q)
            lmax = pixel_sphere_bound(pixel_cone(M, sensor, film, W, H, q), pos, centre, rad)
            assert not np.any(np.isnan(lmax))
            pairs += q.size
            claims += int(np.sum(lmax > 0))
            none += int(np.sum(lmax == 0))
            o = np.repeat(np.float32(pos)[None, :], q.size, axis=0)
            dirs = [d[q] for _, d in rays] + footprint_directions(M, np.float32(pos), sensor, film, W, H, q)
            bad += violations_of(lmax, o, dirs, centre, rad, rng)
    print("pairs %d, with a claim %d (%.1f %%), without %d (%.1f %%)" % (pairs, claims, 100.0 * claims / pairs, none, 100.0 * none / pairs))
    assert bad == 0
    assert claims >= pairs / 5 and none >= pairs / 20  # both answers are exercised


def test_bench_camera_claims_the_wall_spheres():
    """what the speed-up rests on: on the bench camera with the reference's table, the share of pixels that have a claim
    for all six wall spheres (printed, not asserted), at the test size and at the bench's 1920x1080; and no sphere of
    the table gets a NaN"""
    import oracle_lib as O
    import vermilion_amd as va
    from vermilion_amd import scenes
    c = scenes.sponza_camera()
    for W, H in ((160, 90), (1920, 1080)):
        cam = va.make_camera(c["position"], c["rotation_deg"], W, H, 256, back_size=(3.6, 3.6 * H / W))
        M = O.camera_matrix(cam).T
        cone = pixel_cone(M, (cam.back_size[0], cam.back_size[1]), cam.back_distance, W, H, np.arange(W * H))
        rows = np.stack([pixel_sphere_bound(cone, c["position"], centre, rad) for centre, rad in REFERENCE_TABLE], axis=1)
        assert not np.any(np.isnan(rows))
        walls = np.all(rows[:, 2:] > 0, axis=1)
        lights = np.all(np.isinf(rows[:, :2]), axis=1)
        print("%dx%d: claim for all six wall spheres %.2f %% of pixels, both lights never matter %.2f %%, smallest wall bound "
              "%.1f ... %.1f units" % (W, H, 100.0 * walls.mean(), 100.0 * lights.mean(), rows[:, 2:].min(axis=1).min(),
                                       rows[:, 2:].min(axis=1).max()))
