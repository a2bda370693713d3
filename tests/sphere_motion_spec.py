"""Motion records of pixels on a moved analytic sphere (include/vermilion_hip.h, vmx_motion_spheres_device) restated in
numpy: what k_motion_spheres (vermilion_amd/csrc/vmx_motion_spheres.inc) is held to, bit for bit.  A helper, not a test.

Every array and every scalar is float32, so each written operation rounds once to float32, in the order written; the
discriminant and the roots of sphereIntersect are float64, as in the reference (meshEngine.cpp:182-194)."""
import ctypes as C

import numpy as np

from motion_spec import MOVED, words_of

F = np.float32
D = np.float64


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def table_of(spheres):
    """dict of float32 arrays (centre [n, 3], radius [n], normal_centre [n, 3], sign [n]) of a ctypes array of vmx_sphere
    (or any sequence of them); sign as scene creation reads normal_sign"""
    n = len(spheres)
    t = dict(centre=np.zeros((n, 3), F), radius=np.zeros(n, F), normal_centre=np.zeros((n, 3), F), sign=np.ones(n, F))
    for i, s in enumerate(spheres):
        t["centre"][i] = list(s.centre)
        t["radius"][i] = s.radius
        t["normal_centre"][i] = list(s.normal_centre)
        t["sign"][i] = F(-1) if s.normal_sign < 0 else F(1)
    return t


def moved_of(now, prev):
    """[n] bool: centre, radius or normal_centre differ bitwise, or the sign differs"""
    u = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
    return ((u(now["centre"]) != u(prev["centre"])).any(axis=-1) | (u(now["radius"]) != u(prev["radius"]))
            | (u(now["normal_centre"]) != u(prev["normal_centre"])).any(axis=-1) | (now["sign"] != prev["sign"]))


def sphere_hit(O, d, c, r):
    """sphereIntersect: float32 dots and rad*rad, float64 discriminant and roots; 0 where there is no root > 1e-4.
    O [3], d [..., 3], c [3], r scalar, all float32"""
    op = (c - O).astype(F)
    B = _dot(op, d)
    Cc = _dot(op, op)
    R2 = F(r) * F(r)
    assert B.dtype == np.float32 and np.asarray(Cc).dtype == np.float32 and R2.dtype == np.float32
    b = B.astype(D)
    det = (b * b - D(Cc)) + D(R2)
    q = np.sqrt(np.where(det < 0, D(0), det))
    t0, t1 = b - q, b + q
    th = np.where(t0 > 1e-4, t0.astype(F), np.where(t1 > 1e-4, t1.astype(F), F(0)))
    return np.where(det < 0, F(0), th).astype(F)  # (a NaN det is not < 0: its roots are NaN and fail both tests)


def choose(P, O, now):
    """[...] int: the sphere MeshEngine::RayCast leaves as the hit for the ray from O through P, or -1"""
    O = np.asarray(O, F)
    with np.errstate(all="ignore"):
        d = P - O
        s = F(1) / np.sqrt(_dot(d, d))
        d = d * s[..., None]
    assert d.dtype == np.float32
    fin = np.isfinite(d).all(axis=-1)
    nearest = np.full(P.shape[:-1], np.inf, F)
    which = np.full(P.shape[:-1], -1, np.int64)
    for i in range(len(now["radius"])):
        th = sphere_hit(O, d, now["centre"][i], now["radius"][i])
        acc = fin & (th > 0) & (th < nearest)
        nearest = np.where(acc, th, nearest)
        which = np.where(acc, i, which)
    return which


def sphere_records(rec):
    """[...] bool: the record is a hit that does not lie on its triangle"""
    w = words_of(rec)
    f = w.view(np.float32)
    tid = w[..., 7].view(np.int32)
    with np.errstate(all="ignore"):
        return ((w[..., 11] & 1) != 0) & ~((tid >= 0) & (f[..., 3] == f[..., 10]))


def motion(rec, origin, spheres_now, spheres_prev, motion_in=None):
    """vmx_motion_spheres_device: [..., 8] float32 words (prev_location, flags, prev_normal, pad) of the records rec [...];
    spheres_now / spheres_prev: sequences of vmx_sphere of one length; motion_in: [..., 8] words or None"""
    w = words_of(rec)
    f = w.view(np.float32)
    now, prev = table_of(spheres_now), table_of(spheres_prev)
    assert len(now["radius"]) == len(prev["radius"]) <= 16
    if motion_in is None:
        out = np.zeros(w.shape[:-1] + (8,), np.uint32)
        out[..., 0:3], out[..., 4:7] = w[..., 0:3], w[..., 4:7]
    else:
        out = np.array(np.ascontiguousarray(motion_in).view(np.uint32))
        assert out.shape == w.shape[:-1] + (8,)
    if len(now["radius"]) == 0:
        return out.view(np.float32)
    P = np.array(f[..., 0:3])
    with np.errstate(all="ignore"):
        sphere = sphere_records(rec)
        which = choose(P, origin, now)
        found = which >= 0
        i = np.where(found, which, 0)
        moved = found & moved_of(now, prev)[i]
        k = prev["radius"][i] / now["radius"][i]
        Xh = prev["centre"][i] + (P - now["centre"][i]) * k[..., None]
        m = Xh - prev["normal_centre"][i]
        s = F(1) / np.sqrt(_dot(m, m))
        nh = (m * s[..., None]) * prev["sign"][i][..., None]
        assert Xh.dtype == np.float32 and nh.dtype == np.float32 and k.dtype == np.float32
        nfin = np.isfinite(nh).all(axis=-1)
        nh = np.where(nfin[..., None], nh.view(np.uint32), w[..., 4:7])
        valid = sphere & moved & np.isfinite(Xh).all(axis=-1)
    out[..., 0:3] = np.where(valid[..., None], Xh.view(np.uint32), out[..., 0:3])
    out[..., 3] = np.where(valid, MOVED, out[..., 3])
    out[..., 4:7] = np.where(valid[..., None], nh, out[..., 4:7])
    out[..., 7] = np.where(valid, np.uint32(0), out[..., 7])
    return out.view(np.float32)


# ---- tables and synthetic records for the tests of motion() and k_motion_spheres ----------------------------------------
def copy_table(spheres, n=None):
    """a fresh ctypes array of the first n entries of `spheres`"""
    n = len(spheres) if n is None else n
    out = (type(spheres[0]) * n)() if n else None
    for i in range(n):
        C.memmove(C.byref(out[i]), C.byref(spheres[i]), C.sizeof(spheres[i]))
    return out


ORIGIN = (50.0, 300.0, 600.0)  # the common ray origin of the synthetic records: a point inside the reference's room


def ray_towards(O, aim):
    """float32 unit direction from O to aim (normalised in float64, rounded once)"""
    d = np.asarray(aim, D) - np.asarray(O, D)
    return (d / np.linalg.norm(d)).astype(F)


def hit_point(O, d, c, r):
    """(location, distance) as RayCast leaves them for the ray (O, d) on the sphere (c, r): o + d * (float)t; distance 0:
    no hit"""
    O = np.asarray(O, F)
    th = sphere_hit(O, d[None, :], np.asarray(c, F), F(r))[0]
    return (O + d * th).astype(F), th


def moved_tables(base, nspheres, origin=ORIGIN):
    """(now, prev): ctypes arrays of `nspheres` entries.  `base` is the reference's eight (default_spheres()); further
    entries are small spheres strung out inside the room.  Between prev and now: sphere 0 (the small light) is translated
    and resized, sphere 1 (the big light, brought into the room at (-900, 700, 200) with radius 60 in both tables) only
    dimmed (not moved), sphere 2 (the floor, radius 5e7) lowered by 8.  With
    more entries: sphere 8 sits at origin + (256, 0, 0) and has radius 0 now (the ray through its centre has det == 0
    exactly and is accepted: r_now == 0); sphere 9 keeps centre and radius, and prev's normal_centre is exactly the x_prev of
    the record the ray towards its centre leaves (normal_centre == x_prev: no finite previous normal); sphere 10 only flips
    its sign."""
    S = type(base[0])
    O = np.asarray(origin, F)
    now = (S * nspheres)()
    for i in range(nspheres):
        if i < len(base):
            C.memmove(C.byref(now[i]), C.byref(base[i]), C.sizeof(S))
        else:
            now[i].centre[:] = [-600.0 + 150.0 * (i - 8), 300.0 + 40.0 * (i % 3), -400.0 + 90.0 * (i - 8)]
            now[i].radius = 30.0 + 5.0 * (i - 8)
            now[i].colour[:] = [1.0, 2.0, 3.0]
            now[i].flags = i & 1
            now[i].normal_centre[:] = list(now[i].centre)
            now[i].normal_sign = 1.0
    if nspheres > 1:  # (the reference's big light hangs outside the room, behind the ceiling: here it is in sight)
        now[1].centre[:] = [-900.0, 700.0, 200.0]
        now[1].radius = 60.0
    if nspheres > 8:
        now[8].centre[:] = [float(O[0]) + 256.0, float(O[1]), float(O[2])]
        now[8].normal_centre[:] = list(now[8].centre)
    prev = (S * nspheres)()
    if nspheres:
        C.memmove(prev, now, C.sizeof(now))
    if nspheres > 0:
        prev[0].centre[:] = [now[0].centre[0] - 12.0, now[0].centre[1] + 5.0, now[0].centre[2] + 7.0]
        prev[0].radius = now[0].radius * 1.5
    if nspheres > 1:
        prev[1].colour[:] = [c * 4.0 for c in now[1].colour]
    if nspheres > 2:
        prev[2].centre[1] = now[2].centre[1] + 8.0
        prev[2].normal_centre[1] = now[2].normal_centre[1] + 8.0
    if nspheres > 8:
        now[8].radius = 0.0
    if nspheres > 9:
        c = np.array(list(now[9].centre), F)
        P, th = hit_point(O, ray_towards(O, c), c, now[9].radius)
        assert th > 0
        k = F(prev[9].radius) / F(now[9].radius)
        prev[9].normal_centre[:] = [float(v) for v in c + (P - c) * k]
    if nspheres > 10:
        prev[10].normal_sign = -1.0
    return now, prev


# ---- the moving emitter of the history test and of the device test on a real G-buffer -----------------------------------
# radius 120 above the block of scenes.cornell8(), moving +25 x, +40 z a frame (towards the camera: a sphere that only
# slid sideways would pass the accumulation's plane test at its middle even without motion records); its normals are its own
EMITTER0, EMITTER_STEP, EMITTER_R = (-300.0, 650.0, 100.0), (25.0, 0.0, 40.0), 120.0


def emitter_table(base, i):
    """`base` (default_spheres()) with sphere 0 replaced by the emitter of frame i"""
    t = copy_table(base)
    c = [EMITTER0[k] + EMITTER_STEP[k] * i for k in range(3)]
    t[0].centre[:] = c
    t[0].normal_centre[:] = c
    t[0].normal_sign = 1.0
    t[0].radius = EMITTER_R
    t[0].colour[:] = [6.0, 4.5, 3.0]
    return t


KINDS = ("miss", "triangle", "unmoved_sphere", "unmoved_small", "moved_emitter", "wall", "sphere_nearer", "at_origin", "nan_location",
         "inf_location", "zero_radius", "normal_centre", "flipped_sign")


def synthetic_records(n, spheres_now, origin, seed):
    """(rec [n, 16] float32 words, kind [n] of str): records of every kind motion() tells apart, in turn, for the tables
    of moved_tables().  Locations on a sphere are made as RayCast makes them: a ray from `origin`, the float64
    intersection, location = o + d * (float)t.  Kinds whose sphere the table does not have fall back to a miss."""
    rng = np.random.RandomState(seed)
    now = table_of(spheres_now) if spheres_now is not None else table_of([])
    ns = len(now["radius"])
    O = np.asarray(origin, F)
    kind = np.array([KINDS[i % len(KINDS)] for i in range(n)])
    target = {"unmoved_sphere": 1, "unmoved_small": 11, "moved_emitter": 0, "wall": 2, "sphere_nearer": 0, "zero_radius": 8, "normal_centre": 9,
              "flipped_sign": 10}
    rec = np.zeros((n, 16), np.float32)
    words = rec.view(np.uint32)
    rec[:, 0:3] = rng.uniform(-500, 500, (n, 3))
    rec[:, 3] = rec[:, 10] = rng.uniform(1, 100, n).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    rec[:, 4:7] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    rec[:, 8:10] = rng.uniform(0, 1, (n, 2))
    rec[:, 12:15] = rng.uniform(0, 1, (n, 3))
    words[:, 7] = np.int32(-1).view(np.uint32)
    words[:, 11] = 3
    for j in range(n):
        k = kind[j]
        if k in target and target[k] < ns:
            i = target[k]
            c, r = now["centre"][i].astype(D), D(now["radius"][i])
            if k in ("zero_radius", "normal_centre"):
                aim = c  # (the one ray moved_tables() made these two spheres for)
            elif r > 1e6:  # a wall, from inside: towards its centre, so that it is the nearest of the six
                aim = O.astype(D) + (c - O) / np.linalg.norm(c - O) * 100.0 + rng.normal(size=3) * 30.0
            else:
                v = rng.normal(size=3)
                aim = c + v / np.linalg.norm(v) * r * rng.uniform(0.0, 0.9)
            d = ray_towards(O, aim)
            P, th = hit_point(O, d, now["centre"][i], now["radius"][i])
            rec[j, 10] = F(999999999.0)
            if th > 0:
                rec[j, 0:3] = P
                rec[j, 3] = th
            else:
                rec[j, 0:3] = aim.astype(F)  # (a sphere record no sphere accepts)
            if k == "sphere_nearer":
                words[j, 7] = 5
                rec[j, 10] = rec[j, 3] * F(2)
        elif k == "triangle":
            words[j, 7] = j % 7
        elif k == "at_origin":
            rec[j, 0:3] = O
            rec[j, 10] = F(999999999.0)
        elif k == "nan_location":
            rec[j, 0] = np.nan
            rec[j, 10] = F(999999999.0)
        elif k == "inf_location":
            rec[j, 1] = np.inf
            rec[j, 10] = F(999999999.0)
        else:
            words[j, 11] = 2
            rec[j, 3] = np.inf
            rec[j, 10] = F(999999999.0)
            kind[j] = "miss"
    rec.setflags(write=False)
    return rec, kind
