"""Shared by test_guide_cull.py (CPU) and test_gpu_guide_cull.py (the device's walk, ray by ray): the stand-alone host
program tests/cpp/guide_cull_test.cpp — the guide walk of vermilion_amd/csrc/guide_walk.h with and without the skip of
boxes that end behind the ray's origin, premise (B) there — and one seeded generator of the rays that premise is about:
origins a little PAST a triangle along the ray, so that the triangle and its boxes lie behind the origin, where the float
triangle test of an ill-conditioned record has no reliable sign.  The oracle judges what either walk settles."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

import guide_spec as G

ROOT = G.ROOT
_exe = {}


def host_program(sanitize=False):
    if sanitize not in _exe:
        if shutil.which("g++") is None:
            import pytest
            pytest.skip("no g++")
        d = tempfile.mkdtemp(prefix="guide_cull_")
        exe = os.path.join(d, "guide_cull_test")
        csrc = os.path.join(ROOT, "vermilion_amd", "csrc")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + flags + ["-I", csrc,
                        os.path.join(ROOT, "tests", "cpp", "guide_cull_test.cpp"), os.path.join(csrc, "bvh_build.cpp"),
                        "-o", exe], check=True)
        _exe[sanitize] = exe
    return _exe[sanitize]


def host_cull(pos, tree, o, d, limits=(), sanitize=False):
    """The rays (o, d) over the guide of the triangles pos beside the reference tree `tree`, walked once without any skip
    (set 0) and once per limit (a number, or "inf": every child box may be skipped — the plain cull); no limits: once with
    the library's own marks.  Returns a list of dicts, one per set: verdict, slot, t, inner, tris per ray, and flagged
    (triangles beyond the limit), unmarked (child boxes that may not be skipped), children, and shape_max: kGwShapeMax as the
    program was compiled with it (guide_walk.h; run without limits it also checks make_guide_records' marks against it)."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    rays = np.ascontiguousarray(np.concatenate([np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d, np.float32).reshape(-1, 3)], axis=1))
    n = rays.shape[0]
    tmp = tempfile.mkdtemp(prefix="guide_cull_io_")
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    try:
        with open(fin, "wb") as f:
            f.write(np.array([pos.shape[0], len(tree["start"]), n], np.uint32).tobytes())
            f.write(pos.tobytes())
            for k in ("start", "nprims", "right_offset"):
                f.write(np.ascontiguousarray(tree[k], np.uint32).tobytes())
            f.write(np.ascontiguousarray(tree["bbox"], np.float32).tobytes())
            f.write(np.ascontiguousarray(tree["prim_order"], np.uint32).tobytes())
            f.write(rays.tobytes())
        subprocess.run([host_program(sanitize), fin, fout] + [str(x) for x in limits], check=True)
        raw = np.fromfile(fout, np.uint32)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    nsets = int(raw[0])
    assert nsets == (len(limits) + 1 if limits else 2)
    shape_max = float(raw[1:3].view(np.float64)[0])
    counts = raw[3:3 + 3 * nsets].reshape(nsets, 3)
    rec = raw[3 + 3 * nsets:].reshape(n, nsets, 5)
    return [{"verdict": rec[:, s, 0].copy(), "slot": rec[:, s, 1].copy(), "t": rec[:, s, 2].copy().view(np.float32),
             "inner": rec[:, s, 3].copy(), "tris": rec[:, s, 4].copy(), "flagged": int(counts[s, 0]),
             "unmarked": int(counts[s, 1]), "children": int(counts[s, 2]), "shape_max": shape_max} for s in range(nsets)]


def wrong(tri, rt, tree, res):
    """rays the rule settled wrongly given the oracle's (tri, t) of every ray (G.verdict with the trace hoisted out)"""
    hit, miss = res["verdict"] == G.SETTLED, res["verdict"] == G.MISS
    order = np.asarray(tree["prim_order"])
    want = order[np.minimum(res["slot"], len(order) - 1)].astype(np.int64)
    bad = hit & ((tri != want) | (rt.view(np.uint32) != res["t"].view(np.uint32)))
    bad |= miss & (tri >= 0)
    return bad


def shape(pos):
    """gw_shape of every triangle's record edges: |e1| |e2| / |e1 x e2| from the float edges, in double"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    e1 = (pos[:, 3:6] - pos[:, 0:3]).astype(np.float64)
    e2 = (pos[:, 6:9] - pos[:, 0:3]).astype(np.float64)
    c = np.linalg.norm(np.cross(e1, e2), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(c > 0, np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) / c, np.inf)


def min_pad(pos):
    """the smallest pad a guide box of this scene can have: 2^-18 M, M = four times the largest |coordinate|"""
    return 2.0 ** -18 * 4.0 * float(np.max(np.abs(np.asarray(pos, np.float64))))


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# (sliver width, length = 141), centre of the fan: shapes from 1.41 to ~40,000, coordinates near 0 and near 4096.  Width 0:
# two right-angled isosceles members whose records start at a 45-degree corner, shape sqrt(2).
FANS = ((0.005, 0.0), (0.02, 0.0), (0.1, 0.0), (0.5, 0.0), (2.0, 0.0), (8.0, 0.0), (18.0, 0.0), (35.0, 0.0), (70.0, 0.0),
        (141.0, 0.0), (18.0, 4096.0), (141.0, 4096.0), (0.1, 4096.0), (0.0, 0.0), (0.0, 4096.0))


def fan_case(rng, width, centre, n, length=141.0):
    """A fan of eight slivers `width` x `length` (two from a width of 18) (the construction of tests/test_claim_lists.py's fan_scene: a common
    apex, the short edges side by side) and one large triangle in its plane, turned by a random rotation, with one large
    triangle 40 units before and one 40 units behind the plane.  Origins p + s pad d: p a point of a sliver, mostly far
    from the apex, s between 0.1 and 316 (log-uniform), pad the scene's smallest guide pad — the sliver lies that far
    BEHIND the origin.  Half of the directions are within 3 degrees of the plane, the others uniform."""
    R = _rotation(rng)
    c = np.full(3, centre) + rng.uniform(-1, 1, 3)
    u, v, w = R[:, 0], R[:, 1], R[:, 2]
    apex = -(length / np.sqrt(2.0)) * (u + v)
    # (widths of 18 and more: two members next to the apex's foot, or the outer ones would be slivers again)
    members = range(-4, 4) if width < 18 else range(-1, 1)
    local = [(apex, (i * width) * u, ((i + 1) * width) * u) for i in members]
    if width == 0:  # the square on (u, v) of side `length`, cut along its diagonal: v0 at a 45-degree corner of either half
        local = [(length * v, 0 * u, length * u), (length * v, length * u, length * (u + v))]
    n_members = len(local)
    local.append((-200 * u, 200 * u, 300 * v))
    for s in (40.0, -40.0):
        local.append((-300 * u - 300 * v + s * w, 600 * u - 300 * v + s * w, -300 * u + 600 * v + s * w))
    pos = np.array([[c + p for p in t] for t in local], np.float64).reshape(-1, 9).astype(np.float32)
    k = rng.integers(0, n_members, n)
    tri = pos[k].astype(np.float64).reshape(n, 3, 3)
    a = rng.random(n) ** 2 * 0.9  # the apex's weight
    b = (1 - a) * rng.random(n)
    p = a[:, None] * tri[:, 0] + b[:, None] * tri[:, 1] + (1 - a - b)[:, None] * tri[:, 2]
    phi = rng.uniform(0, 2 * np.pi, n)
    theta = np.radians(rng.uniform(-3, 3, n))
    graze = (np.cos(theta) * np.cos(phi))[:, None] * u + (np.cos(theta) * np.sin(phi))[:, None] * v + np.sin(theta)[:, None] * w
    d = np.where((rng.random(n) < 0.5)[:, None], graze, _unit(rng.normal(size=(n, 3))))
    s = 10.0 ** rng.uniform(-1.0, 2.5, n)
    o = p + (s * min_pad(pos))[:, None] * d
    return pos, o.astype(np.float32), d.astype(np.float32)


def _nearest(pos, o, d):
    """nearest hit distance of every ray over a handful of triangles, in double (inf: none): only to place origins"""
    pos = np.asarray(pos, np.float64).reshape(-1, 3, 3)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    best = np.full(len(o), np.inf)
    for v0, v1, v2 in pos:
        e1, e2 = v1 - v0, v2 - v0
        pv = np.cross(d, e2)
        det = pv @ e1
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = o - v0
            uu = np.sum(tv * pv, axis=1) * inv
            q = np.cross(tv, e1)
            vv = np.sum(d * q, axis=1) * inv
            t = (q @ e2) * inv
        ok = (np.abs(det) > 1e-12) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (t > 0)
        best = np.where(ok & (t < best), t, best)
    return best


def pushed_cases(rng, n):
    """the free-origin constructions of guide_spec.adversarial_cases with every hitting ray's origin pushed 0.1-300 pads
    past the triangle it hits, along the ray: each hitting ray as often as it takes to give the construction n rays"""
    for kind, pos, o, d in G.adversarial_cases():
        pos32 = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
        finite = np.isfinite(d).all(axis=1) & (d != 0).all(axis=1)
        t = _nearest(pos32, o, d)
        keep = finite & np.isfinite(t)
        if not keep.any():
            continue
        reps = -(-n // int(keep.sum()))
        o, d, t = np.tile(o[keep], (reps, 1))[:n], np.tile(d[keep], (reps, 1))[:n], np.tile(t[keep], reps)[:n]
        s = 10.0 ** rng.uniform(-1.0, np.log10(300.0), len(t))
        o2 = o.astype(np.float64) + (t + s * min_pad(pos32))[:, None] * d.astype(np.float64)
        yield "pushed: " + kind, pos32, o2.astype(np.float32), d


def wall_case(rng, width, centre, n, length=60.0, strips=24):
    """A flat wall of slivers — `strips` strips `width` x `length`, each two triangles whose record edges both run along
    the strip (shape ~ length / width) — turned by a random rotation, under a large ceiling 50 units above it.  Rays leave
    the wall from 0.001 above it at grazing angles (0.01 to 5 degrees): the bounce ray's own situation."""
    R = _rotation(rng)
    c = np.full(3, centre) + rng.uniform(-1, 1, 3)
    u, v, w = R[:, 0], R[:, 1], R[:, 2]
    local = []
    for i in range(strips):
        p = (i - strips / 2) * width * v - 0.5 * length * u
        local.append((p, p + length * u, p + length * u + width * v))
        local.append((p + length * u + width * v, p + width * v, p))
    local.append((-300 * u - 300 * v + 50 * w, 600 * u - 300 * v + 50 * w, -300 * u + 600 * v + 50 * w))
    pos = np.array([[c + q for q in t] for t in local], np.float64).reshape(-1, 9).astype(np.float32)
    on = c + (rng.uniform(-0.5, 0.5, n) * length)[:, None] * u + (rng.uniform(-0.5, 0.5, n) * strips * width)[:, None] * v
    phi = rng.uniform(0, 2 * np.pi, n)
    theta = np.radians(10.0 ** rng.uniform(-2.0, np.log10(5.0), n))
    d = (np.cos(theta) * np.cos(phi))[:, None] * u + (np.cos(theta) * np.sin(phi))[:, None] * v + np.sin(theta)[:, None] * w
    o = on + 0.001 * w
    return pos, o.astype(np.float32), d.astype(np.float32)


WALLS = ((0.002, 0.0), (0.05, 0.0), (1.0, 0.0), (0.05, 4096.0))
CULL_SEED = 29


def cull_cases(rays_per_shape, seed=CULL_SEED):
    """Yields (kind, K, pos, o, d): K the worst gw_shape of the case's slivers (None for the pushed constructions, whose
    triangles are what they are).  One seeded generator per case, so a case's rays do not depend on the cases before it."""
    for i, (width, centre) in enumerate(FANS):
        rng = np.random.default_rng([seed, 0, i])
        pos, o, d = fan_case(rng, width, centre, rays_per_shape)
        yield ("fan %g x 141 at %g" % (width, centre) if width else "fan of two right-angled halves of a square at %g" % centre), float(shape(pos[:len(pos) - 3]).max()), pos, o, d
    for i, (width, centre) in enumerate(WALLS):
        rng = np.random.default_rng([seed, 1, i])
        pos, o, d = wall_case(rng, width, centre, rays_per_shape)
        yield "wall of %g x 60 slivers at %g" % (width, centre), float(shape(pos[:-1]).max()), pos, o, d
    rng = np.random.default_rng([seed, 2])
    for kind, pos, o, d in pushed_cases(rng, rays_per_shape):
        yield kind, None, pos, o, d
