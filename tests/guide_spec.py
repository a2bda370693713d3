"""Shared by test_guide_walk.py (CPU) and test_gpu_guide_rays.py (the device's walk, ray by ray): the stand-alone host
program of vermilion_amd/csrc/guide_walk.h (tests/cpp/guide_walk_test.cpp), built once per session as claim_list_spec.py
builds its own, the bounce rays and the adversarial scenes both tests feed it, and the oracle's verdict on what the
per-ray rule settles."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
SETTLED, MISS, INPUT, LIMIT, TIE, BOX = range(6)  # GwVerdict
REASONS = {INPUT: "input", LIMIT: "limit", TIE: "tie", BOX: "own box"}
_exe = {}


def host_program(sanitize=False):
    """path of the built program (g++, the library's own flags for the arithmetic: no FMA contraction)"""
    if sanitize not in _exe:
        if shutil.which("g++") is None:
            import pytest
            pytest.skip("no g++")
        d = tempfile.mkdtemp(prefix="guide_walk_")
        exe = os.path.join(d, "guide_walk_test")
        csrc = os.path.join(ROOT, "vermilion_amd", "csrc")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + flags + ["-I", csrc,
                        os.path.join(ROOT, "tests", "cpp", "guide_walk_test.cpp"), os.path.join(csrc, "bvh_build.cpp"),
                        "-o", exe], check=True)
        _exe[sanitize] = exe
    return _exe[sanitize]


def host_guide(pos, tree, o, d, sanitize=False):
    """Walk and rule for the rays (o, d) [n, 3] over the guide of the triangles pos, beside the reference tree `tree`.
    Returns a dict: verdict, slot (reference leaf slot of the winner, NONE: no hit), t, visits on both trees per ray,
    kappa: the guide's (inner, triangle) visits per walking ray at kappa = 2^-10, 2^-8, 2^-6, and guide_depth / ref_depth:
    the depth of the deepest node of either tree (the root is 0), as the builders count it."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    rays = np.ascontiguousarray(np.concatenate([np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d, np.float32).reshape(-1, 3)], axis=1))
    n = rays.shape[0]
    tmp = tempfile.mkdtemp(prefix="guide_walk_io_")
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
        subprocess.run([host_program(sanitize), fin, fout], check=True)
        raw = np.fromfile(fout, np.uint8)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    head = raw[:64].view(np.uint64)
    visits = head[:6].astype(np.float64)
    rec = raw[64:].view(np.uint32).reshape(n, 7)
    walking = max(int(np.sum(rec[:, 0] != INPUT)), 1)
    return {"verdict": rec[:, 0].copy(), "slot": rec[:, 1].copy(), "t": rec[:, 2].copy().view(np.float32),
            "guide_inner": rec[:, 3].copy(), "guide_tris": rec[:, 4].copy(), "ref_inner": rec[:, 5].copy(), "ref_tris": rec[:, 6].copy(),
            "kappa": (visits / walking).reshape(3, 2), "guide_depth": int(head[6]), "ref_depth": int(head[7])}


def verdict(osc, tree, o, d, res):
    """(rays the rule settled wrongly, rays it settled with a hit, rays it settled as misses): a settled hit must carry
    the oracle's triangle and the bits of its t over the reference tree, a settled miss must be the oracle's miss"""
    o, d = np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d, np.float32).reshape(-1, 3)
    hit, miss = res["verdict"] == SETTLED, res["verdict"] == MISS
    tri, rt = osc.trace(o, d)
    order = np.asarray(tree["prim_order"])
    want = order[np.minimum(res["slot"], len(order) - 1)].astype(np.int64)
    bad = hit & ((tri != want) | (rt.view(np.uint32) != res["t"].view(np.uint32)))
    bad |= miss & (tri >= 0)
    return int(bad.sum()), int(hit.sum()), int(miss.sum())


def report(name, res, tri):
    """one line per scene: settled share of the hit rays, reasons for fallback, visits per ray on both trees"""
    v = res["verdict"]
    hits = tri >= 0
    walk = v != INPUT
    share = float(np.sum((v == SETTLED) & hits)) / max(int(hits.sum()), 1)
    why = ", ".join("%s %d" % (REASONS[k], int(np.sum(v == k))) for k in (INPUT, LIMIT, TIE, BOX))
    w = max(int(walk.sum()), 1)
    print("%s: %d rays, %d hit, settled %.2f %% of the hit rays, %d misses settled; fallback: %s; visits per walking ray: "
          "reference %.1f inner + %.1f tri, guide %.1f + %.1f (kappa 2^-10 / 2^-8 / 2^-6: %s)"
          % (name, len(v), int(hits.sum()), 100 * share, int(np.sum(v == MISS)), why,
             res["ref_inner"][walk].sum() / w, res["ref_tris"][walk].sum() / w, res["guide_inner"][walk].sum() / w,
             res["guide_tris"][walk].sum() / w, " / ".join("%.1f + %.1f" % tuple(k) for k in res["kappa"])))
    return share


def bounce_rays(osc, cam, seed, kind):
    """Bounce rays from the first hits of the camera's sample-0 rays, as the oracle's own RayCast reports them (location,
    normal) and pathtracer.cpp:155-164 forms the next ray: origin = location - 0.001 d, direction from (r1, r2) around the
    normal turned against the ray.  kind: "parity" (r2 = 10 U: most directions are NaN, as in the reference), "corrected"
    (r2 = U) or "uniform" (uniform on the sphere).  The draws are numpy's, not the oracle's stream: the oracle library
    exports whole paths (radiance) and single queries (trace, raycast), not the rays in between, and oracle/ is not to be
    changed for a test.  What the rule is checked on is therefore the oracle's hit records and the reference's formula for
    the next ray; the verdict on every ray is still the oracle's own trace of that ray."""
    import oracle_lib as O
    import vermilion_amd as va
    o, d = O.primary_rays(cam, va.make_opts(seed=seed), 0)
    h = osc.raycast(o, d)
    keep = h["tri_id"] >= 0
    loc, nrm, d = h["location"][keep], h["normal"][keep], d[keep]
    f32 = np.float32
    start = (loc - d * f32(0.001)).astype(f32)
    rng = np.random.default_rng(seed)
    n = start.shape[0]
    if kind == "uniform":
        v = rng.normal(size=(n, 3))
        return start, (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)
    r1 = (2 * np.pi * rng.random(n)).astype(f32)
    r2 = ((10.0 if kind == "parity" else 1.0) * rng.random(n)).astype(f32)
    r2s = np.sqrt(r2)
    w = np.where((np.sum(nrm * d, axis=1) < 0)[:, None], nrm, -nrm).astype(f32)
    a = np.where((np.abs(w[:, 0]) > 0.1)[:, None], f32([0, 1, 0]), f32([1, 0, 0]))
    u = np.cross(a, w)
    u = (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(f32)
    v = np.cross(w, u).astype(f32)
    with np.errstate(invalid="ignore"):
        nd = u * (np.cos(r1) * r2s)[:, None] + v * (np.sin(r1) * r2s)[:, None] + w * np.sqrt(f32(1) - r2)[:, None]
        nd = (nd / np.linalg.norm(nd, axis=1, keepdims=True)).astype(f32)
    return start, nd


def flat_normals(pos):
    """the face normal of every triangle at its three vertices [n, 9] (a zero-area triangle: +y)"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 9)
    e1, e2 = pos[:, 3:6] - pos[:, 0:3], pos[:, 6:9] - pos[:, 0:3]
    nr = np.cross(e1, e2)
    ln = np.linalg.norm(nr, axis=1, keepdims=True)
    nr = np.where(ln > 0, nr / np.maximum(ln, 1e-30), np.float32([0, 1, 0])).astype(np.float32)
    return np.repeat(nr[:, None, :], 3, axis=1).reshape(-1, 9)


def _dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _towards(rng, o, target, spread, n):
    """n rays from o (one origin or [n, 3]) towards points within `spread` of target"""
    o = np.broadcast_to(np.asarray(o, np.float64), (n, 3))
    p = np.asarray(target, np.float64) + rng.uniform(-spread, spread, (n, 3))
    v = p - o
    return o.astype(np.float32), (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


ADVERSARIAL_SEED = 17


def adversarial_cases(seed=ADVERSARIAL_SEED):
    """Yields (kind, pos, o, d): the constructions of tests/test_claim_lists.py (its _tri and fan_scene, imported; the
    coplanar pair, the T-junction and the two planes a few floats apart built as it builds them) under free origins, and
    the cases a free origin adds: rays that start on a triangle or on a shared edge, grazing rays, a zero direction
    component, origins outside the scene's bounds.  One seeded generator draws everything, in this order, so the host
    program and the device see the same rays.  "close planes" comes three times (1, 4 and 64 floats apart), "sliver fan in
    a coordinate plane" eight times."""
    from test_claim_lists import _tri, fan_scene
    rng = np.random.default_rng(seed)
    r, u, f = np.array([1.0, 0.2, 0.1]), np.array([-0.1, 1.0, 0.3]), np.array([0.2, -0.3, 1.0])
    r, u, f = r / np.linalg.norm(r), u / np.linalg.norm(u), f / np.linalg.norm(f)
    # the shared edge of a coplanar pair, rays aimed at and around the edge
    c = np.array([3.0, 2.0, 51.0])
    a, b = c - 40 * u, c + 40 * u
    pair = np.concatenate([_tri(a, b, c - 60 * r), _tri(b, a, c + 60 * r)])
    o, d = _towards(rng, (3.0, 2.0, 1.0), c, 0.01, 4000)
    o2, d2 = _towards(rng, (3.0, 2.0, 1.0), c, 30.0, 2000)
    yield "coplanar pair", pair, np.concatenate([o, o2]), np.concatenate([d, d2])
    # ... and rays that hit the edge itself: points of the edge from the float vertices, t near 50
    k = rng.uniform(-0.9, 0.9, (2000, 1))
    edge = (np.float32(c) + k * np.float32(40 * u)).astype(np.float64)
    o = np.broadcast_to(np.array([3.0, 2.0, 1.0]), edge.shape)
    v = edge - o
    yield "coplanar pair, edge points", pair, o.astype(np.float32), (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    # a T-junction
    a, b = c - 50 * r, c + 50 * r
    tj = np.concatenate([_tri(a, b, c - 60 * u), _tri(a, c, c + 60 * u), _tri(c, b, c + 60 * u)])
    o, d = _towards(rng, (3.0, 2.0, 1.0), c, 0.02, 3000)
    o2, d2 = _towards(rng, (3.0, 2.0, 1.0), c, 30.0, 1000)
    yield "T-junction", tj, np.concatenate([o, o2]), np.concatenate([d, d2])
    # two parallel planes 1, 4 and 64 floats apart: every ray that hits both is a tie within 2^-16
    for steps in (1, 4, 64):
        big = _tri(c - 25 * r - 25 * u, c + 50 * r - 25 * u, c - 25 * r + 50 * u).astype(np.float32)
        other = (big.view(np.int32) + np.int32(steps) * np.sign(big).astype(np.int32)).view(np.float32)
        o, d = _towards(rng, (3.0, 2.0, 1.0), c, 8.0, 2000)
        yield "close planes", np.concatenate([big, other]).astype(np.float64), o, d
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
        yield "sliver fan in a coordinate plane", fan, np.concatenate([o, o2]), np.concatenate([d, d2])

    # ---- free origins
    # rays that start ON a triangle or on the shared edge of the pair (t near 0), into the half space of a second wall
    wall = _tri(c + 30 * f - 200 * r - 200 * u, c + 30 * f + 400 * r - 200 * u, c + 30 * f - 200 * r + 400 * u)
    room = np.concatenate([pair, wall])
    k = rng.uniform(-0.9, 0.9, (1500, 1))
    on_edge = (np.float32(c) + k * np.float32(40 * u)).astype(np.float32)
    on_face = (np.float32(c) + k * np.float32(30 * u) + rng.uniform(-20, 20, (1500, 1)) * np.float32(r)).astype(np.float32)
    o = np.concatenate([on_edge, on_face])
    yield "origins on a triangle", room, o, _dirs(rng, len(o))
    # grazing rays: within 1e-4 of the plane of the pair, from beside it
    side = c - 70 * r + rng.uniform(-1e-4, 1e-4, (3000, 1)) * np.cross(r, u)
    tgt = c + 70 * r + rng.uniform(-30, 30, (3000, 1)) * u + rng.uniform(-1e-4, 1e-4, (3000, 1)) * np.cross(r, u)
    v = tgt - side
    yield "grazing rays", room, side.astype(np.float32), (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    # a direction with a zero component must fall back (its reciprocal is infinite)
    o, d = _towards(rng, (3.0, 2.0, 1.0), c, 20.0, 600)
    d = d.copy()
    d[:200, 0], d[200:400, 1], d[400:, 2] = 0.0, 0.0, -0.0
    yield "zero direction component", room, o, d
    # origins outside the scene's bounds: beyond M = four times the largest |coordinate| (about 450 here) the rule falls
    # back; inside it, it may settle
    o, d = _towards(rng, (9000.0, -7000.0, 8000.0), c, 30.0, 1000)
    yield "origins outside the bounds", room, o, d
    o, d = _towards(rng, (-900.0, 700.0, -800.0), c, 30.0, 1000)  # outside the vertex box, within M
    yield "origins outside the vertex box", room, o, d
    # a tie across subtrees: a patch of 16 small triangles in z = 100 in front of two large ones in z = 100.005.  SAH
    # parts the patch from the large pair at the root.  From z = -390 (inside M = 400) the patch is hit at t = 490 and the
    # large pair 0.005 farther: beyond the pad of the pair's box (0.0023), so its node's near exceeds best, and within the
    # tie band 2^-16 t = 0.0075.  The pair's node waits on the stack while the patch is hit: only a pop that prunes on
    # cut, not on best, still visits it and sees the tie.  (Drawn last, so the cases above keep their rays.)
    xs, ys = np.linspace(-10.0, 10.0, 3), np.linspace(-10.0, 10.0, 5)
    patch = [_tri((xs[i], ys[j], 100.0), (xs[i + 1], ys[j], 100.0), (xs[i + 1], ys[j + 1], 100.0)) for i in range(2) for j in range(4)]
    patch += [_tri((xs[i], ys[j], 100.0), (xs[i + 1], ys[j + 1], 100.0), (xs[i], ys[j + 1], 100.0)) for i in range(2) for j in range(4)]
    far = [_tri((-100.0, -100.0, 100.005), (100.0, -100.0, 100.005), (100.0, 100.0, 100.005)),
           _tri((-100.0, -100.0, 100.005), (100.0, 100.0, 100.005), (-100.0, 100.0, 100.005))]
    o, d = _towards(rng, (0.5, -0.7, -390.0), (0.0, 0.0, 100.0), 12.0, 2000)
    yield "tie across subtrees", np.concatenate(patch + far), o, d
