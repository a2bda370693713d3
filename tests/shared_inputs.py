"""Inputs that several test files feed to more than one side (kernels, oracle, the compiled reference)."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def random_soup(rng, n, kind):
    """triangle soups that stress the tree and the traversal: flat axis-aligned sheets (zero-thickness boxes),
    duplicated triangles (exact distance ties), slivers and degenerate (zero-area) triangles, huge + tiny mixed"""
    if kind == "sheets":  # triangles lying in a few axis-aligned planes, shared edges
        ax = rng.integers(0, 3, n)
        plane = rng.choice(np.float32([-300, 0, 250, 600]), n)
        c = rng.uniform(-800, 800, (n, 1, 3)).astype(np.float32)
        p = c + rng.uniform(-120, 120, (n, 3, 3)).astype(np.float32)
        p[np.arange(n), :, ax] = plane[:, None]
    elif kind == "duplicates":
        m = max(n // 3, 1)
        base = (rng.uniform(-600, 600, (m, 1, 3)) + rng.uniform(-90, 90, (m, 3, 3))).astype(np.float32)
        p = base[rng.integers(0, m, n)]  # every triangle several times: ties are resolved by test order
    elif kind == "slivers":
        c = rng.uniform(-700, 700, (n, 1, 3)).astype(np.float32)
        p = c + rng.uniform(-200, 200, (n, 3, 3)).astype(np.float32)
        k = rng.random(n) < 0.3
        p[k, 2] = p[k, 0] + (p[k, 1] - p[k, 0]) * rng.uniform(0, 1, (int(k.sum()), 1)).astype(np.float32)  # collinear
        z = rng.random(n) < 0.05
        p[z, 1] = p[z, 0]  # two equal vertices
    else:  # "scales": a few huge triangles over many tiny ones
        c = rng.uniform(-500, 500, (n, 1, 3)).astype(np.float32)
        s = np.where(rng.random((n, 1, 1)) < 0.03, 2500.0, 12.0).astype(np.float32)
        p = c + rng.uniform(-1, 1, (n, 3, 3)).astype(np.float32) * s
    p = np.ascontiguousarray(p, np.float32)
    nr = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).astype(np.float32)
    ln = np.linalg.norm(nr, axis=1, keepdims=True)
    nr = np.where(ln > 0, nr / np.maximum(ln, 1e-30), np.float32([0, 1, 0])).astype(np.float32)
    return p, np.repeat(nr[:, None, :], 3, axis=1).copy(), None


SOUP_KINDS = ("sheets", "duplicates", "slivers", "scales")
SOUP_SEEDS = {"sheets": 11, "duplicates": 12, "slivers": 13, "scales": 14}
SOUP_SIZES = ((1, 4), (37, 1), (700, 4), (5000, 2), (20000, 7))  # (triangles, leaf size)


def flat_normals(p):
    """geometric normals, (0, 1, 0) for zero-area triangles, repeated per vertex"""
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        nr = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).astype(np.float32)
        ln = np.linalg.norm(nr, axis=1, keepdims=True)
        nr = np.where((ln > 0) & np.isfinite(ln), nr / np.maximum(ln, 1e-30), np.float32([0, 1, 0])).astype(np.float32)
    return np.repeat(nr[:, None, :], 3, axis=1).copy()


# ---- inputs for the tree builders (tree_spec.py): each family(n, seed) -> positions [n, 3, 3], at most 4096 triangles.
# Another seed is another member of the same family with the same count.
def _coincident(rng, n):
    return np.repeat(rng.uniform(-50, 50, (1, 3, 3)).astype(np.float32), n, axis=0)


def _same_box(rng, n):
    """different triangles, every one spanning the box [10, 110]^3: two opposite corners and a point inside"""
    corner = rng.integers(0, 2, (n, 3)).astype(np.float32)
    p = np.stack([corner, 1 - corner, rng.uniform(0.05, 0.95, (n, 3)).astype(np.float32)], axis=1)
    return p * np.float32(100) + np.float32(10)


def _strip(rng, n):
    x = rng.permutation(n).astype(np.float32)[:, None]
    return np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 1]])[None] + x[:, :, None] * np.float32([1, 0, 0])


def _grid(rng, n):
    w = int(np.ceil(np.sqrt(n)))
    k = rng.permutation(n)
    cell = np.stack([k % w, k // w, np.zeros(n)], axis=1).astype(np.float32)
    return np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 1]])[None] + cell[:, None, :]


def _one_cell(rng, n):
    """a cluster 10^-9 of the extent wide, so that its centroids share one Morton cell, and one far outlier (a large
    triangle, which rays through the scene's box do hit)"""
    p = (rng.uniform(-1e-3, 1e-3, (n, 3, 3)) + rng.uniform(-1e-3, 1e-3, (n, 1, 3))).astype(np.float32)
    p[n // 2] = p[n // 2] * np.float32(3e8) + np.float32(1e6)
    return p


def _zero_extent(rng, n):
    """all centroids equal in z, and for every other seed in y as well: the scale of that axis is 0"""
    p = rng.uniform(-40, 40, (n, 1, 3)).astype(np.float32) + np.float32([[0, 0, 0], [3, 0, 0], [0, 2, 0]])[None]
    p[:, :, 2] = np.float32([4, 5, 6])
    if rng.integers(0, 2):
        p[:, :, 1] = np.float32([1, 1, 3])
    return p


def _huge(rng, n):
    """finite coordinates up to 3.3e38: centroid sums and box extents overflow to inf, and flat triangles (every third is
    flat in y) give inf * 0 in the half area of a union"""
    c = rng.choice(np.float32([-3e38, -1e38, 0, 2e38, 3e38]), (n, 1, 3))
    p = np.clip(c.astype(np.float64) + rng.uniform(-3e37, 3e37, (n, 3, 3)), -3.3e38, 3.3e38).astype(np.float32)
    p[::3, :, 1] = p[::3, :1, 1]
    return p


TREE_FAMILIES = {"coincident": _coincident, "same_box": _same_box, "strip": _strip, "grid": _grid, "one_cell": _one_cell,
                 "zero_extent": _zero_extent, "huge": _huge}
TREE_FAMILY_NAMES = ("coincident", "same_box", "strip", "grid") + SOUP_KINDS + ("one_cell", "zero_extent", "huge")


def tree_family(name, n, seed=0):
    """(pos [n, 9], nrm [n, 9]) of a member of the family"""
    assert 1 <= n <= 4096
    rng = np.random.default_rng([TREE_FAMILY_NAMES.index(name), n, seed])
    p = random_soup(rng, n, name)[0] if name in SOUP_KINDS else TREE_FAMILIES[name](rng, n)
    p = np.ascontiguousarray(p, np.float32).reshape(n, 3, 3)
    return p.reshape(n, 9).copy(), flat_normals(p).reshape(n, 9)


def uniform_soup(n, seed=0):
    """small triangles at uniformly random places: the yardstick for the number of PLOC rounds"""
    rng = np.random.default_rng([99, n, seed])
    p = (rng.uniform(-500, 500, (n, 1, 3)) + rng.uniform(-10, 10, (n, 3, 3))).astype(np.float32)
    return p.reshape(n, 9).copy(), flat_normals(p).reshape(n, 9)


def nan_cycle():
    """Three flat triangles in y = 0 at x = -2e38, 1e38, 2e38 (one Morton cell: the extent overflows).  The outer two
    unite to inf * 0 = NaN; the middle one prefers the right one, the right one's first candidate is the left one.  With
    a comparison that a NaN never loses, 0 -> 1 -> 2 -> 0 and no pair is mutual."""
    p = np.float32([[0, 0, 0], [1e30, 0, 0], [0, 0, 1e-3]])[None] + np.float32([-2e38, 1e38, 2e38])[:, None, None] * np.float32([1, 0, 0])
    p = np.ascontiguousarray(p, np.float32)
    return p.reshape(3, 9).copy(), flat_normals(p).reshape(3, 9)


def deep_lbvh():
    """65 small triangles whose Morton keys are 0, every single set bit 2^0 .. 2^62 and (the corner that fixes the bounds
    at 2^21 - 1, so a cell is 1 wide) all ones: the radix tree over them is a chain of 63 nodes"""
    cells = [(0, 0, 0)] + [tuple((1 << (k // 3)) if a == 2 - k % 3 else 0 for a in range(3)) for k in range(63)]
    cells.append((2097151,) * 3)
    c = np.float32(cells)[:, None, :]
    p = c + np.float32([[-0.125, -0.125, 0], [0.125, -0.125, 0], [0, 0.25, 0]])[None]  # the centroid is c, exactly
    p = np.ascontiguousarray(p, np.float32)
    return p.reshape(-1, 9).copy(), flat_normals(p).reshape(-1, 9)


def numpy_boxes(tree, pos):
    """every node's tight box over its triangles' vertices, for the given topology"""
    p = np.asarray(pos, np.float32).reshape(-1, 3, 3)
    order = tree["prim_order"]
    slo, shi = p.min(axis=1)[order], p.max(axis=1)[order]
    ro = tree["right_offset"]
    n = len(tree["start"])
    box = np.zeros((n, 6), np.float32)
    leaf = ro == 0
    li = np.nonzero(leaf)[0]
    li = li[np.argsort(tree["start"][li], kind="stable")]  # leaves partition the slots
    st = tree["start"][li].astype(np.int64)
    box[li, :3] = np.minimum.reduceat(slo, st, axis=0)
    box[li, 3:] = np.maximum.reduceat(shi, st, axis=0)
    for i in np.nonzero(~leaf)[0][::-1]:
        l, r = i + 1, i + ro[i]
        box[i, :3] = np.minimum(box[l, :3], box[r, :3])
        box[i, 3:] = np.maximum(box[l, 3:], box[r, 3:])
    return box


def special_rays():
    """NaN / zero direction components, rays lying in box faces, starts on shared edges of the lattice"""
    g = np.load(os.path.join(GOLD, "lattice.npz"))
    o, d = [g["ray_o"][:60]], [g["ray_d"][:60]]
    xs = np.float32([-600, -250, 0, 150, 600, -250.00002, 149.99998])
    for x in xs:
        for y in np.float32([1, 400, 900, 200]):
            for dvec in ((0, 0, -1), (0, 0, 1), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0)):
                o.append(np.float32([[x, y, 300.0], [x, y, 0.0]])), d.append(np.float32([dvec, dvec]))
    return np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32)


def wall_rays(n=60000, seed=7):
    """rays starting on and just off the six 5e7-radius wall spheres of RayCast's table, a quarter of them grazing"""
    rng = np.random.default_rng(seed)
    oo, dd = [], []
    for ax, val in ((0, -2000), (0, 2000), (2, -2000), (2, 2000), (1, 0), (1, 1000)):
        o = np.empty((n, 3), np.float32)
        o[:, 0], o[:, 1], o[:, 2] = rng.uniform(-2000, 2000, n), rng.uniform(0, 1000, n), rng.uniform(-2000, 2000, n)
        o[:, ax] = val + rng.uniform(-0.7, 0.7, n)
        d = rng.normal(size=(n, 3))
        d[: n // 4, ax] *= 1e-5  # grazing
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        oo.append(o), dd.append(d.astype(np.float32))
    return np.concatenate(oo), np.concatenate(dd)


LIGHT1 = np.float32([15, 140, 25])      # the reference's first light sphere (meshEngine.cpp:377), radius 3.5
LIGHT2 = np.float32([0, 3300, 1300])    # its second (meshEngine.cpp:410), radius 250


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def rays_inside_and_outside(pos, n, seed):
    """origins inside the scene's box and in a shell around it, directions random and aimed back at the box"""
    r = np.random.default_rng(seed)
    p = np.asarray(pos, np.float32).reshape(-1, 3)
    lo, hi = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
    ext = np.maximum(hi - lo, 1.0)
    inside = r.uniform(lo, hi, (n // 2, 3))
    shell = r.uniform(lo - 1.5 * ext, hi + 1.5 * ext, (n - n // 2, 3))
    o = np.concatenate([inside, shell]).astype(np.float32)
    d = r.normal(size=(n, 3))
    aim = r.uniform(lo, hi, (n, 3)) - o
    k = r.random(n) < 0.5
    d[k] = aim[k]
    return o, unit(d)


def light_rays(n, seed):
    """from points in the room toward and around the two light spheres"""
    r = np.random.default_rng(seed)
    o = r.uniform((-1900, 5, -1900), (1900, 990, 1900), (n, 3))
    tgt = np.where(r.random((n, 1)) < 0.6, LIGHT1.astype(np.float64), LIGHT2.astype(np.float64))
    rad = np.where(tgt[:, 1:2] < 1000, 3.5, 250.0)
    tgt = tgt + r.normal(size=(n, 3)) * rad * 0.8  # through, grazing and just past the sphere
    return o.astype(np.float32), unit(tgt - o)
