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
