"""Scenes, sphere tables, textures and rays that the light-sampling tests feed to more than one side (nee_spec, the oracle,
the kernels)."""
import ctypes as C
import os

import numpy as np

import vermilion_amd as va
from vermilion_amd import _lib as L

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CORRECTED = L.VMX_SAMPLING_CORRECTED


def golden(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    return g["pos"], g["nrm"], g["uv"], g["primary_o"], g["primary_d"], g


def opts(seed, sampling=CORRECTED, **kw):
    return va.make_opts(seed=seed, early_stop=False, sampling=sampling, **kw)


def _copy(table):
    out = (L.Sphere * len(table))()
    for i, s in enumerate(table):
        C.memmove(C.byref(out[i]), C.byref(s), C.sizeof(L.Sphere))
    return out


def _emitter(centre, radius, colour):
    s = L.Sphere()
    s.centre[:] = centre
    s.radius = radius
    s.colour[:] = colour
    s.flags = L.VMX_SPHERE_EMIT
    s.normal_centre[:] = centre
    s.normal_sign = 1.0
    return s


def table(name):
    """default: the reference's eight; none: the same with no emitter; single: one mid-size emitter alone inside the room;
    overlap: two emitters above each other, whose cones overlap from the floor below them; three: a non-emitter between
    emitters (table indices and emitter indices differ) and a different emitter count"""
    d = va.default_spheres()
    walls = [d[i] for i in range(2, 8)]
    if name == "default":
        return d
    if name == "none":
        out = _copy(d)
        for s in out:
            s.flags = 0
        return out
    if name == "single":
        return _copy([_emitter((300.0, 600.0, 200.0), 60.0, (9.0, 8.0, 6.0))] + walls)
    if name == "overlap":
        return _copy([_emitter((100.0, 500.0, 150.0), 60.0, (12.0, 6.0, 3.0)), _emitter((100.0, 800.0, 150.0), 120.0, (3.0, 6.0, 12.0))]
                     + walls)
    if name == "three":
        return _copy([_emitter((300.0, 600.0, 200.0), 60.0, (9.0, 8.0, 6.0)), walls[0], _emitter((-400.0, 300.0, -100.0), 40.0, (2.0, 9.0, 4.0))]
                     + walls[1:] + [_emitter((0.0, 700.0, -600.0), 90.0, (6.0, 2.0, 7.0))])
    raise KeyError(name)


def texture(channels, seed=5):
    """[7, 5(, C)] texels in [0.25, 1): sizes that are no power of two, so the wrap and the rounding both matter"""
    r = np.random.default_rng([seed, channels])
    t = r.uniform(0.25, 1.0, (7, 5, channels)).astype(np.float32)
    return t[:, :, 0].copy() if channels == 1 else t


def inside_rays(n=64):
    """n camera rays that start inside an emitter and first hit a triangle inside it: (table, o, d).  The emitter (dim) is
    centred on a golden primary hit of a cornell8 triangle and holds the n nearest other hits with 30 units to spare; the
    rays are those golden primary rays, started 20 units before their hit."""
    pos, nrm, uv, o, d, g = golden("cornell8")
    hit = g["primary_id"] >= 0
    p = (o + d * g["primary_t"][:, None])[hit]
    dd = d[hit]
    c = p[len(p) // 2]
    dist = np.linalg.norm(p - c, axis=1)
    near = np.argsort(dist, kind="stable")[:n]
    radius = float(np.ceil(dist[near].max() + 30.0))
    start = (p[near] - dd[near] * np.float32(20.0)).astype(np.float32)
    walls = [va.default_spheres()[i] for i in range(2, 8)]
    tb = _copy([_emitter(tuple(float(v) for v in c), radius, (1.5, 1.25, 1.0)), _emitter((300.0, 600.0, 200.0), 60.0, (9.0, 8.0, 6.0))]
               + walls)
    return tb, start, dd[near].copy()
