"""Scenes, emitter tables and rays that the emissive-triangle tests feed to more than one side (nee_mesh_spec, the oracle, the
kernels).  A case is a dict: pos / nrm / uv (the arrays a scene is created on), moved (positions a refit then brings, or
None), ids / radiance (the emitter table), spheres (a nee_cases table name), o / d (camera rays), camera (for frames)."""
import os

import numpy as np

import nee_cases as K
from vermilion_amd import scenes

F = np.float32
QUAD_RADIANCE = (6.0, 5.0, 4.0)
DIM_RADIANCE = (0.5, 0.45, 0.4)  # length 0.78 <= 1: the path goes on from the emitter (self-exclusion)


def ceiling_quad():
    """two triangles under the room's ceiling, over the block and over nee_cases' "overlap" spheres (which it cuts: their
    cones reach it from the floor), facing down"""
    return scenes._quad((-300, 880, 300), (300, 880, 300), (300, 880, -300), (-300, 880, -300), (0, -1, 0))


def cornell_quad():
    """cornell8 plus the ceiling quad: 10 triangles, the quad's ids 8 and 9"""
    pos, nrm, uv, o, d, _ = K.golden("cornell8")
    qp, qn, qt = ceiling_quad()
    return (np.concatenate([pos, qp.reshape(-1, 9)]).astype(F), np.concatenate([nrm, qn.reshape(-1, 9)]).astype(F),
            np.concatenate([uv, qt.reshape(-1, 6)]).astype(F), o, d)


def lattice_table(n, seed=11):
    """n of the lattice's 200 triangles in a shuffled order with radiances in [0.5, 8); from two entries on entry 1 is
    black (weight 0), from three on entry 2 is the one `moved` collapses to a point (area 0)"""
    r = np.random.default_rng([seed, n])
    ids = r.permutation(200)[:n].astype(np.int64)
    rad = r.uniform(0.5, 8.0, (n, 3)).astype(F)
    if n >= 2:
        rad[1] = 0
    return ids, rad


@np.errstate(all="ignore")
def case(name):
    cam = scenes.cornell_camera()
    if name.startswith("quad_"):  # quad_none, quad_single, quad_overlap
        pos, nrm, uv, o, d = cornell_quad()
        return dict(pos=pos, nrm=nrm, uv=uv, moved=None, ids=np.array([8, 9]), radiance=np.array([QUAD_RADIANCE] * 2, F),
                    spheres=name[5:], o=o, d=d, camera=cam)
    if name == "block_top":
        pos, nrm, uv, o, d, _ = K.golden("cornell8")
        # (beside the "single" sphere: the reference's 3.5-unit light is found by chance too rarely for a brute-force mean)
        return dict(pos=pos, nrm=nrm, uv=uv, moved=None, ids=np.array([6, 7]), radiance=np.array([DIM_RADIANCE] * 2, F),
                    spheres="single", o=o, d=d, camera=cam)
    if name.startswith("lattice_"):  # lattice_1, _2, _3, _63, _65, _200
        n = int(name[8:])
        pos, nrm, uv, o, d, _ = K.golden("lattice")
        ids, rad = lattice_table(n)
        moved = None
        if n >= 3:
            moved = pos.copy()
            moved[ids[2], 3:6] = moved[ids[2], 0:3]
            moved[ids[2], 6:9] = moved[ids[2], 0:3]
        return dict(pos=pos, nrm=nrm, uv=uv, moved=moved, ids=ids, radiance=rad, spheres="default", o=o, d=d,
                    camera=scenes.lattice_camera())
    if name == "soup":
        g = np.load(os.path.join(K.GOLD, "ref_soup_duplicates.npz"))
        pos, nrm = g["pos"].reshape(-1, 9).astype(F), g["nrm"].reshape(-1, 9).astype(F)
        # the coincident pairs the camera rays hit most: one of each pair emits (the later id of the first, the earlier of the second)
        hit = g["cam_trace_id"]
        ids = []
        for t in np.unique(hit[hit >= 0]):
            twins = np.nonzero((pos == pos[t]).all(axis=1))[0]
            if len(twins) >= 2 and not set(twins) & set(ids):
                ids.append(int(twins[-1] if len(ids) % 2 == 0 else twins[0]))
            if len(ids) == 4:
                break
        c = g["cam"]
        return dict(pos=pos, nrm=nrm, uv=None, moved=None, ids=np.array(ids), radiance=np.array([[3.0, 0.5, 0.25]] * len(ids), F),
                    spheres="default", o=g["ray_o"].astype(F), d=g["ray_d"].astype(F), camera=dict(position=tuple(c[:3]),
                                                                                                  rotation_deg=tuple(c[3:6])))
    raise KeyError(name)


LIT = ["quad_none", "quad_single", "quad_overlap", "block_top"]
LATTICE = ["lattice_1", "lattice_2", "lattice_3", "lattice_63", "lattice_65", "lattice_200"]
ALL = LIT + LATTICE + ["soup"]


def current(c):
    """the positions the case's table and frames are defined on: after the refit where there is one"""
    return c["pos"] if c["moved"] is None else c["moved"]
