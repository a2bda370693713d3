"""Shared by test_guide_walk.py (CPU): the stand-alone host program of vermilion_amd/csrc/guide_walk.h
(tests/cpp/guide_walk_test.cpp), built once per session as claim_list_spec.py builds its own, the bounce rays the tests
feed it, and the oracle's verdict on what the per-ray rule settles."""
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
    Returns a dict: verdict, slot (reference leaf slot of the winner, NONE: no hit), t, visits on both trees per ray, and
    kappa: the guide's (inner, triangle) visits per walking ray at kappa = 2^-10, 2^-8, 2^-6."""
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
    visits = raw[:48].view(np.uint64).astype(np.float64)
    rec = raw[48:].view(np.uint32).reshape(n, 7)
    walking = max(int(np.sum(rec[:, 0] != INPUT)), 1)
    return {"verdict": rec[:, 0].copy(), "slot": rec[:, 1].copy(), "t": rec[:, 2].copy().view(np.float32),
            "guide_inner": rec[:, 3].copy(), "guide_tris": rec[:, 4].copy(), "ref_inner": rec[:, 5].copy(), "ref_tris": rec[:, 6].copy(),
            "kappa": (visits / walking).reshape(3, 2)}


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
