#!/usr/bin/env python3
"""Device ray queries (vmx_query_device, k_query) on the bench scene: Mrays/s of NEAREST and ANY for three ray sets,
over the reference tree and over PLOC, with the quad-cooperative and the per-lane record fetch.

    python tools/query_bench.py [--reps 20] [--warmup 3] [--out FILE]

Ray sets (sponza260k, 1920x1080 bench camera of bench.py):
  (a) primary: one sample of every pixel's camera ray (oracle ray generation)
  (b) bounce:  cosine-lobe rays from the (a) hits (normal flipped toward the ray), origins 0.01 off the surface
  (c) shadow:  from the (a) hits toward the emitting spheres' centres, tmax = distance - radius
Times: torch CUDA events around one device call, median of --reps after --warmup; plus the old host vmx_trace wall
time of the same set (copies and allocation included) for context."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle_lib as O  # noqa: E402
import vermilion_amd as va  # noqa: E402
from vermilion_amd import scenes  # noqa: E402


def ray_sets(sc, W, H):
    c = scenes.sponza_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], W, H, 1, back_size=(3.6, 3.6 * H / W))
    o, d = O.primary_rays(cam, va.make_opts(seed=1), 0)
    sets = {"a_primary": (o, d, None)}
    h = sc.raycast(o, d)
    keep = h["tri_id"] >= 0
    p, nrm, din = h["location"][keep], h["normal"][keep].astype(np.float64), d[keep].astype(np.float64)
    nrm = np.where((np.sum(nrm * din, axis=1) > 0)[:, None], -nrm, nrm)
    r = np.random.RandomState(5)
    u1, u2 = r.rand(len(p)), r.rand(len(p))
    a = np.where(np.abs(nrm[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    t1 = np.cross(a, nrm)
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(nrm, t1)
    rr, ph = np.sqrt(u1)[:, None], 2 * np.pi * u2[:, None]
    bd = t1 * rr * np.cos(ph) + t2 * rr * np.sin(ph) + nrm * np.sqrt(1 - u1)[:, None]
    bd /= np.linalg.norm(bd, axis=1, keepdims=True)
    sets["b_bounce"] = ((p + 0.01 * nrm).astype(np.float32), bd.astype(np.float32), None)
    so, sd, st = [], [], []
    for s in va.default_spheres():
        if s.flags & va._lib.VMX_SPHERE_EMIT:
            v = np.float32(list(s.centre))[None, :].astype(np.float64) - p
            dist = np.linalg.norm(v, axis=1)
            so.append(p), sd.append(v / dist[:, None]), st.append(dist - s.radius)
    sets["c_shadow"] = (np.concatenate(so).astype(np.float32), np.concatenate(sd).astype(np.float32),
                        np.concatenate(st).astype(np.float32))
    return sets


def time_query(sc, O_, D_, T_, mode, per_lane, reps, warmup):
    for _ in range(warmup):
        sc.query(O_, D_, T_, mode=mode, per_lane_fetch=per_lane)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sc.query(O_, D_, T_, mode=mode, per_lane_fetch=per_lane)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("query_bench: no GPU (nothing is measured on the CPU)")
    lines = [f"# tools/query_bench.py: sponza260k, {args.width}x{args.height} bench camera, median of {args.reps} "
             f"after {args.warmup} warm-up calls (min / max in brackets); {torch.cuda.get_device_name(0)}"]
    pos, nrm, uv = scenes.sponza260k()
    torch.cuda.set_stream(torch.cuda.Stream())  # an explicit stream: the events and the queries share it
    for bname, builder in (("reference", va._lib.VMX_BVH_REFERENCE), ("ploc", va._lib.VMX_BVH_PLOC)):
        with va.Scene(pos, nrm, uv, builder=builder) as sc:
            for sname, (o, d, tm) in ray_sets(sc, args.width, args.height).items():
                n = len(o)
                t0 = time.perf_counter()
                id_ref, t_ref = sc.trace(o, d)
                host_ms = (time.perf_counter() - t0) * 1e3
                O_, D_ = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
                T_ = torch.from_numpy(tm).cuda() if tm is not None else None
                # results first: the timed calls compute what vmx_trace computes (identities of vermilion_hip.h)
                tri, t, _ = sc.query(O_, D_, T_)
                hit = sc.query(O_, D_, T_, mode="any")
                torch.cuda.synchronize()
                lim = np.float32(999999999.0) if tm is None else np.minimum(tm, np.float32(999999999.0))
                inside = (id_ref >= 0) & (t_ref < lim)
                assert np.array_equal(tri.cpu().numpy(), np.where(inside, id_ref, -1)), (bname, sname)
                assert np.array_equal(hit.cpu().numpy(), inside), (bname, sname)
                row = f"{bname:9s} {sname:9s} n={n:8d} hit={inside.mean():.3f}"
                for mode in ("nearest", "any"):
                    for per_lane in (False, True):
                        med, lo, hi = time_query(sc, O_, D_, T_, mode, per_lane, args.reps, args.warmup)
                        tag = f"{mode}/{'lane' if per_lane else 'quad'}"
                        row += f" | {tag} {med:7.3f} ms [{lo:.3f} {hi:.3f}] {n / med / 1e3:7.1f} Mrays/s"
                row += f" | host vmx_trace {host_ms:8.1f} ms wall"
                print(row, flush=True)
                lines.append(row)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
