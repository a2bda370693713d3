#!/usr/bin/env python3
"""MeshEngine::RayCast of device batches (vmx_raycast_device, vmx_raycast_camera_device) on the bench scene, against
the traversal alone (vmx_query_device NEAREST on the same rays) and the host parity hooks.

    python tools/raycast_bench.py [--reps 20] [--warmup 3] [--out FILE]

Ray sets (a) primary, (b) bounce, (c) shadow: tools/query_bench.py's ray_sets (sponza260k, 1920x1080 bench camera),
over the reference tree and over PLOC.  Per set: vmx_raycast_device with the quad-cooperative and the per-lane record
fetch, NEAREST alone (quad / lane), and the wall time of the host vmx_raycast (copies and allocation included).  Per
tree: the camera G-buffer vmx_raycast_camera_device at k = 0 against the wall time of vmx_primary_ids.  Device times:
torch CUDA events around one call, median of --reps after --warmup (min / max in brackets).  Every device result is
first checked against the host hook, word for word."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vermilion_amd as va  # noqa: E402
from vermilion_amd import scenes  # noqa: E402
from query_bench import ray_sets  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def same_words(dev_raw, host):
    a = dev_raw.cpu().numpy().reshape(-1, 16).view(np.uint32)
    b = np.ascontiguousarray(host).view(np.uint32).reshape(-1, 16)
    af, bf = a.view(np.float32), b.view(np.float32)
    return bool(np.all((a == b) | (np.isnan(af) & np.isnan(bf))))


def fmt(tag, t):
    return f" | {tag} {t[0]:7.3f} ms [{t[1]:.3f} {t[2]:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raycast_bench: no GPU (nothing is measured on the CPU)")
    W, H = args.width, args.height
    lines = [f"# tools/raycast_bench.py: sponza260k, {W}x{H} bench camera, median of {args.reps} after {args.warmup} "
             f"warm-up calls (min / max in brackets); {torch.cuda.get_device_name(0)}"]
    pos, nrm, uv = scenes.sponza260k()
    torch.cuda.set_stream(torch.cuda.Stream())  # an explicit stream: the events and the calls share it
    c = scenes.sponza_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], W, H, 4, back_size=(3.6, 3.6 * H / W))
    opts = va.make_opts(seed=1)
    for bname, builder in (("reference", va._lib.VMX_BVH_REFERENCE), ("ploc", va._lib.VMX_BVH_PLOC)):
        with va.Scene(pos, nrm, uv, builder=builder) as sc:
            for sname, (o, d, _) in ray_sets(sc, W, H).items():
                n = len(o)
                t0 = time.perf_counter()
                host = sc.raycast(o, d)
                host_ms = (time.perf_counter() - t0) * 1e3
                O_, D_ = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
                for per_lane in (False, True):
                    r = sc.raycast(O_, D_, per_lane_fetch=per_lane)
                    torch.cuda.synchronize()
                    assert same_words(r["raw"], host), (bname, sname, per_lane)
                row = f"{bname:9s} {sname:9s} n={n:8d}"
                for per_lane in (False, True):
                    tag = "lane" if per_lane else "quad"
                    rc = timed(lambda: sc.raycast(O_, D_, per_lane_fetch=per_lane), args.reps, args.warmup)
                    nq = timed(lambda: sc.query(O_, D_, per_lane_fetch=per_lane), args.reps, args.warmup)
                    row += fmt(f"raycast/{tag}", rc) + fmt(f"nearest/{tag}", nq) + f" tail {rc[0] - nq[0]:6.3f} ms"
                row += f" | host vmx_raycast {host_ms:8.1f} ms wall"
                print(row, flush=True)
                lines.append(row)
            t0 = time.perf_counter()
            tri, t = sc.primary_ids(cam, opts, 0)
            host_ms = (time.perf_counter() - t0) * 1e3
            row = f"{bname:9s} camera    n={W * H:8d}"
            for per_lane in (False, True):
                g = sc.raycast_camera(cam, opts, 0, per_lane_fetch=per_lane)
                torch.cuda.synchronize()
                assert np.array_equal(g["tri_id"].cpu().numpy().reshape(-1), tri), (bname, per_lane)
                assert np.array_equal(g["tri_t"].cpu().numpy().reshape(-1).view(np.uint32), t.view(np.uint32))
                gb = timed(lambda: sc.raycast_camera(cam, opts, 0, per_lane_fetch=per_lane), args.reps, args.warmup)
                row += fmt(f"gbuffer/{'lane' if per_lane else 'quad'}", gb)
            row += f" | host vmx_primary_ids {host_ms:8.1f} ms wall"
            print(row, flush=True)
            lines.append(row)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
