#!/usr/bin/env python3
"""In-place geometry updates (vmx_scene_update*, vmx_update.inc) on the bench scene: what a moving scene costs per
frame, against destroying and creating it again.

    python tools/update_bench.py [--reps 20] [--warmup 3] [--spp 64] [--out FILE]

sponza260k (256,152 triangles), median of --reps calls after --warmup (min / max in brackets):
  refit/device   vmx_scene_update_device REFIT, positions already on the device: torch CUDA events on the stream
  refit/host     vmx_scene_update REFIT from host arrays: wall time (upload + refit + synchronise)
  rebuild/device vmx_scene_update_device REBUILD (LBVH, PLOC): events on the stream and wall time (it blocks)
  recreate       destroy + vmx_scene_create_ex + the first render of a small frame (256x144x16), wall time; the
                 render alone on a warm scene beside it
  frame          the headline-form frame (reserved[0] bit 8, fixed spp) of the bench camera after a moderate
                 deformation, once refitted and once rebuilt: what a refit costs in traversal quality"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vermilion_amd as va  # noqa: E402
from vermilion_amd import _lib as L  # noqa: E402
from vermilion_amd import scenes  # noqa: E402

BUILDERS = {"reference": L.VMX_BVH_REFERENCE, "sah": L.VMX_BVH_SAH, "lbvh": L.VMX_BVH_LBVH, "ploc": L.VMX_BVH_PLOC}


def deform(pos, amp, phase=0.0):
    v = np.asarray(pos, np.float64).reshape(-1, 3)
    ext = float((v.max(axis=0) - v.min(axis=0)).max())
    k = 12.0 / ext
    d = np.stack([np.sin(k * v[:, 1] + phase), np.cos(k * v[:, 2] + 2 * phase), np.sin(k * v[:, 0] - phase)], axis=1)
    return (v + amp * ext * d).astype(np.float32).reshape(-1, 9)


def stats(xs):
    xs = sorted(xs)
    return f"{xs[len(xs) // 2]:8.3f} ms [{xs[0]:.3f} {xs[-1]:.3f}]"


def timed_device(fn, reps, warmup, stream):
    out = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn(i)
        b.record(stream)
        b.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return out


def timed_wall(fn, reps, warmup):
    out = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(i)
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spp", type=int, default=64, help="samples per pixel of the headline-form frames")
    ap.add_argument("--amp", type=float, default=0.005, help="deformation amplitude, fraction of the scene's extent")
    ap.add_argument("--skip-frames", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pos, nrm, uv = scenes.sponza260k()
    geo = [deform(pos, args.amp, 0.0), deform(pos, args.amp, 1.0)]
    d_geo = [torch.from_numpy(g).to(dev) for g in geo]
    s = torch.cuda.Stream(dev)
    lines = [f"# tools/update_bench.py: sponza260k ({pos.shape[0]} triangles), median of {args.reps} after {args.warmup} "
             f"warm-up calls (min / max in brackets); {torch.cuda.get_device_name(0)}"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    for name, b in BUILDERS.items():
        with va.Scene(pos, nrm, uv, builder=b) as sc:
            d = sc.describe()
            sc.update(pos=d_geo[1], stream=s)  # the first update derives the refit plan
            torch.cuda.synchronize()
            dt = timed_device(lambda i: sc.update(pos=d_geo[i % 2], stream=s), args.reps, args.warmup, s)
            ht = timed_wall(lambda i: sc.update(pos=geo[i % 2]), args.reps, args.warmup)
            emit(f"{name:9s} levels={d['max_depth'] + 1:3d} | refit/device {stats(dt)} | refit/host {stats(ht)} wall")
            if name in ("lbvh", "ploc"):
                rd = timed_device(lambda i: sc.update(pos=d_geo[i % 2], rebuild=True, stream=s), args.reps, args.warmup, s)
                rw = timed_wall(lambda i: sc.update(pos=d_geo[i % 2], rebuild=True, stream=s), args.reps, args.warmup)
                emit(f"{name:9s} rebuild/device {stats(rd)} on the stream | {stats(rw)} wall")
    c = scenes.sponza_camera()
    cam_s = va.make_camera(c["position"], c["rotation_deg"], 256, 144, 16, back_size=(3.6, 3.6 * 144 / 256))
    opts_s = va.make_opts(seed=1)
    for name, b in BUILDERS.items():
        keep = [va.Scene(pos, nrm, uv, builder=b)]

        def recreate(i):
            keep[0].close()
            keep[0] = va.Scene(geo[i % 2], nrm, uv, builder=b)
            keep[0].render(cam_s, opts_s)

        rt = timed_wall(recreate, max(3, args.reps // 4), 1)
        warm = timed_wall(lambda i: keep[0].render(cam_s, opts_s), max(3, args.reps // 4), 1)
        keep[0].close()
        emit(f"{name:9s} recreate = destroy + create + first 256x144x16 render {stats(rt)} wall | render alone {stats(warm)}")
    if not args.skip_frames:
        W, H = 1920, 1080
        cam = va.make_camera(c["position"], c["rotation_deg"], W, H, args.spp, back_size=(3.6, 3.6 * H / W))
        opts = va.make_opts(seed=1, early_stop=False, pipeline=0x100)
        moved = deform(pos, 4 * args.amp, 2.0)
        for name in ("reference", "lbvh", "ploc"):
            with va.Scene(pos, nrm, uv, builder=BUILDERS[name]) as sc:
                res = {}
                for how in ("fresh", "refit", "rebuild"):
                    if how == "refit":
                        sc.update(pos=moved)
                    elif how == "rebuild":
                        sc.update(pos=moved, rebuild=True)
                    sc.render(cam, opts)
                    res[how] = [sc.render(cam, opts)[1]["ms_device"] for _ in range(3)]
                emit(f"{name:9s} headline form {W}x{H}x{args.spp}: original geometry {min(res['fresh']):8.2f} ms | "
                     f"deformed x{4 * args.amp:g}: refitted {min(res['refit']):8.2f} ms, rebuilt {min(res['rebuild']):8.2f} ms")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
