#!/usr/bin/env python3
"""What changing the lights costs: vmx_scene_set_spheres against making the scene again, and k_motion_spheres against
k_motion and a byte model.

    python tools/spheres_bench.py [--reps 20] [--create-reps 3] [--sizes 1920x1080,3840x2160] [--out FILE]

The bench scene (sponza260k, bench camera).
  - vmx_scene_set_spheres alternating between two tables (the reference's, and that with the small light moved and the
    big one dimmed), and, for the same change, vmx_scene_destroy + vmx_scene_create_ex with the new table: host wall
    clock around each call (both return once the scene is ready), median (min / max in brackets).  The first render
    after either is not in the figure.
  - per size, on the G-buffer of the bench camera, torch CUDA event pairs on the stream the work runs on, median of
    `reps` after 3 warm-up calls: vmx_motion_spheres_device (k_motion_spheres) standing alone, after motion records
    (d_motion_in given) and in place, under tables between which the small light moved and the floor sphere sank;
    and in the same run vmx_motion_device (k_motion), the previous positions being the scene's own moved by
    (0.5, 0, 0.3).  Models: 64 B read + 32 B written per record, + 32 B read with d_motion_in; k_motion's gathers by
    tri_id and the sphere tables (kernel arguments) are not counted.  The bench camera's rays all end on triangles, which
    times the kernel's pass-through path.  The sphere loop and the rewrite are timed per size on a G-buffer whose every
    record lies on a sphere (the Cornell set's room seen from behind its camera): under the same tables, where that wall
    did not move and no record is rewritten, and under tables in which all six walls moved and every record is.
There are no thresholds here: the figures go to profiles/spheres_bench.txt."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vermilion_amd as va  # noqa: E402
from vermilion_amd import scenes  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, as bench.py


def relit():
    """the reference's table with the small light 40 units along and the big one at a quarter"""
    t = va.default_spheres()
    t[0].centre[:] = [t[0].centre[0] + 40.0, t[0].centre[1], t[0].centre[2]]
    t[1].colour[:] = [c * 0.25 for c in t[1].colour]
    return t


def moved_pair():
    """(now, prev): the small light moved by (12, -5, -7) and the floor sphere sunk by 8 between them"""
    now, prev = va.default_spheres(), va.default_spheres()
    prev[0].centre[:] = [now[0].centre[0] - 12.0, now[0].centre[1] + 5.0, now[0].centre[2] + 7.0]
    prev[2].centre[:] = [now[2].centre[0], now[2].centre[1] + 8.0, now[2].centre[2]]
    prev[2].normal_centre[:] = list(prev[2].centre)
    return now, prev


def walls_moved():
    """(now, prev): the reference's table, and that with each of the six wall spheres 8 units further out along its axis"""
    now, prev = va.default_spheres(), va.default_spheres()
    for i in range(2, 8):
        c = list(now[i].centre)
        k = max(range(3), key=lambda a: abs(c[a]))
        c[k] += 8.0 if c[k] > 0 else -8.0
        prev[i].centre[:] = c
        prev[i].normal_centre[:] = c
    return now, prev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--create-reps", type=int, default=3)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spheres_bench: no GPU (nothing is measured on the CPU)")
    lines = [f"# tools/spheres_bench.py: sponza260k; host wall clock for the scene calls, torch CUDA event pairs for the "
             f"kernels, median of {args.reps} after 3 warm-up calls (min / max in brackets); {torch.cuda.get_device_name(0)}"]

    def emit(row):
        print(row, flush=True)
        lines.append(row)

    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)

    def timed(fn):
        ms = []
        for i in range(args.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn(i)
            e1.record(stream)
            e1.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    def row(tag, t, nbytes):
        rate = nbytes / (t[0] * 1e-3) / 1e9
        emit(f"  {tag:58s} {t[0] * 1e3:8.1f} us [{t[1] * 1e3:.1f} {t[2] * 1e3:.1f}]  model {nbytes / 1e6:7.1f} MB = "
             f"{rate:7.1f} GB/s ({rate / HBM_PEAK_GBS:.1%} of {HBM_PEAK_GBS:.0f} GB/s)")
        return rate

    def wall(fn, reps):
        ms = []
        for i in range(reps):
            t0 = time.perf_counter()
            fn(i)
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    pos, nrm, uv = scenes.sponza260k()
    c = scenes.sponza_camera()
    tables = [va.default_spheres(), relit()]
    emit(f"the sphere table of a live scene, {pos.reshape(-1, 9).shape[0]} triangles")
    sc = va.Scene(pos, nrm, uv)
    cam = va.make_camera(c["position"], c["rotation_deg"], 64, 64, 16)
    sc.render(cam, va.make_opts(seed=1))  # (the workspace exists: what a live scene looks like)
    t = wall(lambda i: sc.set_spheres(tables[(i + 1) % 2]), args.reps + 3)
    emit(f"  vmx_scene_set_spheres                                      {t[0] * 1e3:10.1f} us [{t[1] * 1e3:.1f} {t[2] * 1e3:.1f}]")
    set_ms = t[0]

    def recreate(i):
        nonlocal sc
        sc.close()
        sc = va.Scene(pos, nrm, uv, spheres=tables[(i + 1) % 2])

    t = wall(recreate, args.create_reps)
    emit(f"  vmx_scene_destroy + vmx_scene_create_ex with the new table {t[0] * 1e3:10.1f} us [{t[1] * 1e3:.1f} {t[2] * 1e3:.1f}]"
         f"  = {t[0] / set_ms:.0f} x")
    sc.set_spheres(None)

    d_pos = torch.from_numpy(pos).cuda()
    d_prev = (d_pos.view(-1, 3) + torch.tensor([0.5, 0.0, 0.3], device="cuda")).view(-1, 9).contiguous()
    now, prev = moved_pair()
    sc.set_spheres(now)
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        npix = W * H
        emit(f"{W}x{H}")
        cam = va.make_camera(c["position"], c["rotation_deg"], W, H, 16, back_size=(3.6, 3.6 * H / W))
        raw = sc.raycast_camera(cam, va.make_opts(seed=1), 0, stream=stream)["raw"]
        stream.synchronize()
        mv = torch.empty((H, W, 8), dtype=torch.float32, device="cuda")
        out = torch.empty((H, W, 8), dtype=torch.float32, device="cuda")
        tm = timed(lambda i: va.motion_vectors(raw, d_pos, d_prev, out=mv, stream=stream))
        base = row("vmx_motion_device (k_motion), no normals", tm, npix * 96)
        tm = timed(lambda i: va.sphere_motion_vectors(raw, c["position"], now, prev, out=out, stream=stream))
        alone = row("vmx_motion_spheres_device (k_motion_spheres), alone", tm, npix * 96)
        flags = out.view(torch.int32)[..., 3] & 1
        tm = timed(lambda i: va.sphere_motion_vectors(raw, c["position"], now, prev, motion=mv, out=out, stream=stream))
        row("vmx_motion_spheres_device, after vmx_motion_device's records", tm, npix * 128)
        tm = timed(lambda i: va.sphere_motion_vectors(raw, c["position"], now, prev, motion=mv, out=mv, stream=stream))
        row("vmx_motion_spheres_device, in place", tm, npix * 128)
        words = raw.view(torch.int32)
        sphere = ((words[..., 11] & 1) != 0) & ~((words[..., 7] >= 0) & (raw[..., 3] == raw[..., 10]))
        emit(f"  {float(sphere.float().mean()):.1%} of the records lie on a sphere, {float(flags.float().mean()):.1%} are rewritten; "
             f"k_motion_spheres alone reaches {alone / base:.2f} x the model rate of k_motion")
    sc.close()
    # the bench camera sees triangles only, so the rows above time the pass-through path; the sphere loop and the rewrite
    # are timed on the Cornell set seen from behind its camera, where every ray ends on a wall sphere of the room: under
    # the tables above (that wall did not move: the loop runs, nothing is rewritten) and under tables in which all six
    # walls moved (every record is rewritten)
    cpos, cnrm, cuv = scenes.cornell8()
    cc = scenes.cornell_camera()
    walls_now, walls_prev = walls_moved()
    with va.Scene(cpos, cnrm, cuv, spheres=now) as room:
        for size in args.sizes.split(","):
            W, H = (int(v) for v in size.split("x"))
            npix = W * H
            cam = va.make_camera(cc["position"], (0.0, 180.0, 0.0), W, H, 16, back_size=(3.6, 3.6 * H / W))
            raw = room.raycast_camera(cam, va.make_opts(seed=1), 0, stream=stream)["raw"]
            stream.synchronize()
            out = torch.empty((H, W, 8), dtype=torch.float32, device="cuda")
            words = raw.view(torch.int32)
            sphere = ((words[..., 11] & 1) != 0) & ~((words[..., 7] >= 0) & (raw[..., 3] == raw[..., 10]))
            emit(f"{W}x{H}, the Cornell set's room seen from behind its camera: {float(sphere.float().mean()):.1%} of the "
                 f"records lie on a sphere")
            for tag, a, b in (("that wall unmoved", now, prev), ("all six walls moved", walls_now, walls_prev)):
                tm = timed(lambda i: va.sphere_motion_vectors(raw, cc["position"], a, b, out=out, stream=stream))
                row(f"vmx_motion_spheres_device alone, {tag}", tm, npix * 96)
                flags = out.view(torch.int32)[..., 3] & 1
                emit(f"    {float(flags.float().mean()):.1%} of the records are rewritten")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
