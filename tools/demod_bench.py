#!/usr/bin/env python3
"""What albedo-demodulated denoising costs: the albedo plane against the loop of camera raycasts it replaces, and the
demodulated filter call beside the plain one.

    python tools/demod_bench.py [--reps 20] [--sizes 1920x1080,3840x2160] [--spp 16] [--out FILE]

The bench scene (sponza260k, bench camera, seed 1) with a 256 x 256 x 3 checker bound; the frame is a progressive
handle's preview with 4 samples in.  Everything is timed with torch CUDA event pairs on the stream the work runs on,
median of `reps` after 3 warm-up calls (min / max in brackets), all in one run:
  - Scene.albedo_camera (vmx_albedo_camera_device) for 1, 4 and 16 samples, and beside each the same number of
    Scene.raycast_camera calls (vmx_raycast_camera_device), with its default record fetch and with
    VMX_QUERY_FETCH_PER_LANE (the form the plane's query uses) — what a caller had to do before the entry existed,
    without yet the pass over the records that samples the texture.
  - Filter.apply at the defaults and at iterations = 1, rgbaz + rgba8 out, plain and with albedo= (a pre-pass divides, the last
    iteration multiplies).
  - the filtered preview, plain and demodulated (the handle's plane is built before the timing).
Model bytes: the plane's least traffic is per pixel and sample the 8 B the query leaves and the finish reads back, and
16 B of plane written once (read and written between samples: 32 B per further sample); the raycast loop writes 64 B
per pixel and sample after the same 8.  The filter's model is tools/filter_bench.py's plus, for the pre-pass, 20 B of frame and
16 B of albedo read and 16 B written, minus the 4 B by which a plane is smaller than the frame the first iteration would
have read, and 16 B of albedo in the last iteration."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vermilion_amd as va  # noqa: E402
from vermilion_amd import scenes  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, as bench.py


def filter_bytes(npix, iterations, rgbaz, rgba8, demod):
    per_pixel = 0
    for it in range(iterations):
        per_pixel += 16 + (20 if it == 0 else 16)
        if it + 1 == iterations:
            per_pixel += (20 if rgbaz else 0) + (4 if rgba8 else 0)
        else:
            per_pixel += 16
    if demod:
        per_pixel += (20 + 16 + 16) - 4 + 16
    return npix * per_pixel


def checker(n=256):
    y, x = np.mgrid[0:n, 0:n]
    chk = ((x // 8 + y // 8) & 1).astype(np.float32)
    return np.ascontiguousarray(np.stack([0.25 + 0.7 * chk, 0.9 - 0.6 * chk, 0.3 + 0.5 * ((x // 4) & 1)], axis=-1), np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("demod_bench: no GPU (nothing is measured on the CPU)")
    lines = [f"# tools/demod_bench.py: sponza260k with a 256x256x3 checker bound, {args.spp} spp target, 4 samples in, seed 1; "
             f"torch CUDA event pairs, median of {args.reps} after 3 warm-up calls (min / max in brackets); "
             f"{torch.cuda.get_device_name(0)}"]

    def emit(row):
        print(row, flush=True)
        lines.append(row)

    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the handle, the filter and the events share this stream

    def timed(fn):
        ms = []
        for i in range(args.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    def row(tag, t, nbytes):
        rate = nbytes / (t[0] * 1e-3) / 1e9
        emit(f"  {tag:58s} {t[0] * 1e3:9.1f} us [{t[1] * 1e3:.1f} {t[2] * 1e3:.1f}]  model {nbytes / 1e6:7.1f} MB = "
             f"{rate:7.1f} GB/s ({rate / HBM_PEAK_GBS:.1%} of {HBM_PEAK_GBS:.0f} GB/s)")

    pos, nrm, uv = scenes.sponza260k()
    c = scenes.sponza_camera()
    with va.Scene(pos, nrm, uv) as sc:
        sc.bind_texture(checker())
        for size in args.sizes.split(","):
            W, H = (int(v) for v in size.split("x"))
            npix = W * H
            cam = va.make_camera(c["position"], c["rotation_deg"], W, H, args.spp, back_size=(3.6, 3.6 * H / W))
            opts = va.make_opts(seed=1, early_stop=False)
            emit(f"{W}x{H}")
            plane = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
            for n in (1, 4, 16):
                if n > 4 * (args.spp // 4):
                    continue
                t_plane = timed(lambda: sc.albedo_camera(cam, opts, samples=n, out=plane, stream=stream))
                row(f"albedo plane, {n:2d} samples", t_plane, npix * (8 * n + 16 + 32 * (n - 1)))

                for tag, per_lane in (("default fetch", False), ("per-lane fetch", True)):
                    def loop():
                        for k in range(n):  # (each record tensor comes from torch's caching allocator)
                            sc.raycast_camera(cam, opts, k, stream=stream, per_lane_fetch=per_lane)

                    t_loop = timed(loop)
                    row(f"  {n:2d} x raycast_camera, {tag} (no texture pass yet)", t_loop, npix * (8 + 64) * n)
                    emit(f"    plane / loop = {t_plane[0] / t_loop[0]:.3f}")
            d5 = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
            o5 = torch.empty_like(d5)
            o4 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
            with sc.progressive(cam, opts, stream=stream) as p, va.Filter(W, H) as f:
                p.step(4)
                p.preview_device(d5)
                f.set_guide(sc.raycast_camera(cam, opts, 0, stream=stream)["raw"], stream=stream)
                sc.albedo_camera(cam, opts, samples=4, out=plane, stream=stream)
                stream.synchronize()
                for k in (5, 1):
                    prm = va.make_filter_params(iterations=k)
                    t_plain = timed(lambda: f.apply(d5, out=o5, rgba8=o4, params=prm, stream=stream))
                    row(f"apply, iterations {k}, plain", t_plain, filter_bytes(npix, k, True, True, False))
                    t_demod = timed(lambda: f.apply(d5, out=o5, rgba8=o4, params=prm, stream=stream, albedo=plane))
                    row(f"apply, iterations {k}, demodulated", t_demod, filter_bytes(npix, k, True, True, True))
                    t_again = timed(lambda: f.apply(d5, out=o5, rgba8=o4, params=prm, stream=stream))
                    row(f"apply, iterations {k}, plain again", t_again, filter_bytes(npix, k, True, True, False))
                    emit(f"    demodulation adds {(t_demod[0] - t_plain[0]) * 1e3:+.1f} us ({t_demod[0] / t_plain[0]:.3f} x)")
                p.preview_filtered_device(o5, o4, albedo_samples=4)  # builds the handle's guide and plane
                stream.synchronize()
                t = timed(lambda: p.preview_filtered_device(o5, o4))
                row("filtered preview, defaults, plain", t, filter_bytes(npix, 5, True, True, False) + 4 * npix)
                t = timed(lambda: p.preview_filtered_device(o5, o4, albedo_samples=4))
                row("filtered preview, defaults, demodulated", t, filter_bytes(npix, 5, True, True, True) + 4 * npix)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
