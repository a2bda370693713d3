#!/usr/bin/env python3
"""What the G-buffer-guided filter costs: per call, per iteration, against its byte model and against a plain preview.

    python tools/filter_bench.py [--reps 20] [--sizes 1920x1080,3840x2160] [--spp 16] [--out FILE]

The bench scene (sponza260k, bench camera, seed 1), a progressive handle with 4 samples in, so the frame is the noisy
one a preview shows.  Everything is timed with torch CUDA event pairs on the stream the work runs on, median of `reps`
after 3 warm-up calls (min / max in brackets):
  - vmx_filter_apply_device on the preview's RGBAZ frame with iterations = 1 .. 5, rgbaz + rgba8 out.  A call of k
    iterations is k launches of k_atrous; `+` is what the k-th iteration (step 2^(k-1)) added to the call.
  - the whole call at the defaults: rgbaz alone, rgba8 alone, both, in place.
  - vmx_progressive_preview_filtered_device (the first iteration reads the pixel state) beside
    vmx_progressive_preview_device (k_preview alone) on the same handle.
Achieved bytes per second are against the least traffic the filter needs: per pixel and iteration 16 B of guide, 16 B of
colour read and 16 B written; the first iteration reads and the last writes 20 B instead, plus 4 B where rgba8 is
written.  The taps' re-reads are served by the caches and are not in the model."""
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


def model_bytes(npix, iterations, rgbaz, rgba8):
    per_pixel = 0
    for it in range(iterations):
        per_pixel += 16 + (20 if it == 0 else 16)
        if it + 1 == iterations:
            per_pixel += (20 if rgbaz else 0) + (4 if rgba8 else 0)
        else:
            per_pixel += 16
    return npix * per_pixel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("filter_bench: no GPU (nothing is measured on the CPU)")
    lines = [f"# tools/filter_bench.py: sponza260k, {args.spp} spp target, 4 samples in, seed 1; torch CUDA event pairs, "
             f"median of {args.reps} after 3 warm-up calls (min / max in brackets); {torch.cuda.get_device_name(0)}"]

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
        emit(f"  {tag:58s} {t[0] * 1e3:8.1f} us [{t[1] * 1e3:.1f} {t[2] * 1e3:.1f}]  model {nbytes / 1e6:7.1f} MB = "
             f"{rate:7.1f} GB/s ({rate / HBM_PEAK_GBS:.1%} of {HBM_PEAK_GBS:.0f} GB/s)")

    pos, nrm, uv = scenes.sponza260k()
    c = scenes.sponza_camera()
    with va.Scene(pos, nrm, uv) as sc:
        for size in args.sizes.split(","):
            W, H = (int(v) for v in size.split("x"))
            npix = W * H
            cam = va.make_camera(c["position"], c["rotation_deg"], W, H, args.spp, back_size=(3.6, 3.6 * H / W))
            opts = va.make_opts(seed=1, early_stop=False)
            emit(f"{W}x{H}")
            d5 = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
            o5 = torch.empty_like(d5)
            o4 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
            with sc.progressive(cam, opts, stream=stream) as p, va.Filter(W, H) as f:
                p.step(4)
                p.preview_device(d5)
                f.set_guide(sc.raycast_camera(cam, opts, 0, stream=stream)["raw"], stream=stream)
                stream.synchronize()
                prev = 0.0
                for k in range(1, 6):
                    prm = va.make_filter_params(iterations=k)
                    t = timed(lambda: f.apply(d5, out=o5, rgba8=o4, params=prm, stream=stream))
                    row(f"apply, iterations {k} (step {1 << (k - 1):2d} added {(t[0] - prev) * 1e3:+7.1f} us)", t,
                        model_bytes(npix, k, True, True))
                    prev = t[0]
                for tag, kw in (("rgbaz", dict(out=o5)), ("rgba8", dict(rgba8=o4)), ("rgbaz + rgba8", dict(out=o5, rgba8=o4))):
                    t = timed(lambda: f.apply(d5, stream=stream, **kw))
                    row(f"apply, defaults, {tag}", t, model_bytes(npix, 5, "out" in kw, "rgba8" in kw))
                inplace = d5.clone()
                t = timed(lambda: f.apply(inplace, out=inplace, stream=stream))
                row("apply, defaults, in place (rgbaz)", t, model_bytes(npix, 5, True, False))
                for tag, a, b in (("rgbaz", o5, None), ("rgbaz + rgba8", o5, o4), ("rgba8", None, o4)):
                    t = timed(lambda: p.preview_device(a, b))
                    row(f"k_preview alone, {tag}", t, npix * (24 + (20 if a is not None else 0) + (4 if b is not None else 0)))
                    t = timed(lambda: p.preview_filtered_device(a, b))
                    # the first iteration reads the state (24 B) instead of a frame (20 B)
                    row(f"filtered preview, defaults, {tag}", t, model_bytes(npix, 5, a is not None, b is not None) + 4 * npix)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
