#!/usr/bin/env python3
"""What a progressive render costs over the one blocking call, and what a preview costs.

    python tools/progressive_bench.py [--reps 3] [--width 1920 --height 1080 --spp 256] [--out FILE]

The bench scene (sponza260k, bench camera, fixed count, seed 1, bench.py's headline form).  One vmx_render against a
vmx_progressive handle stepped by spp, 64, 16 and 4 samples, each with and without a device preview (rgbaz + rgba8)
after every step: total wall ms of the frame (begin to the last step's return, previews enqueued in between and waited
for at the end) and ms per step.  The difference to the one call, divided by the steps, is a step's fixed cost: the
workspace binding and camera tables, a launch chain that no longer amortises, one host synchronisation per pass.
Then the preview kernel alone: torch CUDA events around one vmx_progressive_preview_device on the handle's stream,
median of 20 after 3, for a half-finished and a finished frame, beside its byte model — after 2 GiB of other traffic
(as after a step: the state comes from HBM) and back to back (the 0.1 GB of state and frame still in the 256 MB
Infinity Cache).  Every stepped frame is first checked against the one call's, bit for bit."""
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

HEADLINE_FORM = 0x100   # bench.py's: every Radiance step shaded in full
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak, as bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("progressive_bench: no GPU (nothing is measured on the CPU)")
    W, H, spp = args.width, args.height, args.spp
    lines = [f"# tools/progressive_bench.py: sponza260k, {W}x{H}x{spp} spp fixed count, seed 1, pipeline 0x100; "
             f"median of {args.reps} frames after one warm-up frame (min / max in brackets); {torch.cuda.get_device_name(0)}"]

    def emit(row):
        print(row, flush=True)
        lines.append(row)

    pos, nrm, uv = scenes.sponza260k()
    c = scenes.sponza_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], W, H, spp, back_size=(3.6, 3.6 * H / W))
    opts = va.make_opts(seed=1, early_stop=False, pipeline=HEADLINE_FORM)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the handle, the previews and the events share this stream
    d5 = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
    d4 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    with va.Scene(pos, nrm, uv) as sc:
        def one_call():
            t0 = time.perf_counter()
            sc.render_device(cam, opts, d5.data_ptr(), stream.cuda_stream)
            return (time.perf_counter() - t0) * 1e3, 1

        def stepped(samples, preview):
            t0 = time.perf_counter()
            steps = 0
            with sc.progressive(cam, opts, stream=stream) as p:
                while p.info()["pixels_active"]:
                    p.step(samples)
                    steps += 1
                    if preview:
                        p.preview_device(d5, d4)
                stream.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                if not preview:
                    p.preview_device(d5)
                    stream.synchronize()
            return ms, steps

        def measure(fn):
            fn()
            runs = [fn() for _ in range(args.reps)]
            ms = [r[0] for r in runs]
            return float(np.median(ms)), float(np.min(ms)), float(np.max(ms)), runs[0][1]

        base = measure(one_call)
        ref = d5.cpu().numpy().view(np.uint32).copy()
        emit(f"vmx_render_device (one call)      total {base[0]:9.2f} ms [{base[1]:.2f} {base[2]:.2f}]")
        for samples in (spp, 64, 16, 4):
            for preview in (False, True):
                t = measure(lambda: stepped(samples, preview))
                assert np.array_equal(d5.cpu().numpy().view(np.uint32), ref), (samples, preview)
                emit(f"step {samples:4d} x {t[3]:3d} {'+ preview' if preview else '         '}          total {t[0]:9.2f} ms "
                     f"[{t[1]:.2f} {t[2]:.2f}]  per step {t[0] / t[3]:8.3f} ms  over one call {t[0] - base[0]:+8.2f} ms "
                     f"({(t[0] - base[0]) / t[3]:+.3f} ms per step)")

        # the preview kernel alone
        flush = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")  # 1 GiB: four times the 256 MB Infinity Cache

        def kernel_ms(p, a, b, cold):
            ms = []
            for i in range(23):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if cold:
                    flush.add_(1.0)  # what a step's passes do to the caches: the state comes from HBM
                e0.record(stream)
                p.preview_device(a, b)
                e1.record(stream)
                e1.synchronize()
                if i >= 3:
                    ms.append(e0.elapsed_time(e1))
            return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

        npix = W * H
        with sc.progressive(cam, opts, stream=stream) as p:
            for state, finished in (("half-finished frame", False), ("finished frame", True)):
                p.step(0 if finished else spp // 2)
                for tag, a, b in (("rgbaz", d5, None), ("rgbaz + rgba8", d5, d4), ("rgba8", None, d4)):
                    t, hot = kernel_ms(p, a, b, True), kernel_ms(p, a, b, False)
                    # read: accum 16 + count 4 + cursor 4 of an unfinished pixel, cursor 4 + frame 20 of a finished one (the
                    # fixed-count frame has no finished pixel before its last pass); written: 20 and / or 4
                    nbytes = npix * (24 + (20 if a is not None else 0) + (4 if b is not None else 0))
                    emit(f"k_preview {state:20s} {tag:14s} {t[0] * 1e3:8.1f} us [{t[1] * 1e3:.1f} {t[2] * 1e3:.1f}]  "
                         f"{nbytes / 1e6:6.1f} MB moved = {nbytes / (t[0] * 1e-3) / 1e9:7.1f} GB/s "
                         f"({nbytes / (t[0] * 1e-3) / 1e9 / HBM_PEAK_GBS:.1%} of {HBM_PEAK_GBS:.0f} GB/s) | "
                         f"back to back, state still in the Infinity Cache: {hot[0] * 1e3:6.1f} us")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
