#!/usr/bin/env python3
"""What temporal accumulation costs: per call, against its byte model, beside one a-trous iteration at the same size.

    python tools/temporal_bench.py [--reps 20] [--sizes 1920x1080,3840x2160] [--spp 16] [--out FILE]

The bench scene (sponza260k, bench camera, seeds 1 and 2), two 4-sample previews of a progressive handle each at two
cameras a slow pan apart, so the frames are the noisy ones a preview shows and the reprojection is a real one.
Everything is timed with torch CUDA event pairs on the stream the work runs on, median of `reps` after 3 warm-up calls
(min / max in brackets):
  - vmx_temporal_accumulate_device alternating between the two cameras (every call after the first reprojects): rgbaz
    alone, rgbaz + rgba8, rgbaz + rgba8 + history lengths, in place; and the first call after a reset (no history read).
  - in the same run, vmx_filter_apply_device with iterations = 1 on the same frame (rgbaz + rgba8), with its model rate
    as tools/filter_bench.py counts it: the rate the temporal kernel is expected to reach at least.
Achieved bytes per second are against the least traffic a call needs, per pixel: 64 B record + 20 B frame + 48 B old
state read, 48 B new state + 20 B frame written (+ 4 B rgba8, + 4 B history length); a first call reads no state.  The
four taps' re-reads are served by the caches and are not in the model.
  - the motion leg: vmx_motion_device alone (k_motion) on the second camera's G-buffer, with and without previous normals,
    the previous positions being the scene's own moved by (0.5, 0, 0.3) — every record on a triangle is flagged — and
    vmx_temporal_accumulate_motion_device with those records (rgbaz + rgba8), the call without them timed beside it.
    Models: the motion call reads 32 B per pixel more; k_motion reads the 64 B record and writes 32 B per record.  Its
    gathers by tri_id (two or three times 36 B per record, neighbouring pixels mostly the same triangle: served by the
    caches) are not in the model."""
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


def model_bytes(npix, first=False, rgbaz=True, rgba8=False, history=False):
    per_pixel = 64 + 20 + (0 if first else 48) + 48 + (20 if rgbaz else 0) + (4 if rgba8 else 0) + (4 if history else 0)
    return npix * per_pixel


def motion_model_bytes(npix):
    """vmx_motion_device: the record read, the motion record written; the gathers by tri_id are not counted"""
    return npix * (64 + 32)


def filter_model_bytes(npix):
    """one iteration of vmx_filter_apply_device with both outputs, as tools/filter_bench.py's model_bytes(npix, 1, True, True)"""
    return npix * (16 + 20 + 20 + 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("temporal_bench: no GPU (nothing is measured on the CPU)")
    lines = [f"# tools/temporal_bench.py: sponza260k, {args.spp} spp target, 4 samples in, seeds 1 and 2, two cameras a slow "
             f"pan apart; torch CUDA event pairs, median of {args.reps} after 3 warm-up calls (min / max in brackets); "
             f"{torch.cuda.get_device_name(0)}"]

    def emit(row):
        print(row, flush=True)
        lines.append(row)

    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the handles and the events share this stream

    def timed(fn, before=None):
        ms = []
        for i in range(args.reps + 3):
            if before is not None:
                before()
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

    pos, nrm, uv = scenes.sponza260k()
    c = scenes.sponza_camera()
    d_pos, d_nrm = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
    d_prev = (d_pos.view(-1, 3) + torch.tensor([0.5, 0.0, 0.3], device="cuda")).view(-1, 9).contiguous()
    with va.Scene(pos, nrm, uv) as sc:
        for size in args.sizes.split(","):
            W, H = (int(v) for v in size.split("x"))
            npix = W * H
            emit(f"{W}x{H}")
            views = []
            for i in range(2):
                p, r = c["position"], c["rotation_deg"]
                cam = va.make_camera((p[0] + 6.0 * i, p[1], p[2]), (r[0], r[1] + 0.15 * i, r[2]), W, H, args.spp,
                                     back_size=(3.6, 3.6 * H / W))
                opts = va.make_opts(seed=1 + i, early_stop=False)
                d5 = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
                with sc.progressive(cam, opts, stream=stream) as prog:
                    prog.step(4)
                    prog.preview_device(d5)
                raw = sc.raycast_camera(cam, opts, 0, stream=stream)["raw"]
                stream.synchronize()
                views.append((cam, raw, d5))
            o5 = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
            o4 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
            hist = torch.empty((H, W), dtype=torch.float32, device="cuda")
            with va.Temporal(W, H) as t, va.Filter(W, H) as f:
                def call(i, **kw):
                    cam, raw, d5 = views[i % 2]
                    t.accumulate(cam, raw, d5, stream=stream, **kw)

                call(1, out=o5)  # (a history for the first timed call)
                rates = []
                for tag, kw in (("rgbaz", dict(out=o5)), ("rgbaz + rgba8", dict(out=o5, rgba8=o4)),
                                ("rgbaz + rgba8 + history", dict(out=o5, rgba8=o4, history=hist))):
                    tm = timed(lambda i: call(i, **kw))
                    rates.append(row(f"accumulate, {tag}", tm,
                                     model_bytes(npix, False, True, "rgba8" in kw, "history" in kw)))
                inplace = [v[2].clone() for v in views]
                tm = timed(lambda i: t.accumulate(views[i % 2][0], views[i % 2][1], inplace[i % 2], out=inplace[i % 2], stream=stream))
                row("accumulate, in place (rgbaz)", tm, model_bytes(npix, False, True))
                tm = timed(lambda i: call(i, out=o5, rgba8=o4), before=t.reset)
                row("accumulate, first call after reset, rgbaz + rgba8", tm, model_bytes(npix, True, True, True))
                emit(f"  history lengths last written: mean {float(hist.mean()):.2f} frames, "
                     f"{float((hist > 1).float().mean()):.1%} of the pixels took history")
                f.set_guide(views[0][1], stream=stream)
                one = va.make_filter_params(iterations=1)
                tm = timed(lambda i: f.apply(views[0][2], out=o5, rgba8=o4, params=one, stream=stream))
                filt = row("filter apply, iterations 1, rgbaz + rgba8", tm, filter_model_bytes(npix))
                emit(f"  accumulate (rgbaz + rgba8) reaches {rates[1] / filt:.2f} x the model rate of that filter call")
                # the motion leg: the records of the second view, then calls that alternate as above, the second view's with them
                mv = torch.empty((H, W, 8), dtype=torch.float32, device="cuda")
                raw1 = views[1][1]
                tm = timed(lambda i: va.motion_vectors(raw1, d_pos, d_prev, out=mv, stream=stream))
                row("motion records (k_motion), no normals", tm, motion_model_bytes(npix))
                tm = timed(lambda i: va.motion_vectors(raw1, d_pos, d_prev, d_nrm, out=mv, stream=stream))
                row("motion records (k_motion), previous normals", tm, motion_model_bytes(npix))
                emit(f"  {float((mv.view(torch.int32)[..., 3] & 1).float().mean()):.1%} of the records are flagged")
                mvs = [va.motion_vectors(v[1], d_pos, d_prev, d_nrm, stream=stream) for v in views]
                call(1, out=o5)
                tm = timed(lambda i: call(i, out=o5, rgba8=o4))
                plain = row("accumulate, rgbaz + rgba8 (again, beside the motion call)", tm, model_bytes(npix, False, True, True))
                tm = timed(lambda i: call(i, out=o5, rgba8=o4, motion=mvs[i % 2]))
                with_mv = row("accumulate with motion records, rgbaz + rgba8", tm, model_bytes(npix, False, True, True) + npix * 32)
                emit(f"  the motion call reaches {with_mv / plain:.2f} x the model rate of the call without")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
