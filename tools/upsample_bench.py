#!/usr/bin/env python3
"""What guided upsampling costs: the apply call alone against its byte model and against one a-trous iteration at the
output size, and the whole render-small chain against the full-size chain at the same ray count.

    python tools/upsample_bench.py [--reps 20] [--runs 3] [--chain-reps 5] [--sizes 1920x1080:960x540,3840x2160:1920x1080]
                                   [--spp 16] [--out FILE]

The bench scene (sponza260k, bench camera, seed 1).  The kernels are timed with torch CUDA event pairs on the stream the
work runs on; one run is the median of `reps` calls after 3 warm-up calls, a figure is the median of `runs` runs and the
spread is the least and the greatest of them.  The sides of a comparison take their runs in turn (A B A B A B), so that
drift hits both alike.
  - apply: vmx_upsample_apply_device on a 4-sample low preview, rgbaz + rgba8, rgbaz alone, rgba8 alone, at the defaults
    (k_upsample<5>) and at normal_squarings 3 (the general form).
  - the yardstick, in the same turn: vmx_filter_apply_device at the output size with iterations = 1 (one launch of
    k_atrous, 25 taps against the apply call's 4).
  - set_guides: the two k_filter_guide launches.
  - the chains, with a host clock around calls that end in a stream synchronise (vmx_render_device blocks anyway), median
    of `chain-reps` after one warm-up, in turn:
      full   render W x H at spp, G-buffer at W x H, set_guide, filter (defaults)                  — what there was
      small  render lw x lh at spp * (W*H)/(lw*lh) rounded down to a multiple of 4, G-buffers at both sizes, filter at
             lw x lh (defaults), set_guides, upsample                                              — the same ray count
    and the parts of each beside it, so that the sums can be checked.
Byte models, the least traffic a call needs (re-reads by neighbouring lanes are the caches' and not counted):
  apply            per full pixel 16 B of guide read, 20 B + 4 B written; per low pixel 16 B of guide + 20 B of frame, read once
  one iteration    per pixel 16 B of guide + 20 B of frame read, 20 B + 4 B written (tools/filter_bench.py's)
  set_guides       per pixel of either size 64 B of record read, 16 B written"""
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


def apply_model(npix, nlow, rgbaz=True, rgba8=True):
    return npix * (16 + (20 if rgbaz else 0) + (4 if rgba8 else 0)) + nlow * 36


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chain-reps", type=int, default=5)
    ap.add_argument("--sizes", default="1920x1080:960x540,3840x2160:1920x1080")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("upsample_bench: no GPU (nothing is measured on the CPU)")
    lines = [f"# tools/upsample_bench.py: sponza260k, seed 1, {args.spp} spp at full size; kernels: torch CUDA event pairs, a "
             f"run = median of {args.reps} after 3 warm-up calls, a figure = median of {args.runs} runs taken in turn with the "
             f"other sides' [least greatest run]; chains: host clock to a stream synchronise, median of {args.chain_reps} "
             f"after 1 warm-up [least greatest]; {torch.cuda.get_device_name(0)}"]

    def emit(row):
        print(row, flush=True)
        lines.append(row)

    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the handles and the events share this stream

    def one_run(fn):
        ms = []
        for i in range(args.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def in_turn(sides):
        """sides: [(tag, fn, model bytes)] -> {tag: median ms}, each side's runs taken in turn with the others'"""
        runs = {tag: [] for tag, *_ in sides}
        for _ in range(args.runs):
            for tag, fn, _ in sides:
                runs[tag].append(one_run(fn))
        out = {}
        for tag, _, nbytes in sides:
            r = sorted(runs[tag])
            med = float(np.median(r))
            rate = nbytes / (med * 1e-3) / 1e9
            emit(f"  {tag:58s} {med * 1e3:8.1f} us [{r[0] * 1e3:.1f} {r[-1] * 1e3:.1f}]  model {nbytes / 1e6:7.1f} MB = "
                 f"{rate:7.1f} GB/s ({rate / HBM_PEAK_GBS:.1%} of {HBM_PEAK_GBS:.0f} GB/s)")
            out[tag] = med
        return out

    def chains_in_turn(sides):
        """sides: [(tag, fn)], fn ends synchronised -> {tag: median ms}"""
        ms = {tag: [] for tag, _ in sides}
        for i in range(args.chain_reps + 1):
            for tag, fn in sides:
                stream.synchronize()
                t0 = time.perf_counter()
                fn()
                stream.synchronize()
                if i >= 1:
                    ms[tag].append((time.perf_counter() - t0) * 1e3)
        out = {}
        for tag, _ in sides:
            r = sorted(ms[tag])
            out[tag] = float(np.median(r))
            emit(f"  {tag:58s} {out[tag]:8.2f} ms [{r[0]:.2f} {r[-1]:.2f}]")
        return out

    pos, nrm, uv = scenes.sponza260k()
    c = scenes.sponza_camera()
    with va.Scene(pos, nrm, uv) as sc:
        for pair in args.sizes.split(","):
            full, low = pair.split(":")
            W, H = (int(v) for v in full.split("x"))
            lw, lh = (int(v) for v in low.split("x"))
            npix, nlow = W * H, lw * lh
            low_spp = max(4, (args.spp * npix // nlow) // 4 * 4)
            cam = va.make_camera(c["position"], c["rotation_deg"], W, H, args.spp, back_size=(3.6, 3.6 * H / W))
            lcam = va.low_camera(cam, lw, lh)
            lcam.rays_per_pixel = low_spp
            opts = va.make_opts(seed=1, early_stop=False)
            emit(f"{W}x{H} from {lw}x{lh}")
            d_low = torch.empty((lh, lw, 5), dtype=torch.float32, device="cuda")
            d_lowf = torch.empty_like(d_low)
            d_full = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
            o5 = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
            o4 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
            with va.Upsample(lw, lh, W, H) as u, va.Filter(W, H) as f, va.Filter(lw, lh) as fl:
                with sc.progressive(lcam, opts, stream=stream) as p:
                    p.step(4)
                    p.preview_device(d_low)
                with sc.progressive(cam, opts, stream=stream) as p:
                    p.step(4)
                    p.preview_device(d_full)
                raw_lo = sc.raycast_camera(lcam, opts, 0, stream=stream)["raw"]
                raw_hi = sc.raycast_camera(cam, opts, 0, stream=stream)["raw"]
                u.set_guides(raw_lo, raw_hi, stream=stream)
                f.set_guide(raw_hi, stream=stream)
                fl.set_guide(raw_lo, stream=stream)
                stream.synchronize()
                one = va.make_filter_params(iterations=1)
                m3 = va.make_upsample_params(normal_squarings=3)
                res = in_turn([
                    ("upsample apply, rgbaz + rgba8", lambda: u.apply(d_low, out=o5, rgba8=o4, stream=stream), apply_model(npix, nlow)),
                    ("one a-trous iteration at the output size, rgbaz + rgba8",
                     lambda: f.apply(d_full, out=o5, rgba8=o4, params=one, stream=stream), npix * (16 + 20 + 20 + 4)),
                    ("upsample apply, rgbaz", lambda: u.apply(d_low, out=o5, stream=stream), apply_model(npix, nlow, True, False)),
                    ("upsample apply, rgba8", lambda: u.apply(d_low, rgba8=o4, stream=stream), apply_model(npix, nlow, False, True)),
                    ("upsample apply, normal_squarings 3, rgbaz + rgba8",
                     lambda: u.apply(d_low, out=o5, rgba8=o4, params=m3, stream=stream), apply_model(npix, nlow)),
                    ("set_guides (both sizes)", lambda: u.set_guides(raw_lo, raw_hi, stream=stream), (npix + nlow) * 80),
                ])
                a, b = res["upsample apply, rgbaz + rgba8"], res["one a-trous iteration at the output size, rgbaz + rgba8"]
                emit(f"  the apply call takes {a / b:.2f} of one a-trous iteration at the output size")

                def render(cm, dst):
                    sc.render_device(cm, opts, dst.data_ptr(), stream.cuda_stream)

                def gbuffer(cm):
                    return sc.raycast_camera(cm, opts, 0, stream=stream)["raw"]

                def chain_full():
                    render(cam, d_full)
                    f.set_guide(gbuffer(cam), stream=stream)
                    f.apply(d_full, out=o5, rgba8=o4, stream=stream)

                def chain_small():
                    render(lcam, d_low)
                    g_lo, g_hi = gbuffer(lcam), gbuffer(cam)
                    fl.set_guide(g_lo, stream=stream)
                    fl.apply(d_low, out=d_lowf, stream=stream)
                    u.set_guides(g_lo, g_hi, stream=stream)
                    u.apply(d_lowf, out=o5, rgba8=o4, stream=stream)

                emit(f"  chains at {args.spp * npix / 1e6:.1f} M camera paths: full {W}x{H}x{args.spp}, small {lw}x{lh}x{low_spp}")
                res = chains_in_turn([
                    ("full: render + G-buffer + filter", chain_full),
                    ("small: render + 2 G-buffers + filter + upsample", chain_small),
                    ("  render, full size", lambda: render(cam, d_full)),
                    ("  render, low size", lambda: render(lcam, d_low)),
                    ("  G-buffer, full size", lambda: gbuffer(cam)),
                    ("  G-buffer, low size", lambda: gbuffer(lcam)),
                    ("  filter (set_guide + defaults), full size",
                     lambda: (f.set_guide(raw_hi, stream=stream), f.apply(d_full, out=o5, rgba8=o4, stream=stream))),
                    ("  filter (set_guide + defaults), low size",
                     lambda: (fl.set_guide(raw_lo, stream=stream), fl.apply(d_low, out=d_lowf, stream=stream))),
                    ("  upsample (set_guides + apply)",
                     lambda: (u.set_guides(raw_lo, raw_hi, stream=stream), u.apply(d_lowf, out=o5, rgba8=o4, stream=stream))),
                ])
                s, g = res["small: render + 2 G-buffers + filter + upsample"], res["full: render + G-buffer + filter"]
                emit(f"  the small chain takes {s / g:.3f} of the full chain ({s - g:+.2f} ms)")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
