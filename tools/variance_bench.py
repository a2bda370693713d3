#!/usr/bin/env python3
"""What variance-guided denoising costs: the moments accumulate with its variance kernel, and the variance-guided filter
call, per call, against their byte models and beside the calls there were before.

    python tools/variance_bench.py [--reps 20] [--runs 3] [--sizes 1920x1080,3840x2160] [--spp 16]
                                   [--parent-lib PATH] [--out FILE]

The bench scene and frames of tools/temporal_bench.py (sponza260k, two 4-sample previews at two cameras a slow pan apart,
seeds 1 and 2), motion records as there (every triangle moved by (0.5, 0, 0.3)), the albedo of tools/demod_bench.py's kind
(a checker bound, 4 samples).  Everything is timed with torch CUDA event pairs on the stream the work runs on; one run is
the median of `reps` calls after 3 warm-up calls, a figure is the median of `runs` runs and the spread is the least and
the greatest of them.  The sides of a comparison take their runs in turn (A B A B A B), so that drift hits both alike.
  - accumulate: vmx_temporal_accumulate_motion_device on a plain handle against
    vmx_temporal_accumulate_variance_device on a moments handle (k_temporal<.., MOMENTS> + k_variance), rgbaz + rgba8 +
    history, with motion records; at steady state with min_history 1 (no pixel takes the window), 4 (the default) and 64
    (every pixel does), and the first call after a reset (every pixel does, and no history is read).
  - filter: vmx_filter_apply_device and vmx_filter_apply_demodulated_device at five iterations against
    vmx_filter_apply_variance_device without and with albedo, rgbaz + rgba8.
  - with --parent-lib (a libvermilion_hip.so built from the parent commit): that library's motion, plain and demodulated
    calls in turn with this one's — the instantiations are the same instruction streams, so the medians must lie within
    the runs' spread — and, as a control, the same calls on a second handle of this library: what two handles of one
    library differ by is what their buffers' placement does, not the code.
Byte models, the least traffic a call needs, per pixel (re-reads by neighbouring lanes are the caches' and not counted):
  motion call     64 record + 32 motion + 20 frame + 48 old state read; 48 new state + 20 frame + 4 rgba8 + 4 history written
  variance call   that + 8 old moments read + 8 new written; k_variance: 4 n' + 8 moments read (+ 16 guide where a wave
                  takes the window), 4 written; a first call reads no old state
  filter calls    tools/filter_bench.py's and tools/demod_bench.py's; the variance call: pre-pass 20 + 4 (+ 16 albedo) read,
                  16 written; an iteration 16 guide + 16 plane read, 16 written; the last one 20 frame (alpha, depth) more
                  read (+ 16 albedo) and 20 + 4 written instead"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vermilion_amd as va  # noqa: E402
from vermilion_amd import _lib as L  # noqa: E402
from vermilion_amd import scenes  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, as bench.py


def accumulate_model(npix, first=False, moments=False, window=False):
    per_pixel = 64 + 20 + 20 + 48 + 4 + 4 + (0 if first else 48 + 32)
    if moments:
        per_pixel += 8 + (0 if first else 8) + 4 + 8 + 4 + (16 if window else 0)
    return npix * per_pixel


def filter_model(npix, iterations, demod=False, variance=False):
    per_pixel = 0
    for it in range(iterations):
        per_pixel += 16 + (20 if it == 0 else 16)
        per_pixel += 20 + 4 if it + 1 == iterations else 16
    if variance:
        per_pixel += (20 + 4 + 16) - 4 + 16  # the pre-pass; iteration 0 reads a plane, the last one the frame's alpha and depth
        per_pixel += 2 * 16 if demod else 0
    elif demod:
        per_pixel += (20 + 16 + 16) - 4 + 16  # as tools/demod_bench.py
    return npix * per_pixel


def load_other(path):
    """another build of the library beside the package's own: the symbols it has, declared as the package declares them"""
    lib = C.CDLL(path)
    for name, (res, args) in L.SYMBOLS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def checker(n=256):
    y, x = np.mgrid[0:n, 0:n]
    chk = ((x // 8 + y // 8) & 1).astype(np.float32)
    return np.ascontiguousarray(np.stack([0.25 + 0.7 * chk, 0.9 - 0.6 * chk, 0.3 + 0.5 * ((x // 4) & 1)], axis=-1), np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("variance_bench: no GPU (nothing is measured on the CPU)")
    parent = load_other(args.parent_lib) if args.parent_lib else None
    lines = [f"# tools/variance_bench.py: sponza260k, {args.spp} spp target, 4 samples in, seeds 1 and 2, two cameras a slow pan "
             f"apart; torch CUDA event pairs, a run = median of {args.reps} after 3 warm-up calls, a figure = median of "
             f"{args.runs} runs taken in turn with the other sides' [least greatest run]; {torch.cuda.get_device_name(0)}"]

    def emit(row):
        print(row, flush=True)
        lines.append(row)

    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the handles and the events share this stream

    def one_run(fn, before=None):
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
        return float(np.median(ms))

    def in_turn(sides):
        """sides: [(tag, fn, before, model bytes)] -> {tag: median ms}, each side's runs taken in turn with the others'"""
        runs = {tag: [] for tag, *_ in sides}
        for _ in range(args.runs):
            for tag, fn, before, _ in sides:
                runs[tag].append(one_run(fn, before))
        out = {}
        for tag, _, _, nbytes in sides:
            r = sorted(runs[tag])
            med = float(np.median(r))
            rate = nbytes / (med * 1e-3) / 1e9
            emit(f"  {tag:66s} {med * 1e3:8.1f} us [{r[0] * 1e3:.1f} {r[-1] * 1e3:.1f}]  model {nbytes / 1e6:7.1f} MB = "
                 f"{rate:7.1f} GB/s ({rate / HBM_PEAK_GBS:.1%} of {HBM_PEAK_GBS:.0f} GB/s)")
            out[tag] = (med, r[0], r[-1])
        return out

    pos, nrm, uv = scenes.sponza260k()
    c = scenes.sponza_camera()
    d_pos, d_nrm = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
    d_prev = (d_pos.view(-1, 3) + torch.tensor([0.5, 0.0, 0.3], device="cuda")).view(-1, 9).contiguous()
    with va.Scene(pos, nrm, uv) as sc:
        sc.bind_texture(checker())
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
                mv = va.motion_vectors(raw, d_pos, d_prev, d_nrm, stream=stream)
                stream.synchronize()
                views.append((cam, raw, d5, mv))
            albedo = sc.albedo_camera(views[1][0], va.make_opts(seed=2, early_stop=False), samples=4, stream=stream)
            o5 = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
            o4 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
            hist = torch.empty((H, W), dtype=torch.float32, device="cuda")
            var = torch.empty((H, W), dtype=torch.float32, device="cuda")
            with va.Temporal(W, H) as plain, va.Temporal(W, H, moments=True) as mom, va.Filter(W, H) as f:
                old_t = va.Temporal(W, H, lib=parent) if parent else None
                old_f = va.Filter(W, H, lib=parent) if parent else None
                twin_t = va.Temporal(W, H) if parent else None
                twin_f = va.Filter(W, H) if parent else None

                def acc(t, i, **kw):
                    cam, raw, d5, mv = views[i % 2]
                    t.accumulate(cam, raw, d5, out=o5, rgba8=o4, history=hist, motion=mv, stream=stream, **kw)

                vp = {mh: va.make_variance_params(min_history=mh) for mh in (1.0, 4.0, 64.0)}
                for t in (plain, old_t, twin_t):
                    if t is not None:
                        acc(t, 1)
                acc(mom, 1, variance=var)
                sides = [("motion call (plain handle)", lambda i: acc(plain, i), None, accumulate_model(npix))]
                if parent:
                    sides.append(("motion call, the parent's library", lambda i: acc(old_t, i), None, accumulate_model(npix)))
                    sides.append(("motion call, a second handle of this library", lambda i: acc(twin_t, i), None, accumulate_model(npix)))
                for mh, window in ((1.0, False), (4.0, True), (64.0, True)):
                    sides.append((f"variance call, min_history {mh:g}",
                                  lambda i, mh=mh: acc(mom, i, variance=var, variance_params=vp[mh]), None,
                                  accumulate_model(npix, False, True, window)))
                res = in_turn(sides)
                base = res["motion call (plain handle)"][0]
                emit(f"  history lengths last written: mean {float(hist.mean()):.2f}; at min_history 4 "
                     f"{float((hist < 4).float().mean()):.1%} of the pixels take the window")
                for mh in (1.0, 4.0, 64.0):
                    d = res[f"variance call, min_history {mh:g}"][0] - base
                    emit(f"  moments + k_variance over the motion call, min_history {mh:g}: {d * 1e3:+.1f} us "
                         f"({d / base:+.1%})")
                res = in_turn([
                    ("motion call, first call after reset", lambda i: acc(plain, i), plain.reset, accumulate_model(npix, True)),
                    ("variance call, first call after reset (all window)", lambda i: acc(mom, i, variance=var), mom.reset,
                     accumulate_model(npix, True, True, True))])
                # the filter: the accumulated frame and its variance as they stand
                acc(mom, 0, variance=var), acc(mom, 1, variance=var)
                frame = o5.clone()
                f.set_guide(views[1][1], stream=stream)
                five = va.make_filter_params(iterations=5)
                sides = [("filter, plain call, 5 iterations", lambda i: f.apply(frame, out=o5, rgba8=o4, params=five, stream=stream),
                          None, filter_model(npix, 5)),
                         ("filter, demodulated call, 5 iterations",
                          lambda i: f.apply(frame, out=o5, rgba8=o4, params=five, albedo=albedo, stream=stream), None,
                          filter_model(npix, 5, demod=True))]
                if parent:
                    old_f.set_guide(views[1][1], stream=stream)
                    twin_f.set_guide(views[1][1], stream=stream)
                    sides += [("filter, plain call, the parent's library",
                               lambda i: old_f.apply(frame, out=o5, rgba8=o4, params=five, stream=stream), None, filter_model(npix, 5)),
                              ("filter, demodulated call, the parent's library",
                               lambda i: old_f.apply(frame, out=o5, rgba8=o4, params=five, albedo=albedo, stream=stream), None,
                               filter_model(npix, 5, demod=True)),
                              ("filter, plain call, a second handle of this library",
                               lambda i: twin_f.apply(frame, out=o5, rgba8=o4, params=five, stream=stream), None, filter_model(npix, 5)),
                              ("filter, demodulated call, a second handle of this library",
                               lambda i: twin_f.apply(frame, out=o5, rgba8=o4, params=five, albedo=albedo, stream=stream), None,
                               filter_model(npix, 5, demod=True))]
                sides += [("filter, variance-guided call, 5 iterations",
                           lambda i: f.apply(frame, out=o5, rgba8=o4, params=five, variance=var, stream=stream), None,
                           filter_model(npix, 5, variance=True)),
                          ("filter, variance-guided call with albedo, 5 iterations",
                           lambda i: f.apply(frame, out=o5, rgba8=o4, params=five, variance=var, albedo=albedo, stream=stream),
                           None, filter_model(npix, 5, demod=True, variance=True))]
                res = in_turn(sides)
                emit(f"  variance-guided / plain: {res['filter, variance-guided call, 5 iterations'][0] / res['filter, plain call, 5 iterations'][0]:.2f} x;"
                     f" with albedo / demodulated: "
                     f"{res['filter, variance-guided call with albedo, 5 iterations'][0] / res['filter, demodulated call, 5 iterations'][0]:.2f} x")
                stream.synchronize()
                for h in (old_t, old_f, twin_t, twin_f):
                    if h is not None:
                        h.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
