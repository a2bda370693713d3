#!/usr/bin/env python3
"""What adaptive temporal accumulation costs: vmx_temporal_accumulate_adaptive_device (k_temporal_gather + k_rectify, on a
moments handle + k_variance) per call, against the motion and variance calls of the same library in the same run, and
those two against the parent commit's library.

    python tools/adaptive_bench.py [--reps 20] [--runs 3] [--sizes 1920x1080,3840x2160] [--spp 16]
                                   [--parent-lib PATH] [--out FILE]

The bench scene and frames of tools/variance_bench.py (sponza260k, two 4-sample previews at two cameras a slow pan apart,
seeds 1 and 2, motion records: every triangle moved by (0.5, 0, 0.3)).  Everything is timed with torch CUDA event pairs
on the stream the work runs on; one run is the median of `reps` calls after 3 warm-up calls, a figure is the median of
`runs` runs and the spread is the least and the greatest of them.  The sides of a comparison take their runs in turn
(A B C A B C), so that drift hits all alike.  All calls write rgbaz + rgba8 + history (the adaptive ones d_change too)
and read motion records, at steady state (the two views alternate, so the detector has differences to look at).
  - with --parent-lib (a libvermilion_hip.so built from the parent commit): that library's motion and variance calls
    in turn with this one's — no existing kernel was touched, so the medians must lie within the runs' spread — and, as a
    control, the same calls on a second handle of this library: what two handles of one library differ by is what their
    buffers' placement does, not the code.
Byte models, the least traffic a call needs, per pixel (re-reads by neighbouring lanes are the caches' and not counted):
  motion call     64 record + 32 motion + 20 frame + 48 old state read; 48 new state + 20 frame + 4 rgba8 + 4 history written
  variance call   that + 8 old moments read + 8 new written; k_variance: 4 n' + 8 moments read, 4 written (+ 16 guide
                  where a wave takes the window)
  adaptive call   gather: 64 record + 32 motion + 48 old state read, 16 plane + 32 new guide and X written;
                  rectify: 12 colour + 16 plane + 16 guide read (x 1.45 with the halo of 3 around a 32 x 8 tile: the
                  model counts the halo, it is this kernel's own traffic), 8 alpha and depth read, 16 new colour + 20
                  frame + 4 rgba8 + 4 history + 4 change written; in place: 20 frame written less by k_rectify, 16 read
                  and 12 written by k_adaptive_store
                  with moments: + 8 old moments read and 8 plane written (gather), 8 plane read and 8 moments written
                  (rectify), and k_variance as above"""
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
HALO = (38 * 14) / (32 * 8)


def existing_model(npix, moments=False):
    per_pixel = 64 + 32 + 20 + 48 + 48 + 20 + 4 + 4
    if moments:
        per_pixel += 8 + 8 + 4 + 8 + 4
    return npix * per_pixel


def adaptive_model(npix, moments=False, in_place=False):
    gather = 64 + 32 + 48 + 16 + 32
    rectify = (12 + 16 + 16) * HALO + 8 + 16 + 20 + 4 + 4 + 4
    if in_place:
        rectify += -20 + 16 + 12
    if moments:
        gather += 8 + 8
        rectify += 8 + 8 + (4 + 8 + 4)
    return int(npix * (gather + rectify))


def load_other(path):
    """another build of the library beside the package's own: the symbols it has, declared as the package declares them"""
    lib = C.CDLL(path)
    for name, (res, args) in L.SYMBOLS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


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
        raise SystemExit("adaptive_bench: no GPU (nothing is measured on the CPU)")
    parent = load_other(args.parent_lib) if args.parent_lib else None
    lines = [f"# tools/adaptive_bench.py: sponza260k, {args.spp} spp target, 4 samples in, seeds 1 and 2, two cameras a slow pan "
             f"apart; torch CUDA event pairs, a run = median of {args.reps} after 3 warm-up calls, a figure = median of "
             f"{args.runs} runs taken in turn with the other sides' [least greatest run]; {torch.cuda.get_device_name(0)}"]

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
            fn(i)
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
                mv = va.motion_vectors(raw, d_pos, d_prev, d_nrm, stream=stream)
                stream.synchronize()
                views.append((cam, raw, d5, mv))
            o5 = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
            o4 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
            hist, var, chg = (torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(3))
            scratch = [v[2].clone() for v in views]
            handles = dict(plain=va.Temporal(W, H), mom=va.Temporal(W, H, moments=True), a_plain=va.Temporal(W, H),
                           a_mom=va.Temporal(W, H, moments=True), a_place=va.Temporal(W, H))
            if parent:
                handles.update(old_plain=va.Temporal(W, H, lib=parent), old_mom=va.Temporal(W, H, lib=parent, moments=True),
                               twin_plain=va.Temporal(W, H), twin_mom=va.Temporal(W, H, moments=True))

            def acc(name, i, **kw):
                cam, raw, d5, mv = views[i % 2]
                handles[name].accumulate(cam, raw, d5, out=o5, rgba8=o4, history=hist, motion=mv, stream=stream, **kw)

            def acc_in_place(i):
                cam, raw, d5, mv = views[i % 2]
                buf = scratch[i % 2]  # (accumulated over: the timing does not depend on the values)
                handles["a_place"].accumulate(cam, raw, buf, out=buf, rgba8=o4, history=hist, motion=mv, stream=stream,
                                              adaptive=True, change=chg)

            sides = [("motion call", lambda i: acc("plain", i), existing_model(npix)),
                     ("variance call", lambda i: acc("mom", i, variance=var), existing_model(npix, True))]
            if parent:
                sides += [("motion call, the parent's library", lambda i: acc("old_plain", i), existing_model(npix)),
                          ("variance call, the parent's library", lambda i: acc("old_mom", i, variance=var),
                           existing_model(npix, True)),
                          ("motion call, a second handle of this library", lambda i: acc("twin_plain", i), existing_model(npix)),
                          ("variance call, a second handle of this library", lambda i: acc("twin_mom", i, variance=var),
                           existing_model(npix, True))]
            sides += [("adaptive call, plain handle", lambda i: acc("a_plain", i, adaptive=True, change=chg), adaptive_model(npix)),
                      ("adaptive call, moments handle", lambda i: acc("a_mom", i, adaptive=True, change=chg, variance=var),
                       adaptive_model(npix, True)),
                      ("adaptive call, plain handle, in place", acc_in_place, adaptive_model(npix, False, True))]
            res = in_turn(sides)
            emit(f"  last adaptive call: mean history {float(hist.mean()):.2f} frames, r > 1 in {float((chg > 1).float().mean()):.2%} "
                 f"of the pixels")
            emit(f"  adaptive / motion call: {res['adaptive call, plain handle'] / res['motion call']:.2f} x; "
                 f"adaptive / variance call: {res['adaptive call, moments handle'] / res['variance call']:.2f} x")
            if parent:
                old_m, old_v = res["motion call, the parent's library"], res["variance call, the parent's library"]
                emit(f"  this library / the parent's: motion call {res['motion call'] / old_m:.3f}, "
                     f"variance call {res['variance call'] / old_v:.3f}; a second handle of this library / the first: motion call "
                     f"{res['motion call, a second handle of this library'] / res['motion call']:.3f}, variance call "
                     f"{res['variance call, a second handle of this library'] / res['variance call']:.3f}")
            stream.synchronize()
            for h in handles.values():
                h.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
