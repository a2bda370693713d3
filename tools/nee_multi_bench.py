#!/usr/bin/env python3
"""What the rank, device-list and device-batch forms of light sampling cost on ONE device.

    python tools/nee_multi_bench.py [--runs 3] [--spp 16] [--size 1920x1080] [--parent OLD.so] [--out FILE]

No node with several GPUs has run this project: nothing here is a scaling curve.  What one device can say is the
compute-side ceiling of a split — the sum of the ranks' times over the whole frame's time: a k_nee launch never takes under
some milliseconds, so the ranks of a world together take longer than the frame, and a world of N devices cannot be faster
than whole / max(rank) even before its gather.

A figure is the median of `runs` calls after one warm-up call, the spread the least and the greatest.  Render times are
vmx_stats.ms_device (an event pair around the call's device work); the device-list and batch figures, which include copies
and host work, are the host's clock around the call.
  1. the bench scene (sponza260k, bench.py's camera) at --size and --spp: render_nee_device of the whole frame, then
     render_nee_rank_device for every rank of a world of 2 and of 4 and for ranks 0 and 5 of 8 (stripes of 16 rows).
  2. MultiScene([0]).render_nee_device against Scene.render_nee_device: the cost of the gather path alone (one replica, a
     same-device copy and k_assemble).
  3. radiance_nee_device against radiance_nee on the 1,048,576 camera rays of a 1024 x 1024 view of the bench scene.
  4. --parent: the entries that existed before (render_nee_device, render_device under `corrected`, radiance_nee) on the
     parent commit's library and on this one, calls in turn (A B A B ...) in the same run, and the frames' bytes compared.
None of these is a gate."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import vermilion_amd as va  # noqa: E402
from vermilion_amd import _lib as L  # noqa: E402
from vermilion_amd import scenes  # noqa: E402

CORRECTED = va.VMX_SAMPLING_CORRECTED
STRIPE = 16
LINES = []


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    LINES.append(line)


def opts(seed=1, **kw):
    return va.make_opts(seed=seed, early_stop=False, sampling=CORRECTED, **kw)


def med(xs):
    return "%.2f [%.2f, %.2f]" % (float(np.median(xs)), min(xs), max(xs))


def timed(call, runs, key="ms_device"):
    """`runs` calls after a warm-up: (times, last result); key None: the host's clock around the call"""
    import torch
    call()
    ts, last = [], None
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = call()
        torch.cuda.synchronize()
        ts.append(last[key] if key else (time.perf_counter() - t0) * 1e3)
    return ts, last


def load_parent(path):
    """an older build of the library: the symbols it has, with this build's prototypes"""
    lib = C.CDLL(path)
    for name, (res, args) in L.SYMBOLS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def ranks(sc, cam, args, out):
    whole, _ = timed(lambda: sc.render_nee_device(cam, opts(), out.data_ptr()), args.runs)
    say("render_nee_device, whole frame          %s ms" % med(whole))
    w = float(np.median(whole))
    for world, which in ((2, range(2)), (4, range(4)), (8, (0, 5))):
        ms = []
        for rank in which:
            o = opts(rank=rank, world=world, stripe_rows=STRIPE)
            t, st = timed(lambda: sc.render_nee_rank_device(cam, o, out.data_ptr()), args.runs)
            rows = va.local_rows(cam.image_res[1], STRIPE, rank, world)
            say("render_nee_rank_device rank %d of %d (%4d rows) %s ms   %d passes" % (rank, world, rows, med(t), st["passes"]))
            ms.append(float(np.median(t)))
        if len(ms) == world:
            say("  world %d: sum of ranks / whole = %.3f   whole / slowest rank = %.2f (the compute-side ceiling of %d devices)" % (
                world, sum(ms) / w, w / max(ms), world))
        else:
            say("  world %d: ranks %s only; whole / slowest of them = %.2f" % (world, list(which), w / max(ms)))
    return w


def gather_path(pos, nrm, uv, sc, cam, args, out):
    with va.MultiScene(pos, nrm, uv, devices=[0]) as multi:
        single, _ = timed(lambda: sc.render_nee_device(cam, opts(), out.data_ptr()), args.runs, key=None)
        ref = out.cpu().numpy().tobytes()
        listed, _ = timed(lambda: multi.render_nee_device(cam, opts(), out.data_ptr()), args.runs, key=None)
        same = out.cpu().numpy().tobytes() == ref
        tm = multi.timings()
    say("Scene.render_nee_device, host clock           %s ms" % med(single))
    say("MultiScene([0]).render_nee_device, host clock %s ms   (copy %.3f ms, k_assemble %.3f ms; frames identical: %s)" % (
        med(listed), tm["gather_ms"], tm["assemble_ms"], same))
    say("  the gather path alone: %+.2f ms" % (float(np.median(listed)) - float(np.median(single))))


def batches(sc, args):
    import oracle_lib as O
    import torch
    c = scenes.sponza_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], 1024, 1024, 4)
    o, d = O.primary_rays(cam, opts(), 0)
    n = len(o)
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    host, hres = timed(lambda: sc.radiance_nee(o, d, opts())[1], args.runs, key=None)
    dev, dres = timed(lambda: sc.radiance_nee_device(d_o.data_ptr(), d_d.data_ptr(), n, opts(), out.data_ptr()), args.runs, key=None)
    same = out.cpu().numpy().tobytes() == sc.radiance_nee(o, d, opts())[0].tobytes()
    say("radiance_nee, %d rays, host arrays          %s ms   (device work %.2f ms)" % (n, med(host), hres["ms_device"]))
    say("radiance_nee_device, the same rays on the device %s ms   (device work %.2f ms; results identical: %s)" % (
        med(dev), dres["ms_device"], same))
    return o, d


def against_parent(pos, nrm, uv, cam, o, d, args, out):
    import torch
    old = load_parent(args.parent)
    out2 = torch.empty_like(out)
    with va.Scene(pos, nrm, uv, lib=old) as a, va.Scene(pos, nrm, uv) as b:
        for name, fa, fb, buf in (
                ("render_nee_device", lambda: a.render_nee_device(cam, opts(), out.data_ptr()),
                 lambda: b.render_nee_device(cam, opts(), out2.data_ptr()), True),
                ("render_device corrected", lambda: a.render_device(cam, opts(), out.data_ptr()),
                 lambda: b.render_device(cam, opts(), out2.data_ptr()), True),
                ("radiance_nee %d rays" % len(o), lambda: a.radiance_nee(o, d, opts())[1], lambda: b.radiance_nee(o, d, opts())[1], False)):
            fa(), fb()
            ta, tb = [], []
            for _ in range(args.runs):
                ta.append(fa()["ms_device"])
                tb.append(fb()["ms_device"])
            torch.cuda.synchronize()
            same = (out.cpu().numpy().tobytes() == out2.cpu().numpy().tobytes()) if buf else \
                (a.radiance_nee(o, d, opts())[0].tobytes() == b.radiance_nee(o, d, opts())[0].tobytes())
            say("%-28s parent %s ms   this build %s ms   ratio %.3f   identical: %s" % (
                name, med(ta), med(tb), float(np.median(tb)) / float(np.median(ta)), same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    W, H = (int(v) for v in args.size.split("x"))
    pos, nrm, uv = scenes.sponza260k()
    c = scenes.sponza_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], W, H, args.spp)
    out = torch.empty((H, W, 5), dtype=torch.float32, device="cuda")
    say("# one MI355X; sponza260k %dx%d, %d spp, stripes of %d rows; median [min, max] of %d calls after a warm-up" % (
        W, H, args.spp, STRIPE, args.runs))
    say("# no node with several GPUs has run this project: these are one device's figures, not a scaling curve")
    with va.Scene(pos, nrm, uv) as sc:
        say("# 1. a rank's stripes (vmx_stats.ms_device)")
        ranks(sc, cam, args, out)
        say("# 2. the device list's gather path")
        gather_path(pos, nrm, uv, sc, cam, args, out)
        say("# 3. device batches")
        o, d = batches(sc, args)
    if args.parent:
        say("# 4. the entries that existed before, on the parent commit's library and on this one, calls in turn")
        against_parent(pos, nrm, uv, cam, o, d, args, out)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
