#!/usr/bin/env python3
"""What light sampling (vmx_render_nee) costs and what it buys, beside vmx_render under VMX_SAMPLING_CORRECTED.

    python tools/nee_bench.py [--runs 3] [--spp 16] [--small 128x96] [--ref-spp 4096] [--out FILE]

Times are vmx_stats.ms_device (an event pair around the call's device work) of whole calls; a figure is the median of
`runs` calls after one warm-up call, the spread the least and the greatest; the two entries take their calls in turn
(A B A B ...), so that drift hits both alike.
  1. the bench scene (sponza260k, bench.py's camera) at 1920x1080: both entries at --spp samples, fixed count; rays per
     sample and Grays/s from the call's own ray counts.  The shadow-ray share of light sampling's traced rays is
     (its secondary rays per sample - the bounce rays per sample of `corrected`) / (its rays per sample): both integrators
     walk the same path distribution, so their bounce rays per sample agree in expectation.
  2. cornell8 and the lattice at --small, under the default sphere table and under tables with emitters in direct view
     (tests/nee_cases.py's `single` and `overlap`): the mean squared error (rgb, the frames as written: clamped at 1) against
     a light-sampled frame of --ref-spp samples with another seed, averaged over three seeds —
     at equal samples (both at --spp), and at equal time (`corrected` given the multiple of 4 samples that fills the time
     light sampling took).
None of these is a gate."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import vermilion_amd as va  # noqa: E402
from vermilion_amd import scenes  # noqa: E402

CORRECTED = va.VMX_SAMPLING_CORRECTED
LINES = []


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    LINES.append(line)


def opts(seed):
    return va.make_opts(seed=seed, early_stop=False, sampling=CORRECTED)


def med(xs):
    return "%.2f [%.2f, %.2f]" % (float(np.median(xs)), min(xs), max(xs))


def timed_pair(sc, cam, runs, seed=1):
    """(ms list, last stats) of render_nee and of render, calls in turn after a warm-up each"""
    import torch
    out = torch.empty((cam.image_res[1], cam.image_res[0], 5), dtype=torch.float32, device="cuda")
    sc.render_nee_device(cam, opts(seed), out.data_ptr())
    sc.render_device(cam, opts(seed), out.data_ptr())
    tn, tc, sn, scs = [], [], None, None
    for _ in range(runs):
        sn = sc.render_nee_device(cam, opts(seed), out.data_ptr())
        tn.append(sn["ms_device"])
        scs = sc.render_device(cam, opts(seed), out.data_ptr())
        tc.append(scs["ms_device"])
    return tn, sn, tc, scs


def rays(st):
    return st["rays_primary"] + st["rays_secondary"]


def bench_scene(args):
    pos, nrm, uv = scenes.sponza260k()
    c = scenes.sponza_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], 1920, 1080, args.spp)
    with va.Scene(pos, nrm, uv) as sc:
        tn, sn, tc, st = timed_pair(sc, cam, args.runs)
    say("# 1. sponza260k 1920x1080, %d spp, fixed count, median [min, max] of %d calls" % (args.spp, args.runs))
    for name, t, s in (("vmx_render_nee_device", tn, sn), ("vmx_render_device corrected", tc, st)):
        say("%-30s %s ms   %.2f rays/sample   %.3f Grays/s" % (name, med(t), rays(s) / s["samples"], rays(s) / np.median(t) / 1e6))
    say("time ratio light sampling / corrected: %.2f" % (np.median(tn) / np.median(tc)))
    sec_n, sec_c = sn["rays_secondary"] / sn["samples"], st["rays_secondary"] / st["samples"]
    say("shadow-ray share of light sampling's traced rays: %.1f %% (%.2f secondary rays per sample against %.2f bounce rays)" % (
        100.0 * (sec_n - sec_c) / (rays(sn) / sn["samples"]), sec_n, sec_c))


def mse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float((d * d).mean())


def small_scenes(args):
    import nee_cases as K
    W, H = (int(v) for v in args.small.split("x"))
    say("# 2. squared error against a %d-spp light-sampled frame, %dx%d, mean of 3 seeds; frames as written (clamped at 1)" % (
        args.ref_spp, W, H))
    say("%-22s %10s %10s %7s | %8s %8s %10s %7s | %s" % ("scene / table", "mse nee", "mse corr", "ratio", "ms nee", "ms corr",
                                                          "mse corr@t", "ratio", "corr spp@t, share of ref pixels at the clamp"))
    for scene, cm in (("cornell8", scenes.cornell_camera()), ("lattice", scenes.lattice_camera())):
        pos, nrm, uv = (scenes.cornell8 if scene == "cornell8" else scenes.lattice)()
        for table in ("default", "single", "overlap"):
            with va.Scene(pos, nrm, uv, spheres=K.table(table)) as sc:
                ref, _ = sc.render_nee(va.make_camera(cm["position"], cm["rotation_deg"], W, H, args.ref_spp), opts(1000))
                cam = va.make_camera(cm["position"], cm["rotation_deg"], W, H, args.spp)
                tn, _, tc, _ = timed_pair(sc, cam, args.runs)
                t_nee, t_corr = float(np.median(tn)), float(np.median(tc))
                spp_t = max(4, int(round(args.spp * t_nee / t_corr / 4.0)) * 4)
                cam_t = va.make_camera(cm["position"], cm["rotation_deg"], W, H, spp_t)
                en, ec, et = [], [], []
                for seed in (1, 2, 3):
                    en.append(mse(sc.render_nee(cam, opts(seed))[0], ref))
                    ec.append(mse(sc.render(cam, opts(seed))[0], ref))
                    et.append(mse(sc.render(cam_t, opts(seed))[0], ref))
            clamp = float((ref[..., :3] >= 1.0).any(axis=-1).mean())
            say("%-22s %10.3e %10.3e %7.2f | %8.2f %8.2f %10.3e %7.2f | %d spp, %.1f %%" % (
                scene + " / " + table, np.mean(en), np.mean(ec), np.mean(ec) / np.mean(en), t_nee, t_corr, np.mean(et),
                np.mean(et) / np.mean(en), spp_t, 100 * clamp))
    say("(ratio: corrected's error over light sampling's — above 1, light sampling is the better estimator of that frame)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--small", default="128x96")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-bench-scene", action="store_true")
    args = ap.parse_args()
    if not args.skip_bench_scene:
        bench_scene(args)
    small_scenes(args)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
