#!/usr/bin/env python3
"""What the progressive form of light sampling costs, and what adaptive and budgeted steps buy on it.

    python tools/nee_progressive_bench.py [--runs 3] [--spp 16] [--small 128x96] [--ref-spp 4096] [--kmax 64] [--out FILE]
                                          [--skip-bench-scene]

A time is the median [least, greatest] of `runs` measurements after one warm-up; ms_device is vmx_stats.ms_device summed
over a handle's steps (an event pair around each step's device work), wall the host clock around the same calls.
  1. Cost of the handle form.  A handle (vmx_progressive_begin_nee) stepped to kmax in steps of 1, 4 and all, beside the
     one-call vmx_render_nee_device on the same frame: the bench scene (sponza260k, bench.py's camera) at 1920x1080x--spp and
     cornell8 / lattice at --small.  The one call and the handle run the same pass routine; the parent commit's figure for
     the one call is in profiles/nee_bench.txt.  Handle and one call take their measurements in turn.
  2. Quality at equal samples.  cornell8 and the lattice at --small under the sphere tables of tools/nee_bench.py; handles
     with a ceiling of --kmax samples per pixel (VMX_PROGRESSIVE_MOMENTS), 8 uniform samples, then
       (b) vmx_progressive_step_adaptive in steps of 4,     (c) vmx_progressive_step_budgeted with max_step 4,
     each until its samples reach --spp per pixel on average or nothing is selected; (a) a uniform handle stepped to the
     whole number of samples per pixel nearest to what (b) and (c) took on average.  Squared error of the displayed rgb
     (the preview, clamped at 1) against a light-sampled frame of --ref-spp samples with another seed, over the thresholds
     of profiles/sampling_quality.txt at the default floor.
  3. Steps and time to "no pixel selected" for (b) and (c) at the same parameters with no sample target (the ceiling
     --kmax ends a pixel), max_step 0 for (c), and the share of the budgeted steps' wall time spent outside k_nee (the
     selection, the compactions, the scan, the fold, the read-backs and the host).
None of these is a gate."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import vermilion_amd as va  # noqa: E402
from vermilion_amd import scenes  # noqa: E402

CORRECTED = va.VMX_SAMPLING_CORRECTED
THRESHOLDS = (0.25, 0.5, 1.0, 2.0)
LINES = []


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    LINES.append(line)


def opts(seed, **kw):
    return va.make_opts(seed=seed, early_stop=False, sampling=CORRECTED, **kw)


def med(xs):
    return "%.2f [%.2f, %.2f]" % (float(np.median(xs)), min(xs), max(xs))


def run_handle(sc, cam, step):
    """(ms_device, wall ms, steps) of a handle stepped to completion in steps of `step` (0: all)"""
    t0 = time.perf_counter()
    ms, steps = 0.0, 0
    with sc.progressive_nee(cam, opts(1)) as p:
        while True:
            st = p.step(step)
            if st["samples"] == 0:
                break
            ms += st["ms_device"]
            steps += 1
            if step == 0:
                break
    return ms, (time.perf_counter() - t0) * 1e3, steps


def handle_cost(sc, cam, runs, title):
    import torch
    out = torch.empty((cam.image_res[1], cam.image_res[0], 5), dtype=torch.float32, device="cuda")
    forms = [("one call", None), ("handle, steps of 1", 1), ("handle, steps of 4", 4), ("handle, one step", 0)]

    def once(step):
        if step is None:
            t0 = time.perf_counter()
            st = sc.render_nee_device(cam, opts(1), out.data_ptr())
            return st["ms_device"], (time.perf_counter() - t0) * 1e3, 1
        return run_handle(sc, cam, step)

    for _, step in forms:
        once(step)  # warm-up
    got = {name: [] for name, _ in forms}
    for _ in range(runs):
        for name, step in forms:  # in turn, so that drift hits all alike
            got[name].append(once(step))
    say("# 1. %s, median [min, max] of %d" % (title, runs))
    base = float(np.median([g[0] for g in got["one call"]]))
    for name, _ in forms:
        g = got[name]
        say("%-22s ms_device %s   wall %s   steps %d   device time / one call %.3f" % (
            name, med([x[0] for x in g]), med([x[1] for x in g]), g[0][2], float(np.median([x[0] for x in g])) / base))


def mse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float((d * d).mean())


def adaptive_run(sc, cam, how, thr, target, max_step):
    """a moments handle: 8 uniform samples, then adaptive ('b') or budgeted ('c') steps until `target` samples (0: none) or
    nothing is selected.  Returns (preview, samples, steps, wall ms of the steps, ms in k_nee of the steps, counts)"""
    import torch
    prm_b = va.make_sampling_params(threshold=thr)
    prm_c = va.make_sampling_budget_params(threshold=thr, max_step=max_step)
    with sc.progressive_nee(cam, opts(1), moments=True) as p:
        p.step(8)
        steps, wall, nee_ms = 0, 0.0, 0.0
        while p.info()["pixels_active"] and not (target and p.info()["samples"] >= target):
            t0 = time.perf_counter()
            st, nsel = p.step_adaptive(4, prm_b) if how == "b" else p.step_budgeted(prm_c)
            dt = (time.perf_counter() - t0) * 1e3
            if nsel == 0:
                break
            steps, wall = steps + 1, wall + dt
            nee_ms += sc.timings()["other"]["ms"]
        counts = torch.empty(p.shape, dtype=torch.int32, device="cuda")
        p.state_device(None, counts)
        img = p.preview()
        return img, p.info()["samples"], steps, wall, nee_ms, counts.cpu().numpy()


def uniform_run(sc, cam, n):
    with sc.progressive_nee(cam, opts(1)) as p:
        p.step(n)
        return p.preview()


def quality(args):
    import nee_cases as K
    W, H = (int(v) for v in args.small.split("x"))
    npix = W * H
    say("# 2. squared error of the preview against a %d-spp light-sampled frame, %dx%d, ceiling %d samples per pixel, target %d "
        "per pixel on average; 8 uniform samples first; floor and radius the defaults, min_samples 8" % (args.ref_spp, W, H, args.kmax, args.spp))
    part3 = []
    for scene, cm in (("cornell8", scenes.cornell_camera()), ("lattice", scenes.lattice_camera())):
        pos, nrm, uv = (scenes.cornell8 if scene == "cornell8" else scenes.lattice)()
        for table in ("default", "single", "overlap"):
            with va.Scene(pos, nrm, uv, spheres=K.table(table)) as sc:
                ref, _ = sc.render_nee(va.make_camera(cm["position"], cm["rotation_deg"], W, H, args.ref_spp), opts(1000))
                cam = va.make_camera(cm["position"], cm["rotation_deg"], W, H, args.kmax)
                say("%s / %s" % (scene, table))
                for thr in THRESHOLDS:
                    ib, sb, nb, _, _, cb = adaptive_run(sc, cam, "b", thr, args.spp * npix, 4)
                    ic, s_c, nc, _, _, cc = adaptive_run(sc, cam, "c", thr, args.spp * npix, 4)
                    nu = max(8, int(round((sb + s_c) / 2.0 / npix)))
                    iu = uniform_run(sc, cam, nu)
                    eu, eb, ec = mse(iu, ref), mse(ib, ref), mse(ic, ref)
                    say("  threshold %4g: uniform %.4e (%d spp)  adaptive %.4e (%.2f spp, %d steps, counts %d..%d)  budgeted %.4e "
                        "(%.2f spp, %d steps, counts %d..%d)  adaptive/uniform %.3f  budgeted/uniform %.3f  budgeted/adaptive %.3f" % (
                            thr, eu, nu, eb, sb / npix, nb, cb.min(), cb.max(), ec, s_c / npix, nc, cc.min(), cc.max(), eb / eu, ec / eu,
                            ec / eb))
                # 3. to "no pixel selected" at the defaults' threshold
                thr = 0.5
                rows = []
                for how in ("b", "c"):
                    runs = [adaptive_run(sc, cam, how, thr, 0, 0) for _ in range(args.runs + 1)][1:]
                    rows.append((how, runs))
                part3.append((scene, table, rows))
    say("# 3. from 8 uniform samples to \"no pixel selected\" at threshold 0.5 (ceiling %d): steps, samples per pixel, wall ms of the "
        "steps, median [min, max] of %d; budgeted: max_step 0 (up to the handle's samples per batch in one pass)" % (args.kmax, args.runs))
    for scene, table, rows in part3:
        for how, runs in rows:
            wall = [r[3] for r in runs]
            share = [1.0 - r[4] / r[3] if r[3] > 0 else 0.0 for r in runs]
            say("%-20s %-9s steps %3d  samples/pixel %6.2f  wall %s ms  outside k_nee %.0f %% of the wall time" % (
                scene + " / " + table, "adaptive" if how == "b" else "budgeted", runs[0][2], runs[0][1] / npix, med(wall),
                100.0 * float(np.median(share))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--small", default="128x96")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--kmax", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-bench-scene", action="store_true")
    args = ap.parse_args()
    W, H = (int(v) for v in args.small.split("x"))
    if not args.skip_bench_scene:
        pos, nrm, uv = scenes.sponza260k()
        c = scenes.sponza_camera()
        with va.Scene(pos, nrm, uv) as sc:
            handle_cost(sc, va.make_camera(c["position"], c["rotation_deg"], 1920, 1080, args.spp), args.runs,
                        "sponza260k 1920x1080, %d spp" % args.spp)
    for scene, cm in (("cornell8", scenes.cornell_camera()), ("lattice", scenes.lattice_camera())):
        pos, nrm, uv = (scenes.cornell8 if scene == "cornell8" else scenes.lattice)()
        with va.Scene(pos, nrm, uv) as sc:
            handle_cost(sc, va.make_camera(cm["position"], cm["rotation_deg"], W, H, args.spp), args.runs,
                        "%s %dx%d, %d spp" % (scene, W, H, args.spp))
    quality(args)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
