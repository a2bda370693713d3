#!/usr/bin/env python3
"""What a table of emissive triangles (vmx_scene_set_emitters) costs the light-sampled integrator, and that a scene without
one costs what it did.

    python tools/nee_mesh_bench.py [--parent PARENT.so] [--runs 3] [--spp 16] [--out FILE]

All on the bench scene (sponza260k, bench.py's camera) at 1920x1080.  Frame times are vmx_stats.ms_device of whole
vmx_render_nee_device calls, the median [min, max] of `runs` calls after one warm-up call.
  1. no table: this library and, with --parent, a build of the parent commit loaded beside it, their calls in turn
     (A B A B ...).  The six k_nee instruction streams are identical (profiles/nee_mesh_isa.txt), so the times should agree
     within their spread.
  2. tables of 2, 256 and 65,536 triangles (the first n of a fixed shuffle of the scene's ids, radiance 4): ms per frame,
     rays per sample, and the secondary rays per sample beside the no-table frame's.  The difference is NOT the area shadow
     rays alone: paths now end on emitters (length(hitColour) > 1), so bounce rays fall while shadow rays are added; the
     library counts no shadow rays apart.
     Host wall time, after a device synchronise, of set_emitters (validation + upload) and of the first emitters() after
     it (k_emitter_slots + k_emitter_table + k_emitter_cdf, then the read-back of 24 n bytes): an upper bound of the
     kernels' time.
  3. an update (refit, same positions) followed by a 64-ray light-sampled batch, with the 65,536-entry table and without:
     the batch after an update is where the table is derived again.
None of these is a gate."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import vermilion_amd as va  # noqa: E402
from vermilion_amd import _lib as L  # noqa: E402
from vermilion_amd import scenes  # noqa: E402

LINES = []


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    LINES.append(line)


def opts(seed=1):
    return va.make_opts(seed=seed, early_stop=False, sampling=va.VMX_SAMPLING_CORRECTED)


def med(xs):
    return "%.2f [%.2f, %.2f]" % (float(np.median(xs)), min(xs), max(xs))


def frames(scs, cam, runs):
    """per scene: (ms list, last stats); the scenes take their calls in turn after a warm-up each"""
    import torch
    out = torch.empty((cam.image_res[1], cam.image_res[0], 5), dtype=torch.float32, device="cuda")
    for sc in scs:
        sc.render_nee_device(cam, opts(), out.data_ptr())
    ms, st = [[] for _ in scs], [None] * len(scs)
    for _ in range(runs):
        for i, sc in enumerate(scs):
            st[i] = sc.render_nee_device(cam, opts(), out.data_ptr())
            ms[i].append(st[i]["ms_device"])
    return ms, st


def load_parent(path):
    """the parent commit's library: _lib.load without the entries it does not have yet"""
    import ctypes as C
    import torch  # noqa: F401  (one HIP runtime per process, as _lib.load)
    lib = C.CDLL(path)
    for name, (res, args) in L.SYMBOLS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pos, nrm, uv = scenes.sponza260k()
    c = scenes.sponza_camera()
    cam = va.make_camera(c["position"], c["rotation_deg"], 1920, 1080, a.spp)
    ntris = len(pos)
    order = np.random.default_rng(3).permutation(ntris)

    say("# 1. sponza260k (%d triangles) 1920x1080, %d spp, no table: median [min, max] of %d calls" % (ntris, a.spp, a.runs))
    with va.Scene(pos, nrm, uv) as sc:
        if a.parent:
            with va.Scene(pos, nrm, uv, lib=load_parent(a.parent)) as old:
                (t_new, t_old), (s_new, s_old) = frames([sc, old], cam, a.runs)
            say("parent commit's library        %s ms" % med(t_old))
            assert (s_new["rays_primary"], s_new["rays_secondary"]) == (s_old["rays_primary"], s_old["rays_secondary"])
        else:
            (t_new,), (s_new,) = frames([sc], cam, a.runs)
        say("this library                   %s ms   %.2f rays/sample" % (med(t_new), (s_new["rays_primary"] + s_new["rays_secondary"]) / s_new["samples"]))
        sec0 = s_new["rays_secondary"] / s_new["samples"]

        say("# 2. with a table: ms per frame, rays per sample, secondary rays per sample (no table: %.2f), host wall ms" % sec0)
        for n in (2, 256, 65536):
            ids = order[:n]
            t_set, _ = wall(lambda: sc.set_emitters(ids, (4.0, 4.0, 4.0)))
            t_tab, tb = wall(sc.emitters)
            (t,), (s,) = frames([sc], cam, a.runs)
            say("n = %-6d %s ms   %.2f rays/sample   %.2f secondary/sample (%+.2f)   set_emitters %.2f ms, first emitters() %.2f ms (W = %.4g)" % (
                n, med(t), (s["rays_primary"] + s["rays_secondary"]) / s["samples"], s["rays_secondary"] / s["samples"],
                s["rays_secondary"] / s["samples"] - sec0, t_set, t_tab, tb["cdf"][-1]))

        say("# 3. update (refit, same positions) + a 64-ray light-sampled batch, host wall ms, median [min, max] of %d" % a.runs)
        o = np.tile(np.asarray(c["position"], np.float32), (64, 1))
        d = np.tile(np.array([0.0, -0.6, -0.8], np.float32), (64, 1))

        def update_then_batch():
            sc.update(pos=pos)
            sc.radiance_nee(o, d, opts())

        for what in ("65,536-entry table", "no table"):
            if what == "no table":
                sc.set_emitters(None)
            update_then_batch()
            say("%-20s %s ms" % (what, med([wall(update_then_batch)[0] for _ in range(a.runs)])))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
