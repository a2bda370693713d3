#!/usr/bin/env python3
"""What adaptive sampling costs on the bench scene (sponza260k) at 1920x1080.

    python tools/sampling_bench.py [--reps 10] [--runs 3] [--size 1920x1080] [--parent-lib PATH] [--out FILE]

  1. vmx_progressive_select_device: torch CUDA event pairs on the handle's stream, at the default parameters (radius 1) and
     at radius 3, on a state of 8 samples per pixel.
  2. The split and merge overhead of a selected step: a step of 4 samples with every pixel selected (two list compactions,
     two read-backs, the ragged schedule) against a plain step of 4 samples on a handle that was never ragged.  Steps block,
     so a step is timed on the host (perf_counter around the call) and its vmx_stats.ms_device is reported beside it.
  3. One adaptive run as tests/test_gpu_sampling.py measures quality — 8 uniform samples, then step_adaptive(4) until 16
     samples per pixel are in on average, kmax 64 — against a uniform handle stepped to 16 samples in steps of 4: host time
     of the whole run, begin to the last step.
  4. With --parent-lib (a libvermilion_hip.so built from the parent commit): plain steps of 4 samples of this library in
     turn with the parent's, twice the parent's (two scenes of it): the existing kernels' instruction streams and the
     schedule of a never ragged handle are unchanged, so this library must differ from the parent by no more than the two
     parents differ from each other or a side's own runs spread.  Exit status 1 if it does.
A run is the median of `reps` calls after 3 warm-up calls; a figure is the median of `runs` runs, [least greatest] beside it;
the sides of a comparison take their runs in turn (A B C A B C), so that drift hits all alike.  All handles
are begun with samples_per_batch = 4 (passes of 4 samples: the path buffers are sized for that) and, but for item 3, a ceiling of
1024 samples per pixel, so that every timed step has samples to take."""
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

sys.path.insert(0, os.path.join(ROOT, "tools"))
from adaptive_bench import load_other  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampling_bench: no GPU (nothing is measured on the CPU)")
    W, H = (int(v) for v in args.size.split("x"))
    lines = [f"# tools/sampling_bench.py: sponza260k {W}x{H}; a run = median of {args.reps} after 3 warm-up calls, a figure = median "
             f"of {args.runs} runs taken in turn with the other sides' [least greatest run]; {torch.cuda.get_device_name(0)}"]

    def emit(row):
        print(row, flush=True)
        lines.append(row)

    def in_turn(sides, unit="ms"):
        """sides: [(tag, fn)] with fn() -> one sample of the figure; -> {tag: (median, least, greatest)}"""
        runs = {tag: [] for tag, _ in sides}
        for _ in range(args.runs):
            for tag, fn in sides:
                vals = [fn() for _ in range(args.reps + 3)][3:]
                runs[tag].append(float(np.median(vals)))
        out = {}
        for tag, _ in sides:
            r = sorted(runs[tag])
            out[tag] = (float(np.median(r)), r[0], r[-1])
            emit(f"  {tag:64s} {out[tag][0]:9.3f} {unit} [{r[0]:.3f} {r[-1]:.3f}]")
        return out

    pos, nrm, uv = scenes.sponza260k()
    c = scenes.sponza_camera()
    cam_of = lambda spp: va.make_camera(c["position"], c["rotation_deg"], W, H, spp, back_size=(3.6, 3.6 * H / W))  # noqa: E731
    long_opts = va.make_opts(seed=1, early_stop=False, samples_per_batch=4)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    verdict = 0
    with va.Scene(pos, nrm, uv) as sc:
        # 1. the select call
        emit("1. vmx_progressive_select_device, 8 samples per pixel in")
        with sc.progressive(cam_of(1024), long_opts, stream=stream, moments=True) as p:
            p.step(8)
            d_m = torch.empty((H, W), dtype=torch.uint8, device="cuda")
            d_c = torch.zeros((1,), dtype=torch.int32, device="cuda")

            def select(prm):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                p.select_device(d_m, d_c, prm)
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3

            in_turn([("default parameters (radius 1)", lambda: select(None)),
                     ("radius 3", lambda: select(va.make_sampling_params(radius=3))),
                     ("radius 0", lambda: select(va.make_sampling_params(radius=0)))], unit="us")
            p.select_device(d_m, d_c)
            stream.synchronize()
            emit(f"  (the default map selects {int(d_c.item())} of {W * H} pixels; the kernel reads 24 B per pixel and its halo's, writes 1 B)")

        # 2. a step with everything selected against a plain step
        emit("2. a step of 4 samples: every pixel selected (ragged schedule) against a plain step (never ragged)")
        everything = torch.ones((H, W), dtype=torch.uint8, device="cuda")
        with sc.progressive(cam_of(1024), long_opts, stream=stream) as plain, sc.progressive(cam_of(1024), long_opts, stream=stream) as ragged:
            device_ms = {"plain": [], "selected": []}

            def step_plain():
                t = time.perf_counter()
                st = plain.step(4)
                dt = (time.perf_counter() - t) * 1e3
                device_ms["plain"].append(st["ms_device"])
                return dt

            def step_selected():
                t = time.perf_counter()
                st, n = ragged.step_selected(4, everything)
                dt = (time.perf_counter() - t) * 1e3
                assert n == W * H
                device_ms["selected"].append(st["ms_device"])
                return dt

            r = in_turn([("plain step, host time", step_plain), ("step with every pixel selected, host time", step_selected)])
            emit(f"  vmx_stats.ms_device of the same steps, median: plain {np.median(device_ms['plain']):.3f} ms, selected "
                 f"{np.median(device_ms['selected']):.3f} ms (the compactions lie outside the step's device interval)")
            a, b = r["plain step, host time"][0], r["step with every pixel selected, host time"][0]
            emit(f"  split and merge overhead: {b - a:+.3f} ms per step ({b / a:.3f} x)")

        # 3. one adaptive run against a uniform one
        emit("3. one run to 16 samples per pixel on average, kmax 64: adaptive (8 uniform, then adaptive steps of 4) against uniform steps of 4")
        opts = long_opts  # (passes of 4 samples on both sides)
        facts = {}

        def run_adaptive():
            t = time.perf_counter()
            with sc.progressive(cam_of(64), opts, stream=stream, moments=True) as p:
                p.step(8)
                rounds = 0
                while p.info()["samples"] < 16 * W * H and p.info()["pixels_active"]:
                    if p.step_adaptive(4)[1] == 0:
                        break
                    rounds += 1
                facts["adaptive"] = (p.info()["samples"], rounds)
            return (time.perf_counter() - t) * 1e3

        def run_uniform():
            t = time.perf_counter()
            with sc.progressive(cam_of(64), opts, stream=stream) as p:
                for _ in range(4):
                    p.step(4)
                facts["uniform"] = (p.info()["samples"], 4)
            return (time.perf_counter() - t) * 1e3

        saved = args.reps
        args.reps = max(2, args.reps // 3)
        r = in_turn([("uniform, 4 steps of 4", run_uniform), ("adaptive, 8 then steps of 4", run_adaptive)])
        args.reps = saved
        emit(f"  adaptive: {facts['adaptive'][0]} samples in 1 + {facts['adaptive'][1]} steps; uniform: {facts['uniform'][0]} samples; "
             f"adaptive / uniform host time {r['adaptive, 8 then steps of 4'][0] / r['uniform, 4 steps of 4'][0]:.3f} x")

        # 4. existing behaviour against the parent's library
        if args.parent_lib:
            emit("4. plain steps of 4 samples (never ragged handles): this library in turn with the parent's, twice")
            parent = load_other(args.parent_lib)
            with va.Scene(pos, nrm, uv, lib=parent) as pa, va.Scene(pos, nrm, uv, lib=parent) as pb:
                handles = {"this library": sc.progressive(cam_of(1024), long_opts, stream=stream),
                           "the parent's library": pa.progressive(cam_of(1024), long_opts, stream=stream),
                           "the parent's library, a second scene": pb.progressive(cam_of(1024), long_opts, stream=stream)}

                def stepper(h):
                    def fn():
                        t = time.perf_counter()
                        h.step(4)
                        return (time.perf_counter() - t) * 1e3
                    return fn

                r = in_turn([(tag, stepper(h)) for tag, h in handles.items()])
                for h in handles.values():
                    h.close()
            this, p1, p2 = r["this library"], r["the parent's library"], r["the parent's library, a second scene"]
            allowed = max(abs(p1[0] - p2[0]), p1[2] - p1[1], p2[2] - p2[1], this[2] - this[1])
            diff = min(abs(this[0] - p1[0]), abs(this[0] - p2[0]))
            ok = diff <= allowed
            emit(f"  this - parent: {this[0] - p1[0]:+.3f} ms / {this[0] - p2[0]:+.3f} ms; parent - parent: {p1[0] - p2[0]:+.3f} ms; the "
                 f"widest run spread {max(p1[2] - p1[1], p2[2] - p2[1], this[2] - this[1]):.3f} ms: {'within' if ok else 'OUTSIDE'} what the parent differs from itself by")
            verdict = 0 if ok else 1
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return verdict


if __name__ == "__main__":
    sys.exit(main())
