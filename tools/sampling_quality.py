#!/usr/bin/env python3
"""What adaptive sampling buys at equal samples: the squared error of the displayed rgb against a converged frame, adaptive
against uniform, over the grid of thresholds and floors that vmx_sampling_default_params is chosen from.

    python tools/sampling_quality.py [--out profiles/sampling_quality.txt]

The measurement is tests/test_gpu_sampling.py's measure_quality (the test pins the default's ratio): the Cornell set at
70x41 and the lattice at 64x48, kmax 64; adaptive = 8 uniform samples, then vmx_progressive_step_adaptive(4) until
16 * npix samples are in; uniform = a plain handle stepped to ceil(total / npix) samples, so uniform never has fewer;
converged = a one-call render at 4096 spp with another seed.  Everything is deterministic: a figure is one run."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import test_gpu_sampling as T  # noqa: E402
import vermilion_amd as va  # noqa: E402

THRESHOLDS = (0.25, 0.5, 1.0, 2.0)
FLOORS = (0.01, 0.05, 0.2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampling_quality: no GPU (nothing is measured on the CPU)")
    d = va.make_sampling_params()
    lines = [f"# tools/sampling_quality.py: adaptive / uniform squared error of the displayed rgb against a 4096-spp frame; kmax 64, "
             f"8 uniform samples then adaptive steps of 4 up to 16 samples per pixel on average; min_samples {d.min_samples}, "
             f"radius {d.radius}; {torch.cuda.get_device_name(0)}",
             f"# the library's defaults: threshold {d.threshold:g}, floor {d.floor:g}"]

    def emit(row):
        print(row, flush=True)
        lines.append(row)

    product = {}
    for name in sorted(T.QUALITY_SCENES):
        geometry, cam_of = T.QUALITY_SCENES[name]
        emit(name)
        with va.Scene(*geometry()) as sc:
            for thr in THRESHOLDS:
                for floor in FLOORS:
                    q = T.measure_quality(sc, cam_of, va.make_sampling_params(threshold=thr, floor=floor))
                    product[(thr, floor)] = product.get((thr, floor), 1.0) * q["ratio"]
                    emit(f"  threshold {thr:4g} floor {floor:4g}: adaptive {q['adaptive']:.6g} uniform {q['uniform']:.6g} ratio "
                         f"{q['ratio']:.4f}  samples {q['samples']} (uniform {q['uniform_samples']}) in {q['rounds']} adaptive steps")
            q = T.measure_quality(sc, cam_of)
            emit(f"  defaults: adaptive {q['adaptive']:.6g} uniform {q['uniform']:.6g} ratio {q['ratio']:.6f}  samples {q['samples']} "
                 f"(uniform {q['uniform_samples']}) in {q['rounds']} adaptive steps")
            hist = q["histogram"]
            emit("  per-pixel counts at the defaults (count: pixels): " + ", ".join(f"{n}: {c}" for n, c in enumerate(hist) if c))
    least = min(product.values())
    ties = [k for k in product if product[k] <= least * 1.001]
    emit(f"least product of the scenes' ratios {least:.4f}, reached (within 0.1 %) by " + ", ".join(f"({t:g}, {f:g})" for t, f in ties))
    emit(f"the defaults ({d.threshold:g}, {d.floor:g}) are {'among them' if (round(d.threshold, 6), round(d.floor, 6)) in [(round(t, 6), round(f, 6)) for t, f in ties] else 'NOT among them'}: "
         "of the pairs that tie, the largest threshold (it selects no pixel a smaller one would not) and the middle floor")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
