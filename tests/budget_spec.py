"""Budgeted steps restated in float32 numpy (include/vermilion_hip.h, "light sampling in progressive handles"): the number of
samples a pixel's error asks for, and what one budgeted step does to a handle's state.  It builds on tests/sampling_spec.py
(the error, the moment fold) — every operation is one float32 operation of numpy in the order the header writes it.  What
the GPU tests compare k_budget and a budgeted step with, uint32 for uint32 and bit for bit; tests/test_budget_spec.py
holds the restatement itself to the conditions it can be held to without a GPU."""
import numpy as np

import sampling_spec as SS

F = np.float32
DEFAULTS = dict(SS.DEFAULTS, max_step=0)


def cap_of(B, max_step=0):
    """cap = max_step ? min(max_step, B) : B"""
    return min(int(max_step), int(B)) if max_step else int(B)


def window_max(e, radius):
    """E per pixel: the largest e of the (2 * radius + 1)^2 window clipped to the image, taken as x > E ? x : E from E = 0 —
    a NaN never wins and E is never below 0, so a NaN counts as 0 and the order of the taps does not matter"""
    e = np.asarray(e, F)
    rows, w = e.shape
    with np.errstate(invalid="ignore"):
        z = np.where(e > F(0), e, F(0)).astype(F)
    out = np.zeros_like(z)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ys, yd = slice(max(dy, 0), rows + min(dy, 0)), slice(max(-dy, 0), rows + min(-dy, 0))
            xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
            out[yd, xd] = np.maximum(out[yd, xd], z[ys, xs])
    return out


def budget(sums, counts, kmax, B, threshold=DEFAULTS["threshold"], floor=DEFAULTS["floor"], min_samples=DEFAULTS["min_samples"],
           radius=DEFAULTS["radius"], max_step=0):
    """the budget plane [rows, W] uint32 of a fixed-spp handle's state (its cursor is its count); B: the handle's samples per
    batch"""
    n = np.asarray(counts).astype(np.int64)
    cap = cap_of(B, max_step)
    e, _ = SS.error_variance(sums, n, floor)
    E = window_max(e, int(radius))
    fn = n.astype(F)
    with np.errstate(all="ignore"):
        r = E / F(threshold)
        t = (fn * r) * r
        d = np.ceil(t) - fn
        big = d >= F(cap)  # (inf: cap; a NaN: false here and below, so 1)
        mid = d >= F(1)
        whole = np.where(mid & ~big, d, F(1)).astype(np.int64)
        want_err = np.where(big, cap, whole)
        above = E > F(threshold)
    want = np.where(n < min_samples, min_samples - n, np.where(above, want_err, 0))
    b = np.minimum(np.minimum(want, cap), kmax - n)
    return np.where(n >= kmax, 0, b).astype(np.uint32)


def step_counts(counts, budgets, kmax, B):
    """the samples each pixel takes in a budgeted step: min(budget, B, kmax - n) of an active pixel, else 0"""
    n = np.asarray(counts).astype(np.int64)
    b = np.asarray(budgets).astype(np.int64)
    return np.where(n < kmax, np.minimum(np.minimum(b, B), kmax - n), 0)


def step(sums, counts, budgets, kmax, B, samples, moments=True):
    """one budgeted step: (sums, counts, taken) afterwards.  sums [rows, W, 4], counts [rows, W], samples [kmax, rows, W, >= 3]:
    sample k of every pixel; a pixel at count n folds its samples n .. n + take - 1 in order, as k_resolve folds a taken
    sample (moments: the l * l fold too)"""
    take = step_counts(counts, budgets, kmax, B)
    acc = np.array(sums, F)
    n = np.asarray(counts).astype(np.int64).copy()
    for j in range(int(take.max()) if take.size else 0):
        m = take > j
        s = samples[n[m], np.nonzero(m)[0], np.nonzero(m)[1]][:, :3].astype(F)
        a = acc[m]
        a[:, 0] = a[:, 0] + s[:, 0]
        a[:, 1] = a[:, 1] + s[:, 1]
        a[:, 2] = a[:, 2] + s[:, 2]
        if moments:
            l = SS.luminance(s[:, 0], s[:, 1], s[:, 2])
            a[:, 3] = a[:, 3] + l * l
        acc[m] = a
        n[m] += 1
    return acc, n, take
