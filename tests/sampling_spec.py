"""Adaptive sampling restated in float32 numpy (include/vermilion_hip.h, "adaptive sampling"): the moment a
VMX_PROGRESSIVE_MOMENTS handle folds, the per-pixel error and variance of the mean luminance, and the selection map.  Every
operation below is one float32 operation of numpy, in the order the header writes it, so each rounds once; numpy's float32
division and square root are correctly rounded and keep denormals.  What the GPU tests compare the kernels with, bit for
bit; tests/test_sampling_abi.py holds the restatement itself to the conditions it can be held to without a GPU."""
import numpy as np

F = np.float32
NO_ESTIMATE = F(3.402823466e+38)  # e of a pixel with fewer than two samples
DEFAULTS = dict(threshold=0.5, floor=0.05, min_samples=8, radius=1)


def params_of(p=None, **kw):
    """the fields of a vmx_sampling_params (or the defaults) as a dict, with overrides"""
    d = dict(DEFAULTS)
    if p is not None:
        d.update(threshold=p.threshold, floor=p.floor, min_samples=p.min_samples, radius=p.radius)
    d.update(kw)
    return d


def luminance(r, g, b):
    r, g, b = (np.asarray(x, F) for x in (r, g, b))
    return (F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b


def fold(samples, sums=None):
    """samples [n, ..., 3] float32, folded in order into sums [..., 4] = (r, g, b sums, m2) as k_resolve<true> folds a
    pixel's taken samples; sums: the state to go on from (default zeros)"""
    samples = np.asarray(samples, F)
    acc = np.zeros(samples.shape[1:-1] + (4,), F) if sums is None else np.array(sums, F)
    for s in samples:
        acc[..., 0] = acc[..., 0] + s[..., 0]
        acc[..., 1] = acc[..., 1] + s[..., 1]
        acc[..., 2] = acc[..., 2] + s[..., 2]
        l = luminance(s[..., 0], s[..., 1], s[..., 2])
        acc[..., 3] = acc[..., 3] + l * l
    return acc


def error_variance(sums, counts, floor=DEFAULTS["floor"]):
    """(e, var) per pixel from sums [..., 4] float32 and counts [...] integers"""
    sums = np.asarray(sums, F)
    n = np.asarray(counts).astype(np.int64)
    with np.errstate(all="ignore"):
        fn = np.maximum(n, 2).astype(F)  # (n < 2 is overwritten below; keeps the divisions defined)
        m1 = luminance(sums[..., 0], sums[..., 1], sums[..., 2]) / fn
        v = sums[..., 3] / fn - m1 * m1
        v = np.where(v > 0, v, F(0))  # (a NaN gives 0)
        var = v / (fn - F(1))
        e = np.sqrt(var) / (np.abs(m1) + F(floor))
    few = n < 2
    return np.where(few, NO_ESTIMATE, e).astype(F), np.where(few, F(0), var).astype(F)


def dilate(mask, radius):
    """mask [rows, W] of booleans, true within `radius` pixels (a square window clipped to the image) of a true pixel"""
    rows, w = mask.shape
    out = np.zeros_like(mask)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ys, yd = slice(max(dy, 0), rows + min(dy, 0)), slice(max(-dy, 0), rows + min(-dy, 0))
            xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
            out[yd, xd] |= mask[ys, xs]
    return out


def select(sums, counts, kmax, threshold=DEFAULTS["threshold"], floor=DEFAULTS["floor"], min_samples=DEFAULTS["min_samples"],
           radius=DEFAULTS["radius"]):
    """the selection map [rows, W] uint8 of a fixed-spp handle's state (its cursor is its count): an unfinished pixel with
    fewer than min_samples samples, or with an error above the threshold in its window.  The window's maximum is above the
    threshold exactly where some tap is (a comparison with a NaN is false), so no tap order is involved."""
    n = np.asarray(counts).astype(np.int64)
    e, _ = error_variance(sums, n, floor)
    with np.errstate(invalid="ignore"):
        above = dilate(e > F(threshold), int(radius))
    return ((n < kmax) & ((n < min_samples) | above)).astype(np.uint8)
