"""G-buffer-guided upsampling (include/vermilion_hip.h, "guided upsampling") restated in numpy float32: what k_upsample
of vermilion_amd/csrc/vmx_upsample.inc is held to, bit for bit.  A helper, not a test.

Every array and every scalar is float32, so each written operation rounds once to float32, in the order written."""
import numpy as np

from filter_spec import F, guide_of, same_bits  # noqa: F401  (the guide is the filter's; re-exported for the tests)

DEFAULTS = dict(normal_squarings=5, sigma_depth=0.1)


def params_of(p=None, **kw):
    """a dict of the two parameters from None (defaults), a dict, or a ctypes vmx_upsample_params; kw replaces fields"""
    d = dict(DEFAULTS)
    if p is not None:
        for k in d:
            d[k] = p[k] if isinstance(p, dict) else getattr(p, k)
    d.update(kw)
    return d


def footprint(n_full, n_low):
    """per full coordinate 0..n_full-1: the first low tap (int64) and the fraction towards the second (float32)"""
    r = F(n_low) / F(n_full)
    u = np.arange(n_full, dtype=np.float32) * r
    x0 = np.minimum(np.floor(u).astype(np.int64), n_low - 1)
    f = u - x0.astype(np.float32)
    assert u.dtype == np.float32 and f.dtype == np.float32
    return x0, f


def replicated(lo, W, H):
    """pixel replication, what a caller without this call does: low pixel min((x*lw + W//2)//W, lw-1), alike in y"""
    lh, lw = lo.shape[:2]
    qx = np.minimum((np.arange(W) * lw + W // 2) // W, lw - 1)
    qy = np.minimum((np.arange(H) * lh + H // 2) // H, lh - 1)
    return lo[qy[:, None], qx[None, :]]


def upsample(lo, n_lo, z_lo, n_hi, z_hi, params=None, details=False):
    """lo [lh, lw, 5] (RGBAZ), n_lo [lh, lw, 3], z_lo [lh, lw], n_hi [H, W, 3], z_hi [H, W], all float32 -> the full
    RGBAZ frame [H, W, 5]; details=True: also the mask of the pixels that took the fallback and the anchors (y, x)"""
    prm = params_of(params)
    lo = np.ascontiguousarray(lo, np.float32)
    n_lo, z_lo = np.ascontiguousarray(n_lo, np.float32), np.ascontiguousarray(z_lo, np.float32)
    n_p, z_p = np.ascontiguousarray(n_hi, np.float32), np.ascontiguousarray(z_hi, np.float32)
    lh, lw = lo.shape[:2]
    Hh, Ww = z_p.shape
    assert lo.shape == (lh, lw, 5) and n_lo.shape == (lh, lw, 3) and z_lo.shape == (lh, lw) and n_p.shape == (Hh, Ww, 3)
    assert 1 <= lw <= Ww <= 4 * lw and 1 <= lh <= Hh <= 4 * lh
    m = int(prm["normal_squarings"])
    sigma_depth = F(prm["sigma_depth"])
    X0, fx = footprint(Ww, lw)
    Y0, fy = footprint(Hh, lh)
    hit = z_p >= 0
    sum_c = np.zeros((Hh, Ww, 3), np.float32)
    sum_w = np.zeros((Hh, Ww), np.float32)
    best_b = np.full((Hh, Ww), -1, np.float32)
    anchor_y = np.zeros((Hh, Ww), np.int64)
    anchor_x = np.zeros((Hh, Ww), np.int64)
    with np.errstate(all="ignore"):
        isz = F(1) / (sigma_depth * z_p)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = X0 + i, Y0 + j
                inside = (qy < lh)[:, None] & (qx < lw)[None, :]
                qyc, qxc = np.minimum(qy, lh - 1)[:, None], np.minimum(qx, lw - 1)[None, :]
                b = (fy if j else F(1) - fy)[:, None] * (fx if i else F(1) - fx)[None, :]
                better = inside & (b > best_b)
                best_b = np.where(better, b, best_b)
                anchor_y = np.where(better, qyc, anchor_y)
                anchor_x = np.where(better, qxc, anchor_x)
                n_q, z_q, c_q = n_lo[qyc, qxc], z_lo[qyc, qxc], lo[qyc, qxc, :3]
                d = n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1] + n_p[..., 2] * n_q[..., 2]
                d = np.where(d > 0, d, F(0))
                for _ in range(m):
                    d = d * d
                t = (z_p - z_q) * isz
                num = np.where(hit, b * d, b)
                g = np.where(hit, F(1) + t * t, F(1))
                w = num / g
                assert w.dtype == np.float32
                ok = inside & ((z_q >= 0) == hit) & (w > 0) & np.isfinite(w)
                sum_c = np.where(ok[..., None], sum_c + w[..., None] * c_q, sum_c)
                sum_w = np.where(ok, sum_w + w, sum_w)
        any_w = sum_w > 0
        out = np.array(lo[anchor_y, anchor_x])  # the anchor's five words, bitwise
        out[..., :3] = np.where(any_w[..., None], sum_c / sum_w[..., None], out[..., :3])
    assert out.dtype == np.float32 and sum_w.dtype == np.float32
    if details:
        return out, ~any_w, (anchor_y, anchor_x)
    return out
