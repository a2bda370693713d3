"""The G-buffer-guided a-trous filter (include/vermilion_hip.h, "G-buffer-guided denoising") restated in numpy float32:
what the kernels of vermilion_amd/csrc/vmx_filter.inc are held to, bit for bit.  A helper, not a test.

Every array and every scalar is float32, so each written operation rounds once to float32, in the order written."""
import numpy as np

F = np.float32
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)  # exact
DEFAULTS = dict(iterations=5, normal_squarings=5, sigma_colour=2.0, sigma_depth=0.1)


def params_of(p=None, **kw):
    """a dict of the four parameters from None (defaults), a dict, or a ctypes vmx_filter_params; kw replaces fields"""
    d = dict(DEFAULTS)
    if p is not None:
        for k in d:
            d[k] = p[k] if isinstance(p, dict) else getattr(p, k)
    d.update(kw)
    return d


def guide_of(rayhit):
    """(n [..., 3], z [...]) from an array of vmx_rayhit records: a structured RAYHIT_DTYPE array, or [..., 16] words
    (float32 or uint32)"""
    if rayhit.dtype.names:
        normal, dist, flags = rayhit["normal"], rayhit["distance"], rayhit["flags"]
    else:
        w = np.ascontiguousarray(rayhit)
        normal, dist, flags = w.view(np.float32)[..., 4:7], w.view(np.float32)[..., 3], w.view(np.uint32)[..., 11]
    hit = (flags & 1) != 0
    n = np.where(hit[..., None], normal, F(0)).astype(np.float32)
    z = np.where(hit, dist, F(-1)).astype(np.float32)
    return n, z


def _shifted(a, ox, oy, fill):
    """b[y, x] = a[y + oy, x + ox] where that is inside the image, `fill` elsewhere; and the inside mask"""
    Hh, Ww = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((Hh, Ww), bool)
    y0, y1 = max(0, -oy), min(Hh, Hh - oy)
    x0, x1 = max(0, -ox), min(Ww, Ww - ox)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return b, inside


def tap_weight(hh, n_p, z_p, n_q, z_q, c_p, c_q, m, isc2, kz):
    """w of one tap for arrays of pixels p and their neighbours q (the skip rules are the caller's)"""
    with np.errstate(all="ignore"):
        hit = z_p >= 0
        isz = F(1) / (kz * z_p)
        d = n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1] + n_p[..., 2] * n_q[..., 2]
        d = np.where(d > 0, d, F(0))
        for _ in range(m):
            d = d * d
        t = (z_p - z_q) * isz
        num = np.where(hit, hh * d, hh)
        g = np.where(hit, F(1) + t * t, F(1))
        dr, dg, db = c_p[..., 0] - c_q[..., 0], c_p[..., 1] - c_q[..., 1], c_p[..., 2] - c_q[..., 2]
        e = dr * dr + dg * dg + db * db
        w = num / (g * (F(1) + e * isc2))
    assert w.dtype == np.float32
    return w


def atrous(rgb, n, z, params=None):
    """rgb [H, W, 3], n [H, W, 3], z [H, W] float32 -> the filtered rgb [H, W, 3] (float32)"""
    prm = params_of(params)
    c = np.array(rgb, np.float32)
    n = np.ascontiguousarray(n, np.float32)
    z = np.ascontiguousarray(z, np.float32)
    assert c.ndim == 3 and c.shape[2] == 3 and n.shape == c.shape and z.shape == c.shape[:2]
    m = int(prm["normal_squarings"])
    sc = F(prm["sigma_colour"])
    sigma_depth = F(prm["sigma_depth"])
    hit = z >= 0
    for it in range(int(prm["iterations"])):
        s = 1 << it
        with np.errstate(all="ignore"):
            isc2 = F(1) / (sc * sc)
            kz = sigma_depth * F(s)
            sc = sc * F(0.5)
        sum_c = np.zeros_like(c)
        sum_w = np.zeros_like(z)
        with np.errstate(all="ignore"):
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    hh = H5[dy + 2] * H5[dx + 2]
                    c_q, inside = _shifted(c, s * dx, s * dy, F(0))
                    n_q, _ = _shifted(n, s * dx, s * dy, F(0))
                    z_q, _ = _shifted(z, s * dx, s * dy, F(-1))
                    w = tap_weight(hh, n, z, n_q, z_q, c, c_q, m, isc2, kz)
                    ok = inside & ((z_q >= 0) == hit) & (w > 0) & np.isfinite(w)
                    sum_c = np.where(ok[..., None], sum_c + w[..., None] * c_q, sum_c)
                    sum_w = np.where(ok, sum_w + w, sum_w)
            any_w = sum_w > 0
            c = np.where(any_w[..., None], sum_c / sum_w[..., None], c)
        assert c.dtype == np.float32 and sum_w.dtype == np.float32
    return c


def filtered_frame(rgbaz, n, z, params=None):
    """the whole RGBAZ frame [H, W, 5]: filtered colour, alpha and depth bitwise as they came"""
    out = np.array(rgbaz, np.float32)
    out[..., :3] = atrous(out[..., :3], n, z, params)
    return out


def same_bits(got, want):
    """got == want as uint32 bits, every element; NaN only where `want` has NaN (any payload)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))
