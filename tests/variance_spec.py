"""Variance-guided denoising (include/vermilion_hip.h, "variance-guided denoising") restated in numpy float32: what
k_temporal<.., MOMENTS> (vermilion_amd/csrc/vmx_temporal.inc) and k_variance, k_variance_pack and k_atrous_var
(vmx_variance.inc) are held to, bit for bit.  A helper, not a test.

Every array and every scalar is float32, so each written operation rounds once to float32, in the order written.

The moments ride the colour's taps with the colour's ok, wt and a, and m' = h + (l - h)*a is the colour's own blend: so the
moments of a call ARE temporal_spec.step (motion_spec.step with records) run on a frame whose "colour" is (l, l*l, 0) and a
state whose "colour" is (m1, m2, 0) — by import, not by copy."""
import numpy as np

import demod_spec as DS
import filter_spec as FS
import motion_spec as MS
import temporal_spec as TS
from filter_spec import same_bits  # noqa: F401  (for the tests that compare with this restatement)

F = np.float32
EPS = F(1e-10)  # VMX_VARIANCE_EPS
K3 = np.array([0.25, 0.5, 0.25], np.float32)  # exact
DEFAULTS = dict(min_history=4.0, normal_squarings=5, sigma_depth=0.1)
SIGMA_LUMINANCE = 4.0  # VMX_SIGMA_LUMINANCE_DEFAULT


def params_of(p=None, **kw):
    """a dict of the three parameters from None (defaults), a dict of some of them, or a ctypes vmx_variance_params"""
    d = dict(DEFAULTS)
    if isinstance(p, dict):
        assert set(p) <= set(d), p
        d.update(p)
    elif p is not None:
        for k in d:
            d[k] = getattr(p, k)
    d.update(kw)
    return d


def lum(c):
    """(0.2126f*r + 0.7152f*g) + 0.0722f*b of c [..., 3+]"""
    c = np.asarray(c, np.float32)
    with np.errstate(all="ignore"):
        out = (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]
    assert out.dtype == np.float32
    return out


def _accumulate(state, frame, rec, cam, motion, params):
    if motion is None:
        return TS.step(state, frame, rec, cam, params)
    return MS.step(state, frame, rec, cam, motion, params)


def step(state, frame, rec, cam, motion=None, params=None):
    """One call of vmx_temporal_accumulate_variance_device without its variance: (frame_out, state, history_len) of
    temporal_spec.step / motion_spec.step, the state with one more entry, "m" [H, W, 2] = (m1', m2')."""
    frame = np.ascontiguousarray(frame, np.float32)
    out, new_state, n_new = _accumulate(state, frame, rec, cam, motion, params)
    l = lum(frame)
    mom = np.zeros_like(frame)
    with np.errstate(all="ignore"):
        mom[..., 0], mom[..., 1] = l, l * l
    mstate = None
    if state is not None:
        mstate = dict(state)
        mstate["c"] = np.concatenate([state["m"], np.zeros_like(state["m"][..., :1])], axis=-1)
    mout, _, n_again = _accumulate(mstate, mom, rec, cam, motion, params)
    assert same_bits(n_again, n_new)
    new_state["m"] = np.array(mout[..., :2])
    return out, new_state, n_new


def variance(state, params=None):
    """d_variance [H, W] of the state a call just wrote"""
    prm = params_of(params)
    min_history, m, sigma_depth = F(prm["min_history"]), int(prm["normal_squarings"]), F(prm["sigma_depth"])
    m1, m2, n_h = state["m"][..., 0], state["m"][..., 1], state["n_h"]
    n, z = state["n"], state["z"]
    with np.errstate(all="ignore"):
        vt = m2 - m1 * m1
        vt = np.where(vt > 0, vt, F(0))
        hit = z >= 0
        isz = F(1) / (sigma_depth * z)
        s1, s2, sw = np.zeros_like(z), np.zeros_like(z), np.zeros_like(z)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                n_q, inside = FS._shifted(n, dx, dy, F(0))
                z_q, _ = FS._shifted(z, dx, dy, F(-1))
                m1_q, _ = FS._shifted(m1, dx, dy, F(0))
                m2_q, _ = FS._shifted(m2, dx, dy, F(0))
                d = n[..., 0] * n_q[..., 0] + n[..., 1] * n_q[..., 1] + n[..., 2] * n_q[..., 2]
                d = np.where(d > 0, d, F(0))
                for _ in range(m):
                    d = d * d
                t = (z - z_q) * isz
                w = np.where(hit, d / (F(1) + t * t), F(1))
                ok = inside & ((z_q >= 0) == hit) & (w > 0) & np.isfinite(w)
                s1 = np.where(ok, s1 + w * m1_q, s1)
                s2 = np.where(ok, s2 + w * m2_q, s2)
                sw = np.where(ok, sw + w, sw)
        a1, a2 = s1 / sw, s2 / sw
        vs = a2 - a1 * a1
        vs = np.where(vs > 0, vs, F(0))
        spatial = np.where(sw > 0, vs * (min_history / n_h), vt)
        var = np.where(n_h >= min_history, vt, spatial)
    assert var.dtype == np.float32 and sw.dtype == np.float32
    return var


def packed(rgb, var, albedo=None):
    """the pre-pass: (c [H, W, 3], v [H, W]) of the filter's plane"""
    c = np.array(rgb, np.float32)
    v = np.array(var, np.float32)
    if albedo is not None:
        am = DS.clamped_albedo(albedo)
        with np.errstate(all="ignore"):
            c = c / am
            la = lum(am)
            v = v / (la * la)
    assert c.dtype == np.float32 and v.dtype == np.float32
    return c, v


def atrous(rgb, var, n, z, params=None, sigma_luminance=SIGMA_LUMINANCE, albedo=None, with_variance=False):
    """rgb [H, W, 3], var [H, W], n [H, W, 3], z [H, W] float32 -> the filtered rgb [H, W, 3]; params: the plain filter's
    (filter_spec.params_of; sigma_colour is not used); albedo [H, W, 3+] or None.  with_variance: (rgb, the variance the
    last iteration would have handed on) — the call itself drops it."""
    prm = FS.params_of(params)
    c, v = packed(rgb, var, albedo)
    n = np.ascontiguousarray(n, np.float32)
    z = np.ascontiguousarray(z, np.float32)
    assert c.ndim == 3 and c.shape[2] == 3 and n.shape == c.shape and z.shape == c.shape[:2] == v.shape
    m = int(prm["normal_squarings"])
    sigma_depth = F(prm["sigma_depth"])
    sl = F(sigma_luminance)
    hit = z >= 0
    for it in range(int(prm["iterations"])):
        s = 1 << it
        with np.errstate(all="ignore"):
            kz = sigma_depth * F(s)
            vbar = np.zeros_like(v)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    v_q, inside = FS._shifted(v, dx, dy, F(0))
                    vbar = vbar + (K3[dy + 1] * K3[dx + 1]) * np.where(inside, v_q, v)
            den = (sl * sl) * vbar + EPS
            l_p = lum(c)
            isz = F(1) / (kz * z)
            sum_c, sum_v, sum_w = np.zeros_like(c), np.zeros_like(v), np.zeros_like(z)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    hh = FS.H5[dy + 2] * FS.H5[dx + 2]
                    c_q, inside = FS._shifted(c, s * dx, s * dy, F(0))
                    v_q, _ = FS._shifted(v, s * dx, s * dy, F(0))
                    n_q, _ = FS._shifted(n, s * dx, s * dy, F(0))
                    z_q, _ = FS._shifted(z, s * dx, s * dy, F(-1))
                    d = n[..., 0] * n_q[..., 0] + n[..., 1] * n_q[..., 1] + n[..., 2] * n_q[..., 2]
                    d = np.where(d > 0, d, F(0))
                    for _ in range(m):
                        d = d * d
                    t = (z - z_q) * isz
                    num = np.where(hit, hh * d, hh)
                    g = np.where(hit, F(1) + t * t, F(1))
                    dl = l_p - lum(c_q)
                    w = num / (g * (F(1) + (dl * dl) / den))
                    ok = inside & ((z_q >= 0) == hit) & (w > 0) & np.isfinite(w)
                    sum_c = np.where(ok[..., None], sum_c + w[..., None] * c_q, sum_c)
                    sum_v = np.where(ok, sum_v + (w * w) * v_q, sum_v)
                    sum_w = np.where(ok, sum_w + w, sum_w)
            any_w = sum_w > 0
            c = np.where(any_w[..., None], sum_c / sum_w[..., None], c)
            v = np.where(any_w, sum_v / (sum_w * sum_w), v)
        assert c.dtype == np.float32 and v.dtype == np.float32 and sum_w.dtype == np.float32 and den.dtype == np.float32
    if albedo is not None:
        with np.errstate(all="ignore"):
            c = c * DS.clamped_albedo(albedo)
    return (c, v) if with_variance else c


def filtered_frame(rgbaz, var, n, z, params=None, sigma_luminance=SIGMA_LUMINANCE, albedo=None):
    """the whole RGBAZ frame [H, W, 5]: filtered colour, alpha and depth bitwise as they came"""
    out = np.array(rgbaz, np.float32)
    out[..., :3] = atrous(out[..., :3], var, n, z, params, sigma_luminance, albedo)
    return out
