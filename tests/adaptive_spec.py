"""Adaptive temporal accumulation (include/vermilion_hip.h, "adaptive temporal accumulation") restated in numpy float32:
what k_temporal_gather and k_rectify (vermilion_amd/csrc/vmx_adaptive.inc) are held to, bit for bit.  A helper, not a test.

Every array and every scalar is float32, so each written operation rounds once to float32, in the order written.

The reprojection is temporal_spec's / motion_spec's with its blend taken off (`gather`: their projection, parameters and
records by import, their four taps restated so that h, nh and any can be had before the blend); that the restated taps
ARE theirs is held by tests/test_adaptive_abi.py: with gamma*gamma = +inf no pixel is cut and `step` must equal
temporal_spec.step, motion_spec.step and variance_spec.step bit for bit.  The moments ride the colour's taps as in
variance_spec: the same gather run on a state whose "colour" is (m1, m2, 0)."""
import numpy as np

import filter_spec as FS
import motion_spec as MS
import temporal_spec as TS
import variance_spec as VS
from filter_spec import guide_of, same_bits  # noqa: F401  (same_bits: for the tests that compare with this restatement)

F = np.float32
EPS = F(1e-10)  # VMX_ADAPTIVE_EPS
DEFAULTS = dict(gamma=3.0, min_support=4.0, normal_squarings=5, sigma_depth=0.1)
OFF = dict(gamma=3e38)  # gamma*gamma = +inf in float32: r is 0 or NaN, nothing is cut


def params_of(p=None, **kw):
    """a dict of the four parameters from None (defaults), a dict of some of them, or a ctypes vmx_adaptive_params"""
    d = dict(DEFAULTS)
    if isinstance(p, dict):
        assert set(p) <= set(d), p
        d.update(p)
    elif p is not None:
        for k in d:
            d[k] = getattr(p, k)
    d.update(kw)
    return d


def gather(state, planes, rec, cam, motion=None, params=None):
    """The reprojection of temporal_spec.step / motion_spec.step without the blend.  planes: the arrays [H, W, k] of the
    state to reproject besides n_h.  Returns (any [H, W], [h of each plane], nh [H, W]); where !any the quotients are
    0/0, as in the calls themselves."""
    prm = TS.params_of(params)
    normal_min, plane_tol = F(prm["normal_min"]), F(prm["plane_tol"])
    hit, n_p, z_p, X = TS.records_of(rec)
    Hh, Ww = hit.shape
    Xh, nh = MS.motion_of(motion, X, n_p)
    camera = TS.camera_of(cam)
    with np.errstate(all="ignore"):
        u_c, w_c, _ = TS.proj(X, camera, Ww, Hh)
        u_h, w_h, front = TS.proj(Xh, state["camera"], Ww, Hh)
        ys, xs = np.meshgrid(np.arange(Hh), np.arange(Ww), indexing="ij")
        gx = xs.astype(np.float32) + (u_h - u_c)
        gy = ys.astype(np.float32) + (w_h - w_c)
        inrange = hit & front & (gx >= F(-1)) & (gx < F(Ww)) & (gy >= F(-1)) & (gy < F(Hh))
        x0, y0 = np.floor(gx), np.floor(gy)
        fx, fy = gx - x0, gy - y0
        x0i = np.where(inrange, x0, F(0)).astype(np.int64)
        y0i = np.where(inrange, y0, F(0)).astype(np.int64)
        zz = (plane_tol * plane_tol) * (z_p * z_p)
        sums = [np.zeros(pl.shape, np.float32) for pl in planes]
        sum_n = np.zeros((Hh, Ww), np.float32)
        sum_w = np.zeros((Hh, Ww), np.float32)
        for dy in (0, 1):
            for dx in (0, 1):
                qx, qy = x0i + dx, y0i + dy
                inside = (qx >= 0) & (qx < Ww) & (qy >= 0) & (qy < Hh)
                qxc, qyc = np.where(inside, qx, xs), np.where(inside, qy, ys)
                nh_q = state["n_h"][qyc, qxc]
                n_q, z_q, X_q = state["n"][qyc, qxc], state["z"][qyc, qxc], state["X"][qyc, qxc]
                wx = fx if dx else F(1) - fx
                wy = fy if dy else F(1) - fy
                wt = wx * wy
                d = MS._dot(nh, n_q)
                pd = MS._dot(nh, Xh - X_q)
                ok = inrange & inside & (z_q >= 0) & (d >= normal_min) & (pd * pd <= zz) & (wt > 0)
                sums = [np.where(ok[..., None], s + wt[..., None] * pl[qyc, qxc], s) for s, pl in zip(sums, planes)]
                sum_n = np.where(ok, sum_n + wt * nh_q, sum_n)
                sum_w = np.where(ok, sum_w + wt, sum_w)
        any_w = sum_w > 0
        hs = [s / sum_w[..., None] for s in sums]
        nhl = sum_n / sum_w
    assert all(h.dtype == np.float32 for h in hs) and nhl.dtype == np.float32 and sum_w.dtype == np.float32
    return any_w, hs, nhl


def window(c, hh, any_w, n, z, aparams=None):
    """the 7 x 7 test of every pixel: (support [H, W] of bool, r [H, W]); c the input's colour [H, W, 3], hh the
    reprojected history (0 where !any), n / z this frame's guide"""
    prm = params_of(aparams)
    gamma, min_support = F(prm["gamma"]), F(prm["min_support"])
    m, sigma_depth = int(prm["normal_squarings"]), F(prm["sigma_depth"])
    with np.errstate(all="ignore"):
        isz = F(1) / (sigma_depth * z)
        sw, sww = np.zeros_like(z), np.zeros_like(z)
        sc, scc, sh = np.zeros_like(c), np.zeros_like(c), np.zeros_like(c)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                n_q, inside = FS._shifted(n, dx, dy, F(0))
                z_q, _ = FS._shifted(z, dx, dy, F(-1))
                c_q, _ = FS._shifted(c, dx, dy, F(0))
                hh_q, _ = FS._shifted(hh, dx, dy, F(0))
                any_q, _ = FS._shifted(any_w, dx, dy, False)
                d = n[..., 0] * n_q[..., 0] + n[..., 1] * n_q[..., 1] + n[..., 2] * n_q[..., 2]
                d = np.where(d > 0, d, F(0))
                for _ in range(m):
                    d = d * d
                t = (z - z_q) * isz
                w = d / (F(1) + t * t)
                ok = inside & (z_q >= 0) & any_q & (w > 0) & np.isfinite(w)
                okc = ok[..., None]
                sw = np.where(ok, sw + w, sw)
                sww = np.where(ok, sww + w * w, sww)
                sc = np.where(okc, sc + w[..., None] * c_q, sc)
                scc = np.where(okc, scc + w[..., None] * (c_q * c_q), scc)
                sh = np.where(okc, sh + w[..., None] * hh_q, sh)
        support = (sw > 0) & (sw * sw >= min_support * sww)
        sw3 = sw[..., None]
        mc, mh = sc / sw3, sh / sw3
        v = scc / sw3 - mc * mc
        v = np.where(v > 0, v, F(0))
        s2 = (F(2) * v) * (sww / (sw * sw))[..., None] + EPS
        dm = mc - mh
        k = (dm * dm) / s2
        K = np.array(k[..., 0])
        K = np.where(k[..., 1] > K, k[..., 1], K)
        K = np.where(k[..., 2] > K, k[..., 2], K)
        r = K / (gamma * gamma)
    assert r.dtype == np.float32 and sw.dtype == np.float32 and s2.dtype == np.float32
    return support, r


def step(state, frame, rec, cam, motion=None, params=None, aparams=None, moments=False):
    """One call of vmx_temporal_accumulate_adaptive_device (without its variance: variance_spec.variance of the returned
    state).  Arguments and the first three results as motion_spec.step / variance_spec.step (moments=True: the state
    carries "m"); the fourth is d_change [H, W]."""
    frame = np.ascontiguousarray(frame, np.float32)
    Hh, Ww = frame.shape[:2]
    if state is None:  # the existing call
        out, new_state, n_new = (VS.step if moments else MS.step)(None, frame, rec, cam, motion, params)
        return out, new_state, n_new, np.zeros((Hh, Ww), np.float32)
    max_history = F(TS.params_of(params)["max_history"])
    c = frame[..., :3]
    planes = [state["c"]] + ([state["m"]] if moments else [])
    any_w, hs, nh = gather(state, planes, rec, cam, motion, params)
    h = hs[0]
    g_n, g_z = guide_of(rec)
    with np.errstate(all="ignore"):
        hh = np.where(any_w[..., None], h, F(0))
        support, r = window(c, hh, any_w, g_n, g_z, aparams)
        cut = support & (r > F(1))
        nh_e = np.where(cut, nh / r, nh)
        t = nh_e + F(1)
        n1 = np.where(t < max_history, t, max_history)
        a = F(1) / n1
        out = np.where(any_w[..., None], h + (c - h) * a[..., None], c)
        n_new = np.where(any_w, n1, F(1))
        change = np.where(any_w & support, r, F(0))
    assert out.dtype == np.float32 and n_new.dtype == np.float32 and change.dtype == np.float32
    _, _, _, X = TS.records_of(rec)
    new_state = dict(c=np.array(out), n_h=np.array(n_new), n=g_n, z=g_z, X=X, camera=TS.camera_of(cam))
    if moments:
        l = VS.lum(frame)
        with np.errstate(all="ignore"):
            lm = np.stack([l, l * l], axis=-1)
            g = hs[1]
            new_state["m"] = np.where(any_w[..., None], g + (lm - g) * a[..., None], lm)
        assert new_state["m"].dtype == np.float32
    frame_out = np.array(frame)
    frame_out[..., :3] = out
    return frame_out, new_state, n_new, change
