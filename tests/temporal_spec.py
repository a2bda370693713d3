"""Temporal accumulation (include/vermilion_hip.h, "temporal accumulation") restated in numpy float32: what the kernel of
vermilion_amd/csrc/vmx_temporal.inc is held to, bit for bit.  A helper, not a test.

Every array and every scalar is float32, so each written operation rounds once to float32, in the order written."""
import numpy as np

import oracle_lib as O
from filter_spec import guide_of, same_bits  # noqa: F401  (same_bits: for the tests that compare with this restatement)

F = np.float32
DEFAULTS = dict(normal_min=0.9, plane_tol=0.01, max_history=32.0)


def params_of(p=None, **kw):
    """a dict of the three parameters from None (defaults), a dict of some of them, or a ctypes vmx_temporal_params; kw
    replaces fields"""
    d = dict(DEFAULTS)
    if isinstance(p, dict):
        assert set(p) <= set(d), p
        d.update(p)
    elif p is not None:
        for k in d:
            d[k] = getattr(p, k)
    d.update(kw)
    return d


def camera_of(cam):
    """what proj reads of a vmx_camera: (m [col][row], pos [3], d, sx, sy), all float32"""
    m = np.array(O.camera_matrix(cam), np.float32)
    pos = np.array([cam.position[0], cam.position[1], cam.position[2]], np.float32)
    return m, pos, F(cam.back_distance), F(cam.back_size[0]), F(cam.back_size[1])


def records_of(rec):
    """(hit [...], n_p [..., 3], z_p [...], X [..., 3]) of vmx_rayhit records as they stand: a structured RAYHIT_DTYPE
    array, or [..., 16] words (float32 or uint32)"""
    if rec.dtype.names:
        normal, dist, flags, loc = rec["normal"], rec["distance"], rec["flags"], rec["location"]
    else:
        w = np.ascontiguousarray(rec)
        f = w.view(np.float32)
        normal, dist, flags, loc = f[..., 4:7], f[..., 3], w.view(np.uint32)[..., 11], f[..., 0:3]
    return (flags & 1) != 0, np.array(normal, np.float32), np.array(dist, np.float32), np.array(loc, np.float32)


def proj(X, camera, W, H):
    """(u, w, front) of the points X [..., 3]"""
    m, pos, d, sx, sy = camera
    with np.errstate(all="ignore"):
        v = X - pos
        c = [(m[k, 0] * v[..., 0] + m[k, 1] * v[..., 1]) + m[k, 2] * v[..., 2] for k in range(3)]
        t = d / (-c[2])
        u = ((c[0] * t) / sx + F(0.5)) * F(W)
        w = ((-(c[1] * t)) / sy + F(0.5)) * F(H)
    assert u.dtype == np.float32 and w.dtype == np.float32
    return u, w, c[2] < 0


def step(state, frame, rec, cam, params=None):
    """One call.  state: None (the first call after create or reset) or what the previous call returned; frame [H, W, 5]
    float32; rec [H, W] vmx_rayhit records; cam a vmx_camera.  Returns (frame_out [H, W, 5], state, history_len [H, W])."""
    prm = params_of(params)
    normal_min, plane_tol, max_history = F(prm["normal_min"]), F(prm["plane_tol"]), F(prm["max_history"])
    frame = np.ascontiguousarray(frame, np.float32)
    Hh, Ww = frame.shape[:2]
    assert frame.shape == (Hh, Ww, 5)
    hit, n_p, z_p, X = records_of(rec)
    assert hit.shape == (Hh, Ww)
    camera = camera_of(cam)
    c = frame[..., :3]
    out = np.array(c)
    n_new = np.ones((Hh, Ww), np.float32)
    if state is not None:
        with np.errstate(all="ignore"):
            u_c, w_c, _ = proj(X, camera, Ww, Hh)
            u_h, w_h, front = proj(X, state["camera"], Ww, Hh)
            ys, xs = np.meshgrid(np.arange(Hh), np.arange(Ww), indexing="ij")
            gx = xs.astype(np.float32) + (u_h - u_c)
            gy = ys.astype(np.float32) + (w_h - w_c)
            inrange = hit & front & (gx >= F(-1)) & (gx < F(Ww)) & (gy >= F(-1)) & (gy < F(Hh))
            x0, y0 = np.floor(gx), np.floor(gy)
            fx, fy = gx - x0, gy - y0
            x0i = np.where(inrange, x0, F(0)).astype(np.int64)
            y0i = np.where(inrange, y0, F(0)).astype(np.int64)
            zz = (plane_tol * plane_tol) * (z_p * z_p)
            sum_c = np.zeros((Hh, Ww, 3), np.float32)
            sum_n = np.zeros((Hh, Ww), np.float32)
            sum_w = np.zeros((Hh, Ww), np.float32)
            for dy in (0, 1):
                for dx in (0, 1):
                    qx, qy = x0i + dx, y0i + dy
                    inside = (qx >= 0) & (qx < Ww) & (qy >= 0) & (qy < Hh)
                    qxc, qyc = np.where(inside, qx, xs), np.where(inside, qy, ys)
                    c_q, nh_q = state["c"][qyc, qxc], state["n_h"][qyc, qxc]
                    n_q, z_q, X_q = state["n"][qyc, qxc], state["z"][qyc, qxc], state["X"][qyc, qxc]
                    wx = fx if dx else F(1) - fx
                    wy = fy if dy else F(1) - fy
                    wt = wx * wy
                    d = (n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1]) + n_p[..., 2] * n_q[..., 2]
                    e = X - X_q
                    pd = (n_p[..., 0] * e[..., 0] + n_p[..., 1] * e[..., 1]) + n_p[..., 2] * e[..., 2]
                    ok = inrange & inside & (z_q >= 0) & (d >= normal_min) & (pd * pd <= zz) & (wt > 0)
                    sum_c = np.where(ok[..., None], sum_c + wt[..., None] * c_q, sum_c)
                    sum_n = np.where(ok, sum_n + wt * nh_q, sum_n)
                    sum_w = np.where(ok, sum_w + wt, sum_w)
            any_w = sum_w > 0
            h = sum_c / sum_w[..., None]
            nh = sum_n / sum_w
            t = nh + F(1)
            n1 = np.where(t < max_history, t, max_history)
            a = F(1) / n1
            blended = h + (c - h) * a[..., None]
            out = np.where(any_w[..., None], blended, c)
            n_new = np.where(any_w, n1, F(1))
        assert out.dtype == np.float32 and n_new.dtype == np.float32 and sum_w.dtype == np.float32
    g_n, g_z = guide_of(rec)
    new_state = dict(c=np.array(out), n_h=np.array(n_new), n=g_n, z=g_z, X=X, camera=camera)
    frame_out = np.array(frame)
    frame_out[..., :3] = out
    return frame_out, new_state, n_new
