"""Motion records and the accumulation that uses them (include/vermilion_hip.h, "motion records") restated in numpy
float32: what k_motion (vermilion_amd/csrc/vmx_motion.inc) and k_temporal<.., MOTION> (vmx_temporal.inc) are held to, bit
for bit.  A helper, not a test.

Every array and every scalar is float32, so each written operation rounds once to float32, in the order written."""
import numpy as np

from filter_spec import guide_of, same_bits  # noqa: F401  (same_bits: for the tests that compare with this restatement)
from temporal_spec import camera_of, params_of, proj, records_of

F = np.float32
MOVED = np.uint32(1)  # VMX_MOTION_MOVED


def words_of(rec):
    """[..., 16] uint32 words of vmx_rayhit records: a structured RAYHIT_DTYPE array, or words (float32 or uint32)"""
    if rec.dtype.names:
        assert rec.dtype.itemsize == 64
        return np.ascontiguousarray(rec).view(np.uint32).reshape(rec.shape + (16,))
    assert rec.shape[-1] == 16 and rec.dtype.itemsize == 4
    return np.ascontiguousarray(rec).view(np.uint32)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def motion(rec, pos_now, pos_prev, nrm_prev=None):
    """vmx_motion_device: [..., 8] float32 words (prev_location, flags, prev_normal, pad) of the records rec [...]; pos_now,
    pos_prev and nrm_prev are [ntris, 9] float32 (any shape of ntris * 9 words)"""
    w = words_of(rec)
    f = w.view(np.float32)
    pn = np.ascontiguousarray(pos_now, np.float32).reshape(-1, 9)
    pp = np.ascontiguousarray(pos_prev, np.float32).reshape(-1, 9)
    ntris = pn.shape[0]
    assert pp.shape == pn.shape and ntris > 0
    P, dist, tri_t = f[..., 0:3], f[..., 3], f[..., 10]
    tid = w[..., 7].view(np.int32).astype(np.int64)
    with np.errstate(all="ignore"):
        on = ((w[..., 11] & 1) != 0) & (tid >= 0) & (tid < ntris) & (dist == tri_t)
        idc = np.where(on, tid, 0)  # (where !on nothing is read: triangle 0's values are computed with and dropped)
        a, q = pn[idc], pp[idc]
        moved = (a.view(np.uint32) != q.view(np.uint32)).any(axis=-1)
        a0, a1, a2 = a[..., 0:3], a[..., 3:6], a[..., 6:9]
        q0, q1, q2 = q[..., 0:3], q[..., 3:6], q[..., 6:9]
        e1, e2, ep = a1 - a0, a2 - a0, P - a0
        d11, d12, d22, dp1, dp2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(ep, e1), _dot(ep, e2)
        den = d11 * d22 - d12 * d12
        b1 = (d22 * dp1 - d12 * dp2) / den
        b2 = (d11 * dp2 - d12 * dp1) / den
        b0 = (F(1) - b1) - b2
        b0, b1, b2 = b0[..., None], b1[..., None], b2[..., None]
        Xh = (b0 * q0 + b1 * q1) + b2 * q2
        good = (den > 0) & np.isfinite(Xh).all(axis=-1)
        nh = np.array(f[..., 4:7])
        if nrm_prev is not None:
            n = np.ascontiguousarray(nrm_prev, np.float32).reshape(-1, 9)[idc]
            assert n.shape == a.shape
            m = (b0 * n[..., 0:3] + b1 * n[..., 3:6]) + b2 * n[..., 6:9]
            s = F(1) / np.sqrt(_dot(m, m))
            h = -(m * s[..., None])
            assert h.dtype == np.float32
            fin = np.isfinite(h).all(axis=-1)
            nh = np.where(fin[..., None], h.view(np.uint32), w[..., 4:7]).view(np.float32)
        assert Xh.dtype == np.float32 and nh.dtype == np.float32 and den.dtype == np.float32
    valid = on & moved & good
    out = np.zeros(w.shape[:-1] + (8,), np.uint32)
    out[..., 0:3] = np.where(valid[..., None], Xh.view(np.uint32), w[..., 0:3])
    out[..., 3] = np.where(valid, MOVED, np.uint32(0))
    out[..., 4:7] = np.where(valid[..., None], nh.view(np.uint32), w[..., 4:7])
    return out.view(np.float32)


def motion_of(mv, X, n_p):
    """(Xh [..., 3], nh [..., 3]) of motion records: None (X and n_p themselves), a structured MOTION_DTYPE array, or
    [..., 8] words (float32 or uint32)"""
    if mv is None:
        return X, n_p
    if mv.dtype.names:
        return np.array(mv["prev_location"], np.float32), np.array(mv["prev_normal"], np.float32)
    f = np.ascontiguousarray(mv).view(np.float32)
    assert f.shape == X.shape[:-1] + (8,)
    return np.array(f[..., 0:3]), np.array(f[..., 4:7])


def step(state, frame, rec, cam, motion=None, params=None):
    """One call of vmx_temporal_accumulate_motion_device: temporal_spec.step with the history looked up and tested at
    (Xh, nh) of the motion records.  state: None (the first call after create or reset: the records are ignored) or what
    the previous call returned; frame [H, W, 5] float32; rec [H, W] vmx_rayhit records; cam a vmx_camera; motion [H, W, 8]
    words or None.  Returns (frame_out [H, W, 5], state, history_len [H, W])."""
    prm = params_of(params)
    normal_min, plane_tol, max_history = F(prm["normal_min"]), F(prm["plane_tol"]), F(prm["max_history"])
    frame = np.ascontiguousarray(frame, np.float32)
    Hh, Ww = frame.shape[:2]
    assert frame.shape == (Hh, Ww, 5)
    hit, n_p, z_p, X = records_of(rec)
    assert hit.shape == (Hh, Ww)
    Xh, nh = motion_of(motion, X, n_p)
    camera = camera_of(cam)
    c = frame[..., :3]
    out = np.array(c)
    n_new = np.ones((Hh, Ww), np.float32)
    if state is not None:
        with np.errstate(all="ignore"):
            u_c, w_c, _ = proj(X, camera, Ww, Hh)
            u_h, w_h, front = proj(Xh, state["camera"], Ww, Hh)
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
                    d = _dot(nh, n_q)
                    e = Xh - X_q
                    pd = _dot(nh, e)
                    ok = inrange & inside & (z_q >= 0) & (d >= normal_min) & (pd * pd <= zz) & (wt > 0)
                    sum_c = np.where(ok[..., None], sum_c + wt[..., None] * c_q, sum_c)
                    sum_n = np.where(ok, sum_n + wt * nh_q, sum_n)
                    sum_w = np.where(ok, sum_w + wt, sum_w)
            any_w = sum_w > 0
            h = sum_c / sum_w[..., None]
            nhl = sum_n / sum_w
            t = nhl + F(1)
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


# ---- synthetic records for the tests of motion() and k_motion ----------------------------------------------------------
# every kind of record but these two must leave with the flag clear and its location and normal as they came, bitwise
FLAGGED = ("regular", "zero_normals")


def synthetic_records(n, ntris, seed):
    """(rec [n, 16] float32 words, pos_now, pos_prev, nrm_prev [ntris, 9], kind [n] of str): records of every kind motion()
    tells apart, in turn.  Triangles have random coordinates in -10..10 and move by a random
    translation plus a small deformation each; with ntris >= 8 the last three are special: ntris - 3 did not move (all
    nine words equal), ntris - 2 is degenerate now (three collinear vertices: den == 0) and ntris - 1 has zero previous
    normals.  Kinds: regular; miss (flags bit 0 clear); no_triangle (tri_id -1); sphere_nearer (distance != tri_t);
    id_ntris, id_ntris_plus_1, id_minus_2; nan_location, inf_location; nan_tri_t; and with ntris >= 8 unmoved,
    degenerate, zero_normals."""
    rng = np.random.RandomState(seed)
    pos_now = rng.uniform(-10, 10, (ntris, 9)).astype(np.float32)
    pos_prev = (pos_now + np.tile(rng.uniform(-3, 3, (ntris, 1, 3)), (1, 3, 1)).reshape(ntris, 9)
                + rng.uniform(-0.05, 0.05, (ntris, 9))).astype(np.float32)
    nrm_prev = rng.normal(size=(ntris, 9)).astype(np.float32)
    kinds = ["regular", "miss", "no_triangle", "sphere_nearer", "id_ntris", "id_ntris_plus_1", "id_minus_2", "nan_location",
             "inf_location", "nan_tri_t"]
    plain = ntris
    if ntris >= 8:
        plain = ntris - 3
        pos_prev[ntris - 3] = pos_now[ntris - 3]
        pos_now[ntris - 2, 6:9] = pos_now[ntris - 2, 0:3]  # (a2 == a0: e2 = 0 and den = d11*0 - 0*0 = 0 exactly)
        nrm_prev[ntris - 1] = 0.0
        kinds += ["unmoved", "degenerate", "zero_normals", "regular"]
    kind = np.array([kinds[i % len(kinds)] for i in range(n)])
    tid = rng.randint(0, plain, n)
    tid = np.where(kind == "unmoved", ntris - 3, tid)
    tid = np.where(kind == "degenerate", ntris - 2, tid)
    tid = np.where(kind == "zero_normals", ntris - 1, tid)
    b = rng.dirichlet((1, 1, 1), n).astype(np.float32)
    tri = pos_now[tid].reshape(n, 3, 3)
    rec = np.zeros((n, 16), np.float32)
    words = rec.view(np.uint32)
    rec[:, 0:3] = (b[:, :, None] * tri).sum(axis=1)
    rec[:, 3] = rec[:, 10] = rng.uniform(1, 100, n).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    rec[:, 4:7] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    rec[:, 8:10] = rng.uniform(0, 1, (n, 2))
    rec[:, 12:15] = rng.uniform(0, 1, (n, 3))
    tid = np.where(kind == "no_triangle", -1, tid)
    tid = np.where(kind == "id_ntris", ntris, tid)
    tid = np.where(kind == "id_ntris_plus_1", ntris + 1, tid)
    tid = np.where(kind == "id_minus_2", -2, tid)
    words[:, 7] = tid.astype(np.int32).view(np.uint32)
    words[:, 11] = np.where(kind == "miss", 2, 3)
    rec[kind == "miss", 3] = np.inf
    rec[kind == "sphere_nearer", 3] *= 0.5
    rec[kind == "nan_location", 0] = np.nan
    rec[kind == "inf_location", 1] = np.inf
    rec[kind == "nan_tri_t", 10] = np.nan
    for a in (rec, pos_now, pos_prev, nrm_prev):
        a.setflags(write=False)
    return rec, pos_now, pos_prev, nrm_prev, kind


# ---- the moving block of the Cornell set: the sequences the quality caps and the device tests run ----------------------
# per frame: the block's translation, its rotation about y (radians) through PIVOT, the camera's step in x and in
# y-rotation (degrees)
CASES = {"A": ((30.0, 0.0, 40.0), 0.0, (0.0, 0.0)),
         "B": ((30.0, 0.0, 40.0), 0.0, (6.0, 0.15)),
         "D": ((20.0, 0.0, 30.0), 0.04, (6.0, 0.15))}
PIVOT = (-50.0, 0.0, -200.0)  # the middle of the block's footprint
BLOCK = slice(4, 8)           # its triangles in scenes.cornell8()


def moved_block(pos, nrm, shift, angle, i, tris=BLOCK):
    """(pos, nrm) [ntris, 9] float32 of frame i: triangles `tris` of the set turned by i * angle about y through PIVOT,
    then moved by i * shift (computed in float64 from the set as it was made, rounded once); their normals turned too"""
    P = np.array(pos, np.float64).reshape(-1, 3, 3)
    N = np.array(nrm, np.float64).reshape(-1, 3, 3)
    c, s = np.cos(i * angle), np.sin(i * angle)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    P[tris] = (P[tris] - PIVOT) @ R.T + PIVOT + i * np.array(shift, np.float64)
    N[tris] = N[tris] @ R.T
    return P.reshape(-1, 9).astype(np.float32), N.reshape(-1, 9).astype(np.float32)
