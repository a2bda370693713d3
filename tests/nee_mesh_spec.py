"""Light sampling with emissive triangles restated in numpy: nee_spec's path loop (every statement of it, in its order) with
the additions E1 - E4 of include/vermilion_hip.h ("emissive triangles as area lights"), which the kernel is held to bit for
bit.  Test infrastructure only.

  E1  override: a RayCast whose returned hit is the BVH's triangle (tri_id >= 0 and distance == tri_t) and whose triangle
      is emitter e has hitColour = radiance_e — path rays, cone shadow rays and area shadow rays alike
  E2  derived table in double from the float32 v0, e1 = v1 - v0, e2 = v2 - v0: `table`
  E4  one area sample after the last sphere emitter: three draws, selection by cdf, a point on the triangle, the weight
      float((double(dot(w, omega)) / pi) / (p_e d2 / (area_e cosl))), the drops, and the contribution only where the
      shadow ray's returned hit is triangle e
With emitters=None and light_sampling either way this is nee_spec.radiance bit for bit (tests/test_nee_mesh_spec.py pins it).
light_sampling=False with a table keeps the override and samples nothing: the brute-force estimator of the same integral.
"""
import numpy as np

import oracle_lib as O
from nee_spec import (F, PI, TWO_PI, _DRAWS_PER_STEP, _Streams, _combine, _dot, _dtrig, _frame, _normalize, cone, table_of)
from vermilion_amd import _lib as L

D = np.float64


def luminance(rgb):
    """vmx_image.inc's float32 luminance"""
    rgb = np.asarray(rgb, F).reshape(-1, 3)
    return (F(0.2126) * rgb[:, 0] + F(0.7152) * rgb[:, 1]) + F(0.0722) * rgb[:, 2]


def table(pos, ids, radiance):
    """E2: the derived table of the emitters (ids [n], radiance [n, 3] or [3]) over the triangles pos [ntris, 9]"""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 9)
    ids = np.asarray(ids, np.int64).reshape(-1)
    rad = np.ascontiguousarray(np.broadcast_to(np.asarray(radiance, F).reshape(-1, 3), (ids.size, 3)))
    p = pos[ids]
    v0 = p[:, 0:3]
    e1 = p[:, 3:6] - p[:, 0:3]  # float32, as the triangle record holds them
    e2 = p[:, 6:9] - p[:, 0:3]
    A, B = e1.astype(D), e2.astype(D)
    with np.errstate(all="ignore"):
        nraw = np.stack([A[:, 1] * B[:, 2] - B[:, 1] * A[:, 2], A[:, 2] * B[:, 0] - B[:, 2] * A[:, 0],
                         A[:, 0] * B[:, 1] - B[:, 0] * A[:, 1]], axis=1)
        nn = (nraw[:, 0] * nraw[:, 0] + nraw[:, 1] * nraw[:, 1]) + nraw[:, 2] * nraw[:, 2]
        area = 0.5 * np.sqrt(nn)
        normal = nraw / np.sqrt(nn)[:, None]
    weight = area * luminance(rad).astype(D)
    cdf = np.empty(ids.size, D)
    run = D(0.0)
    for e in range(ids.size):  # sequentially: the order of the additions is the definition
        run = run + weight[e]
        cdf[e] = run
    id_em = np.full(pos.shape[0], -1, np.int64)
    id_em[ids] = np.arange(ids.size)
    return {"ids": ids, "radiance": rad, "v0": v0, "e1": e1, "e2": e2, "area": area, "normal": normal, "weight": weight,
            "cdf": cdf, "id_em": id_em, "n": ids.size}


def _hit_emitter(h, tb):
    """E1's condition per record: the emitter index of the returned hit, -1 where it is none"""
    if tb is None:
        return np.full(len(h), -1, np.int64)
    tri = h["tri_id"].astype(np.int64)
    is_tri = (tri >= 0) & (h["distance"] == h["tri_t"])
    return np.where(is_tri, tb["id_em"][np.where(is_tri, tri, 0)], -1)


def _colour(h, he, tb):
    col = h["colour"].astype(F)
    if tb is not None:
        on = he >= 0
        col[on] = tb["radiance"][he[on]]
    return col


def radiance(osc, o, d, seed, spheres=None, sampling=L.VMX_SAMPLING_CORRECTED, light_sampling=True, tex=None, pixel=None,
             k=None, emitters=None):
    """nee_spec.radiance with a table of emissive triangles: emitters = table(pos, ids, radiance) or None.  Returns the
    unclamped accumColour [n, 4] float32 and the ray counts (rays_shadow: cone and area shadow rays)."""
    assert (sampling & 0xFF) == L.VMX_SAMPLING_CORRECTED
    libm_double = bool(sampling & L.VMX_SAMPLING_LIBM_DOUBLE)
    tb = table_of(spheres)
    mt = emitters if (emitters is not None and emitters["n"] > 0) else None
    em = np.nonzero(tb["emit"])[0] if light_sampling else np.zeros(0, np.int64)
    ec, er2 = tb["centre"][em], (tb["radius"][em] * tb["radius"][em]).astype(F)
    o = np.ascontiguousarray(o, F).reshape(-1, 3).copy()
    d = np.ascontiguousarray(d, F).reshape(-1, 3).copy()
    n = o.shape[0]
    pixel = np.arange(n, dtype=np.int64) if pixel is None else np.asarray(pixel, np.int64)
    k = np.zeros(n, np.int64) if k is None else np.asarray(k, np.int64)
    rng = _Streams(seed, pixel, k)
    acc = np.zeros((n, 4), F)
    acc[:, 3] = F(-100)
    thr = np.ones((n, 4), F)
    depth = np.zeros(n, np.int64)
    lit = np.zeros(n, bool)
    live = np.arange(n)
    st = {"rays_primary": n, "rays_secondary": 0, "rays_shadow": 0, "samples": n}
    with np.errstate(all="ignore"):
        while live.size:
            rng.reserve(live, _DRAWS_PER_STEP + 3)
            st["rays_secondary"] += int((np.isfinite(d[live]).all(axis=1) & (depth[live] > 0)).sum())
            h = osc.raycast(o[live], d[live])
            hit = (h["flags"] & 1) != 0
            live, h = live[hit], h[hit]
            he = _hit_emitter(h, mt)
            col = _colour(h, he, mt)  # E1
            add = ~lit[live]
            ia = live[add]
            acc[ia, :3] = acc[ia, :3] + thr[ia, :3] * col[add]
            acc[ia, 3] = acc[ia, 3] + thr[ia, 3] * F(0)
            d0 = depth[live] == 0
            acc[live[d0], 3] = h["distance"][d0]
            go = ~(np.sqrt(_dot(col, col)) > F(1))
            live, h, he = live[go], h[go], he[go]
            depth[live] += 1
            rr = depth[live] > 5
            ends = np.zeros(live.size, bool)
            if rr.any():
                u = rng.u01(live[rr])
                ends[rr] = (u > float(F(0.95))) | (depth[live[rr]] > 1000)
            live, h, he = live[~ends], h[~ends], he[~ends]
            if live.size == 0:
                break
            mat = (h["flags"] & 2) != 0
            dir_in = d[live].copy()
            nrm = h["normal"].astype(F)
            x = h["location"].astype(F) - dir_in * F(0.001)
            spec = np.zeros(live.size, bool)
            if mat.any():
                spec[mat] = rng.u01(live[mat]) >= 0.96
            new_d = np.zeros((live.size, 3), F)
            if spec.any():
                i = live[spec]
                rng.skip(i, 3)
                kk = _dot(nrm[spec], dir_in[spec])
                new_d[spec] = _normalize(dir_in[spec] - nrm[spec] * F(2) * kk[:, None])
                lit[i] = False
            facing = _dot(nrm, dir_in) < F(0)
            w = np.where(facing[:, None], nrm, nrm * F(-1))
            u_, v_ = _frame(w)
            dt = mat & ~spec
            if dt.any():
                i = live[dt]
                if tex is not None:
                    thr[i] = thr[i] * O.texture_sample(tex, h["uv"][dt]).astype(F)
                r1 = (TWO_PI * rng.u01(i)).astype(F)
                r2 = (1.0 * rng.u01(i)).astype(F)
                if libm_double:
                    cs, sn = (t.astype(F) for t in _dtrig(r1))
                else:
                    cs, sn = O.trig(r1)
                new_d[dt] = _combine(u_[dt], v_[dt], w[dt], cs, sn, np.sqrt(r2), np.sqrt(F(1) - r2))
            ds = ~mat
            if ds.any():
                i = live[ds]
                r1 = TWO_PI * rng.u01(i)
                r2 = 1.0 * rng.u01(i)
                rng.skip(i, 3)
                cs, sn = (t.astype(F) for t in _dtrig(r1))
                new_d[ds] = _combine(u_[ds], v_[ds], w[ds], cs, sn, np.sqrt(r2).astype(F), np.sqrt(1.0 - r2).astype(F))
            # the emitter loop of the diffuse arms
            dif = ~spec
            if light_sampling and dif.any():
                i = live[dif]
                xs, ws, step_em = x[dif], w[dif], he[dif]
                op = ec[None, :, :] - xs[:, None, :]
                Cs = (op[..., 0] * op[..., 0] + op[..., 1] * op[..., 1]) + op[..., 2] * op[..., 2]
                inside = (Cs <= er2[None, :]).any(axis=1)
                lit[i] = ~inside
                out = ~inside
                io, xs, ws, op, Cs, step_em = i[out], xs[out], ws[out], op[out], Cs[out], step_em[out]
                axes, qs = [], []
                for e in range(len(em)):
                    xi1, xi2 = rng.u01(io), rng.u01(io)
                    q, omega_ = cone(np.broadcast_to(er2[e], Cs[:, e].shape), Cs[:, e])
                    z = xi1 * q
                    ct, sth = (1.0 - z).astype(F), np.sqrt(z * (2.0 - z)).astype(F)
                    phi = (TWO_PI * xi2).astype(F)
                    if libm_double:
                        cs, sn = (t.astype(F) for t in _dtrig(phi))
                    else:
                        cs, sn = O.trig(phi)
                    a = _normalize(op[:, e, :])
                    ua, va = _frame(a)
                    om = _combine(ua, va, a, cs, sn, sth, ct)
                    keep = np.ones(io.size, bool)
                    for aj, qj in zip(axes, qs):
                        e_ = om - aj
                        keep &= ~(0.5 * _dot(e_, e_).astype(D) <= qj)
                    dw = _dot(ws, om)
                    keep &= ~(dw <= F(0))
                    axes.append(a), qs.append(q)
                    if keep.any():
                        sh = osc.raycast(xs[keep], om[keep])
                        scol = _colour(sh, _hit_emitter(sh, mt), mt)  # E1
                        wt = (dw[keep].astype(D) / PI * omega_[keep]).astype(F)
                        ik = io[keep]
                        acc[ik, :3] = acc[ik, :3] + (thr[ik, :3] * scol) * wt[:, None]
                        st["rays_shadow"] += int(keep.sum())
                # E4: the area sample of the emissive triangles
                if mt is not None and io.size and not (mt["cdf"][-1] == 0.0):
                    W = mt["cdf"][-1]
                    xi0, xi1, xi2 = rng.u01(io), rng.u01(io), rng.u01(io)
                    u = xi0 * W
                    e = np.minimum(np.searchsorted(mt["cdf"], u, side="right"), mt["n"] - 1)  # smallest e with cdf_e > u
                    we, ar = mt["weight"][e], mt["area"][e]
                    V0, E1, E2 = mt["v0"][e].astype(D), mt["e1"][e].astype(D), mt["e2"][e].astype(D)
                    s = np.sqrt(xi1)
                    b1, b2 = s * (1.0 - xi2), s * xi2
                    y = (V0 + b1[:, None] * E1) + b2[:, None] * E2
                    dd = y - xs.astype(D)
                    d2 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
                    inv = 1.0 / np.sqrt(d2)
                    od = dd * inv[:, None]
                    om = od.astype(F)
                    N = mt["normal"][e]
                    cosl = np.abs((N[:, 0] * od[:, 0] + N[:, 1] * od[:, 1]) + N[:, 2] * od[:, 2])
                    dw = _dot(ws, om)
                    pdf = ((we / W) * d2) / (ar * cosl)
                    wt = ((dw.astype(D) / PI) / pdf).astype(F)
                    keep = ~(we == 0.0) & ~(d2 == 0.0) & ~(cosl == 0.0) & ~(dw <= F(0)) & np.isfinite(wt) & (step_em != e)
                    for aj, qj in zip(axes, qs):  # the spheres own their cones
                        e_ = om - aj
                        keep &= ~(0.5 * _dot(e_, e_).astype(D) <= qj)
                    if keep.any():
                        sh = osc.raycast(xs[keep], om[keep])
                        she = _hit_emitter(sh, mt)
                        scol = _colour(sh, she, mt)
                        seen = she == e[keep]
                        ik = io[keep][seen]
                        acc[ik, :3] = acc[ik, :3] + (thr[ik, :3] * scol[seen]) * wt[keep][seen][:, None]
                        st["rays_shadow"] += int(keep.sum())
            o[live] = x
            d[live] = new_d
    st["rays_secondary"] += st["rays_shadow"]
    return acc, st


def frame(osc, cam, opts, spheres=None, tex=None, emitters=None):
    """nee_spec.frame with the table: vmx_render_nee's frame [H, W, 5] and the ray counts"""
    W, H = cam.image_res[0], cam.image_res[1]
    kmax = 4 * (cam.rays_per_pixel // 4)
    npix = W * H
    acc = np.zeros((npix, 3), F)
    total = {"rays_primary": 0, "rays_secondary": 0, "rays_shadow": 0, "samples": 0}
    pix = np.arange(npix, dtype=np.int64)
    for k in range(kmax):
        o, d = O.primary_rays(cam, opts, k)
        s, st = radiance(osc, o, d, opts.seed, spheres, opts.sampling, True, tex, pix, np.full(npix, k, np.int64), emitters)
        acc = acc + s[:, :3]
        for key in total:
            total[key] += st[key]
    out = np.empty((npix, 5), F)
    with np.errstate(all="ignore"):
        m = acc / F(kmax)
    m = np.where(F(1) < m, F(1), m)
    out[:, :3] = np.where(m < F(0), F(0), m)
    out[:, 3] = F(1)
    out[:, 4] = F(kmax)
    return out.reshape(H, W, 5), total
