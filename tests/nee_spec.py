"""Light sampling (next-event estimation) restated in numpy: the definition vmx_radiance_nee / vmx_render_nee are held to,
bit for bit (DESIGN.md "Light sampling").  Test infrastructure only.

The estimator is Radiance (pathtracer.cpp:21-198, oracle/vmx_oracle.cpp: radiance) with r2 = U and one more bit of state
per path, `lit`:
  1. RayCast; a miss returns.
  2. !lit: accumColour += accumRadiance * hitColour (the whole vec4).  Depth 0: accumColour.w = distance.
  3. length(hitColour) > 1 returns, lit or not.
  4. Russian roulette, texture sample, branch draw, the specular arm (lit = false) and the diffuse arms, draw for draw.
  5. A diffuse arm leaves w (the flipped normal), the new origin x = hit - dir * 0.001 and the bounce direction, then
  6. runs the emitter loop over the VMX_SPHERE_EMIT spheres in table order:
       op_i = c_i - x, C_i = dot(op_i, op_i) (float32, as sphere_hit forms them);  inside = any C_i <= float(r_i * r_i)
       inside: no draws, lit = false.  Else for every emitter i, xi1 and xi2 drawn (always), then in DOUBLE
         s2 = r_i^2 / C_i   cmax = sqrt(1 - s2)   q_i = s2 / (1 + cmax)   Omega = 2 pi q_i
         z = xi1 q_i        cos t = 1 - z          sin t = sqrt(z (2 - z))
       phi = float(2 pi xi2), cos / sin of it by the kernels' cosf / sinf (LIBM_DOUBLE: C's double functions),
       a_i = normalize(op_i), frame u = normalize(cross(|a.x| > .1 ? (0,1,0) : (1,0,0), a)), v = cross(a, u),
       omega = normalize((u cos(phi) float(sin t) + v sin(phi) float(sin t)) + a float(cos t))       (float32, GLM order)
       dropped if for some emitter j < i: 0.5 * double(|omega - a_j|^2) <= q_j        (the earlier cone owns the direction)
       dropped if dot(w, omega) <= 0
       else RayCast(x, omega) and accumColour.rgb += (accumRadiance.rgb * hitColour) * float(double(dot(w, omega)) / pi * Omega)
     and lit = true.
All float32 arithmetic is one rounding per operation in GLM's order, as the oracle's; every intersection is
OracleScene.raycast, every draw oracle_lib.stream, every cosf / sinf oracle_lib.trig.  Vectorised: each loop iteration is
one Radiance step of all live paths.  light_sampling=False is plain `corrected` (orc_radiance), which pins the rest.
"""
import ctypes as C
import math

import numpy as np

import oracle_lib as O
from vermilion_amd import _lib as L

F = np.float32
TWO_PI = 6.283185307179586
PI = 3.141592653589793
_DRAWS_PER_STEP = 8 + 2 * 16  # roulette, branch, three unused or two + three, two per emitter (at most 16 spheres)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _normalize(v):
    s = F(1.0) / np.sqrt(_dot(v, v))
    return v * s[:, None]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0],
                     a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], axis=1)


def _frame(w):
    """(u, v) of the reference's basis around w (pathtracer.cpp:158-161)"""
    use_y = np.abs(w[:, 0]).astype(np.float64) > .1
    ax = np.zeros_like(w)
    ax[:, 0] = np.where(use_y, F(0), F(1))
    ax[:, 1] = np.where(use_y, F(1), F(0))
    u = _normalize(_cross(ax, w))
    return u, _cross(w, u)


def _dtrig(x):
    """C's double cos / sin, element by element (numpy's own vector forms need not round as libm does)"""
    x = np.asarray(x, np.float64)
    return (np.fromiter((math.cos(v) for v in x), np.float64, len(x)),
            np.fromiter((math.sin(v) for v in x), np.float64, len(x)))


def _combine(u, v, w, cs, sn, a, b):
    """normalize((u cs a + v sn a) + w b)"""
    return _normalize((u * cs[:, None] * a[:, None] + v * sn[:, None] * a[:, None]) + w * b[:, None])


def table_of(spheres):
    """the ctypes sphere table (None: the reference's eight) as arrays"""
    if spheres is None:
        n = C.c_uint32(0)
        p = O.lib().orc_default_spheres(C.byref(n))
        spheres = [p[i] for i in range(n.value)]
    return {"centre": np.array([list(s.centre) for s in spheres], F).reshape(-1, 3),
            "radius": np.array([s.radius for s in spheres], F),
            "emit": np.array([bool(s.flags & L.VMX_SPHERE_EMIT) for s in spheres], bool)}


def cone(rad2, C_):
    """(q, Omega) in double from float32 r * r and |c - x|^2"""
    s2 = rad2.astype(np.float64) / C_.astype(np.float64)
    cmax = np.sqrt(1.0 - s2)
    q = s2 / (1.0 + cmax)
    return q, TWO_PI * q


class _Streams:
    """draw j of path i: oracle_lib.stream(seed, pixel_i, k_i), past the two jitter draws"""

    def __init__(self, seed, pixel, k):
        self.seed, self.pixel, self.k = int(seed), pixel, k
        self.n = len(pixel)
        self.pos = np.zeros(self.n, np.int64)
        self.row = np.full(self.n, -1, np.int64)
        self.cap = 0
        self.buf = np.zeros((0, 0), np.uint64)

    def reserve(self, live, need):
        """every live path can take `need` more draws"""
        if live.size == 0 or (self.cap and int(self.pos[live].max()) + need <= self.cap and (self.row[live] >= 0).all()):
            return
        top = int(self.pos[live].max()) + need
        self.cap = max(256, self.cap)
        while self.cap < top:
            self.cap *= 2
        self.buf = np.empty((live.size, self.cap), np.uint64)
        self.row[:] = -1
        for r, i in enumerate(live):
            self.buf[r] = O.stream(self.seed, int(self.pixel[i]), int(self.k[i]), self.cap + 2)[2:]
        self.row[live] = np.arange(live.size)

    def u01(self, idx):
        """the next draw of the paths idx as uniform_real_distribution<double>(0, 1) stands in (52 mantissa bits)"""
        x = self.buf[self.row[idx], self.pos[idx]]
        self.pos[idx] += 1
        return ((x >> np.uint64(12)) | np.uint64(0x3FF0000000000000)).view(np.float64) - 1.0

    def skip(self, idx, n):
        self.pos[idx] += n


def radiance(osc, o, d, seed, spheres=None, sampling=L.VMX_SAMPLING_CORRECTED, light_sampling=True, tex=None, pixel=None,
             k=None, trace=None):
    """Radiance with light sampling for the rays (o, d): path i on stream (seed, pixel[i], k[i]) (default (seed, i, 0)),
    unclamped accumColour [n, 4] float32 and the ray counts.  osc: the OracleScene (built with `spheres`, `tex` bound);
    tex: the bound texture or None.  trace: a dict that receives per-step records (tests of the cone and the inside rule)."""
    assert (sampling & 0xFF) == L.VMX_SAMPLING_CORRECTED
    libm_double = bool(sampling & L.VMX_SAMPLING_LIBM_DOUBLE)
    tb = table_of(spheres)
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
            rng.reserve(live, _DRAWS_PER_STEP)
            st["rays_secondary"] += int((np.isfinite(d[live]).all(axis=1) & (depth[live] > 0)).sum())
            h = osc.raycast(o[live], d[live])
            hit = (h["flags"] & 1) != 0
            live, h = live[hit], h[hit]  # :36-41
            col = h["colour"].astype(F)
            add = ~lit[live]
            ia = live[add]
            acc[ia, :3] = acc[ia, :3] + thr[ia, :3] * col[add]  # :43
            acc[ia, 3] = acc[ia, 3] + thr[ia, 3] * F(0)
            d0 = depth[live] == 0
            acc[live[d0], 3] = h["distance"][d0]  # :44-47
            go = ~(np.sqrt(_dot(col, col)) > F(1))  # :52
            live, h = live[go], h[go]
            depth[live] += 1
            rr = depth[live] > 5  # :56-59
            ends = np.zeros(live.size, bool)
            if rr.any():
                u = rng.u01(live[rr])
                ends[rr] = (u > float(F(0.95))) | (depth[live[rr]] > 1000)
            live, h = live[~ends], h[~ends]
            if live.size == 0:
                break
            mat = (h["flags"] & 2) != 0
            dir_in = d[live].copy()
            nrm = h["normal"].astype(F)
            x = h["location"].astype(F) - dir_in * F(0.001)
            spec = np.zeros(live.size, bool)
            if mat.any():
                spec[mat] = rng.u01(live[mat]) >= 0.96  # :98
            new_d = np.zeros((live.size, 3), F)
            # specular arm (:98-109)
            if spec.any():
                i = live[spec]
                rng.skip(i, 3)
                kk = _dot(nrm[spec], dir_in[spec])
                new_d[spec] = _normalize(dir_in[spec] - nrm[spec] * F(2) * kk[:, None])
                lit[i] = False
            facing = _dot(nrm, dir_in) < F(0)
            w = np.where(facing[:, None], nrm, nrm * F(-1))
            u_, v_ = _frame(w)
            # diffuse arm on a triangle (:151-165)
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
            # diffuse arm on a sphere (:166-196)
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
                xs, ws = x[dif], w[dif]
                op = ec[None, :, :] - xs[:, None, :]  # [paths, emitters, 3]
                Cs = (op[..., 0] * op[..., 0] + op[..., 1] * op[..., 1]) + op[..., 2] * op[..., 2]
                inside = (Cs <= er2[None, :]).any(axis=1)
                lit[i] = ~inside
                if trace is not None:
                    trace.setdefault("inside", []).append((i[inside].copy(), rng.pos[i[inside]].copy(), lit[i[inside]].copy()))
                out = ~inside
                io, xs, ws, op, Cs = i[out], xs[out], ws[out], op[out], Cs[out]
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
                        keep &= ~(0.5 * _dot(e_, e_).astype(np.float64) <= qj)
                    dw = _dot(ws, om)
                    keep &= ~(dw <= F(0))
                    axes.append(a), qs.append(q)
                    if trace is not None:
                        trace.setdefault("cone", []).append((int(em[e]), a.copy(), q.copy(), om.copy(), omega_.copy(),
                                                             Cs[:, e].copy()))
                    if keep.any():
                        sh = osc.raycast(xs[keep], om[keep])
                        wt = (dw[keep].astype(np.float64) / PI * omega_[keep]).astype(F)
                        ik = io[keep]
                        acc[ik, :3] = acc[ik, :3] + (thr[ik, :3] * sh["colour"].astype(F)) * wt[:, None]
                        st["rays_shadow"] += int(keep.sum())
            o[live] = x
            d[live] = new_d
    st["rays_secondary"] += st["rays_shadow"]
    return acc, st


def frame(osc, cam, opts, spheres=None, tex=None):
    """vmx_render_nee's frame [H, W, 5]: per pixel the samples k = 0 .. 4 (spp / 4) - 1 added in ascending order, rgb =
    max(min(sum / n, 1), 0), alpha 1, the sample count; and the ray counts"""
    W, H = cam.image_res[0], cam.image_res[1]
    kmax = 4 * (cam.rays_per_pixel // 4)
    npix = W * H
    acc = np.zeros((npix, 3), F)
    total = {"rays_primary": 0, "rays_secondary": 0, "rays_shadow": 0, "samples": 0}
    pix = np.arange(npix, dtype=np.int64)
    for k in range(kmax):
        o, d = O.primary_rays(cam, opts, k)
        s, st = radiance(osc, o, d, opts.seed, spheres, opts.sampling, True, tex, pix, np.full(npix, k, np.int64))
        acc = acc + s[:, :3]
        for key in total:
            total[key] += st[key]
    out = np.empty((npix, 5), F)
    with np.errstate(all="ignore"):
        m = acc / F(kmax)
    m = np.where(F(1) < m, F(1), m)  # std::min(x, 1.f): (1 < x) ? 1 : x
    out[:, :3] = np.where(m < F(0), F(0), m)
    out[:, 3] = F(1)
    out[:, 4] = F(kmax)
    return out.reshape(H, W, 5), total
