// pixel_claim.h — "every camera ray of this pixel hits triangle T" (or: "hits no triangle"), decided once per pixel.
//
// Plain float C++ for host and device, compiled with -ffp-contract=off on both sides: k_pixel_claims (vmx_kernels.hip)
// and the stand-alone host program tests/cpp/pixel_claim_test.cpp run the same arithmetic and give the same table.
//
// The claim of pixel p is a 32-bit word: kClaimNone, kClaimMiss, or the leaf-order slot of a triangle T.  Contract of a
// slot claim: for every direction primary_ray_keyed can produce for p, BVH::getIntersection (bvh.cpp:47-145) over this
// tree returns T with the t that tri_test_cam computes for T; of kClaimMiss: it returns no hit.  k_trace_w<0> then
// replaces the ray's BVH walk by one triangle test.
//
// Geometry.  All camera rays start at the frame's origin; the tables of k_camera_tables hold the node boxes and the
// triangle records relative to it.  A ray direction of pixel p is d = w / |w| with w = ah + delta, ah the unit centre
// direction of the pixel's film rectangle and |delta| <= rho (pixel_cone: half the pixel's film diagonal over the
// distance of the film point, + 1 %; here widened once more, kConeWiden).  With sin(phi) <= 0.5 (the half-angle
// pixel_sphere_bound accepts) |w| lies in [0.5, 1.5].
//
// Linear forms.  With the camera-relative record (e1, e2, tvec, qvec, cd) the reference's test (triangle.cpp:4-54) is
//   det = d.N, N = e2 x e1      u det = d.A, A = e2 x tvec      v det = d.qvec      t det = cd
// so over the cone every quantity it compares is a linear form L.w, which lies in L.ah +- rho |L| (pc_range).  The
// float results of the reference differ from the exact forms by the roundings of one cross and one dot product:
// at most 9 x 2^-24 |e1||e2| for det, 9 x 2^-24 |tvec||e2| for u det, 3 x 2^-24 |qvec| <= 3 x 2^-24 |tvec||e1| for
// v det (|d| = 1).  The forms here (N, A and the dot with ah) are computed in float as well, with the same kind of
// error, and a bound on L.w is one on L.d only up to |w| <= 1.5.  Every sign test below therefore asks for
//   |L.w| > kSlack x (the product of the two lengths),  kSlack = 2^-17 = 128 x 2^-24
// — an ABSOLUTE slack scaled by |tvec||e|, never one relative to u or v — which is 1.5 x (9 + 9) x 2^-24 with a
// factor 4 to spare.  Lengths outside [1e-6, 1e6] give "unsure": no product under- or overflows.
//
// Margins of the procedure (pc_pixel_claim):
//   (a) T is accepted by every ray: sign(det) fixed with |det| > slack + 1.5e-8 (the reference's 1e-8 parallel test),
//       s u det > slack, s v det > slack, s (det - u det - v det) > the three slacks + 2^-16 det (u + v < 1 by more
//       than the 4 x 2^-24 of forming u, v and their sum in float; with v >= 0 it also gives u <= 1), s cd > 0.
//   (b) any other triangle U in a node the cone may reach no later than T is SURELY REJECTED (det surely below 1e-8,
//       or, with sign(det) fixed: u < 0, v < 0 or u + v > 1 by the slacks, or s cd <= 0, whose sign is exact) or
//       SURELY FARTHER: |cd_U| (s_T N_T.w - slack_T) > (1 + 2^-16) |cd_T| (s_U N_U.w + slack_U), again one linear
//       form; the slacks bound the float det of either side, 2^-16 the three roundings of t = cd * (1 / det).
//       Anything else (a coincident duplicate, a sliver whose det changes sign inside the cone, a neighbour across
//       an edge nearer than the slacks) ends the pixel as kClaimNone.
//       Boxes are culled geometrically and only towards keeping: a box grown by 2^-18 (|lo| + |hi|) per axis against
//       the per-axis ranges of w (a pyramid around the cone) and the distance t_max(T) (1 + 2^-10).
//   (c) the reference reaches T: for every ray the hit point lies inside T's own box (from the record's vertices; the
//       tree's boxes contain it up to 2^-24 |e|) by 2^-19 (|lo| + |hi|) + 2^-22 |e| on each axis where that box has
//       extent — 8 times the three roundings of a slab product (bbox.cpp:72-73), so every slab interval of the leaf
//       and, boxes being nested and rounding monotonic, of every ancestor contains t_T and `near <= far` holds; an
//       axis without extent has equal slab products, within 3 x 2^-24 of t_T, inside the other axes' intervals by
//       the same slack.  No ancestor is pruned (bvh.cpp:69): its near <= t_T (1 + 3 x 2^-24), while the nearest hit
//       so far is T's own or a U's, which is farther by 2^-16.  A cone within rho + 2^-16 of a coordinate plane gives
//       kClaimNone: no zero direction component, infinite reciprocal or NaN slab ever meets a claim.
//   (d) kClaimNone as well on: any NaN or infinity (every comparison is written so that a NaN fails it), a degenerate
//       film, sin(phi) > 0.5, a stack deeper than the caller's, and more than kClaimBudget node and triangle visits.
// kClaimMiss is the same walk with no T and no distance cut: every reached triangle is surely rejected.
// Checked against the reference's own arithmetic in tests/test_pixel_claims.py.
#pragma once
#include <math.h>
#include <stdint.h>
#include "vmx_device.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VMX_PC_FN __host__ __device__ __forceinline__
#else
#define VMX_PC_FN inline
#endif

namespace vmx {

constexpr uint32_t kClaimNone = 0xFFFFFFFFu;
constexpr uint32_t kClaimMiss = 0xFFFFFFFEu;
constexpr uint32_t kClaimBudget = 384;           // node + triangle visits of the culled walk per pixel
constexpr float kPcSlack = 7.62939453125e-06f;   // 2^-17
constexpr float kPcRel = 1.52587890625e-05f;     // 2^-16
constexpr float kPcBoxGrow = 3.814697265625e-06f;  // 2^-18
constexpr float kPcConeWiden = 1.02f;
constexpr float kPcAxisClear = 1.52587890625e-05f;  // 2^-16
constexpr float kPcLenMin = 1e-6f, kPcLenMax = 1e6f;
constexpr float kPcNoCut = 3e9f;  // beyond the reference's 999999999 for every |w| >= 0.5

// the film of a frame, as FrameDev holds it (m: column-major 3x3 camera matrix)
struct PcFilm {
    float m[9];
    uint32_t width, height;
    float sensor_x, sensor_y, film_dist;
};

struct PcCone {
    float ax, ay, az;     // unit centre direction
    float rho;            // |w - a| <= rho
    float il[3], ih[3];   // per axis, for the axis mirrored to a positive direction: 1 / (|a_k| - rho), 1 / (|a_k| + rho)
    bool neg[3];          // a_k < 0
    bool ok;
};

VMX_PC_FN bool pc_finite(float x) { return fabsf(x) <= 3.0e38f; }  // false on NaN

// pixel_cone of the kernels (same film point, same 1 % on the half diagonal), normalised, with guards (c) and (d)
VMX_PC_FN PcCone pc_cone(const PcFilm &fm, uint32_t p) {
    const float fw = (float)fm.width, fh = (float)fm.height;
    const float hx = ((float)(p % fm.width) - 0.25f) / fw - 0.5f;
    const float hy = ((float)(p / fm.width) - 0.25f) / fh - 0.5f;
    const float gx = hx * fm.sensor_x, gy = -(hy * fm.sensor_y), gz = -fm.film_dist;
    const float ax = fm.m[0] * gx + fm.m[3] * gy + fm.m[6] * gz;
    const float ay = fm.m[1] * gx + fm.m[4] * gy + fm.m[7] * gz;
    const float az = fm.m[2] * gx + fm.m[5] * gy + fm.m[8] * gz;
    const float alen = sqrtf(ax * ax + ay * ay + az * az);
    const float px = fm.sensor_x / fw, py = fm.sensor_y / fh;
    const float sphi = 0.505f * sqrtf(px * px + py * py) / alen;
    PcCone c;
    c.ax = ax / alen, c.ay = ay / alen, c.az = az / alen;
    c.rho = sphi * kPcConeWiden + 9.5367431640625e-07f;
    c.ok = alen > 0.0f && pc_finite(alen) && sphi <= 0.5f && sphi > 0.0f;
    const float a[3] = {c.ax, c.ay, c.az};
    for (int k = 0; k < 3; ++k) {
        const float m = fabsf(a[k]);
        c.neg[k] = a[k] < 0.0f;
        if (!(m > c.rho + kPcAxisClear)) c.ok = false;  // (NaN: no claim)
        c.il[k] = 1.0f / (m - c.rho);
        c.ih[k] = 1.0f / (m + c.rho);
    }
    return c;
}

struct PcRange {
    float lo, hi;
};
VMX_PC_FN PcRange pc_range(const PcCone &c, float lx, float ly, float lz) {
    const float mid = lx * c.ax + ly * c.ay + lz * c.az;
    const float r = c.rho * sqrtf(lx * lx + ly * ly + lz * lz);
    return PcRange{mid - r, mid + r};
}

// what the cone's rays can do with one triangle
enum PcClass { kPcRejected = 0, kPcLive = 1, kPcUnsure = 2 };
struct PcTri {
    float nx, ny, nz;   // s N: s det = d.(s N) > 0 over the cone
    float dlo, dhi;     // range of s N.w
    float sd;           // slack of det
    float acd;          // |cd|
    bool covers;        // (a): every ray of the cone is accepted
};

// rec: the 16 floats of a k_camera_tables triangle record — e1, e2, tvec, qvec, cd
VMX_PC_FN PcClass pc_classify(const PcCone &c, const float *rec, PcTri &o) {
    const float e1x = rec[0], e1y = rec[1], e1z = rec[2], e2x = rec[3], e2y = rec[4], e2z = rec[5];
    const float tx = rec[6], ty = rec[7], tz = rec[8], qx = rec[9], qy = rec[10], qz = rec[11], cd = rec[12];
    const float E1 = sqrtf(e1x * e1x + e1y * e1y + e1z * e1z), E2 = sqrtf(e2x * e2x + e2y * e2y + e2z * e2z);
    const float TV = sqrtf(tx * tx + ty * ty + tz * tz);
    if (!(pc_finite(E1) && pc_finite(E2) && pc_finite(TV) && pc_finite(cd) && pc_finite(qx) && pc_finite(qy) && pc_finite(qz)))
        return kPcUnsure;
    const float nx = e2y * e1z - e2z * e1y, ny = e2z * e1x - e2x * e1z, nz = e2x * e1y - e2y * e1x;  // e2 x e1
    const PcRange det = pc_range(c, nx, ny, nz);
    const float sd = kPcSlack * (E1 * E2);
    if (!(E1 <= kPcLenMax && E2 <= kPcLenMax && TV <= kPcLenMax)) return kPcUnsure;
    // surely parallel: |det| <= 9.99999993922529e-09 for every ray (|d.N| <= 2 |w.N|)
    if (2.0f * fmaxf(fabsf(det.lo), fabsf(det.hi)) + sd < 9.9e-9f) return kPcRejected;
    if (!(E1 >= kPcLenMin && E2 >= kPcLenMin && TV >= kPcLenMin)) return kPcUnsure;
    float s;
    if (det.lo > sd + 1.5e-8f) s = 1.0f;
    else if (det.hi < -(sd + 1.5e-8f)) s = -1.0f;
    else return kPcUnsure;
    if (!(s * cd > 0.0f)) return kPcRejected;  // t = cd * (1 / det) <= 0 (or -0): the sign of the product is exact
    const float ax_ = e2y * tz - e2z * ty, ay_ = e2z * tx - e2x * tz, az_ = e2x * ty - e2y * tx;  // e2 x tvec
    const PcRange u = pc_range(c, s * ax_, s * ay_, s * az_);
    const PcRange v = pc_range(c, s * qx, s * qy, s * qz);
    const PcRange w = pc_range(c, s * (nx - ax_ - qx), s * (ny - ay_ - qy), s * (nz - az_ - qz));  // s (det - u det - v det)
    const float su = kPcSlack * (TV * E2), sv = kPcSlack * (TV * E1);
    const float dlo = s > 0.0f ? det.lo : -det.hi, dhi = s > 0.0f ? det.hi : -det.lo;
    const float sw = su + sv + sd + kPcRel * dhi;
    if (u.hi < -su || v.hi < -sv || w.hi < -sw) return kPcRejected;
    o.nx = s * nx, o.ny = s * ny, o.nz = s * nz;
    o.dlo = dlo, o.dhi = dhi, o.sd = sd, o.acd = fabsf(cd);
    o.covers = u.lo > su && v.lo > sv && w.lo > sw && dlo > 2.0f * sd;
    return kPcLive;
}

// (c): the hit point of every ray of the cone lies inside the box of T's own vertices, by the slab slack, on every axis
// where that box has extent
VMX_PC_FN bool pc_inside_own_box(const PcCone &c, const float *rec, const PcTri &t) {
    const float E12 = t.sd * (1.0f / kPcSlack);  // |e1||e2|
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        const float p0 = -rec[6 + k], p1 = p0 + rec[k], p2 = p0 + rec[3 + k];
        const float mn = fminf(p0, fminf(p1, p2)), mx = fmaxf(p0, fmaxf(p1, p2));
        if (rec[k] == 0.0f && rec[3 + k] == 0.0f) continue;  // no extent: v1 = v2 = v0 on this axis
        const float sl = 1.9073486328125e-06f * (fabsf(mn) + fabsf(mx)) + 2.384185791015625e-07f * (fabsf(rec[k]) + fabsf(rec[3 + k]));
        const float lo = mn + sl, hi = mx - sl;
        const float ek[3] = {k == 0 ? t.acd : 0.0f, k == 1 ? t.acd : 0.0f, k == 2 ? t.acd : 0.0f};
        // tau w_k >= lo with tau = |cd| / (s N.w)  <=>  (|cd| e_k - lo s N).w >= 0, and likewise for hi
        const PcRange a = pc_range(c, ek[0] - lo * t.nx, ek[1] - lo * t.ny, ek[2] - lo * t.nz);
        const PcRange b = pc_range(c, hi * t.nx - ek[0], hi * t.ny - ek[1], hi * t.nz - ek[2]);
        const float es = kPcSlack * (t.acd + (fabsf(mn) + fabsf(mx)) * E12);
        if (!(a.lo > es && b.lo > es)) ok = false;
    }
    return ok;
}

// (b): U is hit later than T by every ray of the cone
VMX_PC_FN bool pc_farther(const PcCone &c, const PcTri &t, const PcTri &u) {
    const float ku = u.acd, kt = (1.0f + kPcRel) * t.acd;
    const PcRange r = pc_range(c, ku * t.nx - kt * u.nx, ku * t.ny - kt * u.ny, ku * t.nz - kt * u.nz);
    return r.lo > (ku * t.sd + kt * u.sd) * 1.5f;
}

// may a ray of the cone meet the box (lo, hi: camera-relative) at a distance tau <= tcut along w?  Errs towards yes.
VMX_PC_FN bool pc_box_reached(const PcCone &c, const float *lo, const float *hi, float tcut) {
    float tmn = 0.0f, tmx = tcut;
    for (int k = 0; k < 3; ++k) {
        const float g = kPcBoxGrow * (fabsf(lo[k]) + fabsf(hi[k])) + 1e-30f;
        const float l = (c.neg[k] ? -hi[k] : lo[k]) - g, h = (c.neg[k] ? -lo[k] : hi[k]) + g;
        const float a = l >= 0.0f ? l * c.ih[k] : l * c.il[k];
        const float b = h >= 0.0f ? h * c.il[k] : h * c.ih[k];
        tmn = fmaxf(tmn, a);  // (fmaxf / fminf drop a NaN operand: towards keeping)
        tmx = fminf(tmx, b);
    }
    return !(tmn > tmx);
}

// Nearest accepted triangle of the ray (dx, dy, dz) from the frame's origin: the candidate T.  Its tests are those of
// tri_test_cam and a plain slab test; the claim does not rest on this walk — a wrong candidate fails (a) or (b).
// It is a walk of its own rather than the kernels' bvh_nearest so that the host program runs the same code.  Where its
// fminf / fmaxf slab test could differ from the reference's compare-select form (a NaN slab, a zero direction component)
// the cone lies on a coordinate plane and pc_cone has already answered kClaimNone; for every other ray both forms
// compute the same products and the same min / max, so the candidate is the reference's nearest triangle and no claim
// share is lost to it (tests/test_pixel_claims.py holds the share against the oracle's own).  The `guard` bound only
// keeps a corrupt table from looping: a walk visits each of the at most 2^27 nodes once.
// Stack: put(int level, uint32_t ref, float near) / get(int level, uint32_t &ref, float &near)
template <class Stack>
VMX_PC_FN int pc_nearest(const float *cam_inner, const float *cam_tris, uint32_t root_ref, float dx, float dy, float dz,
                         Stack &stk, int max_sp) {
    const float ix = 1.0f / dx, iy = 1.0f / dy, iz = 1.0f / dz;
    float best = 999999999.f;
    int slot = -1, sp = 0;
    uint32_t cur = root_ref;
    float cur_near = -9999999.f;
    bool have = true;
    for (uint32_t guard = 0; guard < 0x10000000u; ++guard) {
        if (!have) {
            if (sp == 0) break;
            --sp;
            stk.get(sp, cur, cur_near);
        }
        have = false;
        if (cur_near > best) continue;
        if (cur & kLeafBit) {
            const uint32_t first = cur & kLeafStartMask, n = (cur >> kLeafCountShift) & 31u;
            for (uint32_t i = 0; i < n; ++i) {
                const float *r = cam_tris + (size_t)(first + i) * 16;
                const float pvx = dy * r[5] - dz * r[4], pvy = dz * r[3] - dx * r[5], pvz = dx * r[4] - dy * r[3];
                const float det = r[0] * pvx + r[1] * pvy + r[2] * pvz;
                const float inv = 1.0f / det;
                const float u = (r[6] * pvx + r[7] * pvy + r[8] * pvz) * inv;
                const float v = (dx * r[9] + dy * r[10] + dz * r[11]) * inv;
                const float dist = r[12] * inv;
                const bool hit = !(fabsf(det) <= 9.99999993922529e-09f) && !(u < 0.0f || u > 1.0f) && !(v < 0.0f || u + v > 1.0f) && dist > 0.0f;
                if (hit && dist < best) best = dist, slot = (int)(first + i);
            }
        } else {
            const float *q = cam_inner + (size_t)cur * 16;
            float tn[2];
            bool h[2];
            for (int s = 0; s < 2; ++s) {
                const float *b = q + s * 6;
                const float t0x = b[0] * ix, t0y = b[1] * iy, t0z = b[2] * iz, t1x = b[3] * ix, t1y = b[4] * iy, t1z = b[5] * iz;
                const float n = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
                const float f = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
                tn[s] = n, h[s] = n <= f;
            }
            uint32_t lref, rref;
            __builtin_memcpy(&lref, q + 12, 4), __builtin_memcpy(&rref, q + 13, 4);
            if (h[0] && h[1]) {
                const bool sw = tn[1] < tn[0];
                if (sp >= max_sp) return -2;
                stk.put(sp, sw ? lref : rref, sw ? tn[0] : tn[1]);
                ++sp;
                cur = sw ? rref : lref, cur_near = sw ? tn[1] : tn[0], have = true;
            } else if (h[0]) {
                cur = lref, cur_near = tn[0], have = true;
            } else if (h[1]) {
                cur = rref, cur_near = tn[1], have = true;
            }
        }
    }
    return slot;
}

// The per-pixel procedure over the camera-relative tables (octant-0 node copy, triangle records) of the frame's origin
// (cand_out: the candidate of the centre ray, -1: it hits nothing, -2: no cone or no walk; other_out: the live triangle
// that ended the culled walk, or -1 — pc_pixel_list starts from the two)
template <class Stack>
VMX_PC_FN uint32_t pc_pixel_claim_cand(const PcFilm &fm, uint32_t p, const float *cam_inner, const float *cam_tris,
                                       uint32_t root_ref, Stack &stk, int max_sp, int &cand_out, int &other_out) {
    const PcCone c = pc_cone(fm, p);
    cand_out = -2, other_out = -1;
    if (!c.ok) return kClaimNone;
    const int cand = pc_nearest(cam_inner, cam_tris, root_ref, c.ax, c.ay, c.az, stk, max_sp);
    if (cand < -1) return kClaimNone;
    cand_out = cand;
    PcTri T;
    T.nx = T.ny = T.nz = T.dlo = T.dhi = T.sd = T.acd = 0.0f, T.covers = false;
    float tcut = kPcNoCut;
    if (cand >= 0) {
        const float *rec = cam_tris + (size_t)cand * 16;
        if (pc_classify(c, rec, T) != kPcLive || !T.covers) return kClaimNone;
        if (!pc_inside_own_box(c, rec, T)) return kClaimNone;
        const float thi = T.acd / (T.dlo - T.sd);  // the largest tau = t |w| of the cone, float det included
        if (!(thi > 1e-20f && thi < 1e8f)) return kClaimNone;
        tcut = thi * (1.0f + 9.765625e-04f);
    }
    // the culled walk: every node the cone may reach no later than tcut
    uint32_t visits = 0;
    int sp = 0;
    uint32_t cur = root_ref;
    for (;;) {
        if (++visits > kClaimBudget) return kClaimNone;
        if (cur & kLeafBit) {
            const uint32_t first = cur & kLeafStartMask, n = (cur >> kLeafCountShift) & 31u;
            visits += n;
            for (uint32_t i = 0; i < n; ++i) {
                if ((int)(first + i) == cand) continue;
                PcTri U;
                const PcClass k = pc_classify(c, cam_tris + (size_t)(first + i) * 16, U);
                if (k == kPcRejected) continue;
                if (cand < 0 || k == kPcUnsure || !pc_farther(c, T, U)) {
                    if (k == kPcLive) other_out = (int)(first + i);
                    return kClaimNone;
                }
            }
            if (sp == 0) break;
            float unused;
            stk.get(--sp, cur, unused);
        } else {
            const float *q = cam_inner + (size_t)cur * 16;
            const bool h0 = pc_box_reached(c, q, q + 3, tcut), h1 = pc_box_reached(c, q + 6, q + 9, tcut);
            uint32_t lref, rref;
            __builtin_memcpy(&lref, q + 12, 4), __builtin_memcpy(&rref, q + 13, 4);
            if (h0 && h1) {
                if (sp >= max_sp) return kClaimNone;
                stk.put(sp++, rref, 0.0f);
                cur = lref;
            } else if (h0) {
                cur = lref;
            } else if (h1) {
                cur = rref;
            } else {
                if (sp == 0) break;
                float unused;
                stk.get(--sp, cur, unused);
            }
        }
    }
    return cand >= 0 ? (uint32_t)cand : kClaimMiss;
}
template <class Stack>
VMX_PC_FN uint32_t pc_pixel_claim(const PcFilm &fm, uint32_t p, const float *cam_inner, const float *cam_tris,
                                  uint32_t root_ref, Stack &stk, int max_sp) {
    int cand, other;
    return pc_pixel_claim_cand(fm, p, cam_inner, cam_tris, root_ref, stk, max_sp, cand, other);
}

// ---------------------------------------------------------------------------------------------------------------------
// List claims — for a pixel whose claim is kClaimNone: a short list L = {T1..Tk}, k <= kListK, of leaf-order slots.
// Record of a pixel: kListWords words, the slots padded with kClaimNone (one 16-byte load).  An empty list is
// kListWords x kClaimNone.
//
// Per-ray rule (pc_list_settle).  The ray's own test (pc_ray_test: the operations of tri_test_cam, same bits) runs on
// every member.  The ray WALKS
//   - if no member accepts it,
//   - if the two smallest accepted distances lie within 2^-16 (kPcRel) of each other, equality included (the
//     reference's test order decides such ties),
//   - or if the nearest member's hit lies within the containment band of (3).
// Otherwise it is settled with that member's (t, slot).  Contract: whenever the rule settles a ray of the pixel,
// BVH::getIntersection returns exactly that pair.  A list may settle none of the pixel's rays; there is no coverage
// condition.
//
// Why a settled ray is right.  Let m be the winner and t its float distance.
//   (1) Members are kPcLive: sign(det) fixed over the cone, lengths in range, s cd > 0.  So for every ray of the cone
//       that m accepts, t |w| <= thi(m) = |cd| / (dlo - sd), as for T in (b) above.
//   (2) Non-members.  The culled walk of (b) runs with tcut = max thi(m) (1 + 2^-10) over the FINAL list: whenever a
//       reached triangle joins, the walk restarts from the root with the new list.  That is at most kListK restarts;
//       the first two candidates come from pc_pixel_claim_cand's own walk.  So the walk that ends has seen every
//       triangle in a node the cone may reach no later than the final tcut, and each was a member, surely rejected, or
//       surely farther (pc_farther) than EVERY member, hence farther than m by 2^-16 for this ray.  A kPcUnsure
//       triangle, a join that would overflow, or a joining triangle that is not kPcLive with a distance in range: no
//       list.  A triangle in a node beyond tcut is hit, if at all, beyond every member's distance.  So no non-member
//       is accepted at a distance <= t (1 + 2^-16).
//   (3) The reference reaches m (pc_hit_in_own_box).  (c) cannot ask that the whole cone's hits lie inside m's box, so
//       the rule asks it of the ray.  Let mn_k, mx_k be the box of m's vertices from the record, as in
//       pc_inside_own_box, and sl_k = 2^-19 (|mn| + |mx|) + 2^-22 |e| the same slab slack: 8 times the three roundings
//       of a slab product (bbox.cpp:72-73) plus the one of the product below, and the 2^-24 |e| by which the tree's
//       boxes contain the vertices.
//       (3a) The box has extent on all three axes.  The rule asks t d_k in [mn_k + sl_k, mx_k - sl_k] for every k.
//            Then every slab interval of the leaf and, boxes being nested and rounding monotonic, of every ancestor
//            contains the float t itself, whatever the accuracy of t: `near <= far` holds, and near <= t (1 + 3 x
//            2^-24).
//       (3b) The box has no extent on axis f (a triangle in a coordinate plane: a wall, a floor).  There both slab
//            products of m's own box are the one number s = p0_f * (1 / d_f), computed here as bbox.cpp computes it,
//            and the float t of the triangle test need NOT agree with it: for a thin triangle in such a plane the
//            terms of det and cd cancel, and t is off by up to 2^-7 relative while the slab slack is 2^-19.  So the
//            rule does not rest on t there.  It asks |s - t| <= 2^-17 t, and s d_k in [mn_k + sl_k, mx_k - sl_k] on
//            the two other axes as well as t d_k.  Then every slab interval of the leaf and of every ancestor
//            contains s (on axis f by nesting, on the others by the slack), so `near <= far` holds and
//            near <= s (1 + 3 x 2^-24) <= t (1 + 2^-17) (1 + 3 x 2^-24).  Two axes without extent: the ray walks.
//       In both cases no node on the way to m is pruned (bvh.cpp:69): its near is below t (1 + 2^-16), while the
//       nearest hit so far is a non-member's (farther by 2^-16, (2)) or another member's (farther by more than 2^-16:
//       the tie band of the rule).  The band is absolute and a few 2^-19 of the coordinates wide: a triangle thinner
//       than that along an axis settles no ray.
//       (A band on the barycentrics, u, v, 1 - u - v >= delta, was built first.  Its delta has to cover the float
//       error of u, v and t over the whole cone: 0.015 for the median list pixel of the 1080p bench frame, as wide as
//       the pixel, and 40 % of the unclaimed rays settled.)
//   (4) Other members are tested by the rule itself with the reference's arithmetic.  Those that accept lie beyond
//       t (1 + 2^-16) and lose whatever the order; those that reject are rejected by the reference as well.
//   (5) The guards of (c) and (d) stay: pc_cone's answer on a coordinate plane (so no d_k is zero), NaN (every
//       comparison fails on one), stack depth, and kListBudget node and triangle visits over all restarts together.
// kListK = 4: the shares of list lengths on the 1080p bench frame are in profiles/claim_lists.txt; K = 3 loses 3 % of
// the pixels without a single claim.  kListBudget: the walks of one pixel restart at most four times and each is a
// kClaimBudget-sized walk with a longer tcut; the largest pixel of that frame takes 659 visits, none is lost to it.
// Checked against the oracle in tests/test_claim_lists.py.
#ifndef VMX_PC_WHY
#define VMX_PC_WHY(code)  // (tools/claim_list_shares.py --why: the host program counts why a pixel got no list)
#endif
constexpr int kListK = 4;
constexpr int kListWords = 4;
constexpr uint32_t kListBudget = 1536;

// the reference's triangle test on a camera-relative record, with its u and v: the operations of tri_test_cam
VMX_PC_FN bool pc_ray_test(const float *r, float dx, float dy, float dz, float &dist, float &u, float &v) {
    const float pvx = dy * r[5] - r[4] * dz, pvy = dz * r[3] - r[5] * dx, pvz = dx * r[4] - r[3] * dy;
    const float det = (r[0] * pvx + r[1] * pvy) + r[2] * pvz;
    const float inv = 1.0f / det;
    u = ((r[6] * pvx + r[7] * pvy) + r[8] * pvz) * inv;
    v = ((dx * r[9] + dy * r[10]) + dz * r[11]) * inv;
    dist = r[12] * inv;
    const bool parallel = fabsf(det) <= 9.99999993922529e-09f;
    const bool u_out = (u < 0.0f) || (u > 1.0f);
    const bool v_out = (v < 0.0f) || (u + v > 1.0f);
    return !parallel && !u_out && !v_out && (dist > 0.0f);
}

// (3) for one ray: its hit inside the box of the record's vertices by the slab slack — t d on every axis with extent
// (3a), and where one axis has none, the slab distance s of that axis within 2^-17 of t and s d inside as well (3b)
constexpr float kPcFlatRel = 7.62939453125e-06f;  // 2^-17
VMX_PC_FN bool pc_hit_in_own_box(const float *r, float t, float dx, float dy, float dz) {
    const float d[3] = {dx, dy, dz};
    bool ok = true;
    int nflat = 0;
    float s = t;
    for (int k = 0; k < 3; ++k) {
        if (r[k] == 0.0f && r[3 + k] == 0.0f) {  // no extent: v1 = v2 = v0 on this axis
            s = -r[6 + k] * (1.0f / d[k]);
            ++nflat;
        }
    }
    if (nflat > 1 || !(fabsf(s - t) <= kPcFlatRel * t)) ok = false;  // (nflat = 0: s = t)
    for (int k = 0; k < 3; ++k) {
        const float p0 = -r[6 + k], p1 = p0 + r[k], p2 = p0 + r[3 + k];
        const float mn = fminf(p0, fminf(p1, p2)), mx = fmaxf(p0, fmaxf(p1, p2));
        const float sl = 1.9073486328125e-06f * (fabsf(mn) + fabsf(mx)) + 2.384185791015625e-07f * (fabsf(r[k]) + fabsf(r[3 + k]));
        const float h = t * d[k], g = s * d[k];
        const bool flat = r[k] == 0.0f && r[3 + k] == 0.0f;
        if (!flat && !(h >= mn + sl && h <= mx - sl && g >= mn + sl && g <= mx - sl)) ok = false;
    }
    return ok;
}

// the per-ray rule.  l0..l3: the pixel's slots.  true: the ray is settled with (t, slot)
VMX_PC_FN bool pc_list_settle(const float *cam_tris, uint32_t l0, uint32_t l1, uint32_t l2, uint32_t l3, float dx, float dy,
                              float dz, float &t, uint32_t &slot) {
    float t1 = 3.0e38f, t2 = 3.0e38f;
    uint32_t s1 = kClaimNone;
    bool inside = false;
    uint32_t m = l0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int k = 0; k < kListK; ++k) {
        if (m == kClaimNone) break;  // (padding follows the members)
        const float *r = (const float *)__builtin_assume_aligned(cam_tris + (size_t)m * 16, 16);
        float d, u, v;
        if (pc_ray_test(r, dx, dy, dz, d, u, v)) {
            if (d < t1) {
                t2 = t1, t1 = d, s1 = m;
                inside = pc_hit_in_own_box(r, d, dx, dy, dz);
            } else {
                t2 = fminf(t2, d);
            }
        }
        m = k == 0 ? l1 : (k == 1 ? l2 : l3);
    }
    if (s1 == kClaimNone || !inside || !(t1 < 999999999.f)) return false;  // (the walk starts from 999999999: bvh.cpp:48)
    if (t2 <= t1 + t1 * kPcRel) return false;
    t = t1, slot = s1;
    return true;
}

// The per-pixel procedure of a list, for a pixel whose single claim is kClaimNone.  cand, other: what
// pc_pixel_claim_cand left — the centre ray's nearest triangle (-1: none, -2: no list) and the triangle its walk ended
// on (-1: none); both are only the first candidates for membership, and a list that starts from any live triangles is
// sound: what (2) asks is asked of the final list.  out: the record (kListWords words).  Returns the number of members.
// The members are kept as slots alone and classified again where pc_farther needs one: a few reached triangles per
// walk need it, and four PcTri in registers cost k_pixel_claims three of its seven waves per SIMD.
template <class Stack>
VMX_PC_FN int pc_pixel_list(const PcFilm &fm, uint32_t p, const float *cam_inner, const float *cam_tris, uint32_t root_ref,
                            Stack &stk, int max_sp, int cand, int other, uint32_t *out) {
    for (int k = 0; k < kListWords; ++k) out[k] = kClaimNone;
    if (cand < -1) return 0;
    const PcCone c = pc_cone(fm, p);
    if (!c.ok) return 0;
    uint32_t s0 = kClaimNone, s1 = kClaimNone, s2 = kClaimNone, s3 = kClaimNone;
    int n = 0;
    float tcut = kPcNoCut, thi_max = 0.0f;
    uint32_t join = cand >= 0 ? (uint32_t)cand : kClaimNone, join2 = other >= 0 ? (uint32_t)other : kClaimNone;
    uint32_t visits = 0;
    for (;;) {
        if (join == kClaimNone) join = join2, join2 = kClaimNone;
        if (join != kClaimNone) {
            if (n == kListK) { VMX_PC_WHY(3); return 0; }
            PcTri T;
            if (pc_classify(c, cam_tris + (size_t)join * 16, T) != kPcLive) { VMX_PC_WHY(4); return 0; }
            const float thi = T.acd / (T.dlo - T.sd);  // the largest tau = t |w| of the cone, float det included
            if (!(T.dlo > 2.0f * T.sd && thi > 1e-20f && thi < 1e8f)) { VMX_PC_WHY(1); return 0; }
            if (n == 0) s0 = join;
            else if (n == 1) s1 = join;
            else if (n == 2) s2 = join;
            else s3 = join;
            ++n;
            thi_max = fmaxf(thi_max, thi);
            tcut = thi_max * (1.0f + 9.765625e-04f);
            join = kClaimNone;
            if (join2 != kClaimNone) continue;
        }
        // the culled walk with the current list; a triangle that must join ends it
        int sp = 0;
        uint32_t cur = root_ref;
        for (;;) {
            if (++visits > kListBudget) { VMX_PC_WHY(5); return 0; }
            if (cur & kLeafBit) {
                const uint32_t first = cur & kLeafStartMask, cnt = (cur >> kLeafCountShift) & 31u;
                visits += cnt;
                for (uint32_t i = 0; i < cnt && join == kClaimNone; ++i) {
                    const uint32_t t = first + i;
                    if (t == s0 || t == s1 || t == s2 || t == s3) continue;
                    PcTri U;
                    const PcClass k = pc_classify(c, cam_tris + (size_t)t * 16, U);
                    if (k == kPcRejected) continue;
                    if (k == kPcUnsure) { VMX_PC_WHY(6); return 0; }
                    bool far = n > 0;
                    uint32_t m = s0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
                    for (int j = 0; j < kListK && far && m != kClaimNone; ++j) {
                        PcTri T;
                        pc_classify(c, cam_tris + (size_t)m * 16, T);  // (kPcLive: it was when m joined)
                        far = pc_farther(c, T, U);
                        m = j == 0 ? s1 : (j == 1 ? s2 : s3);
                    }
                    if (!far) join = t;
                }
                if (join != kClaimNone) break;
                if (sp == 0) break;
                float unused;
                stk.get(--sp, cur, unused);
            } else {
                const float *q = cam_inner + (size_t)cur * 16;
                const bool h0 = pc_box_reached(c, q, q + 3, tcut), h1 = pc_box_reached(c, q + 6, q + 9, tcut);
                uint32_t lref, rref;
                __builtin_memcpy(&lref, q + 12, 4), __builtin_memcpy(&rref, q + 13, 4);
                if (h0 && h1) {
                    if (sp >= max_sp) return 0;
                    stk.put(sp++, rref, 0.0f);
                    cur = lref;
                } else if (h0) {
                    cur = lref;
                } else if (h1) {
                    cur = rref;
                } else {
                    if (sp == 0) break;
                    float unused;
                    stk.get(--sp, cur, unused);
                }
            }
        }
        if (join == kClaimNone) break;
    }
    if (n == 0) { VMX_PC_WHY(7); return 0; }
    out[0] = s0, out[1] = s1, out[2] = s2, out[3] = s3;
    return n;
}

// both planes of a pixel, as k_pixel_claims and the host program fill them: the claim, and the list of a pixel without one
template <class Stack>
VMX_PC_FN uint32_t pc_pixel_claim_and_list(const PcFilm &fm, uint32_t p, const float *cam_inner, const float *cam_tris,
                                           uint32_t root_ref, Stack &stk, int max_sp, uint32_t *list_out) {
    int cand, other;
    const uint32_t c = pc_pixel_claim_cand(fm, p, cam_inner, cam_tris, root_ref, stk, max_sp, cand, other);
    pc_pixel_list(fm, p, cam_inner, cam_tris, root_ref, stk, max_sp, c == kClaimNone ? cand : -2, other, list_out);
    return c;
}

}  // namespace vmx
