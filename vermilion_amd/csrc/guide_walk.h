// guide_walk.h — "the reference's tree returns exactly this (t, slot) for this bounce ray", decided per ray after a
// nearest-hit walk over ANOTHER hierarchy of the same triangles (the guide: the binned-SAH tree of bvh_build.cpp).
//
// Plain float C++ for host and device, compiled with -ffp-contract=off on both sides, like pixel_claim.h: the GUIDE forms
// of k_trace_w<1> and of k_paths (vmx_kernels.hip) and the stand-alone host program tests/cpp/guide_walk_test.cpp run
// the same arithmetic.  eps = 2^-24 below.
//
// Who runs the walk.  k_trace_w<1, .., GUIDE>: the bounce generations of a split pass; every ray of the launch walks the
// guide, the rule runs at the refill, and the fallback rays go to a list that the unchanged kernel traces in a second
// launch.  k_paths<false, .., GuidePathsDev> (the fused kernel: the tail of a split pass, the passes of pipeline form 1,
// the small passes of form 0): a ray of any depth that passes gw_ray_ok, camera rays included — the rule does not ask
// where a ray comes from — walks the guide, whose records lie behind the reference's in the same allocation; the rule
// runs for the wave's finished guide lanes before they are shaded, and a fallback ray starts again over the reference
// tree in its own lane (ray_start with the reference's root, the reference's own prune), so one wave holds lanes on
// either tree.  A ray that fails gw_ray_ok starts on the reference tree in both kernels.
//
// Contract of gw_settle: whenever it returns true for a ray that finished the guide walk with (best, winner), then
// BVH::getIntersection (bvh.cpp:47-145) over the REFERENCE tree returns the winner's triangle with t = best, bit for bit;
// a guide walk that ends with no hit means the reference returns no hit.  Every other ray is a fallback ray: it is
// traced over the reference tree (by the unchanged kernel, or in its lane of the fused one).  A rule that settles nothing
// is sound; tests/test_guide_walk.py holds both the soundness (0 wrong rays) and the share.
//
// The guide walk (gw_walk here; the GUIDE step of k_trace_w<1>) is the step of k_trace_w<1> over the guide's records —
// nearer child first, one triangle per step, tri_test untouched, so a triangle's t has the bits the reference computes —
// with three changes (the third one is (B) below: a marked child box that ends behind the origin is not entered):
//   * a node is pruned, in choose_child and in the pop, when near > cut, cut = best (1 + kGwKappa), kept up to date
//     with best (the reference prunes on near > best, bvh.cpp:69);
//   * beside (best, slot) the ray keeps `second`, the smallest accepted distance of any OTHER triangle it tested: on a
//     new best, second = the old best; otherwise second = min(second, dist).
// The guide's child boxes are PADDED once, when its records are written (gw_pad): each face moves outwards by
//   pad = 2^-18 (|lo| + |hi| + M),  M = four times the largest |coordinate| of the scene's vertices,
// and the rule asks |o_k| <= M of the ray's origin.  (A bounce ray starts on a triangle or on one of the scene's
// spheres; the reference's sphere table is a room around the mesh, whose walls M has to reach: with M the largest
// |coordinate| itself, the rays that start on a wall sphere — a quarter of a Cornell frame's — never walked.  The pad
// of the Sponza stand-in is 0.03 units with it.)
//
// Margins.
//   (S) A slab product as bbox.cpp:72-73 forms it, s(p) = RN(RN(p - o_k) RN(1 / d_k)), lies within 4 eps (|p| + |o_k|) / |d_k|
//       of the exact (p - o_k) / d_k: three roundings, the first one absolute in |p - o_k| <= |p| + |o_k|.  In coordinates
//       (times |d_k|) that is 4 eps (|lo| + |hi| + pad + M) for a padded face, a sixteenth of the pad (64 eps of the
//       same sum).  So for every EXACT parameter tau whose point o + tau d lies inside a node's unpadded box, every float
//       slab interval of the padded box contains tau: near <= tau <= far, the float test `near <= far` passes, and
//       near <= tau.  Conversely a float slab miss of a guide node means the exact ray does not meet its unpadded box.
//   (P) The premise, the one pixel_claim.h rests its (b) and (2) on ("a triangle in a node beyond tcut is hit, if at all,
//       beyond every member's distance"): the triangle test means what it says at the scale of the cut.  A triangle U
//       that tri_test accepts at the float distance t_U is met by the exact ray inside the box of its vertices at some
//       parameter tau <= t_U (1 + kGwKappa / 2).  It is a statement about tri_test's accuracy, not a theorem: a sliver
//       whose det cancels can miss it, and the adversarial cases of tests/test_guide_walk.py (sliver fans, coplanar
//       pairs, planes a few floats apart, grazing rays) are there to hold it.  A wider kappa asks less of it; the widest
//       one that costs less than 3 % more visits was taken (profiles/guide_tree.txt).
//   (B) The second premise, for the cull below: a triangle U that tri_test accepts (dist > 0) is crossed by the exact
//       line inside the box of its vertices at a parameter tau > -(15/16) pad, pad the smallest pad of any guide box that
//       holds U.  Then by (S) (a sixteenth of the pad, in coordinates) U's padded leaf box and every padded ancestor have
//       float far >= 0.  Like (P) it is a statement about tri_test's accuracy, and it is FALSE for ill-conditioned
//       records: where the origin lies within rounding of the plane of a sliver, the numerator e2 . q of dist has no
//       reliable sign, and a triangle hundreds of pads behind the origin is accepted with a positive float dist (3.5, 92,
//       234 were seen).  The failure rate falls with the conditioning of the record's edge pair,
//         gw_shape(e1, e2) = |e1| |e2| / |e1 x e2|     (1 / sin of the angle between the edges; computed in double),
//       from 372 wrong rays in 200,000 at shape ~40,000 to 4 at ~400 and none at ~107 and below (the sweep of
//       tests/test_guide_cull.py, profiles/guide_cull.txt; an earlier host experiment saw 1 at ~70, none at ~18), so (B) is
//       asked only of triangles with gw_shape <= kGwShapeMax: make_guide_records marks a child box of a guide record
//       (InnerRecord::pad0 for the left child, pad1 for the right; 1 = may be skipped) only if no triangle of the child's
//       subtree is worse.  A zero word means "never skip": the reference tree's records, whose spare words are zero, are
//       walked as the reference walks them, boxes behind the origin included (bbox.cpp:70-83 has no sign test).
//       The cull: a marked child counts as hit only if near <= far AND far >= 0.  `near` keeps its meaning for the
//       order and the prune; only the hit decision changes.  A bounce ray's own surface, 0.001 behind its origin, is
//       never culled: its padded box contains the origin.
//   (1) Completeness of the guide walk.  Let t be the final best.  A triangle U accepted at t_U <= t (1 + 2^-16) was
//       TESTED by the walk.  Its leaf and every ancestor contain U's vertex box, so by (P) and (S) none of them is a slab
//       miss and each has near <= tau <= t_U (1 + kappa / 2) <= t (1 + 2^-16)(1 + kappa / 2) < t (1 + kappa) <= cut at any
//       time (best only falls towards t; kappa >= 2^-10), so none is pruned either.  Nor is any of them skipped by the
//       cull: a box on the way to U that carries a mark holds only triangles of shape <= kGwShapeMax, U among them, so
//       (B) gives it far >= 0; a box without a mark is never skipped.  Hence second, as the walk leaves it,
//       is the smallest accepted distance of every triangle other than the winner, up to those beyond t (1 + 2^-16).
//   (2) The rule asks second > best (1 + 2^-16).  With (1): every triangle other than the winner m that the reference
//       can accept for this ray is accepted beyond t (1 + 2^-16).  Equal distances (a duplicated triangle, a shared
//       edge hit twice) give second = best and fall back: the reference's test order decides such ties, the guide's does not.
//   (3) The reference reaches m: gw_hit_in_own_box, pixel_claim.h's (3) restated for a world-space record (v0, e1, e2)
//       and a free origin.  Box of m's vertices from the record: p0 = v0, p1 = v0 + e1, p2 = v0 + e2 (within 2 eps (|e| +
//       |v|) of the true vertices, whose box the reference's leaf box contains); slab slack
//         sl_k = 2^-19 (|mn_k| + |mx_k| + |o_k|) + 2^-22 (|e1_k| + |e2_k|)
//       — 32 eps of the coordinates: (S)'s 4 eps, the 2 eps of forming h_k = o_k + t d_k here, the record's 2 eps, with
//       a factor 4 to spare; the origin's terms are what a free origin adds to pixel_claim.h's slack.
//       (3a) Extent on all three axes: the rule asks o_k + t d_k in [mn_k + sl_k, mx_k - sl_k] for every k.  Then every
//            float slab interval of the leaf and, boxes being nested and rounding monotonic, of every ancestor contains
//            the float t itself: `near <= far` holds and near <= t.
//       (3b) No extent on axis f (e1_f = e2_f = 0, so the three true vertices agree there exactly): both slab products
//            of m's own box on f are the one number s = RN(RN(v0_f - o_f) RN(1 / d_f)), formed here as bbox.cpp forms it,
//            and the float t need not agree with it (pixel_claim.h (3b)).  The rule asks |s - t| <= 2^-17 t and both
//            o_k + t d_k and o_k + s d_k inside on the two other axes.  Then every slab interval of the leaf and of
//            every ancestor contains s: near <= s <= t (1 + 2^-17).  Two axes without extent: the ray falls back.
//       Either way no node on the way to m is pruned (bvh.cpp:69): its near is below t (1 + 2^-16), while the
//       reference's nearest hit so far is 999999999 (the rule asks best < 999999999), m's own t, or another triangle's,
//       which is beyond t (1 + 2^-16) by (2).
//   (4) So the reference tests m with the same arithmetic, gets t, and every other triangle it accepts lies beyond t:
//       it returns (t, m) whatever its order.  TriRecord::pad[0] of a guide record holds m's leaf slot in the REFERENCE
//       tree, so the hit record and everything downstream keep reference slots.
//   (5) No hit.  best stays 999999999 and cut = 999999999 (1 + kappa).  By (P) and (S) a triangle accepted at t_U in a
//       pruned node has t_U (1 + kappa / 2) > cut, t_U > 999999999, and fails the reference's `dist < 999999999`
//       (bvh.cpp:90) as well; one behind a slab miss is not accepted at all; one in a skipped box (marked, far < 0) is
//       not accepted by (B).  The reference returns no hit.
//   (6) Guards: origin, direction and reciprocals all finite (so no direction component is zero, no slab is NaN and
//       the wave-level NaN-exact box form never meets the guide: such rays are appended to the fallback list unwalked),
//       |o_k| <= M, and every comparison of the rule is written so that a NaN fails it.
#pragma once
#include <math.h>
#include <stdint.h>
#include "vmx_device.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VMX_GW_FN __host__ __device__ inline __attribute__((always_inline))  // (bvh_build.cpp includes no HIP runtime header)
#else
#define VMX_GW_FN inline
#endif

namespace vmx {

#ifndef VMX_GW_KAPPA
#define VMX_GW_KAPPA 1.5625e-02f  // 2^-6 (profiles/guide_tree.txt: visits per ray at 2^-10 / 2^-8 / 2^-6)
#endif
constexpr float kGwKappa = VMX_GW_KAPPA;
constexpr float kGwCut = 1.0f + kGwKappa;
constexpr float kGwRel = 1.52587890625e-05f;      // 2^-16: the tie band of (2)
constexpr float kGwFlatRel = 7.62939453125e-06f;  // 2^-17: (3b)
constexpr float kGwPadRel = 3.814697265625e-06f;  // 2^-18: the pad of a guide box face
constexpr float kGwLimit = 999999999.f;           // bvh.cpp:48
constexpr float kGwOriginReach = 4.0f;            // M over the largest |coordinate| of the vertices
#ifndef VMX_GW_SHAPE_MAX
#define VMX_GW_SHAPE_MAX 8.0  // (B): the worst gw_shape a skippable box may hold (the sweep of tests/test_guide_cull.py)
#endif
constexpr double kGwShapeMax = VMX_GW_SHAPE_MAX;
#ifndef VMX_GW_CULL
#define VMX_GW_CULL 1  // 0: every walk tests the boxes behind the origin, whatever the marks say (the A/B build)
#endif

// (B): the conditioning of a record's edge pair, |e1| |e2| / |e1 x e2|, in double from the record's floats; a zero cross
// product (or a NaN) counts as infinite
VMX_GW_FN double gw_shape(const float *e1, const float *e2) {
    const double ax = e1[0], ay = e1[1], az = e1[2], bx = e2[0], by = e2[1], bz = e2[2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const double cross2 = cx * cx + cy * cy + cz * cz, dots = (ax * ax + ay * ay + az * az) * (bx * bx + by * by + bz * bz);
    if (!(cross2 > 0.0)) return (double)INFINITY;
    return sqrt(dots / cross2);
}
// the bound a child's `far` has to reach to count as hit, from the record's spare word for that child (0: never skipped)
VMX_GW_FN float gw_far_floor(uint32_t mark) { return (VMX_GW_CULL && mark != 0u) ? 0.0f : -INFINITY; }

VMX_GW_FN bool gw_finite(float x) { return fabsf(x) <= 3.0e38f; }  // false on NaN

// the pad of one axis of a guide box [lo, hi]; scene_max = M
VMX_GW_FN float gw_pad(float lo, float hi, float scene_max) { return kGwPadRel * ((fabsf(lo) + fabsf(hi)) + scene_max); }

// (6): what a ray needs to walk the guide at all
VMX_GW_FN bool gw_ray_ok(float ox, float oy, float oz, float dx, float dy, float dz, float ix, float iy, float iz,
                         float scene_max) {
    return gw_finite(dx) && gw_finite(dy) && gw_finite(dz) && gw_finite(ix) && gw_finite(iy) && gw_finite(iz) &&
           fabsf(ox) <= scene_max && fabsf(oy) <= scene_max && fabsf(oz) <= scene_max;
}

// (3) for one ray and the winner's record r = (v0[3], e1[3], e2[3]): its hit inside the box of the record's vertices
// by the slab slack
VMX_GW_FN bool gw_hit_in_own_box(const float *r, float t, const float *o, const float *d, const float *inv) {
    bool ok = true;
    int nflat = 0;
    float s = t;
    for (int k = 0; k < 3; ++k) {
        if (r[3 + k] == 0.0f && r[6 + k] == 0.0f) {  // no extent: v1 = v2 = v0 on this axis
            s = (r[k] - o[k]) * inv[k];              // bbox.cpp:72-73
            ++nflat;
        }
    }
    if (nflat > 1 || !(fabsf(s - t) <= kGwFlatRel * t)) ok = false;  // (nflat = 0: s = t)
    for (int k = 0; k < 3; ++k) {
        const float p0 = r[k], p1 = p0 + r[3 + k], p2 = p0 + r[6 + k];
        const float mn = fminf(p0, fminf(p1, p2)), mx = fmaxf(p0, fmaxf(p1, p2));
        const float sl = 1.9073486328125e-06f * ((fabsf(mn) + fabsf(mx)) + fabsf(o[k])) +
                         2.384185791015625e-07f * (fabsf(r[3 + k]) + fabsf(r[6 + k]));
        const float h = o[k] + t * d[k], g = o[k] + s * d[k];
        const bool flat = r[3 + k] == 0.0f && r[6 + k] == 0.0f;
        if (!flat && !(h >= mn + sl && h <= mx - sl && g >= mn + sl && g <= mx - sl)) ok = false;
    }
    return ok;
}

// why a finished guide ray is not settled (the host program counts them)
enum GwVerdict { kGwSettled = 0, kGwMiss = 1, kGwInput = 2, kGwLimitHit = 3, kGwTie = 4, kGwBox = 5 };

// The per-ray rule.  best / second: what the guide walk left (best = 999999999 and no winner: have = false);
// r: the winner's guide record (read only if have).  kGwSettled and kGwMiss settle the ray; the others fall back.
VMX_GW_FN GwVerdict gw_verdict(bool have, const float *r, float best, float second, const float *o, const float *d,
                               const float *inv, float scene_max) {
    if (!gw_ray_ok(o[0], o[1], o[2], d[0], d[1], d[2], inv[0], inv[1], inv[2], scene_max)) return kGwInput;
    if (!have) return kGwMiss;
    if (!(best < kGwLimit)) return kGwLimitHit;
    if (!(second > best + best * kGwRel)) return kGwTie;
    if (!gw_hit_in_own_box(r, best, o, d, inv)) return kGwBox;
    return kGwSettled;
}
VMX_GW_FN bool gw_settle(bool have, const float *r, float best, float second, const float *o, const float *d,
                         const float *inv, float scene_max) {
    const GwVerdict v = gw_verdict(have, r, best, second, o, d, inv, scene_max);
    return v == kGwSettled || v == kGwMiss;
}

// ---- the walk, as the host program runs it (the kernel's step is this walk on its own stack; the arithmetic of a
// triangle test is tri_test's, of a box child_boxes' — for finite slabs v_min / v_max and the compare-select form agree)
VMX_GW_FN bool gw_tri_test(const float *r, const float *o, const float *d, float &dist) {
    const float e1x = r[3], e1y = r[4], e1z = r[5], e2x = r[6], e2y = r[7], e2z = r[8];
    const float pvx = d[1] * e2z - e2y * d[2], pvy = d[2] * e2x - e2z * d[0], pvz = d[0] * e2y - e2x * d[1];
    const float det = (e1x * pvx + e1y * pvy) + e1z * pvz;
    const float inv_det = 1.0f / det;
    const float tx = o[0] - r[0], ty = o[1] - r[1], tz = o[2] - r[2];
    const float u = ((tx * pvx + ty * pvy) + tz * pvz) * inv_det;
    const float qx = ty * e1z - e1y * tz, qy = tz * e1x - e1z * tx, qz = tx * e1y - e1x * ty;
    const float v = ((d[0] * qx + d[1] * qy) + d[2] * qz) * inv_det;
    dist = ((e2x * qx + e2y * qy) + e2z * qz) * inv_det;
    const bool parallel = fabsf(det) <= 9.99999993922529e-09f;
    const bool u_out = (u < 0.0f) || (u > 1.0f);
    const bool v_out = (v < 0.0f) || (u + v > 1.0f);
    return !parallel && !u_out && !v_out && (dist > 0.0f);
}

struct GwResult {
    float best, second;
    int slot;  // leaf slot in the tree walked, -1: no hit
    uint32_t inner_visits, tri_tests;
};

// nearest hit over (inner, tris, root_ref) with the prune on near > best * cut_factor (1: the reference's own prune).
// Rays must pass gw_ray_ok.  Returns false if the tree is deeper than kMaxStack.
VMX_GW_FN bool gw_walk(const InnerRecord *inner, const TriRecord *tris, uint32_t root_ref, const float *o, const float *d,
                       const float *inv, float cut_factor, GwResult &res) {
    uint32_t ref_stack[kMaxStack + 2];
    float near_stack[kMaxStack + 2];
    int sp = 0;
    float best = kGwLimit, second = 3.0e38f, cut = kGwLimit * cut_factor;
    int slot = -1;
    uint32_t cur = root_ref, nv = 0, nt = 0;
    for (;;) {
        bool pop = false;
        if (cur & kLeafBit) {
            const uint32_t first = cur & kLeafStartMask, n = (cur >> kLeafCountShift) & 31u;
            for (uint32_t i = 0; i < n; ++i) {
                ++nt;
                float dist;
                if (gw_tri_test(tris[first + i].v0, o, d, dist)) {
                    if (dist < best) {
                        second = best, best = dist, slot = (int)(first + i);
                        cut = best * cut_factor;
                    } else {
                        second = fminf(second, dist);
                    }
                }
            }
            pop = true;
        } else {
            ++nv;
            const InnerRecord &q = inner[cur];
            float tn[2];
            bool h[2];
            for (int c = 0; c < 2; ++c) {
                const float *lo = c ? q.rmin : q.lmin, *hi = c ? q.rmax : q.lmax;
                const float ax = (lo[0] - o[0]) * inv[0], ay = (lo[1] - o[1]) * inv[1], az = (lo[2] - o[2]) * inv[2];
                const float bx = (hi[0] - o[0]) * inv[0], by = (hi[1] - o[1]) * inv[1], bz = (hi[2] - o[2]) * inv[2];
                const float n = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
                const float f = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
                tn[c] = n, h[c] = n <= f && f >= gw_far_floor(c ? q.pad1 : q.pad0);  // (B): a marked box behind the origin
            }
            const bool go_right = h[1] && (!h[0] || tn[1] < tn[0]);
            if (h[0] && h[1]) {
                if (sp >= (int)kMaxStack) return false;
                ref_stack[sp] = go_right ? q.left : q.right, near_stack[sp] = go_right ? tn[0] : tn[1];
                ++sp;
            }
            const float near = go_right ? tn[1] : tn[0];
            if (!(h[0] || h[1]) || near > cut) pop = true;
            else cur = go_right ? q.right : q.left;
        }
        if (pop) {
            for (;;) {
                if (sp == 0) {
                    res.best = best, res.second = second, res.slot = slot, res.inner_visits = nv, res.tri_tests = nt;
                    return true;
                }
                --sp;
                if (!(near_stack[sp] > cut)) break;
            }
            cur = ref_stack[sp];
        }
    }
}

}  // namespace vmx
