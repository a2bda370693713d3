// vmx_kernels.hip — hand-written gfx950 (CDNA4, wave64) kernels of the path-tracing hot path.
//
// Compiled with -ffp-contract=off: every float operation rounds once, in the
// operation order of the reference's GLM expressions, so that triangle IDs,
// distances and whole frames are bit-identical to the CPU oracle.  Divide and
// sqrt are hipcc's correctly rounded forms (its default).
//
// Kernels
//   k_trace        BVH::getIntersection for explicit rays          (bvh.cpp:47-145)
//   k_raycast      MeshEngine::RayCast for explicit rays           (meshEngine.cpp:239-509)
//   k_raygen       camera rays of a pass, each with the step_bits of its first Radiance step (pathtracer.cpp:251-280);
//                  <1> + k_raygen_live: only the live ones (VMX_SAMPLING_ELIDE_DEAD, with path_compact.hip);
//                  <0, true>: settles the rays of pixels with a list claim itself (pc_list_settle), in a pass that fuses its claimed pixels
//   k_trace_w      persistent BVH traversal of camera / bounce rays (bvh.cpp:47-145); <0> settles a camera ray by its pixel's
//                  claim or list at refill time, except where the pass handed it only the rays that walk (the slots without
//                  claim or list, and the stragglers of k_raygen<0, true>); <.., SORT>: settles the finished rays
//                  whose step ends by its draws, hands the others on as records (DESIGN_HISTORY.md 5.1); k_trace_q: counting form
//   k_shade        RayCast tail + one Radiance step, id compaction  (meshEngine.cpp:365-508, pathtracer.cpp:36-196);
//                  k_shade_ends: the two-phase form's first phase
//   k_paths        traversal + shading fused, paths kept to their end (small passes, the tail of a pass)
//   k_resolve      per-pixel accumulation, early stop, pixel write (pathtracer.cpp:282-324)
//   k_bruteforce*  BruteForceTracer::Render                        (integrators.cpp:9-186)
//   k_query        device ray queries: nearest hit with a bound, any hit, RayCastCollision (vmx_query.inc)
//   k_update_records, k_refit_level  in-place geometry updates: record rewrite, refit (vmx_update.inc)
// (the first-generation kernels k_primary / k_bounce live in vmx_kernels_ab.inc: A/B library only)
//
// Execution model: persistent blocks stride over block-sized work items; the
// item -> image-region map is XCD-aware (items b and b+8 run on one XCD and
// are given neighbouring pixel tiles, so an XCD's 4 MiB L2 holds the part of
// the BVH its rays walk).  Each lane owns one ray/path; its BVH stack lives in
// LDS, lane-strided (entry e of lane l at [e*64 + l], 8 bytes: node ref +
// entry distance), which is conflict-free for ds_read/write_b64 at any mix of
// per-lane stack depths.  Surviving paths are compacted between bounces with a
// wave ballot + prefix popcount and one atomic per wave on one of 16 sub-queue
// tails.  No MFMA: there is no dense contraction in this workload.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <stdint.h>

#include "vmx_kernels.h"
#include "pixel_claim.h"
#include "guide_walk.h"
#include <type_traits>

#ifndef VMX_CAM_BATCH
#define VMX_CAM_BATCH 16  // steps of a camera-ray wave between two refill tests (a descent counts as 5)
#endif
#ifndef VMX_TRACE_WAVES_PER_SIMD
#define VMX_TRACE_WAVES_PER_SIMD 7  // register budget of the trace kernel: 512 / 7 -> 72 VGPRs
#endif


namespace vmx {
__device__ __forceinline__ float luminance(float r, float g, float b);  // (vmx_image.inc; k_resolve<true> folds its square)
namespace {

constexpr float kInf = __builtin_huge_valf();

struct Cnt {
    uint32_t inner, tris;
};

// wave-uniform tallies, flushed once per wave at kernel exit
struct Tally {
    uint32_t rays[2], hits[2], cont[2];
};

__device__ __forceinline__ uint32_t lane_index() { return __lane_id(); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------
// RNG: xoshiro256** keyed by (seed, pixel, sample)  — DESIGN.md §3
// ---------------------------------------------------------------------------
struct Rng {
    uint64_t s0, s1, s2, s3;
};

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Stream of sample k of pixel p (the reference seeds a thread-local mt19937_64 from std::random_device,
// pathtracer.cpp:231, and is not reproducible: the stream definition is this build's own, shared with the oracle).
// Round 4: the pixel half of the key is two mix64 per PIXEL — a wave of k_raygen / k_shade<0> is 64 samples of one pixel,
// so it runs once per wave on the scalar unit — and the sample half costs three 64-bit multiplies (round 3: ten per
// sample, twice per camera path):
//   a = mix64(seed ^ (p << 32))   b = mix64(a + golden)                       per pixel
//   s0 = mix64(a + k)   t = (s0 ^ b) * M3   s1 = t ^ (t >> 32)   s2 = rotl(s0, 24) ^ b   s3 = rotl(s1, 37) ^ a
struct PixelKey {
    uint64_t a, b;
};
__device__ __forceinline__ PixelKey rng_pixel_key(uint64_t seed, uint32_t pixel) {
    PixelKey pk;
    pk.a = mix64(seed ^ ((uint64_t)pixel << 32));
    pk.b = mix64(pk.a + 0x9E3779B97F4A7C15ull);
    return pk;
}
__device__ __forceinline__ void rng_init_keyed(Rng &r, PixelKey pk, uint32_t k) {
    r.s0 = mix64(pk.a + (uint64_t)k);
    const uint64_t t = (r.s0 ^ pk.b) * 0xD6E8FEB86659FD93ull;
    r.s1 = t ^ (t >> 32);
    r.s2 = rotl64(r.s0, 24) ^ pk.b;
    r.s3 = rotl64(r.s1, 37) ^ pk.a;
}
__device__ __forceinline__ void rng_init(Rng &r, uint64_t seed, uint32_t pixel, uint32_t k) {
    rng_init_keyed(r, rng_pixel_key(seed, pixel), k);
}

__device__ __forceinline__ uint64_t rng_next(Rng &r) {
    const uint64_t out = rotl64(r.s1 * 5, 7) * 9;
    const uint64_t t = r.s1 << 17;
    r.s2 ^= r.s0;
    r.s3 ^= r.s1;
    r.s1 ^= r.s2;
    r.s0 ^= r.s3;
    r.s2 ^= t;
    r.s3 = rotl64(r.s3, 45);
    return out;
}

// stands in for uniform_real_distribution<double>(0,1) (pathtracer.cpp:23)
__device__ __forceinline__ double rng_u01(Rng &r) {
    return __longlong_as_double((long long)(0x3FF0000000000000ull | (rng_next(r) >> 12))) - 1.0;
}
// stands in for uniform_real_distribution<float>(0,0.5) (pathtracer.cpp:230)
__device__ __forceinline__ float rng_jitter(Rng &r) {
    return (__uint_as_float(0x3F800000u | (uint32_t)(rng_next(r) >> 41)) - 1.0f) * 0.5f;
}

// ---------------------------------------------------------------------------
// small vector helpers in GLM's operation order
// ---------------------------------------------------------------------------
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;  // glm::dot: tmp.x + tmp.y + tmp.z
}
// glm::normalize = v * (1 / sqrt(dot(v,v)))
__device__ __forceinline__ void normalize3(float &x, float &y, float &z) {
    const float s = 1.0f / sqrtf(dot3(x, y, z, x, y, z));
    x = x * s;
    y = y * s;
    z = z * s;
}
// glm::cross(a, b)
__device__ __forceinline__ void cross3(float ax, float ay, float az, float bx, float by, float bz,
                                       float &cx, float &cy, float &cz) {
    cx = ay * bz - by * az;
    cy = az * bx - bz * ax;
    cz = ax * by - bx * ay;
}
__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return (fabsf(x) < kInf) && (fabsf(y) < kInf) && (fabsf(z) < kInf);
}

// ---------------------------------------------------------------------------
// BBox::intersect (bbox.cpp:70-83)
// ---------------------------------------------------------------------------
// Fast form: v_min/v_max.  Equal to the reference's compare-select form
// whenever no slab product is NaN, which `exact == false` guarantees (finite
// origin, finite non-zero reciprocal direction).
// The min/max are issued as plain v_min/v_max/v_max3/v_min3 (inline asm): without it hipcc adds a
// canonicalising v_max(x,x) in front of every fminf/fmaxf operand that comes out of a packed multiply.
__device__ __forceinline__ float vmin(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmax(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float vmin3(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ bool box_fast(float lx, float ly, float lz, float hx, float hy, float hz,
                                         float ox, float oy, float oz, float ix, float iy, float iz,
                                         float &tnear) {
    const float t0x = (lx - ox) * ix, t0y = (ly - oy) * iy, t0z = (lz - oz) * iz;
    const float t1x = (hx - ox) * ix, t1y = (hy - oy) * iy, t1z = (hz - oz) * iz;
    const float n = vmax3(vmin(t0x, t1x), vmin(t0y, t1y), vmin(t0z, t1z));
    const float f = vmin3(vmax(t0x, t1x), vmax(t0y, t1y), vmax(t0z, t1z));
    tnear = n;
    return n <= f;
}
// Same with (lo - o), (hi - o) already formed (k_camera_tables)
__device__ __forceinline__ bool box_fast_rel(float lx, float ly, float lz, float hx, float hy, float hz, float ix,
                                             float iy, float iz, float &tnear) {
    const float t0x = lx * ix, t0y = ly * iy, t0z = lz * iz;
    const float t1x = hx * ix, t1y = hy * iy, t1z = hz * iz;
    const float n = vmax3(vmin(t0x, t1x), vmin(t0y, t1y), vmin(t0z, t1z));
    const float f = vmin3(vmax(t0x, t1x), vmax(t0y, t1y), vmax(t0z, t1z));
    tnear = n;
    return n <= f;
}

// Exact form: glm::min/max = (b<a)?b:a / (a<b)?b:a, std::max/min likewise, NaN and all.
__device__ __forceinline__ float sel_min(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float sel_max(float a, float b) { return (a < b) ? b : a; }
__device__ __forceinline__ bool box_exact(float lx, float ly, float lz, float hx, float hy, float hz,
                                       float ox, float oy, float oz, float ix, float iy, float iz,
                                       float &tnear) {
    const float t0x = (lx - ox) * ix, t0y = (ly - oy) * iy, t0z = (lz - oz) * iz;
    const float t1x = (hx - ox) * ix, t1y = (hy - oy) * iy, t1z = (hz - oz) * iz;
    const float sx = sel_min(t0x, t1x), sy = sel_min(t0y, t1y), sz = sel_min(t0z, t1z);
    const float bx = sel_max(t0x, t1x), by = sel_max(t0y, t1y), bz = sel_max(t0z, t1z);
    const float n = sel_max(sel_max(sx, sy), sz);
    const float f = sel_min(sel_min(bx, by), bz);
    tnear = n;
    return n <= f;
}

__device__ __forceinline__ bool box_exact_rel(float lx, float ly, float lz, float hx, float hy, float hz, float ix,
                                              float iy, float iz, float &tnear) {
    const float t0x = lx * ix, t0y = ly * iy, t0z = lz * iz;
    const float t1x = hx * ix, t1y = hy * iy, t1z = hz * iz;
    const float sx = sel_min(t0x, t1x), sy = sel_min(t0y, t1y), sz = sel_min(t0z, t1z);
    const float bx = sel_max(t0x, t1x), by = sel_max(t0y, t1y), bz = sel_max(t0z, t1z);
    const float n = sel_max(sel_max(sx, sy), sz);
    const float f = sel_min(sel_min(bx, by), bz);
    tnear = n;
    return n <= f;
}

// min/max network of one box from the six slab products (k_trace_w, k_paths): one asm block, so that no
// hazard nops land between the pieces; the exact form is the compare-select network of box_exact
__device__ __forceinline__ void box_net(float t0x, float t0y, float t0z, float t1x, float t1y, float t1z,
                                        float &tnear, float &tfar) {
    float n, f, s1, s2;
    asm("v_min_f32 %0, %4, %7\n\t"
        "v_min_f32 %2, %5, %8\n\t"
        "v_min_f32 %3, %6, %9\n\t"
        "v_max3_f32 %0, %0, %2, %3\n\t"
        "v_max_f32 %1, %4, %7\n\t"
        "v_max_f32 %2, %5, %8\n\t"
        "v_max_f32 %3, %6, %9\n\t"
        "v_min3_f32 %1, %1, %2, %3"
        : "=&v"(n), "=&v"(f), "=&v"(s1), "=&v"(s2)
        : "v"(t0x), "v"(t0y), "v"(t0z), "v"(t1x), "v"(t1y), "v"(t1z));
    tnear = n;
    tfar = f;
}
__device__ __forceinline__ void box_net_exact(float t0x, float t0y, float t0z, float t1x, float t1y, float t1z,
                                              float &tnear, float &tfar) {
    const float sx = sel_min(t0x, t1x), sy = sel_min(t0y, t1y), sz = sel_min(t0z, t1z);
    const float bx = sel_max(t0x, t1x), by = sel_max(t0y, t1y), bz = sel_max(t0z, t1z);
    tnear = sel_max(sel_max(sx, sy), sz);
    tfar = sel_min(sel_min(bx, by), bz);
}

// (per-lane traversal stack helpers, defined with the persistent kernels below)
__device__ __forceinline__ void stack_push(uint2 *stk, uint2 *ovf, int lds_entries, int sp, uint2 e);
__device__ __forceinline__ uint2 stack_pop(const uint2 *stk, const uint2 *ovf, int lds_entries, int sp);

// ---------------------------------------------------------------------------
// The traversal primitives: the reference's tests (triangle.cpp:4-54, bbox.cpp:70-83, bvh.cpp:61-134), each written
// down ONCE.  Every traversal kernel — k_paths, k_trace_w, k_trace_q, k_query, bvh_nearest, and the A/B library's
// k_trace_pool — calls these; the operation order of each expression is the contract with the oracle (bit-identical
// results), so a change here is a change everywhere.  The one other statement of the same arithmetic is the assembly
// loop uniform_descent.
// k_trace_q and bvh_nearest share the triangle tests only: their stack has no bottom entry and their lanes carry a
// `cur_near`, so they keep a ray start, node step and pop of their own.
// ---------------------------------------------------------------------------
// Lane states of the persistent kernels, kept in the node reference itself.  Inner references are the values below
// kPop; leaf references have bit 31; these three lie between and are never valid inner indices.
constexpr uint32_t kIdle = 0x7FFFFFFFu;    // the lane is not traversing
constexpr uint32_t kBottom = 0x7FFFFFFEu;  // ref of the stack's level-0 entry (near = -inf): popping it ends the ray
constexpr uint32_t kPop = 0x7FFFFFFDu;     // the lane must pop its next node

// Triangle::getIntersection's four rejections (triangle.cpp:25,34,40,44)
__device__ __forceinline__ bool tri_accept(float det, float u, float v, float dist) {
    // (det < 1e-8 && det > -1e-8) in double  <=>  |det| <= float(1e-8)  (float(1e-8) < 1e-8)
    const bool parallel = fabsf(det) <= 9.99999993922529e-09f;
    const bool u_out = (u < 0.0f) || (u > 1.0f);
    const bool v_out = (v < 0.0f) || (u + v > 1.0f);
    return !parallel && !u_out && !v_out && (dist > 0.0f);
}
// Moeller-Trumbore on a triangle record q0 = (v0, e1.x)  q1 = (e1.yz, e2.xy)  e2z.  The caller keeps
// `if (hit && dist < best)`: strict <, the first triangle tested wins ties (bvh.cpp:90).
__device__ __forceinline__ bool tri_test(float4 q0, float4 q1, float e2z, float ox, float oy, float oz, float dx, float dy,
                                         float dz, float &dist) {
    const float e1x = q0.w, e1y = q1.x, e1z = q1.y, e2x = q1.z, e2y = q1.w;
    float pvx, pvy, pvz;
    cross3(dx, dy, dz, e2x, e2y, e2z, pvx, pvy, pvz);
    const float det = dot3(e1x, e1y, e1z, pvx, pvy, pvz);
    const float inv_det = 1.0f / det;
    const float tx = ox - q0.x, ty = oy - q0.y, tz = oz - q0.z;
    const float u = dot3(tx, ty, tz, pvx, pvy, pvz) * inv_det;
    float qx, qy, qz;
    cross3(tx, ty, tz, e1x, e1y, e1z, qx, qy, qz);
    const float v = dot3(dx, dy, dz, qx, qy, qz) * inv_det;
    dist = dot3(e2x, e2y, e2z, qx, qy, qz) * inv_det;
    return tri_accept(det, u, v, dist);
}
// The same on a camera-relative record (k_camera_tables): a = (e1, e2.x)  b = (e2.yz, tvec.xy)  c = (tvec.z, qvec)
// cd = dot(e2, qvec)
__device__ __forceinline__ bool tri_test_cam(float4 a, float4 b, float4 c, float cd, float dx, float dy, float dz,
                                             float &dist) {
    float pvx, pvy, pvz;
    cross3(dx, dy, dz, a.w, b.x, b.y, pvx, pvy, pvz);
    const float det = dot3(a.x, a.y, a.z, pvx, pvy, pvz);
    const float inv_det = 1.0f / det;
    const float u = dot3(b.z, b.w, c.x, pvx, pvy, pvz) * inv_det;
    const float v = dot3(dx, dy, dz, c.y, c.z, c.w) * inv_det;
    dist = cd * inv_det;
    return tri_accept(det, u, v, dist);
}
// A leaf reference carries its own progress: the next triangle is start + 1, count - 1; after the last one the lane pops
__device__ __forceinline__ uint32_t leaf_advance(uint32_t cur) {
    return (((cur >> kLeafCountShift) & 31u) == 1u) ? kPop : cur + (1u - (1u << kLeafCountShift));
}

// Both child boxes of an inner-node record (lo0, hi0, lo1, hi1 in q0..q2): entry and exit distances (bbox.cpp:70-83)
template <bool EXACT>
__device__ __forceinline__ void child_boxes(float4 q0, float4 q1, float4 q2, float ox, float oy, float oz, float ix, float iy,
                                            float iz, float &tn0, float &tf0, float &tn1, float &tf1) {
    const float a0 = (q0.x - ox) * ix, a1 = (q0.y - oy) * iy, a2 = (q0.z - oz) * iz;
    const float a3 = (q0.w - ox) * ix, a4 = (q1.x - oy) * iy, a5 = (q1.y - oz) * iz;
    const float b0 = (q1.z - ox) * ix, b1 = (q1.w - oy) * iy, b2 = (q2.x - oz) * iz;
    const float b3 = (q2.y - ox) * ix, b4 = (q2.z - oy) * iy, b5 = (q2.w - oz) * iz;
    if (EXACT) {
        box_net_exact(a0, a1, a2, a3, a4, a5, tn0, tf0);
        box_net_exact(b0, b1, b2, b3, b4, b5, tn1, tf1);
    } else {
        box_net(a0, a1, a2, a3, a4, a5, tn0, tf0);
        box_net(b0, b1, b2, b3, b4, b5, tn1, tf1);
    }
}
// Same with (lo - o), (hi - o) already formed (k_camera_tables)
template <bool EXACT>
__device__ __forceinline__ void child_boxes_rel(float4 q0, float4 q1, float4 q2, float ix, float iy, float iz, float &tn0,
                                                float &tf0, float &tn1, float &tf1) {
    const float a0 = q0.x * ix, a1 = q0.y * iy, a2 = q0.z * iz, a3 = q0.w * ix, a4 = q1.x * iy, a5 = q1.y * iz;
    const float b0 = q1.z * ix, b1 = q1.w * iy, b2 = q2.x * iz, b3 = q2.y * ix, b4 = q2.z * iy, b5 = q2.w * iz;
    if (EXACT) {
        box_net_exact(a0, a1, a2, a3, a4, a5, tn0, tf0);
        box_net_exact(b0, b1, b2, b3, b4, b5, tn1, tf1);
    } else {
        box_net(a0, a1, a2, a3, a4, a5, tn0, tf0);
        box_net(b0, b1, b2, b3, b4, b5, tn1, tf1);
    }
}

// Nearer child first (bvh.cpp:103-132).  Both hit: the strictly closer right child, else the left, is next and the
// other one is handed to `push` (farther first, bvh.cpp:120: the caller's own stack store); one hit: that child.
// Returns the next reference, or kPop if no child was hit or the child taken directly fails `near > t` (bvh.cpp:69).
// Two forms, one per instruction-level shape; they decide alike.  This one is plain booleans (k_trace_w<1>, k_query,
// k_trace_pool):
template <class Push>
__device__ __forceinline__ uint32_t choose_child(float tn0, float tf0, float tn1, float tf1, uint32_t lref, uint32_t rref,
                                                 float best, Push push) {
    const bool h0 = tn0 <= tf0, h1 = tn1 <= tf1;
    const bool both = h0 && h1;
    const bool go_right = h1 && (!h0 || tn1 < tn0);
    if (both) push(make_uint2(go_right ? lref : rref, __float_as_uint(go_right ? tn0 : tn1)));
    const float near = go_right ? tn1 : tn0;
    return (!(h0 || h1) || near > best) ? kPop : (go_right ? rref : lref);
}
// ... and this one takes the compares as lane masks (v_cmp into SGPR pairs), combines them with scalar ALU ops and hands
// them back to the lanes as conditions (k_paths, k_trace_w<0>): written with &&/|| hipcc evaluates part of this under
// temporary exec masks (fcmp predicates: 5 = ordered <=, 4 = ordered <, 3 = ordered >=, 2 = ordered >; icmp 32 = equal)
template <class Push>
__device__ __forceinline__ uint32_t choose_child_hit_masks(unsigned long long m0, unsigned long long m1, float tn0, float tn1,
                                                           uint32_t lref, uint32_t rref, float best, Push push) {
    const unsigned long long m_right = m1 & (~m0 | __builtin_amdgcn_fcmpf(tn1, tn0, 4));
    const bool both = __builtin_amdgcn_inverse_ballot_w64(m0 & m1);
    const bool go_right = __builtin_amdgcn_inverse_ballot_w64(m_right);
    if (both) push(make_uint2(go_right ? lref : rref, __float_as_uint(go_right ? tn0 : tn1)));
    const float near = go_right ? tn1 : tn0;
    const bool popn = __builtin_amdgcn_inverse_ballot_w64(~(m0 | m1) | __builtin_amdgcn_fcmpf(near, best, 2));
    return popn ? kPop : (go_right ? rref : lref);
}
template <class Push>
__device__ __forceinline__ uint32_t choose_child_masks(float tn0, float tf0, float tn1, float tf1, uint32_t lref,
                                                       uint32_t rref, float best, Push push) {
    return choose_child_hit_masks(__builtin_amdgcn_fcmpf(tn0, tf0, 5), __builtin_amdgcn_fcmpf(tn1, tf1, 5), tn0, tn1, lref, rref, best, push);
}

// The GUIDE forms of the two (guide_walk.h (B)): only the hit decision differs.  mark0 / mark1 are the record's spare
// words (q3.z, q3.w); a marked child whose box ends behind the origin (far < 0) does not count as hit.  `near` keeps its
// meaning for the order and the prune.  A reference-tree record's words are zero, so a reference lane of the fused kernel
// decides as above.  (Two compares per child, on the ray's far and on the mark.  The fold max(near, floor) <= far needs
// the floor as a float first — 0 or -inf selected by the mark, a compare and a select — and then the v_max: three VALU
// instructions per child against two, and a second value of `near` beside the one that orders the children.
// The lane-mask forms share choose_child_hit_masks.  The boolean form is written out a second time: with its tail in
// a function shared with choose_child, hipcc lays out k_query's and k_trace_w<1>'s branches differently — six scalar
// instructions fewer in each, none of them measured — and the kernels this change does not touch keep their code.)
template <class Push>
__device__ __forceinline__ uint32_t choose_child_cull(float tn0, float tf0, float tn1, float tf1, uint32_t lref, uint32_t rref,
                                                      uint32_t mark0, uint32_t mark1, float cut, Push push) {
#if VMX_GW_CULL
    const bool h0 = tn0 <= tf0 && (tf0 >= 0.0f || mark0 == 0u), h1 = tn1 <= tf1 && (tf1 >= 0.0f || mark1 == 0u);
#else
    const bool h0 = tn0 <= tf0, h1 = tn1 <= tf1;
#endif
    const bool both = h0 && h1;
    const bool go_right = h1 && (!h0 || tn1 < tn0);
    if (both) push(make_uint2(go_right ? lref : rref, __float_as_uint(go_right ? tn0 : tn1)));
    const float near = go_right ? tn1 : tn0;
    return (!(h0 || h1) || near > cut) ? kPop : (go_right ? rref : lref);
}
template <class Push>
__device__ __forceinline__ uint32_t choose_child_masks_cull(float tn0, float tf0, float tn1, float tf1, uint32_t lref,
                                                            uint32_t rref, uint32_t mark0, uint32_t mark1, float cut, Push push) {
    unsigned long long m0 = __builtin_amdgcn_fcmpf(tn0, tf0, 5), m1 = __builtin_amdgcn_fcmpf(tn1, tf1, 5);
#if VMX_GW_CULL
    m0 &= __builtin_amdgcn_fcmpf(tf0, 0.0f, 3) | __builtin_amdgcn_uicmp(mark0, 0u, 32);
    m1 &= __builtin_amdgcn_fcmpf(tf1, 0.0f, 3) | __builtin_amdgcn_uicmp(mark1, 0u, 32);
#endif
    return choose_child_hit_masks(m0, m1, tn0, tn1, lref, rref, cut, push);
}

// Pops until an entry passes `near > t` (bvh.cpp:69) and returns its reference.  Level 0 holds the bottom entry
// (ref kBottom, near = -inf), which always passes: a finished ray falls out of the loop with kBottom.
__device__ __forceinline__ uint32_t pop_to_next(const uint2 *stk, const uint2 *ovf, int lds_entries, int &sp, float best) {
    uint2 e;
    do {
        --sp;
        e = stack_pop(stk, ovf, lds_entries, sp);
    } while (__uint_as_float(e.y) > best);
    return e.x;
}

// Start of a ray's traversal above the bottom entry.  `limit` is 999999999.f (bvh.cpp:48) or a query's bound.
// (The caller sets its `exact` flag itself, `!(finite3(1/d) && finite3(o))`: behind a call boundary hipcc merges the two
// finite tests into one block, which changes the register allocation of k_trace_w<1> and k_query.)
__device__ __forceinline__ void ray_start(float dx, float dy, float dz, uint32_t root_ref, float limit, float &ix, float &iy,
                                          float &iz, float &best, int &slot, int &sp, uint32_t &cur) {
    ix = 1.0f / dx, iy = 1.0f / dy, iz = 1.0f / dz;  // Ray.h:10
    best = limit;
    slot = -1;
    sp = 1;
    cur = root_ref;  // its near value, -9999999 (bvh.cpp:59), passes `near > t` for any limit > 0
}

// ---------------------------------------------------------------------------
// BVH::getIntersection, nearest hit (bvh.cpp:47-145) + Triangle::getIntersection
// (triangle.cpp:4-54).  `stk` points at this lane's column of the wave's LDS stack.
// ---------------------------------------------------------------------------
template <bool COUNT>
__device__ __forceinline__ void bvh_nearest(const SceneDev &sc, float ox, float oy, float oz, float dx,
                                            float dy, float dz, uint2 *stk, float &best_out,
                                            int &slot_out, Cnt &cnt, uint2 *ovf = nullptr,
                                            int lds_entries = 0x7FFFFFFF /* levels of `stk` in LDS; deeper ones in `ovf` */) {
    const float4 *__restrict__ inner = (const float4 *)sc.inner;
    const float4 *__restrict__ tris = (const float4 *)sc.tris;
    const float ix = 1.0f / dx, iy = 1.0f / dy, iz = 1.0f / dz;  // Ray.h:10
    const bool exact = !(finite3(ix, iy, iz) && finite3(ox, oy, oz));

    float best = 999999999.f;  // bvh.cpp:48
    int slot = -1;
    int sp = 0;
    uint32_t cur = sc.root_ref;
    float cur_near = -9999999.f;  // bvh.cpp:59
    bool have = true;
    for (;;) {
        if (!have) {
            if (sp == 0) break;
            --sp;
            const uint2 e = stack_pop(stk, ovf, lds_entries, sp);
            cur = e.x;
            cur_near = __uint_as_float(e.y);
        }
        have = false;
        if (cur_near > best) continue;  // bvh.cpp:69
        if (cur & kLeafBit) {
            const uint32_t first = cur & kLeafStartMask;
            const uint32_t n = (cur >> kLeafCountShift) & 31u;
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t ti = (first + i) * 3;
                const float4 a = tris[ti], b = tris[ti + 1], c = tris[ti + 2];
                if (COUNT) cnt.tris++;
                float dist;
                const bool hit = tri_test(a, b, c.x, ox, oy, oz, dx, dy, dz, dist);
                if (hit && dist < best) {  // strict <: first tested wins ties (bvh.cpp:90)
                    best = dist;
                    slot = (int)(first + i);
                }
            }
        } else {
            const float4 q0 = inner[cur * 4], q1 = inner[cur * 4 + 1], q2 = inner[cur * 4 + 2],
                         q3 = inner[cur * 4 + 3];
            if (COUNT) cnt.inner++;
            float tn0, tn1;
            bool h0, h1;
            if (exact) {
                h0 = box_exact(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, ox, oy, oz, ix, iy, iz, tn0);
                h1 = box_exact(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, ox, oy, oz, ix, iy, iz, tn1);
            } else {
                h0 = box_fast(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, ox, oy, oz, ix, iy, iz, tn0);
                h1 = box_fast(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, ox, oy, oz, ix, iy, iz, tn1);
            }
            const uint32_t lref = __float_as_uint(q3.x), rref = __float_as_uint(q3.y);
            if (h0 && h1) {
                // left assumed closer; swap if the right child is strictly closer (bvh.cpp:106-114)
                const bool sw = tn1 < tn0;
                const uint32_t closer = sw ? rref : lref, other = sw ? lref : rref;
                const float nc = sw ? tn1 : tn0, no = sw ? tn0 : tn1;
                stack_push(stk, ovf, lds_entries, sp, make_uint2(other, __float_as_uint(no)));  // farther first (bvh.cpp:120)
                ++sp;
                cur = closer;
                cur_near = nc;
                have = true;
            } else if (h0) {
                cur = lref;
                cur_near = tn0;
                have = true;
            } else if (h1) {
                cur = rref;
                cur_near = tn1;
                have = true;
            }
        }
    }
    best_out = best;
    slot_out = slot;
}

// Triangle::getNormal (triangle.cpp:67-86) + normalize in the caller (meshEngine.cpp:369)
__device__ __forceinline__ void tri_shading_normal(const SceneDev &sc, int slot, float hx, float hy,
                                                   float hz, float &nx, float &ny, float &nz, float &uvx,
                                                   float &uvy) {
    const float4 *__restrict__ tris = (const float4 *)sc.tris;
    const float4 *__restrict__ attrs = (const float4 *)sc.attrs;
    const float4 a = tris[slot * 3], b = tris[slot * 3 + 1], c = tris[slot * 3 + 2];
    const float f0x = a.w, f0y = b.x, f0z = b.y, f1x = b.z, f1y = b.w, f1z = c.x;
    const float f2x = hx - a.x, f2y = hy - a.y, f2z = hz - a.z;
    const float d00 = dot3(f0x, f0y, f0z, f0x, f0y, f0z);
    const float d01 = dot3(f0x, f0y, f0z, f1x, f1y, f1z);
    const float d11 = dot3(f1x, f1y, f1z, f1x, f1y, f1z);
    const float d20 = dot3(f2x, f2y, f2z, f0x, f0y, f0z);
    const float d21 = dot3(f2x, f2y, f2z, f1x, f1y, f1z);
    const float denom = d00 * d11 - d01 * d01;
    const float w1 = (d11 * d20 - d01 * d21) / denom;
    const float w2 = (d00 * d21 - d01 * d20) / denom;
    const float w0 = 1.0f - w1 - w2;
    const float4 g0 = attrs[slot * 4], g1 = attrs[slot * 4 + 1], g2 = attrs[slot * 4 + 2],
                 g3 = attrs[slot * 4 + 3];
    // n0 = g0.xyz, n1 = (g0.w, g1.x, g1.y), n2 = (g1.z, g1.w, g2.x)
    const float inx = (g0.x * w0 + g0.w * w1) + g1.z * w2;
    const float iny = (g0.y * w0 + g1.x * w1) + g1.w * w2;
    const float inz = (g0.z * w0 + g1.y * w1) + g2.x * w2;
    // uv0 = (g2.y, g2.z), uv1 = (g2.w, g3.x), uv2 = (g3.y, g3.z)
    uvx = (g2.y * w0 + g2.w * w1) + g3.y * w2;
    uvy = (g2.z * w0 + g3.x * w1) + g3.z * w2;
    nx = -inx;
    ny = -iny;
    nz = -inz;
    normalize3(nx, ny, nz);
}

// sphereIntersect (meshEngine.cpp:182-194): float dots, float rad*rad, double discriminant.
// The caller only uses a result in (0, limit) (limit = RayCast's nearest distance so far), and the
// double-precision part (discriminant, square root, two roots: ~75 f64 instructions per sphere, 8
// spheres per RayCast) was more than half of the shading kernels' time.  Four single-precision
// tests on the same float dot products B = op.d, C = op.op and R2 = rad*rad the reference forms
// decide, with a margin far above every rounding error involved (2^-20 relative against 2^-24 float
// and 2^-53 double steps), that the double-precision result cannot matter:
//   miss   : B^2 < (C - R2) - tol                 =>  det < 0, the reference returns 0
//   behind : B < 0 and (C - R2) > tol             =>  det < B^2 although (B^2 - C) + R2 rounds at the magnitude
//            of C (2^-53 C, ~0.3 for the wall spheres), so both roots are <= 1e-4 (|B| < 1e11): returns 0
//   far    : B > limit and (C - R2) - limit (2B - limit) > tol  =>  det < (B - limit)^2 (1 - 2^-40),
//            so the smaller root rounds to >= limit and the caller ignores it
//   inside : (C - R2) < -tol (the origin is inside the sphere: the smaller root is negative, the result is the
//            larger one) and (C - R2) - limit (2B - limit) < -tol  =>  limit lies between the roots, the larger
//            root is > limit and the caller ignores it.  This is the common case of the reference's room: every
//            ray starts inside four of its six 5e7-radius wall spheres and mostly ends on a triangle first
// Only lanes that pass none of them need the exact evaluation; a wave runs it if any lane does (the
// 64 camera rays of a wave belong to one pixel and mostly agree).
// (op = centre - origin and C = op.op are passed in: for camera rays they are the same for every path
// of a frame and come precomputed, by the same float operations, from LDS)
__device__ __forceinline__ float sphere_hit_op(float opx, float opy, float opz, float C, float R2, float dx, float dy,
                                               float dz, float limit) {
    const float B = dot3(opx, opy, opz, dx, dy, dz);
    const float X = C - R2, BB = B * B;
    constexpr float kRel = 9.5367431640625e-07f;  // 2^-20
    const float tol_m = kRel * (C + R2 + BB);
    const float tol_f = kRel * (C + R2 + BB + limit * (2.f * fabsf(B) + limit));
    const bool miss = BB < X - tol_m;
    const bool behind = B < 0.f && B > -1e11f && X > tol_m;
    const float Y = X - limit * (2.f * B - limit);  // limit^2 - 2 B limit + X: negative iff limit lies between the roots
    const bool far = B > limit * (1.f + kRel) && Y > tol_f;
    const bool inside_far = X < -tol_m && Y < -tol_f;
    const bool need = !(miss || behind || far || inside_far);
    float th = 0.f;
    if (__builtin_amdgcn_ballot_w64(need) != 0) {
        const double b = (double)B;
        double det = b * b - (double)C + (double)R2;
        float v = 0.f;
        if (!(det < 0)) {
            det = sqrt(det);
            double t = b - det;
            if (t > 1e-4) v = (float)t;
            else {
                t = b + det;
                if (t > 1e-4) v = (float)t;
            }
        }
        th = need ? v : 0.f;
    }
    return th;
}
// sphere_hit_op(..., limit = infinity) > 0, without the two tests that need a finite limit (they never fire there)
__device__ __forceinline__ bool sphere_in_reach(float opx, float opy, float opz, float C, float R2, float dx, float dy, float dz) {
    const float B = dot3(opx, opy, opz, dx, dy, dz);
    const float X = C - R2, BB = B * B;
    constexpr float kRel = 9.5367431640625e-07f;  // 2^-20
    const float tol_m = kRel * (C + R2 + BB);
    const bool miss = BB < X - tol_m;
    const bool behind = B < 0.f && B > -1e11f && X > tol_m;
    const bool need = !(miss || behind);
    bool reach = false;
    if (__builtin_amdgcn_ballot_w64(need) != 0) {
        const double b = (double)B;
        double det = b * b - (double)C + (double)R2;
        float v = 0.f;
        if (!(det < 0)) {
            det = sqrt(det);
            double t = b - det;
            if (t > 1e-4) v = (float)t;
            else {
                t = b + det;
                if (t > 1e-4) v = (float)t;
            }
        }
        reach = need && v > 0.f;
    }
    return reach;
}
__device__ __forceinline__ float sphere_hit(float ox, float oy, float oz, float dx, float dy, float dz,
                                            float4 geom /* centre, rad*rad */, float limit) {
    const float opx = geom.x - ox, opy = geom.y - oy, opz = geom.z - oz;
    return sphere_hit_op(opx, opy, opz, dot3(opx, opy, opz, opx, opy, opz), geom.w, dx, dy, dz, limit);
}

struct CastResult {
    float nearest;     // INFINITY on a miss
    float nx, ny, nz;  // pHitNormal
    float cr, cg, cb;  // pHitColour
    float uvx, uvy;
    float tri_t;
    int slot;          // leaf-order slot of the BVH hit, -1 if none
    bool material;
};

// MeshEngine::RayCast after the BVH query (meshEngine.cpp:365-508): triangle normal, sphere table
// `geom`: optional copy of the spheres' (centre, rad*rad) in LDS (k_shade) — every path tests every
// sphere, the rest of a sphere's record is read only when it becomes the nearest hit
constexpr uint32_t kLdsSpheres = 16;
static_assert(kLdsSpheres >= kMaxSpheres, "every sphere of a scene has an LDS slot");
// LDS_GEOM / CAM_OP: compile-time, so that the table reads are plain LDS reads (a pointer chosen at run time
// between LDS and global memory makes them flat loads); the API admits at most kLdsSpheres spheres
// BOUNDS (camera rays of ONE pixel in the wave, k_shade<0>): `lmax` is a row in LDS, lmax[i] = pixel_sphere_bound of the
// wave's pixel for sphere i, lmax[kLdsSpheres] their minimum (!use_lmax: no bounds, every sphere is evaluated).  A lane
// whose nearest distance on entry — the triangle's, +inf after a BVH miss — is <= lmax[i] cannot be changed by
// sphere i (nearest only shrinks in the loop, so the decision holds); the comparison is false for a NaN distance and for
// lmax = 0 ("no claim") against any positive one.  Per lane the decision, per wave the branch: no lane needs any
// sphere — the common case, a pixel whose rays end on triangles inside the room — and the loop is not entered;
// otherwise the spheres no lane needs are passed over one by one, and the others run sphere_hit_op as before
template <bool LDS_GEOM = false, bool CAM_OP = false, bool BOUNDS = false>
__device__ __forceinline__ void cast_finish(const SceneDev &sc, float ox, float oy, float oz, float dx,
                                            float dy, float dz, float best, int slot, CastResult &r,
                                            const float4 *geom = nullptr, const float4 *cam_op = nullptr,
                                            const float *lmax = nullptr, bool use_lmax = false) {
    r.nearest = kInf;
    r.nx = r.ny = r.nz = 0.f;
    r.cr = r.cg = r.cb = 0.f;
    r.uvx = r.uvy = 0.f;
    r.tri_t = best;
    r.slot = slot;
    r.material = false;
    if (slot >= 0) {
        r.nearest = best;
        const float hx = ox + dx * best, hy = oy + dy * best, hz = oz + dz * best;  // bvh.cpp:140
        tri_shading_normal(sc, slot, hx, hy, hz, r.nx, r.ny, r.nz, r.uvx, r.uvy);
        r.material = true;  // hitMeshIndex = 0 (meshEngine.cpp:370), never reset
    }
    const uint32_t ns = sc.nspheres;
    const float entry = r.nearest;
    const bool bounded = BOUNDS && use_lmax;
    if (bounded && __builtin_amdgcn_ballot_w64(!(entry <= lmax[kLdsSpheres])) == 0) return;
    for (uint32_t i = 0; i < ns; ++i) {
        if (bounded) {
            if (__builtin_amdgcn_ballot_w64(!(entry <= lmax[i])) == 0) continue;
        }
        float4 g;
        if (LDS_GEOM) {
            g = geom[i];
        } else {
            const SphereDev &q = sc.spheres[i];
            g = make_float4(q.cx, q.cy, q.cz, q.rad2);
        }
        float th;
        if (CAM_OP) {  // (centre - camera, its squared length): camera rays only
            const float4 q = cam_op[i];
            th = sphere_hit_op(q.x, q.y, q.z, q.w, g.w, dx, dy, dz, r.nearest);
        } else {
            th = sphere_hit(ox, oy, oz, dx, dy, dz, g, r.nearest);
        }
        if (th > 0.f && th < r.nearest) {
            const SphereDev s = sc.spheres[i];
            r.nearest = th;
            if (s.flags & 1u) {
                r.cr = s.colr;
                r.cg = s.colg;
                r.cb = s.colb;
            }
            float px = ox + (dx * th) - s.ncx, py = oy + (dy * th) - s.ncy, pz = oz + (dz * th) - s.ncz;
            normalize3(px, py, pz);
            r.nx = px * s.nsign;
            r.ny = py * s.nsign;
            r.nz = pz * s.nsign;
        }
    }
}

// MeshEngine::RayCast (meshEngine.cpp:239-509)
template <bool COUNT>
__device__ __forceinline__ void ray_cast(const SceneDev &sc, float ox, float oy, float oz, float dx,
                                         float dy, float dz, uint2 *stk, CastResult &r, Cnt &cnt, uint2 *ovf = nullptr,
                                         int lds_entries = 0x7FFFFFFF) {
    float best;
    int slot;
    bvh_nearest<COUNT>(sc, ox, oy, oz, dx, dy, dz, stk, best, slot, cnt, ovf, lds_entries);
    cast_finish(sc, ox, oy, oz, dx, dy, dz, best, slot, r);
}

// ---------------------------------------------------------------------------
// one iteration of Radiance's bounce loop (pathtracer.cpp:34-197)
// ---------------------------------------------------------------------------
struct Path {
    float ox, oy, oz, dx, dy, dz;
    float tr, tg, tb, tw;  // accumRadiance; only maintained by the textured kernels (w: the product of the samples' fourth
                           // components — it only ever reaches accumColour.w as tw * 0, i.e. as a NaN when it is not finite)
    float ar, ag, ab, aw;  // accumColour
    uint32_t depth, dest;
    Rng rng;
};

struct StepFlags {
    bool was_ray, tri_hit, continues;
};

// Radiance's loop body after RayCast (pathtracer.cpp:36-196).
// returns true if the path continues with a new ray in P, false if accumColour is final
// VermiTexture::Sample (meshEngine.cpp:21-46): wrap x - floor(x), nearest round(x*(W-1)), 1-4 channels.
// The texel index is clamped (the reference indexes out of bounds on a NaN uv).
__device__ __forceinline__ float4 tex_sample_of(const float *tex, uint32_t tex_w, uint32_t tex_h, uint32_t tex_c, float u,
                                                float v) {
    const float sx = u - floorf(u), sy = v - floorf(v);
    uint32_t mx = (uint32_t)roundf(sx * (float)(int)(tex_w - 1));
    uint32_t my = (uint32_t)roundf(sy * (float)(int)(tex_h - 1));
    mx = min(mx, tex_w - 1);
    my = min(my, tex_h - 1);
    const float *p = tex + ((size_t)my * tex_w + mx) * tex_c;
    switch (tex_c) {
        case 1: return make_float4(p[0], p[0], p[0], p[0]);
        case 2: return make_float4(p[0], p[1], 0.f, 0.f);
        case 3: return make_float4(p[0], p[1], p[2], 0.f);
        default: return make_float4(p[0], p[1], p[2], p[3]);
    }
}
__device__ __forceinline__ float4 tex_sample(const SceneDev &sc, float u, float v) {
    return tex_sample_of(sc.tex, sc.tex_w, sc.tex_h, sc.tex_c, u, v);
}

// cosf / sinf of r1 in [0, 2 pi] as glibc computes them (sysdeps/ieee754/flt-32/s_sinf.c, s_cosf.c, sincosf.h —
// ARM optimized-routines): the default reading of the unqualified cos(r1) / sin(r1) with float r1 at
// pathtracer.cpp:155,162 (include/vermilion_hip.h: VMX_SAMPLING_LIBM_DOUBLE).  Double-precision operations in
// glibc's order, no contraction; the test suite's CPU restatement of the same algorithm is pinned against the
// host libm on every float of the range, and vmx_trig() exposes this function for the comparison.
// which = 0: sinf, 1: cosf.
__device__ __forceinline__ float libm_sincosf_poly(double x, double x2, bool neg, int n) {
    if ((n & 1) == 0) {
        const double x3 = x * x2, s1 = 0x1.1107605230bc4p-7 + x2 * -0x1.994eb3774cf24p-13, x7 = x3 * x2,
                     s = x + x3 * -0x1.555545995a603p-3;
        return (float)(s + x7 * s1);
    }
    // the second table is the first with the cosine coefficients negated
    const double c0 = neg ? -0x1p0 : 0x1p0, c1 = neg ? 0x1.ffffffd0c621cp-2 : -0x1.ffffffd0c621cp-2,
                 c2 = neg ? -0x1.55553e1068f19p-5 : 0x1.55553e1068f19p-5,
                 c3 = neg ? 0x1.6c087e89a359dp-10 : -0x1.6c087e89a359dp-10,
                 c4 = neg ? -0x1.99343027bf8c3p-16 : 0x1.99343027bf8c3p-16;
    const double x4 = x2 * x2, k2 = c3 + x2 * c4, k1 = c0 + x2 * c1, x6 = x4 * x2, c = k1 + x4 * c2;
    return (float)(c + x6 * k2);
}
__device__ __forceinline__ float libm_sincosf(float y, int which) {
    const uint32_t top = (__float_as_uint(y) >> 20) & 0x7ffu;
    double x = (double)y;
    if (top < 0x3f4u) {                      // |y| < pi/4 (abstop12 of 0x1.921FB6p-1f)
        if (top < 0x398u) return which ? 1.0f : y;  // |y| < 2^-12
        return libm_sincosf_poly(x, x * x, false, which);
    }
    const double r = x * 0x1.45F306DC9C883p+23;
    const int n = ((int)r + 0x800000) >> 24;
    x = x - (double)n * 0x1.921FB54442D18p0;
    const double sx = ((n + 1) & 2) ? -x : x;   // sign[n & 3] = {1, -1, -1, 1}
    return libm_sincosf_poly(sx, x * x, (n & 2) != 0, n ^ which);
}

// sampling configuration of a Radiance step: r2 = r2scale * U (pathtracer.cpp:156,170; 10 or 1), and the
// reading of cos/sin(float) at :155,162 (VMX_SAMPLING_LIBM_DOUBLE)
struct SampCfg {
    float r2scale;
    uint32_t libm_double;
    uint32_t elide;  // VMX_SAMPLING_ELIDE_DEAD (step_is_dead)
};

// The loop body is split where the cosine-lobe branch needs cos/sin of r1 (double precision, a few
// hundred instructions): only ~10 % of the paths get there (the others end, or bounce off the
// mirror lobe) — a wave in which no lane gets there skips them.
struct ShadeMid {
    float sx, sy, sz;  // origin of the next ray
    float r2s, q;      // sqrt(r2), sqrt(1 - r2)
    double angle;      // r1
    float angle_f;     // r1 where the reference holds it in a float (material branch, :155); NaN marks the double branch
};
// cos and sin of a path's r1 under the configured reading
__device__ __forceinline__ void shade_trig(const ShadeMid &m, uint32_t libm_double, float &cs, float &sn) {
    if (!libm_double && m.angle_f == m.angle_f) {
        cs = libm_sincosf(m.angle_f, 1);
        sn = libm_sincosf(m.angle_f, 0);
    } else {
        // one range reduction for both (sincos returns exactly sin and cos: same kernels; the frame tests would show)
        double s, c;
        sincos(m.angle, &s, &c);
        cs = (float)c, sn = (float)s;
    }
}
enum { kPathEnded = 0, kPathNextRay = 1, kPathNeedsTrig = 2 };

__device__ __forceinline__ bool path_set_ray(Path &P, StepFlags &fl, float sx, float sy, float sz, float ndx, float ndy,
                                             float ndz) {
    P.ox = sx, P.oy = sy, P.oz = sz;
    P.dx = ndx, P.dy = ndy, P.dz = ndz;
    // An all-NaN direction (r2 > 1, pathtracer.cpp:156-162) misses the BVH and
    // every sphere in RayCast, so Radiance returns accumColour: end the path here.
    if ((ndx != ndx) && (ndy != ndy) && (ndz != ndz)) return false;
    fl.continues = finite3(ndx, ndy, ndz);
    return true;
}

template <bool TEX>
__device__ __forceinline__ int path_shade_begin(const SceneDev &sc, float r2scale, Path &P, const CastResult &c,
                                                StepFlags &fl, ShadeMid &m) {
    m.angle_f = __uint_as_float(0x7FC00000u);
    fl.tri_hit = c.slot >= 0;
    fl.continues = false;
    if (!(c.nearest < kInf)) return kPathEnded;  // pathtracer.cpp:36-41
    if (TEX) {  // :43
        P.ar = P.ar + P.tr * c.cr;
        P.ag = P.ag + P.tg * c.cg;
        P.ab = P.ab + P.tb * c.cb;
        P.aw = P.aw + P.tw * 0.f;  // accumRadiance * vec4(hitColour, 0.f): NaN once the fourth component is not finite
    } else {
        // untextured: accumRadiance stays (1,1,1,1) — the only factor ever applied to it is the white
        // albedo (:75-79,153) — so the product is exactly hitColour
        P.ar = P.ar + c.cr;
        P.ag = P.ag + c.cg;
        P.ab = P.ab + c.cb;
    }
    if (P.depth == 0) P.aw = c.nearest;                                   // :44-47
    if (sqrtf(dot3(c.cr, c.cg, c.cb, c.cr, c.cg, c.cb)) > 1.f) return kPathEnded;  // :52
    P.depth++;
    if (P.depth > 5) {  // :56 — the draw happens only past depth 5
        const double rr = rng_u01(P.rng);
        if (rr > (double)0.95f || P.depth > 1000) return kPathEnded;
    }
    // hit location and back-off along the incoming ray (:108,163,189)
    const float lx = P.ox + (P.dx * c.nearest), ly = P.oy + (P.dy * c.nearest), lz = P.oz + (P.dz * c.nearest);
    m.sx = lx - P.dx * 0.001f, m.sy = ly - P.dy * 0.001f, m.sz = lz - P.dz * 0.001f;
    bool specular = false;
    if (c.material) specular = rng_u01(P.rng) >= 0.96;  // :98
    if (specular) {
        (void)rng_next(P.rng);
        (void)rng_next(P.rng);
        (void)rng_next(P.rng);  // unused noise, :101-103
        const float k = dot3(c.nx, c.ny, c.nz, P.dx, P.dy, P.dz);
        float ndx = P.dx - c.nx * 2.f * k;
        float ndy = P.dy - c.ny * 2.f * k;
        float ndz = P.dz - c.nz * 2.f * k;
        normalize3(ndx, ndy, ndz);
        return path_set_ray(P, fl, m.sx, m.sy, m.sz, ndx, ndy, ndz) ? kPathNextRay : kPathEnded;
    }
    if (c.material) {  // :151-165
        if (TEX) {  // accumRadiance *= sampleColour (:153), sampled at the BVH hit's uv (:63-66)
            const float4 tx = tex_sample(sc, c.uvx, c.uvy);
            P.tr = P.tr * tx.x;
            P.tg = P.tg * tx.y;
            P.tb = P.tb * tx.z;
            P.tw = P.tw * tx.w;
        }
        const float r1 = (float)(6.283185307179586 * rng_u01(P.rng));
        const float r2 = (float)((double)r2scale * rng_u01(P.rng));
        m.r2s = sqrtf(r2);
        m.angle = (double)r1;
        m.angle_f = r1;
        m.q = sqrtf(1.0f - r2);
    } else {  // :166-196 — nearest hit is a sphere and the BVH hit nothing
        const double r1 = 6.283185307179586 * rng_u01(P.rng);
        const double r2 = (double)r2scale * rng_u01(P.rng);
        m.r2s = (float)sqrt(r2);
        (void)rng_next(P.rng);
        (void)rng_next(P.rng);
        (void)rng_next(P.rng);  // :173-175
        m.angle = r1;
        m.q = (float)sqrt(1.0 - r2);
    }
    // r2 > 1 (9 draws in 10 with the reference's r2 = 10 U): q is NaN, so every component of
    // (u cs r2s + v sn r2s) + w q is NaN whatever cos and sin are, and the path ends (path_set_ray)
    if (m.q != m.q) return kPathEnded;
    return kPathNeedsTrig;
}

// second half of the cosine-lobe branch (pathtracer.cpp:158-165,176-196): cs = (float)cos(r1), sn = (float)sin(r1)
__device__ __forceinline__ bool path_shade_end(Path &P, const CastResult &c, StepFlags &fl, const ShadeMid &m, float cs,
                                               float sn) {
    const bool facing = dot3(c.nx, c.ny, c.nz, P.dx, P.dy, P.dz) < 0.f;
    const float wx = facing ? c.nx : c.nx * -1.f, wy = facing ? c.ny : c.ny * -1.f,
                wz = facing ? c.nz : c.nz * -1.f;
    const bool use_y = (double)fabsf(wx) > .1;
    const float ax = use_y ? 0.f : 1.f, ay = use_y ? 1.f : 0.f, az = 0.f;
    float ux, uy, uz, vx, vy, vz;
    cross3(ax, ay, az, wx, wy, wz, ux, uy, uz);
    normalize3(ux, uy, uz);
    cross3(wx, wy, wz, ux, uy, uz, vx, vy, vz);
    float ndx = (ux * cs * m.r2s + vx * sn * m.r2s) + wx * m.q;
    float ndy = (uy * cs * m.r2s + vy * sn * m.r2s) + wy * m.q;
    float ndz = (uz * cs * m.r2s + vz * sn * m.r2s) + wz * m.q;
    normalize3(ndx, ndy, ndz);
    return path_set_ray(P, fl, m.sx, m.sy, m.sz, ndx, ndy, ndz);
}

// VMX_SAMPLING_ELIDE_DEAD: is the Radiance step that would trace this ray provably without effect on the path's colour?
// `rng`, `depth`, the ray and the throughput are the path's state before that step.  The step adds accumRadiance *
// hitColour (pathtracer.cpp:43), and hitColour is non-zero only where a light sphere is the hit (meshEngine.cpp:382-383,
// 415-416); a miss returns accumColour as it is (:36-41).  The step is the path's last one, whatever it hits, iff the
// path's own draws say so for BOTH values of the material flag:
//   Russian roulette (:56, past depth 5): its draw > 0.95f, or
//   material (:98-165): not the mirror branch (next draw < 0.96) and r2 = float(10 * third draw) > 1, so sqrt(1 - r2)
//     is NaN and with it the next direction, which misses everything and
//   no material (:166-196): r2 = 10 * second draw > 1 (double), the same.
// No light sphere can colour it iff sphereIntersect is 0 for every emitting sphere — the reference's own arithmetic with
// nothing nearer yet (limit = infinity).  Then accumColour after the step equals accumColour before it bit for bit
// (x + t * 0 == x for finite t), so the ray need not be traced: with the reference's r2 = 10 U that is 78 % of all rays.
// (Under VMX_SAMPLING_CORRECTED r2 = U never exceeds 1: only Russian roulette, past depth 5, ever ends a path by its draws.)
// The same facts as three bits — what the kernels pass along with a ray (DESIGN_HISTORY.md 5.1), step_is_dead being "bits == 3":
//   bit 0  the step is the path's last one if its hit has a material   (Russian roulette, or the draws of :98 / :156)
//   bit 1  ... if its hit has none                                      (Russian roulette, or the draw of :170)
//   bit 2  some light sphere passes sphereIntersect > 0 for the ray with nothing nearer yet: hitColour may be non-zero
// (bits 0 and 1 are left clear for a path whose throughput is not finite: inf * 0 would be NaN, the step is shaded in full)
// (test_lights == false: the caller has shown that no ray of this pixel can pass sphereIntersect > 0 for any emitting
// sphere — pixel_may_reach_a_light — so bit 2 is clear without the per-ray tests, and the direction is not needed at all)
template <bool TEX>
__device__ __forceinline__ uint32_t step_bits(const SceneDev &sc, float r2scale, Rng rng, uint32_t depth, float ox, float oy,
                                              float oz, float dx, float dy, float dz, float tr, float tg, float tb,
                                              bool test_lights = true) {
    bool rr_end = false;
    if (depth + 1u > 5u) {
        const double rr = rng_u01(rng);
        rr_end = rr > (double)0.95f || depth + 1u > 1000u;
    }
    const double a = rng_u01(rng), b = rng_u01(rng), c = rng_u01(rng);
    const float r2m = (float)((double)r2scale * c);
    bool ends_mat = rr_end || (!(a >= 0.96) && (1.0f - r2m) < 0.0f);
    bool ends_nomat = rr_end || (1.0 - (double)r2scale * b) < 0.0;
    if (TEX && !finite3(tr, tg, tb)) ends_mat = ends_nomat = false;
    bool light = false;
    for (uint32_t i = 0; test_lights && i < sc.emit_prefix; ++i) {
        const SphereDev &q = sc.spheres[i];
        if (q.flags & 1u) {
            const float opx = q.cx - ox, opy = q.cy - oy, opz = q.cz - oz;
            if (sphere_in_reach(opx, opy, opz, dot3(opx, opy, opz, opx, opy, opz), q.rad2, dx, dy, dz)) light = true;
        }
    }
    return (ends_mat ? 1u : 0u) | (ends_nomat ? 2u : 0u) | (light ? 4u : 0u);
}
template <bool TEX>
__device__ __forceinline__ bool step_is_dead(const SceneDev &sc, float r2scale, Rng rng, uint32_t depth, float ox, float oy,
                                             float oz, float dx, float dy, float dz, float tr, float tg, float tb) {
    return step_bits<TEX>(sc, r2scale, rng, depth, ox, oy, oz, dx, dy, dz, tr, tg, tb) == 3u;
}

// Radiance's loop body after RayCast in one piece (the fused kernels)
template <bool TEX, bool LDS_GEOM = false>
__device__ __forceinline__ bool path_shade(const SceneDev &sc, SampCfg cfg, Path &P, const CastResult &c,
                                           StepFlags &fl, const float4 *geom = nullptr) {
    ShadeMid m;
    const int st = path_shade_begin<TEX>(sc, cfg.r2scale, P, c, fl, m);
    bool alive = st == kPathNextRay;
    if (st == kPathNeedsTrig) {
        float sn, cs;
        shade_trig(m, cfg.libm_double, cs, sn);
        alive = path_shade_end(P, c, fl, m, cs, sn);
    }
    if (cfg.elide && alive && step_is_dead<TEX>(sc, cfg.r2scale, P.rng, P.depth, P.ox, P.oy, P.oz, P.dx, P.dy, P.dz, P.tr, P.tg, P.tb))
        alive = false, fl.continues = false;
    return alive;
}

__device__ __forceinline__ void tally_add(Tally &tl, const StepFlags &fl, bool ran, uint32_t stage_depth0) {
    // stage 0 = steps taken at depth 0, stage 1 = bounce steps
    const unsigned long long r0 = __ballot(ran && fl.was_ray && stage_depth0);
    const unsigned long long r1 = __ballot(ran && fl.was_ray && !stage_depth0);
    const unsigned long long h0 = __ballot(ran && fl.tri_hit && fl.was_ray && stage_depth0);
    const unsigned long long h1 = __ballot(ran && fl.tri_hit && fl.was_ray && !stage_depth0);
    const unsigned long long c0 = __ballot(ran && fl.continues && stage_depth0);
    const unsigned long long c1 = __ballot(ran && fl.continues && !stage_depth0);
    tl.rays[0] += (uint32_t)__popcll(r0);
    tl.rays[1] += (uint32_t)__popcll(r1);
    tl.hits[0] += (uint32_t)__popcll(h0);
    tl.hits[1] += (uint32_t)__popcll(h1);
    tl.cont[0] += (uint32_t)__popcll(c0);
    tl.cont[1] += (uint32_t)__popcll(c1);
}

template <bool COUNT>
__device__ __forceinline__ void tally_flush(DevCounters *ctr, const Tally &tl, const Cnt &c0, const Cnt &c1) {
    uint32_t i0 = 0, t0 = 0, i1 = 0, t1 = 0;
    if (COUNT) {
        i0 = wave_sum(c0.inner);
        t0 = wave_sum(c0.tris);
        i1 = wave_sum(c1.inner);
        t1 = wave_sum(c1.tris);
    }
    if (lane_index() == 0) {
        for (int s = 0; s < 2; ++s) {
            if (tl.rays[s]) atomicAdd(&ctr->stage[s].rays, (unsigned long long)tl.rays[s]);
            if (tl.hits[s]) atomicAdd(&ctr->stage[s].tri_hits, (unsigned long long)tl.hits[s]);
            if (tl.cont[s]) atomicAdd(&ctr->stage[s].continued, (unsigned long long)tl.cont[s]);
        }
        if (COUNT) {
            if (i0) atomicAdd(&ctr->stage[0].inner_visits, (unsigned long long)i0);
            if (t0) atomicAdd(&ctr->stage[0].tri_tests, (unsigned long long)t0);
            if (i1) atomicAdd(&ctr->stage[1].inner_visits, (unsigned long long)i1);
            if (t1) atomicAdd(&ctr->stage[1].tri_tests, (unsigned long long)t1);
        }
    }
}

// ---------------------------------------------------------------------------
// ray generation (pathtracer.cpp:251-280); p = global pixel index, k = linear sample index
// ---------------------------------------------------------------------------
// a / n in double, correctly rounded, for an integer 1 <= n < 2^32 whose reciprocal y = RN(1 / n) the host computed by an
// IEEE division (FrameDev::inv_width / inv_height): three operations instead of the ~35 of a double division, two of
// which sat in every camera ray's generation (pathtracer.cpp:251-252 divide by the image size in double).  Markstein's
// correction step: q0 = RN(a y) is within 2 ulp of a / n; e = a - n q0 is exact in an FMA (a multiple of ulp(q0), at
// most 2^33 of them); q0 + e y = a / n + (e / n) delta with |delta| <= 2^-53, i.e. within 2^-104 relative of a / n —
// while a / n, n an integer below 2^32, is either a double or at least 2^-86 relative away from every midpoint
// between two doubles (a - m n, m such a midpoint, is a non-zero multiple of ulp(m) / 2: m n has more than 53
// significant bits and cannot equal a).  So RN(q0 + e y) = RN(a / n), for every finite a.  Checked exhaustively on
// the CPU for every float a camera ray can produce at the bench's and the tests' image sizes
// (tests/test_kernel_shortcuts.py::test_division_by_the_image_size...).
__device__ __forceinline__ double div_by_count(double a, uint32_t n, double y) {
    const double q0 = a * y;
    const double e = __fma_rn(-q0, (double)n, a);
    return __fma_rn(e, y, q0);
}
// (pk: the pixel half of the stream key, which a caller that walks the samples of one pixel forms once)
__device__ __forceinline__ void primary_ray_keyed(const FrameDev &fr, uint32_t p, PixelKey pk, uint32_t k, Rng &rng, float &dx,
                                                  float &dy, float &dz) {
    rng_init_keyed(rng, pk, k);
    const float jx = rng_jitter(rng);  // :251
    const float jy = rng_jitter(rng);  // :252
    const uint32_t s = k / fr.quarter;
    const float sx = (float)(s >> 1), sy = (float)(s & 1u);
    const float fx = (float)(p % fr.width) + (sx * 0.5f - 0.5f) + jx;
    const float fy = (float)(p / fr.width) + (sy * 0.5f - 0.5f) + jy;
    const float hx = (float)(div_by_count((double)fx - 0.25, fr.width, fr.inv_width) - 0.5);
    const float hy = (float)(div_by_count((double)fy - 0.25, fr.height, fr.inv_height) - 0.5);
    const float gx = hx * fr.sensor_x, gy = -(hy * fr.sensor_y), gz = -fr.film_dist;
    // cameraTransform * gridPane, GLM order (m0*x + m1*y) + (m2*z + m3*w), m3.xyz = 0, w = 1
    float rx = (fr.m[0] * gx + fr.m[3] * gy) + (fr.m[6] * gz + 0.0f);
    float ry = (fr.m[1] * gx + fr.m[4] * gy) + (fr.m[7] * gz + 0.0f);
    float rz = (fr.m[2] * gx + fr.m[5] * gy) + (fr.m[8] * gz + 0.0f);
    normalize3(rx, ry, rz);
    dx = rx, dy = ry, dz = rz;
}
__device__ __forceinline__ void primary_ray(const FrameDev &fr, uint32_t p, uint32_t k, Rng &rng, float &dx,
                                            float &dy, float &dz) {
    primary_ray_keyed(fr, p, rng_pixel_key(fr.seed, p), k, rng, dx, dy, dz);
}

// Can ANY camera ray of pixel p pass sphereIntersect > 0 (meshEngine.cpp:182-194, nothing nearer yet) for some emitting
// sphere?  A conservative answer for the whole pixel, so that k_raygen need not run the per-ray tests — nor, where the
// step's draws already say "last step", form the ray's direction at all — for the pixels that cannot: most of a frame.
// The sample directions of a pixel are normalize(M film) with the film point within half a pixel of the centre
// ((px - 0.25) / W - 0.5, pathtracer.cpp:251-252 with the offsets' range [-0.75, 0.25)): a cone of half-angle phi,
// sin phi <= half the pixel's film diagonal / |film point|, around the centre direction a.  For a sphere (centre c,
// radius r), op = c - o, cos theta = op.a / |op|: every ray of the cone has op.d / |op| <= m = cos(theta - phi), and
// sphereIntersect returns 0 when b^2 < |op|^2 - r^2 (negative discriminant) or when b < 0 with the origin outside the
// sphere (both roots negative).  "Cannot reach" is claimed only with max(m, 0)^2 (1 + 1e-4) + 1e-3 < 1 - r^2 / |op|^2:
// a margin five orders of magnitude above the float rounding of b = dot(op, d), |op|^2 and r^2 that the per-ray test
// (sphere_in_reach) computes with — a sphere within ~1.8 degrees of the cone is simply tested per ray as before.
struct PixelCone {
    float ax, ay, az, alen;  // the centre direction a (not normalised) and its length
    float sphi, cphi;        // sine and cosine of the half-angle
};
struct FilmDev {  // the frame's film: FrameDev's width, height, sensor_x, sensor_y, film_dist
    uint32_t width, height;
    float sensor_x, sensor_y, film_dist;
};
__device__ __forceinline__ PixelCone pixel_cone(const FrameDev &fr, const FilmDev &fm, uint32_t p) {
    const float fw = (float)fm.width, fh = (float)fm.height;
    const float hx = ((float)(p % fm.width) - 0.25f) / fw - 0.5f;
    const float hy = ((float)(p / fm.width) - 0.25f) / fh - 0.5f;
    const float gx = hx * fm.sensor_x, gy = -(hy * fm.sensor_y), gz = -fm.film_dist;
    PixelCone cn;
    cn.ax = fr.m[0] * gx + fr.m[3] * gy + fr.m[6] * gz;
    cn.ay = fr.m[1] * gx + fr.m[4] * gy + fr.m[7] * gz;
    cn.az = fr.m[2] * gx + fr.m[5] * gy + fr.m[8] * gz;
    cn.alen = sqrtf(cn.ax * cn.ax + cn.ay * cn.ay + cn.az * cn.az);
    const float px = fm.sensor_x / fw, py = fm.sensor_y / fh;
    cn.sphi = fminf(0.505f * sqrtf(px * px + py * py) / cn.alen, 1.0f);  // half the diagonal, +1 %
    cn.cphi = sqrtf(fmaxf(1.0f - cn.sphi * cn.sphi, 0.0f));
    return cn;
}
__device__ __forceinline__ bool pixel_may_reach_a_light(const SceneDev &sc, const FrameDev &fr, uint32_t p) {
    const PixelCone cn = pixel_cone(fr, FilmDev{fr.width, fr.height, fr.sensor_x, fr.sensor_y, fr.film_dist}, p);
    const float ax = cn.ax, ay = cn.ay, az = cn.az, alen = cn.alen, sphi = cn.sphi, cphi = cn.cphi;
    bool may = !(alen > 0.0f);  // (a degenerate film: no claim)
    for (uint32_t i = 0; i < sc.emit_prefix; ++i) {
        const SphereDev &q = sc.spheres[i];
        if (!(q.flags & 1u)) continue;
        const float opx = q.cx - fr.px, opy = q.cy - fr.py, opz = q.cz - fr.pz;
        const float C = opx * opx + opy * opy + opz * opz;
        const float ct = (opx * ax + opy * ay + opz * az) / (sqrtf(C) * alen);
        const float st = sqrtf(fmaxf(1.0f - ct * ct, 0.0f));
        const float m = ct >= cphi ? 1.0f : fmaxf(ct * cphi + st * sphi, 0.0f);  // cos(theta - phi); 1 inside the cone
        const float clear = 1.0f - q.rad2 / C;                                    // 1 - r^2 / |op|^2
        if (!(m * m * 1.0001f + 1e-3f < clear)) may = true;                      // (NaN / inf / origin inside: may)
    }
    return may;
}

// lmax(p, s): a distance such that for EVERY camera ray d of pixel p and every limit <= lmax, sphereIntersect(o, d, s)
// (meshEngine.cpp:182-194, on the float B = dot(op, d), C = dot(op, op), R2 = rad * rad) is either 0 or >= limit — so
// cast_finish's `th > 0 && th < nearest` is false for a ray whose nearest distance so far is <= lmax, whatever the
// exact value, and the sphere is passed over for it without the per-ray tests of sphere_hit_op.  Four answers:
//   +inf  never matters: the camera is outside the sphere by a margin and no ray of the cone reaches it, or it lies
//         behind the cone — the test of pixel_may_reach_a_light (valid for a ray that hit no triangle, too)
//   > 0   exit beyond: the camera is inside the sphere by a margin, D = R2 - C > 2^-18 (C + R2); D is exact in
//         double for the floats C, R2 the per-ray code uses, while the reference's (b b - C) + R2 rounds by at most
//         2^-52 max(b b, C), 2^-34 of D.  Its result is the larger root T(b) = b + sqrt(b b + D), which grows with b, so
//         T(b_lo) bounds it for b_lo <= every float B of the cone:
//           b_lo = |op| cos(theta + phi) - 2^-10 |op|      (cos = -1 once theta + phi >= pi)
//         The margin stands against: the rounding of dot3 (3 x 2^-24 |op|), of the direction's three components and
//         its length (5 x 2^-24 |op|), the direction's angle against the ideal film point (float film coordinates and
//         matrix product, < 1e-6 rad, i.e. < 1e-6 |op| in b), and this function's own cosine (ct, st from a cross
//         product, cphi with sphi <= 0.5: < 1e-6 absolute) — 2.5e-6 |op| in all, the margin is 400 times that.  For a
//         wall sphere of the reference's room (|op| ~ 5e7, one ulp of B = 4, dT/db = T / sqrt(b b + D) ~ 1e-5) it
//         moves T by 1e-3 of itself.  T is evaluated without cancellation (D / (s - b) for b < 0), 5 float
//         operations of 2^-24 each, and is then shrunk by 2^-13: 250 times that and the 2^-24 of the reference's
//         own (float) t.
//   > 0   entry beyond: the camera is outside the sphere by the same margin, X = C - R2 > 2^-18 (C + R2), and the cone
//         may reach it (in the reference's room: its floor and ceiling spheres, for nearly every pixel).  A ray that
//         misses returns 0; one that hits returns the smaller root t(b) = b - sqrt(b b - X) = X / (b + sqrt(b b - X)),
//         which falls as b grows, so t(b_hi) bounds it from below for
//           b_hi = max(|op| max(cos(theta - phi), 0) + 2^-10 |op|, sqrt(X))    (the margin: as for b_lo)
//         with the square root taken of b_hi b_hi (1 + 2^-20) - X (1 - 2^-20), 16 times the three roundings of that
//         difference, so that it is not below the true one where the two terms cancel (a grazing cone); the
//         reference's own rounding of (b b - C) + R2 moves its root by at most sqrt(2^-52 C), 2^-17 of sqrt(X), the
//         least the bound can be compared with; then the same shrink by 2^-13
//   0     no claim: the camera near the surface, a degenerate film, a half-angle
//         above 30 degrees, any NaN or infinity (every comparison below is false on a NaN).  The ray is tested as before.
// Checked against the reference's arithmetic in tests/test_pixel_sphere_bounds.py.
__device__ __forceinline__ float pixel_sphere_bound(const PixelCone &cn, float opx, float opy, float opz, float C, float R2) {
    constexpr float kMarginB = 9.765625e-04f;        // 2^-10
    constexpr float kInsideRel = 3.814697265625e-06f;  // 2^-18
    constexpr float kShrink = 1.0f - 1.220703125e-04f;  // 1 - 2^-13
    constexpr float kRootRel = 9.5367431640625e-07f;    // 2^-20
    const float len = sqrtf(C), norm = len * cn.alen;
    const float ct = (opx * cn.ax + opy * cn.ay + opz * cn.az) / norm;
    float kx, ky, kz;
    cross3(opx, opy, opz, cn.ax, cn.ay, cn.az, kx, ky, kz);
    const float st = sqrtf(kx * kx + ky * ky + kz * kz) / norm;
    const bool cone_ok = cn.alen > 0.0f && cn.sphi <= 0.5f;
    const float m = ct >= cn.cphi ? 1.0f : fmaxf(ct * cn.cphi + st * cn.sphi, 0.0f);  // cos(theta - phi); 1 inside the cone
    const float clear = 1.0f - R2 / C;                                                // 1 - r^2 / |op|^2
    const bool never = cone_ok && m * m * 1.0001f + 1e-3f < clear;
    const float cmin = ct <= -cn.cphi ? -1.0f : fmaxf(ct * cn.cphi - st * cn.sphi, -1.0f);  // cos(theta + phi)
    const float blo = len * cmin - kMarginB * len;
    const float D = R2 - C;
    const bool inside = cone_ok && D > kInsideRel * (C + R2);
    const float s = sqrtf(blo * blo + D);
    const float T = (blo < 0.0f ? D / (s - blo) : blo + s) * kShrink;
    const float X = C - R2;
    const bool outside = cone_ok && X > kInsideRel * (C + R2);
    const float bhi = fmaxf(len * m + kMarginB * len, sqrtf(X));
    const float s_up = sqrtf(fmaxf(bhi * bhi * (1.0f + kRootRel) - X * (1.0f - kRootRel), 0.0f));
    const float E = X / (bhi + s_up) * kShrink;
    const float lm = inside ? T : E;
    return never ? kInf : ((inside || outside) && lm > 0.0f && lm < kInf ? lm : 0.0f);
}

// n / d for a launch constant d (vmx_device.h: FastDiv)
__device__ __forceinline__ uint32_t fast_div(uint32_t n, const FastDiv &f) {
    const uint32_t t = __umulhi(f.m, n);
    return (t + ((n - t) >> f.sh1)) >> f.sh2;
}
// local pixel index (rank-local packed rows) -> global pixel index
__device__ __forceinline__ uint32_t global_pixel(const FrameDev &fr, uint32_t lp) {
    if (fr.world <= 1) return lp;
    const uint32_t lrow = fast_div(lp, fr.div_width), x = lp - lrow * fr.width;
    const uint32_t ls = fast_div(lrow, fr.div_stripe), r = lrow - ls * fr.stripe_rows;
    const uint32_t grow = (ls * fr.world + fr.rank) * fr.stripe_rows + r;
    return grow * fr.width + x;
}

// ---- path state in per-pass arrays (split wavefront) ---------------------------------------
__device__ __forceinline__ void rng_store(const PathArrays &pa, uint32_t pid, const Rng &r) {
    ((float4 *)pa.state)[(size_t)pid * 4 + 2] = make_float4(__uint_as_float((uint32_t)r.s0), __uint_as_float((uint32_t)(r.s0 >> 32)),
                                           __uint_as_float((uint32_t)r.s1), __uint_as_float((uint32_t)(r.s1 >> 32)));
    ((float4 *)pa.state)[(size_t)pid * 4 + 3] = make_float4(__uint_as_float((uint32_t)r.s2), __uint_as_float((uint32_t)(r.s2 >> 32)),
                                           __uint_as_float((uint32_t)r.s3), __uint_as_float((uint32_t)(r.s3 >> 32)));
}
__device__ __forceinline__ void rng_load(const PathArrays &pa, uint32_t pid, Rng &r) {
    const float4 e = ((const float4 *)pa.state)[(size_t)pid * 4 + 2], f = ((const float4 *)pa.state)[(size_t)pid * 4 + 3];
    r.s0 = (uint64_t)__float_as_uint(e.x) | ((uint64_t)__float_as_uint(e.y) << 32);
    r.s1 = (uint64_t)__float_as_uint(e.z) | ((uint64_t)__float_as_uint(e.w) << 32);
    r.s2 = (uint64_t)__float_as_uint(f.x) | ((uint64_t)__float_as_uint(f.y) << 32);
    r.s3 = (uint64_t)__float_as_uint(f.z) | ((uint64_t)__float_as_uint(f.w) << 32);
}
// bits: step_bits of the step that will trace this ray (k_trace_w<1, .., SORT> reads them back); 0 = "shade it in full"
__device__ __forceinline__ void ray_store(const PathArrays &pa, uint32_t pid, const Path &P, uint32_t bits = 0) {
    ((float4 *)pa.state)[(size_t)pid * 4] = make_float4(P.ox, P.oy, P.oz, P.dx);
    ((float4 *)pa.state)[(size_t)pid * 4 + 1] = make_float4(P.dy, P.dz, __uint_as_float(P.depth), __uint_as_float(bits));
}
__device__ __forceinline__ void ray_load(const PathArrays &pa, uint32_t pid, Path &P) {
    const float4 a = ((const float4 *)pa.state)[(size_t)pid * 4], b = ((const float4 *)pa.state)[(size_t)pid * 4 + 1];
    P.ox = a.x, P.oy = a.y, P.oz = a.z, P.dx = a.w;
    P.dy = b.x, P.dz = b.y, P.depth = __float_as_uint(b.z);
}
// accumColour of a path in the split passes (PathArrays::rad / rad_mask).  The mask bit of a path says "rad[pid] holds a
// non-zero colour": a path that is black so far has neither a stored radiance nor a bit — k_resolve adds an exact +0 for
// it — and the first step that colours it stores the sum and sets the bit (rare: one atomic).  Without a mask (fused
// passes, vmx_radiance) every path's radiance is in rad.
__device__ __forceinline__ bool rad_has(const PathArrays &pa, uint32_t pid) {
    return !pa.rad_mask || ((pa.rad_mask[pid >> 6] >> (pid & 63u)) & 1ull) != 0;
}
__device__ __forceinline__ float4 rad_fetch(const PathArrays &pa, uint32_t pid, bool has) {
    return has ? ((const float4 *)pa.rad)[pid] : make_float4(0.f, 0.f, 0.f, -100.f);
}
__device__ __forceinline__ void rad_commit(const PathArrays &pa, uint32_t pid, float4 v, bool had) {
    if (had || v.x != 0.f || v.y != 0.f || v.z != 0.f) {  // (NaN != 0: a NaN colour is stored)
        ((float4 *)pa.rad)[pid] = v;
        if (!had) atomicOr(&pa.rad_mask[pid >> 6], 1ull << (pid & 63u));
    }
}
// RAD = false: accumColour is not fetched (k_shade<1> fetches and stores it only for the steps that change it)
template <bool TEX, bool RAD = true>
__device__ __forceinline__ void path_load_arrays(const PathArrays &pa, uint32_t pid, Path &P) {
    ray_load(pa, pid, P);
    rng_load(pa, pid, P.rng);
    if (RAD) {
        const float4 acc = rad_fetch(pa, pid, rad_has(pa, pid));
        P.ar = acc.x, P.ag = acc.y, P.ab = acc.z, P.aw = acc.w;
    } else {
        P.ar = P.ag = P.ab = P.aw = 0.f;
    }
    if (TEX) {
        const float4 th = ((const float4 *)pa.thr)[pid];
        P.tr = th.x, P.tg = th.y, P.tb = th.z, P.tw = th.w;
    }
    P.dest = pid;
}
// id compaction: wave ballot + prefix popcount, one atomic per wave
__device__ __forceinline__ void id_append(const IdQueue &q, uint32_t sub, bool alive, uint32_t pid) {
    const unsigned long long m = __ballot(alive);
    if (m == 0) return;
    const uint32_t lane = lane_index();
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&q.counts[sub * 32], (uint32_t)__popcll(m));
    base = __builtin_amdgcn_readfirstlane(base);
    const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    // (the sub-lists are sized so that this cannot fail — ensure_paths — but an append never writes past its list: the
    // tail counter then stays above sub_capacity, which the host reads as an error, run_ids / finish_stats)
    if (alive && base + rank < q.sub_capacity) q.ids[(size_t)sub * q.sub_capacity + base + rank] = pid;
}

// Path id of sample plane j of active-pixel slot s.  pixel_major: the samples of one pixel are
// contiguous (pid = s * samples + j), so the 64 camera rays of a wave differ only by sub-pixel
// jitter and walk the BVH together; else plane-major (pid = j * n_pad + s, first-generation kernels).
__device__ __forceinline__ uint32_t path_id(const WorkDev &wk, uint32_t j, uint32_t s_idx) {
    return wk.pixel_major ? s_idx * wk.samples + j : j * wk.n_pad + s_idx;
}

// band-local work item of the primary source -> path id, global pixel, sample index
// Sample index of the j-th path a pixel gets in this pass.  Bit 31 of the cursor marks a pixel whose
// last stratum ended on the early-stop rule (pathtracer.cpp:290-311): it will most likely end the
// following strata on their first sample too, so its paths of a pass are the first samples of the
// next strata (k = cursor + j * quarter) instead of consecutive samples; k_resolve takes them in
// order and drops what the rule would not have reached.
constexpr uint32_t kCursorStrided = 0x80000000u;
__device__ __forceinline__ uint32_t sample_index(const FrameDev &fr, const PixelStateDev &px, uint32_t lp,
                                                 uint32_t j) {
    // first pass of an early-stop frame: the samples before the rule can fire (j < lead), and already
    // the first samples of the following strata, for the many pixels that stop on the first test
    if (fr.lead != 0 && j >= fr.lead) return (j - fr.lead + 1u) * fr.quarter;
    const uint32_t c = px.cursor[lp];
    return (c & ~kCursorStrided) + j * ((c & kCursorStrided) ? fr.quarter : 1u);
}

__device__ __forceinline__ bool primary_item(const FrameDev &fr, const WorkDev &wk, const PixelStateDev &px,
                                             uint32_t j, uint32_t s_idx, uint32_t &pid, uint32_t &pixel,
                                             uint32_t &k) {
    if (s_idx >= wk.n_active) return false;
    const uint32_t lp = wk.active[s_idx];
    k = sample_index(fr, px, lp, j);
    if (k >= fr.kmax) return false;
    pixel = global_pixel(fr, lp);
    pid = path_id(wk, j, s_idx);
    return true;
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
template <bool COUNT>
__global__ void k_trace(SceneDev sc, const float *__restrict__ o, const float *__restrict__ d, uint32_t n,
                        int32_t *__restrict__ tri_id, float *__restrict__ t, DevCounters *ctr) {
    extern __shared__ uint2 lds_stack[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint2 *stk = lds_stack + (size_t)wave * sc.stack_entries * 64 + lane;
    const float4 *__restrict__ tris = (const float4 *)sc.tris;
    Cnt cnt = {0, 0}, none = {0, 0};
    Tally tl = {{0, 0}, {0, 0}, {0, 0}};
    for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
        const uint32_t i = base + threadIdx.x;
        if (i < n) {
            float best;
            int slot;
            bvh_nearest<COUNT>(sc, o[i * 3], o[i * 3 + 1], o[i * 3 + 2], d[i * 3], d[i * 3 + 1], d[i * 3 + 2], stk,
                               best, slot, cnt);
            tri_id[i] = slot >= 0 ? (int32_t)__float_as_uint(tris[slot * 3 + 2].y) : -1;
            t[i] = best;
        }
    }
    if (COUNT && ctr) tally_flush<true>(ctr, tl, cnt, none);
}

__global__ void k_raycast(SceneDev sc, const float *__restrict__ o, const float *__restrict__ d, uint32_t n,
                          float4 *__restrict__ out) {
    extern __shared__ uint2 lds_stack[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint2 *stk = lds_stack + (size_t)wave * sc.stack_entries * 64 + lane;
    const float4 *__restrict__ tris = (const float4 *)sc.tris;
    Cnt cnt = {0, 0};
    for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
        const uint32_t i = base + threadIdx.x;
        if (i >= n) continue;
        const float ox = o[i * 3], oy = o[i * 3 + 1], oz = o[i * 3 + 2];
        const float dx = d[i * 3], dy = d[i * 3 + 1], dz = d[i * 3 + 2];
        CastResult c;
        ray_cast<false>(sc, ox, oy, oz, dx, dy, dz, stk, c, cnt);
        const int32_t id = c.slot >= 0 ? (int32_t)__float_as_uint(tris[c.slot * 3 + 2].y) : -1;
        const uint32_t flags = ((c.nearest < kInf) ? 1u : 0u) | (c.material ? 2u : 0u);
        // vmx_rayhit: location[3], distance | normal[3], tri_id | uv[2], tri_t, flags | colour[3], pad
        out[(size_t)i * 4] = make_float4(ox + (dx * c.nearest), oy + (dy * c.nearest), oz + (dz * c.nearest), c.nearest);
        out[(size_t)i * 4 + 1] = make_float4(c.nx, c.ny, c.nz, __int_as_float(id));
        out[(size_t)i * 4 + 2] = make_float4(c.uvx, c.uvy, c.tri_t, __uint_as_float(flags));
        out[(size_t)i * 4 + 3] = make_float4(c.cr, c.cg, c.cb, 0.f);
    }
}

__global__ void k_primary_ids(SceneDev sc, FrameDev fr, uint32_t k, int32_t *__restrict__ tri_id,
                              float *__restrict__ t) {
    extern __shared__ uint2 lds_stack[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint2 *stk = lds_stack + (size_t)wave * sc.stack_entries * 64 + lane;
    const float4 *__restrict__ tris = (const float4 *)sc.tris;
    const uint32_t npix = fr.width * fr.height;
    Cnt cnt = {0, 0};
    for (uint32_t base = blockIdx.x * blockDim.x; base < npix; base += gridDim.x * blockDim.x) {
        const uint32_t p = base + threadIdx.x;
        if (p >= npix) continue;
        Rng rng;
        float dx, dy, dz;
        primary_ray(fr, p, k, rng, dx, dy, dz);
        float best;
        int slot;
        bvh_nearest<false>(sc, fr.px, fr.py, fr.pz, dx, dy, dz, stk, best, slot, cnt);
        tri_id[p] = slot >= 0 ? (int32_t)__float_as_uint(tris[slot * 3 + 2].y) : -1;
        t[p] = best;
    }
}

// parity hook: cosf / sinf as the shading kernels evaluate them under the default reading
__global__ void k_trig(const float *__restrict__ x, uint32_t n, float *__restrict__ cs, float *__restrict__ sn) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        cs[i] = libm_sincosf(x[i], 1);
        sn[i] = libm_sincosf(x[i], 0);
    }
}

__global__ void k_init_pixels(PixelStateDev px, uint32_t npix) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    ((float4 *)px.accum)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    px.count[i] = 0;
    px.cursor[i] = 0;
}

__global__ void k_zero_u32(unsigned int *p, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}

// ---------------------------------------------------------------------------
// quad-cooperative record fetch (k_trace_w<1>, k_paths).  A 64-byte record read by ONE lane as four 16-byte
// loads costs four tag lookups in the vector L1; read by the four lanes of a quad — lane j takes
// bytes [16 j, 16 j + 16) — it costs one.  Load i of a step brings the record of quad-lane i, so
// afterwards lane j holds piece j of the four records of its quad; a 4x4 transpose inside every
// quad (two butterfly stages, one v_cndmask_b32_dpp per dword and stage: D = vcc ? src1 : dpp(src0))
// hands every lane the four pieces of its own record.  tools/ta_probe.hip measures both forms.
// ---------------------------------------------------------------------------
#define VMX_XCHG_PAIR(NAME, PERM)                                                                                     \
    __device__ __forceinline__ void NAME(const float4 &p, const float4 &q, float4 &po, float4 &qo,                    \
                                         unsigned long long keep_p, unsigned long long keep_q) {                     \
        asm volatile("s_nop 1\n\t"                                                                                   \
                     "s_mov_b64 vcc, %16\n\t"                                                                        \
                     "v_cndmask_b32_dpp %0, %12, %8, vcc quad_perm:" PERM " row_mask:0xf bank_mask:0xf\n\t"          \
                     "v_cndmask_b32_dpp %1, %13, %9, vcc quad_perm:" PERM " row_mask:0xf bank_mask:0xf\n\t"          \
                     "v_cndmask_b32_dpp %2, %14, %10, vcc quad_perm:" PERM " row_mask:0xf bank_mask:0xf\n\t"         \
                     "v_cndmask_b32_dpp %3, %15, %11, vcc quad_perm:" PERM " row_mask:0xf bank_mask:0xf\n\t"         \
                     "s_mov_b64 vcc, %17\n\t"                                                                        \
                     "v_cndmask_b32_dpp %4, %8, %12, vcc quad_perm:" PERM " row_mask:0xf bank_mask:0xf\n\t"          \
                     "v_cndmask_b32_dpp %5, %9, %13, vcc quad_perm:" PERM " row_mask:0xf bank_mask:0xf\n\t"          \
                     "v_cndmask_b32_dpp %6, %10, %14, vcc quad_perm:" PERM " row_mask:0xf bank_mask:0xf\n\t"         \
                     "v_cndmask_b32_dpp %7, %11, %15, vcc quad_perm:" PERM " row_mask:0xf bank_mask:0xf"             \
                     : "=&v"(po.x), "=&v"(po.y), "=&v"(po.z), "=&v"(po.w), "=&v"(qo.x), "=&v"(qo.y), "=&v"(qo.z),    \
                       "=&v"(qo.w)                                                                                   \
                     : "v"(p.x), "v"(p.y), "v"(p.z), "v"(p.w), "v"(q.x), "v"(q.y), "v"(q.z), "v"(q.w), "s"(keep_p),  \
                       "s"(keep_q)                                                                                   \
                     : "vcc");                                                                                       \
    }
VMX_XCHG_PAIR(xchg_pair_1, "[1,0,3,2]")
VMX_XCHG_PAIR(xchg_pair_2, "[2,3,0,1]")
#undef VMX_XCHG_PAIR

// Fetches the 64 bytes at base + off (off: 32-bit byte offset of the lane's node or triangle record, 16-byte
// aligned) into q0..q3 of every lane.  A lane that is not traversing passes off = 0 (the first record: always
// there, and hot): loading for it unconditionally is cheaper than masking the four loads.  Must be called with
// all 64 lanes active.
__device__ __forceinline__ void quad_fetch_record(const char *base, uint32_t off, uint32_t lane, float4 &q0, float4 &q1,
                                                  float4 &q2, float4 &q3) {
    const uint32_t piece = (lane & 3u) << 4;
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_mov_dpp((int)off, 0x00, 0xF, 0xF, true);  // quad_perm [0,0,0,0]
    const uint32_t r1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)off, 0x55, 0xF, 0xF, true);  // [1,1,1,1]
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_mov_dpp((int)off, 0xAA, 0xF, 0xF, true);  // [2,2,2,2]
    const uint32_t r3 = (uint32_t)__builtin_amdgcn_mov_dpp((int)off, 0xFF, 0xF, 0xF, true);  // [3,3,3,3]
    // (one 32-bit offset per load: scalar base + vector offset addressing, no 64-bit address arithmetic)
    const float4 x0 = *(const float4 *)(base + (uint32_t)(r0 + piece));
    const float4 x1 = *(const float4 *)(base + (uint32_t)(r1 + piece));
    const float4 x2 = *(const float4 *)(base + (uint32_t)(r2 + piece));
    const float4 x3 = *(const float4 *)(base + (uint32_t)(r3 + piece));
    float4 a0, a1, a2, a3;
    xchg_pair_1(x0, x1, a0, a1, 0x5555555555555555ull, 0xAAAAAAAAAAAAAAAAull);  // lanes ^1: even lanes keep (x0, x2)
    xchg_pair_1(x2, x3, a2, a3, 0x5555555555555555ull, 0xAAAAAAAAAAAAAAAAull);
    xchg_pair_2(a0, a2, q0, q2, 0x3333333333333333ull, 0xCCCCCCCCCCCCCCCCull);  // lanes ^2: lanes 0,1 of a quad keep (a0, a1)
    xchg_pair_2(a1, a3, q1, q3, 0x3333333333333333ull, 0xCCCCCCCCCCCCCCCCull);
}


// ---------------------------------------------------------------------------
// k_paths — persistent waves with per-lane refill.
//
// Every lane runs the state machine  fetch -> traverse (one BVH node per loop
// iteration) -> shade -> {write radiance | continue (LOOP) | append to the
// next queue}.  A lane that finishes does not idle until its wave is done: as
// soon as `refill_min` lanes are idle the wave takes that many new items from
// its work source (a wave-private reservation of 256 items, one atomic per
// reservation), and as soon as `shade_min` lanes have finished traversal they
// are shaded together.  Results do not depend on this scheduling: each path
// carries its own RNG stream and radiance slot.
//   SRC 0: work = (sample j, slot) pairs of the active-pixel list, in 8 bands
//          of neighbouring tiles (band = block % 8 = XCD label; exhausted
//          bands are stolen from), paths start with ray generation
//   SRC 2: work = the 16 sub-queues of live path ids (the tail of a pass)
// ---------------------------------------------------------------------------
// LDS holds levels [0, lds_entries) plus one scratch entry at index lds_entries; deeper levels
// (rare) go to the per-wave global slab.  The LDS access is unconditional on a clamped index so
// that it stays a ds_*_b64 (a select between the two address spaces turns into flat accesses).
__device__ __forceinline__ void stack_push(uint2 *stk, uint2 *ovf, int lds_entries, int sp, uint2 e) {
    stk[min(sp, lds_entries) * 64] = e;
    if (sp >= lds_entries) ovf[(sp - lds_entries) * 64] = e;
}
__device__ __forceinline__ uint2 stack_pop(const uint2 *stk, const uint2 *ovf, int lds_entries, int sp) {
    uint2 e = stk[min(sp, lds_entries) * 64];
    // the empty asm pins the LDS read as its own ds_read_b64: without it the two loads are merged
    // into one flat load through a pointer select, which puts every pop on the vector-memory pipe
    asm volatile("" : "+v"(e.x), "+v"(e.y));
    if (sp >= lds_entries) e = ovf[(sp - lds_entries) * 64];
    return e;
}

#ifndef VMX_PATHS_WPS
#define VMX_PATHS_WPS 6  // waves per SIMD the fused kernel is compiled for (80 VGPRs): tail 8.8 -> 7.9 ms, early-stop frame 14.3 -> 13.8 ms (5: 8.1, 7: 8.4, 8: 8.9)
#endif
// GUIDE (COUNT false; a reference-tree scene with a valid guide, guide_walk.h): a ray of any depth that passes gw_ray_ok
// walks the GUIDE's records, which lie in the scene's own record allocation gd.off bytes behind sc.inner, so a lane's
// tree is one 32-bit offset (`toff`) folded into its record offset and guide lanes and reference lanes share a wave.  The
// step is the GUIDE step of k_trace_w<1>: the prune on near > cut = best (1 + kGwKappa) in the child choice and in the
// pop, `second` kept; a reference lane keeps cut == best, so the step has no branch on the tree.  A finished guide walk
// waits for shading like any finished ray; there, before the wave shades, the rule (gw_settle, one 48-byte fetch of the
// winner's guide record) runs for the wave's finished guide lanes together: a settled lane takes the winner's REFERENCE
// slot and is shaded, the others start the same ray again over the reference tree, in the lane, and are shaded when
// that walk ends.  A ray that fails gw_ray_ok starts on the reference tree, so the NaN-exact box form meets guide records
// only in finite lanes of a mixed wave, where both box forms agree (guide_walk.h).
// (the form's one extra kernel argument, a GuidePathsDev, is the pack G: the other instantiations keep their signature)
__device__ __forceinline__ GuidePathsDev guide_arg() { return GuidePathsDev{}; }
__device__ __forceinline__ GuidePathsDev guide_arg(GuidePathsDev g) { return g; }
template <bool COUNT, int SRC, bool TEX, class... G>
__global__ void __launch_bounds__(256, VMX_PATHS_WPS)
k_paths(SceneDev sc, FrameDev fr, WorkDev wk, PixelStateDev px, float4 *__restrict__ rad, PathArrays pa,
        DevCounters *ctr, G... guide) {
    constexpr bool GUIDE = sizeof...(G) != 0;
    static_assert(!GUIDE || !COUNT, "the counting build's visits are the reference tree's");
    const GuidePathsDev gd = guide_arg(guide...);
    extern __shared__ uint2 lds_stack[];
    __shared__ float4 s_geom[kLdsSpheres];  // spheres' (centre, rad*rad): read by every RayCast
    if (threadIdx.x < min(sc.nspheres, kLdsSpheres)) {
        const SphereDev &q = sc.spheres[threadIdx.x];
        s_geom[threadIdx.x] = make_float4(q.cx, q.cy, q.cz, q.rad2);
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // the first lds_entries stack levels live in LDS, deeper ones (rare) in a per-wave global slab
    const int lds_entries = (int)wk.lds_entries;
    uint2 *stk = lds_stack + (size_t)wave * (lds_entries + 1) * 64 + lane;
    uint2 *ovf = (uint2 *)wk.overflow_stack +
                 ((size_t)(blockIdx.x * (blockDim.x >> 6) + wave) * wk.overflow_entries) * 64 + lane;
    const float4 *__restrict__ inner = (const float4 *)sc.inner;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const uint32_t kReserve = wk.reserve;

    // wave-uniform scheduling state
    uint32_t src = blockIdx.x % wk.nsrc, res_lo = 0, res_hi = 0, tried = 0;
    bool exhausted = false;
    // lane state
    // traversal state as in k_trace_w: `cur` = node reference, kIdle while the lane is not traversing
    // (no path, or traversal finished and the path waits for shading); stack level 0 = bottom entry
    bool has = false, exact = false, is_ray = false;
    Path P;
    float ix = 0.f, iy = 0.f, iz = 0.f, best = 0.f;
    int slot = -1, sp = 0;
    uint32_t cur = kIdle;
    stk[0] = make_uint2(kBottom, 0xFF800000u);
    Cnt c0 = {0, 0}, c1 = {0, 0};
    Tally tl = {{0, 0}, {0, 0}, {0, 0}};
    // GUIDE: the prune bound, the smallest accepted distance of any triangle but the nearest (guide_walk.h) and the byte
    // offset of the lane's tree from sc.inner (0: the reference tree; gd.off: the guide, and `slot` is a guide slot)
    float cut = 0.f, second = 0.f;
    uint32_t toff = 0;
    uint32_t n_settled = 0, n_fallback = 0;  // (wave-uniform)

    // returns false for a ray that may not walk the guide (GUIDE only): it starts on the reference tree
    auto start_traversal = [&]() -> bool {
        ray_start(P.dx, P.dy, P.dz, sc.root_ref, 999999999.f, ix, iy, iz, best, slot, sp, cur);
        exact = !(finite3(ix, iy, iz) && finite3(P.ox, P.oy, P.oz));
        is_ray = (P.depth == 0) || finite3(P.dx, P.dy, P.dz);
        if (GUIDE) {
            const bool walks = gw_ray_ok(P.ox, P.oy, P.oz, P.dx, P.dy, P.dz, ix, iy, iz, gd.scene_max);
            cur = walks ? gd.root_ref : cur;
            toff = walks ? gd.off : 0u;
            cut = walks ? best * kGwCut : best;
            second = 3.0e38f;
            return walks;
        }
        return true;
    };

    for (;;) {
        // ---- 1. shade the lanes whose traversal is finished ---------------------
        {
            const unsigned long long fin = __builtin_amdgcn_ballot_w64(has && cur == kIdle);
            const unsigned long long trav = __builtin_amdgcn_ballot_w64(cur != kIdle);
            if (fin != 0 && ((uint32_t)__popcll(fin) >= wk.shade_min || trav == 0)) {
                if (GUIDE) {
                    // the rule for the finished guide walks among them: settled -> the reference slot, shaded below;
                    // not settled -> the same ray over the reference tree, with the reference's own prune (cut == best)
                    const bool walked = has && cur == kIdle && toff != 0;
                    bool fb = false;
                    if (walked) {
                        const bool have = slot >= 0;
                        float r[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                        int ref_slot = -1;
                        if (have) {
                            const float4 *rec = (const float4 *)((const char *)inner + (gd.tri_off + (uint32_t)slot * 48u));
                            const float4 a = rec[0], b = rec[1], c = rec[2];
                            r[0] = a.x, r[1] = a.y, r[2] = a.z, r[3] = a.w, r[4] = b.x, r[5] = b.y, r[6] = b.z, r[7] = b.w, r[8] = c.x;
                            ref_slot = __float_as_int(c.z);  // TriRecord::pad[0]: the triangle's leaf slot in the reference tree
                        }
                        const float o[3] = {P.ox, P.oy, P.oz}, d[3] = {P.dx, P.dy, P.dz}, inv[3] = {ix, iy, iz};
                        toff = 0;
                        if (gw_settle(have, r, best, second, o, d, inv, gd.scene_max)) {
                            slot = ref_slot;
                        } else {
                            fb = true;
                            best = cut = 999999999.f, slot = -1, sp = 1, cur = sc.root_ref;
                        }
                    }
                    n_settled += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(walked && !fb));
                    n_fallback += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(fb));
                }
                const bool shaded = has && cur == kIdle;
                bool alive = false;
                StepFlags fl = {false, false, false};
                uint32_t depth0 = 0;
                if (shaded) {
                    depth0 = P.depth == 0 ? 1u : 0u;
                    CastResult c;
                    cast_finish<true, false>(sc, P.ox, P.oy, P.oz, P.dx, P.dy, P.dz, best, slot, c, s_geom);
                    fl.was_ray = is_ray;
                    alive = path_shade<TEX, true>(sc, SampCfg{fr.r2scale, fr.libm_double, fr.elide_dead}, P, c, fl, s_geom);
                    if (!alive) {
                        // (tail of a split pass: the path's bit says whether it had a stored colour; fused passes: no mask)
                        if (SRC == 2) rad_commit(pa, P.dest, make_float4(P.ar, P.ag, P.ab, P.aw), rad_has(pa, P.dest));
                        else rad[P.dest] = make_float4(P.ar, P.ag, P.ab, P.aw);
                        has = false;
                    }
                }
                tally_add(tl, fl, shaded, depth0);
                bool unwalked = false;  // GUIDE: the lane's next ray never walks the guide (counted with the fallback rays)
                if (shaded && alive) unwalked = !start_traversal();  // the lane keeps its path to the end
                if (GUIDE) n_fallback += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(unwalked));
            }
        }
        // ---- 2. refill idle lanes from the work source ---------------------------
        {
            const unsigned long long idle = __builtin_amdgcn_ballot_w64(!has);
            if (idle != 0 && !exhausted && ((uint32_t)__popcll(idle) >= wk.refill_min || idle == ~0ull)) {
                for (;;) {
                    if (res_lo == res_hi) {
                        const uint32_t lim = SRC == 0 ? wk.band_items : min(wk.qids.counts[src * 32], wk.qids.sub_capacity);
                        uint32_t base = 0;
                        if (lane == 0) base = atomicAdd(&wk.heads[src * 32], kReserve);
                        base = __builtin_amdgcn_readfirstlane(base);
                        if (base >= lim) {
                            src = (src + 1 == wk.nsrc) ? 0 : src + 1;
                            if (++tried == wk.nsrc) {
                                exhausted = true;
                                break;
                            }
                            continue;
                        }
                        tried = 0;
                        res_lo = base;
                        res_hi = min(base + kReserve, lim);
                    }
                    const unsigned long long want = __builtin_amdgcn_ballot_w64(!has);
                    if (want == 0) break;
                    const uint32_t avail = res_hi - res_lo;
                    const uint32_t rank = (uint32_t)__popcll(want & lt_mask);
                    const bool take = !has && rank < avail;
                    const uint32_t item = res_lo + rank;
                    res_lo += min((uint32_t)__popcll(want), avail);
                    bool unwalked = false;  // (GUIDE, as above)
                    if (take) {
                        bool valid = true;
                        if (SRC == 0) {
                            uint32_t j, s_idx;
                            if (wk.pixel_major) {
                                const uint32_t sl = fast_div(item, wk.div_samples);
                                j = item - sl * wk.samples, s_idx = src * wk.band_slots + sl;
                            } else {
                                j = item / wk.band_slots, s_idx = src * wk.band_slots + (item - j * wk.band_slots);
                            }
                            valid = s_idx < wk.n_active;
                            if (valid) {
                                const uint32_t lp = wk.active[s_idx];
                                const uint32_t k = sample_index(fr, px, lp, j);
                                valid = k < fr.kmax;
                                if (valid) {
                                    primary_ray(fr, global_pixel(fr, lp), k, P.rng, P.dx, P.dy, P.dz);
                                    P.ox = fr.px, P.oy = fr.py, P.oz = fr.pz;
                                                        P.ar = P.ag = P.ab = 0.f;
                                    P.aw = -100.f;  // pathtracer.cpp:29
                                    P.tr = P.tg = P.tb = P.tw = 1.f;  // :30
                                    P.depth = 0;
                                    P.dest = path_id(wk, j, s_idx);
                                    if (fr.elide_dead && step_is_dead<false>(sc, fr.r2scale, P.rng, 0, P.ox, P.oy, P.oz, P.dx, P.dy, P.dz, 1.f, 1.f, 1.f)) {
                                        rad[P.dest] = make_float4(0.f, 0.f, 0.f, -100.f);  // untraced: its radiance is zero
                                        valid = false;
                                    }
                                }
                            }
                        } else {
                            path_load_arrays<TEX>(pa, wk.qids.ids[(size_t)src * wk.qids.sub_capacity + item], P);
                        }
                        if (valid) {
                            has = true;
                            unwalked = !start_traversal();
                        }
                    }
                    if (GUIDE) n_fallback += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(unwalked));
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(has) == 0) break;
        // ---- 3. 8 traversal steps (bvh.cpp:61-134), the step of k_trace_w (see there) with counters:
        //         every traversing lane does its triangle step or its inner-node step
        auto push = [&](uint2 e) {
            stack_push(stk, ovf, lds_entries, sp, e);
            ++sp;
        };
        auto step = [&](auto exact_tag) {
            constexpr bool EXACT = decltype(exact_tag)::value;
            // the node or triangle record of every traversing lane, fetched quad-cooperatively in one phase
            // (quad_fetch_record; inner and triangle records share one allocation, SceneDev::tri_off)
            float4 q0, q1, q2, q3;
            // (GUIDE: a guide lane's records lie toff bytes on, its triangle records at gd.tri_off)
            quad_fetch_record((const char *)inner,
                              cur >= kPop && (int)cur >= 0 ? 0u
                              : ((int)cur < 0 ? (GUIDE && toff != 0 ? gd.tri_off : sc.tri_off) + (cur & kLeafStartMask) * 48u
                                              : (GUIDE ? toff + (cur << 6) : (cur << 6))),
                              lane, q0, q1, q2, q3);
            if (cur < kPop) {
                if (COUNT) {
                    if (P.depth == 0) c0.inner++;
                    else c1.inner++;
                }
                float tn0, tf0, tn1, tf1;
                child_boxes<EXACT>(q0, q1, q2, P.ox, P.oy, P.oz, ix, iy, iz, tn0, tf0, tn1, tf1);
                if (GUIDE)  // (a reference lane's record has zero marks: it never skips)
                    cur = choose_child_masks_cull(tn0, tf0, tn1, tf1, __float_as_uint(q3.x), __float_as_uint(q3.y),
                                                  __float_as_uint(q3.z), __float_as_uint(q3.w), cut, push);
                else cur = choose_child_masks(tn0, tf0, tn1, tf1, __float_as_uint(q3.x), __float_as_uint(q3.y), best, push);
            } else if ((int)cur < 0) {
                // one triangle (triangle.cpp:4-54); the leaf ref itself carries the progress
                if (COUNT) {
                    if (P.depth == 0) c0.tris++;
                    else c1.tris++;
                }
                float dist;
                const bool hit = tri_test(q0, q1, q2.x, P.ox, P.oy, P.oz, P.dx, P.dy, P.dz, dist);
                if (hit && dist < best) {  // strict <: first tested wins ties (bvh.cpp:90)
                    if (GUIDE) second = best, cut = toff != 0 ? dist * kGwCut : dist;
                    best = dist;
                    slot = (int)(cur & kLeafStartMask);
                } else if (GUIDE && hit) {
                    second = fminf(second, dist);
                }
                cur = leaf_advance(cur);
            }
            if (cur == kPop) {
                // the bottom entry ends the traversal: the lane then waits for shading
                const uint32_t ref = pop_to_next(stk, ovf, lds_entries, sp, GUIDE ? cut : best);
                cur = ref == kBottom ? kIdle : ref;
            }
        };
        if (__builtin_amdgcn_ballot_w64(exact && cur != kIdle) != 0) {
#pragma unroll 1
            for (int act = 0; act < 8; ++act) step(std::true_type{});
        } else {
#pragma unroll 1
            for (int act = 0; act < 8; ++act) step(std::false_type{});
        }
    }
    tally_flush<COUNT>(ctr, tl, c0, c1);
    if (GUIDE && lane == 0) {
        if (n_settled) atomicAdd(&gd.ctr[0], (unsigned long long)n_settled);
        if (n_fallback) atomicAdd(&gd.ctr[1], (unsigned long long)n_fallback);
    }
}





// ---------------------------------------------------------------------------
// k_camera_tables — every camera ray of a frame starts at the same origin, so
// the origin-dependent half of both intersection tests is the same for all of
// them.  Per frame this kernel writes copies of the node and triangle records
// with that half applied:
//   nodes : (lo - o), (hi - o) of both children     -> the slab test is 6 multiplies per box
//   tris  : e1, e2, tvec = o - v0, qvec = cross(tvec, e1), C = dot(e2, qvec)
// Each value is produced by the same float operation on the same inputs as the
// per-ray code (bbox.cpp:72-73, triangle.cpp:30,36,42), so results stay bit-identical.
// ---------------------------------------------------------------------------
__global__ void k_camera_tables(SceneDev sc, uint32_t n_inner, float ox, float oy, float oz,
                                float4 *__restrict__ cam_inner, float4 *__restrict__ cam_tris) {
    const float4 *__restrict__ inner = (const float4 *)sc.inner;
    const float4 *__restrict__ tris = (const float4 *)sc.tris;
    const uint32_t total = n_inner + sc.ntris;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        if (i < n_inner) {
            const float4 q0 = inner[i * 4], q1 = inner[i * 4 + 1], q2 = inner[i * 4 + 2], q3 = inner[i * 4 + 3];
            // (lo - o), (hi - o) of both children, then one copy per direction octant (bit a: 1/d_a < 0)
            // with each axis' near plane first: for a finite non-NaN reciprocal, min(lo*inv, hi*inv) is
            // the product with lo when inv >= 0 and with hi otherwise (rounding is monotonic), so a wave
            // whose rays share the octant needs 6 multiplies and one max3/min3 per box, no min/max pairs.
            // Octant 0 is the plain (lo, hi) layout that the per-lane path reads.
            const float l0x = q0.x - ox, l0y = q0.y - oy, l0z = q0.z - oz, h0x = q0.w - ox, h0y = q1.x - oy, h0z = q1.y - oz;
            const float l1x = q1.z - ox, l1y = q1.w - oy, l1z = q2.x - oz, h1x = q2.y - ox, h1y = q2.z - oy, h1z = q2.w - oz;
            for (uint32_t o = 0; o < 8; ++o) {
                const bool sx = o & 1u, sy = o & 2u, sz = o & 4u;
                float4 *rec = cam_inner + ((size_t)o * n_inner + i) * 4;
                rec[0] = make_float4(sx ? h0x : l0x, sy ? h0y : l0y, sz ? h0z : l0z, sx ? l0x : h0x);
                rec[1] = make_float4(sy ? l0y : h0y, sz ? l0z : h0z, sx ? h1x : l1x, sy ? h1y : l1y);
                rec[2] = make_float4(sz ? h1z : l1z, sx ? l1x : h1x, sy ? l1y : h1y, sz ? l1z : h1z);
                rec[3] = q3;
            }
        } else {
            const uint32_t t = i - n_inner;
            const float4 a = tris[t * 3], b = tris[t * 3 + 1], c = tris[t * 3 + 2];
            const float e1x = a.w, e1y = b.x, e1z = b.y, e2x = b.z, e2y = b.w, e2z = c.x;
            const float tx = ox - a.x, ty = oy - a.y, tz = oz - a.z;
            float qx, qy, qz;
            cross3(tx, ty, tz, e1x, e1y, e1z, qx, qy, qz);
            const float cdot = dot3(e2x, e2y, e2z, qx, qy, qz);
            cam_tris[t * 4] = make_float4(e1x, e1y, e1z, e2x);
            cam_tris[t * 4 + 1] = make_float4(e2y, e2z, tx, ty);
            cam_tris[t * 4 + 2] = make_float4(tz, qx, qy, qz);
            cam_tris[t * 4 + 3] = make_float4(cdot, c.y, 0.f, 0.f);
        }
    }
}

// ---------------------------------------------------------------------------
// k_pixel_claims — the per-pixel claim of pixel_claim.h for every local pixel of a frame, from the camera tables of
// its origin: one lane per pixel, a wave per 8 x 8 tile (neighbouring pixels walk the same nodes), the stack in LDS
// levels plus the global slab as in k_bruteforce.  The walk itself is the header's, shared with the host program of
// tests/cpp/pixel_claim_test.cpp: same arithmetic, same table.
// lists (or NULL): the second plane.  This kernel settles the record of every pixel that gets the empty one — a pixel with
// a claim, or one whose claim walk left no candidate to start a list from — and parks (cand, other) of the others in
// their records; per tile it leaves one word with the bits of those pixels and its popcount (pend_mask, pend_cnt:
// indexed by tile, every tile written).  launch_live_compact lists them in tile order (entry = tile * 64 + lane) and
// k_pixel_lists walks for them in full waves: the list walks run for a third of the pixels, scattered over most tiles.
// ---------------------------------------------------------------------------
struct ClaimStack {
    uint2 *stk, *ovf;
    int lds_entries;
    __device__ __forceinline__ void put(int i, uint32_t ref, float near) { stack_push(stk, ovf, lds_entries, i, make_uint2(ref, __float_as_uint(near))); }
    __device__ __forceinline__ void get(int i, uint32_t &ref, float &near) const {
        const uint2 e = stack_pop(stk, ovf, lds_entries, i);
        ref = e.x, near = __uint_as_float(e.y);
    }
};
__global__ void __launch_bounds__(256, 7)
k_pixel_claims(SceneDev sc, FrameDev fr, const float *__restrict__ cam_inner, const float *__restrict__ cam_tris,
               unsigned int *__restrict__ claims, unsigned int *__restrict__ lists, unsigned int *n_claimed,
               unsigned long long *__restrict__ pend_mask, unsigned int *__restrict__ pend_cnt, uint32_t lds_levels,
               uint32_t overflow_entries, void *overflow_stack) {
    extern __shared__ uint2 lds_stack[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    ClaimStack stk;
    stk.stk = lds_stack + (size_t)wave * (lds_levels + 1) * 64 + lane;
    stk.ovf = (uint2 *)overflow_stack + ((size_t)(blockIdx.x * (blockDim.x >> 6) + wave) * overflow_entries) * 64 + lane;
    stk.lds_entries = (int)lds_levels;
    PcFilm fm;
    for (int i = 0; i < 9; ++i) fm.m[i] = fr.m[i];
    fm.width = fr.width, fm.height = fr.height, fm.sensor_x = fr.sensor_x, fm.sensor_y = fr.sensor_y, fm.film_dist = fr.film_dist;
    const uint32_t tiles_x = (fr.width + 7u) / 8u, tiles = tiles_x * ((fr.local_rows + 7u) / 8u);
    uint32_t n = 0;
    // a resident grid whose waves take the next tile when they are free (n_claimed[1]: the work head, zeroed with the
    // count).  With equal shares of the tiles and more waves than are resident, the waves of this launch lived 0.57 ms
    // of its 1.45 ms (profiles/claim_walks.txt)
    for (;;) {
        uint32_t tile = 0;
        if (lane == 0) tile = atomicAdd(n_claimed + 1, 1u);
        tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile);
        if (tile >= tiles) break;
        const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const uint32_t x = tx * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);
        bool walks = false, claimed = false;  // walks: this pixel's list is k_pixel_lists' to make
        if (x < fr.width && y < fr.local_rows) {
            const uint32_t lp = y * fr.width + x;
            int cand, other;
            const uint32_t c = pc_pixel_claim_cand(fm, global_pixel(fr, lp), cam_inner, cam_tris, sc.root_ref, stk,
                                                   (int)(lds_levels + overflow_entries), cand, other);
            if (lists) {
                // (pc_pixel_list returns the empty record for a pixel with a claim and for cand < -1 before it looks at anything else)
                walks = c == kClaimNone && cand >= -1;
                ((uint4 *)lists)[lp] = walks ? make_uint4((uint32_t)cand, (uint32_t)other, kClaimNone, kClaimNone)
                                             : make_uint4(kClaimNone, kClaimNone, kClaimNone, kClaimNone);
            }
            claims[lp] = c;
            claimed = c != kClaimNone;
        }
        n += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(claimed));  // (wave-uniform: every lane of the wave is here)
        if (lists) {
            const unsigned long long bits = __builtin_amdgcn_ballot_w64(walks);
            if (lane == 0) pend_mask[tile] = bits, pend_cnt[tile] = (uint32_t)__popcll(bits);
        }
    }
    if (lane == 0 && n) atomicAdd(n_claimed, n);
}

// k_pixel_lists — pc_pixel_list for the entries k_pixel_claims left, one lane per entry: persistent waves take 64
// consecutive entries of the tile-ordered list at a time (*head, zeroed by the host; *count is the list's length, known
// on the device only), so the lanes of a wave are neighbouring edge pixels.  A pixel's record depends on the pixel and
// on the (cand, other) parked in it alone, not on the lane or wave that walks for it.
__global__ void __launch_bounds__(256, 5)
k_pixel_lists(SceneDev sc, FrameDev fr, const float *__restrict__ cam_inner, const float *__restrict__ cam_tris,
              const unsigned int *__restrict__ entries, const unsigned int *__restrict__ count, unsigned int *head,
              unsigned int *__restrict__ lists, uint32_t lds_levels, uint32_t overflow_entries, void *overflow_stack) {
    extern __shared__ uint2 lds_stack[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    ClaimStack stk;
    stk.stk = lds_stack + (size_t)wave * (lds_levels + 1) * 64 + lane;
    stk.ovf = (uint2 *)overflow_stack + ((size_t)(blockIdx.x * (blockDim.x >> 6) + wave) * overflow_entries) * 64 + lane;
    stk.lds_entries = (int)lds_levels;
    PcFilm fm;
    for (int i = 0; i < 9; ++i) fm.m[i] = fr.m[i];
    fm.width = fr.width, fm.height = fr.height, fm.sensor_x = fr.sensor_x, fm.sensor_y = fr.sensor_y, fm.film_dist = fr.film_dist;
    const uint32_t tiles_x = (fr.width + 7u) / 8u;
    const uint32_t n = *count;
    for (;;) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(head, 64u);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (base >= n) break;
        if (base + lane < n) {
            const uint32_t e = entries[base + lane], tile = e >> 6;
            const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
            const uint32_t lp = (ty * 8u + ((e & 63u) >> 3)) * fr.width + tx * 8u + (e & 7u);
            uint4 *rec = (uint4 *)lists + lp;
            const uint4 parked = *rec;
            uint32_t l[kListWords];
            pc_pixel_list(fm, global_pixel(fr, lp), cam_inner, cam_tris, sc.root_ref, stk, (int)(lds_levels + overflow_entries),
                          (int)parked.x, (int)parked.y, l);
            *rec = make_uint4(l[0], l[1], l[2], l[3]);
        }
    }
}

// k_unclaimed_words — for a pass that fuses its claimed pixels: per 64 slots of the pass's pixel list, one word with the
// bits of the slots whose pixel has no claim, and its popcount; launch_slot_lists (k_slot_scatter) makes the ORDERED lists of
// those slots and of the claimed ones from them (ordered: the traversal kernel's 8 bands keep their image regions, see render_pass).  n_pad is a multiple of 64.
__global__ void __launch_bounds__(256)
k_unclaimed_words(const unsigned int *__restrict__ active, uint32_t n_active, uint32_t n_pad, const unsigned int *__restrict__ claims,
                  unsigned long long *__restrict__ mask, unsigned int *__restrict__ cnt) {
    for (uint32_t s_idx = blockIdx.x * blockDim.x + threadIdx.x; s_idx < n_pad; s_idx += gridDim.x * blockDim.x) {
        const bool un = s_idx < n_active && claims[active[s_idx]] == kClaimNone;
        const unsigned long long bits = __builtin_amdgcn_ballot_w64(un);
        if ((threadIdx.x & 63u) == 0) mask[s_idx >> 6] = bits, cnt[s_idx >> 6] = (uint32_t)__popcll(bits);
    }
}

// k_walk_words — the same for the third list of such a pass when the run has list claims: the bits of the slots whose
// pixel has neither a claim nor a list.  Every ray of such a pixel walks the tree, so these slots, in order, are what
// k_trace_w<0> works on; the rays of the other unclaimed pixels are settled where they are formed (k_raygen<0, true>).
__global__ void __launch_bounds__(256)
k_walk_words(const unsigned int *__restrict__ active, uint32_t n_active, uint32_t n_pad, const unsigned int *__restrict__ claims,
             const unsigned int *__restrict__ lists, unsigned long long *__restrict__ mask, unsigned int *__restrict__ cnt) {
    for (uint32_t s_idx = blockIdx.x * blockDim.x + threadIdx.x; s_idx < n_pad; s_idx += gridDim.x * blockDim.x) {
        bool walk = false;
        if (s_idx < n_active) {
            const uint32_t lp = active[s_idx];
            walk = claims[lp] == kClaimNone && lists[(size_t)lp * kListWords] == kClaimNone;
        }
        const unsigned long long bits = __builtin_amdgcn_ballot_w64(walk);
        if ((threadIdx.x & 63u) == 0) mask[s_idx >> 6] = bits, cnt[s_idx >> 6] = (uint32_t)__popcll(bits);
    }
}

// ---------------------------------------------------------------------------
// k_raygen — camera rays of one pass (pathtracer.cpp:251-280), written to rayA[pid] as
// (direction, flag word): all camera rays share the frame's origin, so 16 bytes per ray suffice.
// Slots without a sample (past the pixel's last one, padding) get the word ~0 and are skipped downstream;
// the others the two step_bits of their first Radiance step.
// ---------------------------------------------------------------------------
// LIVE 0: every camera ray of the pass, rayA[pid].   LIVE 1 (VMX_SAMPLING_ELIDE_DEAD): nothing is written but one word
// of live bits and its popcount per 64 consecutive path ids; launch_live_compact turns those into the ordered list of
// live path ids and k_raygen_live writes their rays, densely, to rayA[position in that list].
// LISTS (LIVE 0; a pass that fuses its claimed pixels in a run with list claims, pixel-major, whole chunks of 64): the
// kernel settles the rays of a listed pixel where it forms them.  A wave's rays are samples of ONE pixel, so the pixel's
// list record and its members' camera-relative records are wave-uniform and come through the scalar cache; every lane
// with a sample runs pc_list_settle (pixel_claim.h: the function and the operands of k_trace_w<0>'s refill branch, so
// the same rays settle with the same bits) on the direction it stores.  A settled lane writes hit[pid] beside its ray;
// the path id of any other goes to the straggler list (wk.qids: ids, counts[0], sub_capacity), which k_trace_w<0>
// traces as a work source of its own.  The pixels without a list are left to that kernel's walk-slot list.
template <int LIVE, bool LISTS = false>
__global__ void __launch_bounds__(256)
k_raygen(SceneDev sc, FrameDev fr, WorkDev wk, PixelStateDev px, PathArrays pa) {
    static_assert(!LISTS || !LIVE, "list pixels are settled in the plain form");
    const uint32_t total = wk.samples * wk.n_pad;
    [[maybe_unused]] uint32_t n_listed = 0;  // (wave-uniform) LISTS: rays settled by their pixel's list
    if (wk.pixel_major && (wk.samples & 63u) == 0) {
        // a wave's 64 path ids are 64 samples of ONE pixel: slot, pixel and cursor are wave-uniform — one division and one
        // scalar fetch each per wave instead of per lane (round 3: 3.2 -> 2.9 ms for the 530.8 M rays of the bench frame)
        // Round 4: a wave takes a whole PIXEL — all its samples, 64 at a time — so that the two dependent scalar fetches
        // (active[slot], then the pixel's cursor) and the pixel half of the stream key are paid once per pixel, not once
        // per 64 samples: the kernel was waiting on those fetches for 58 % of its wave cycles (3.2 -> 2.0 ms for the bench frame)
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t waves = gridDim.x * (blockDim.x >> 6);
        const uint32_t chunks = wk.samples >> 6;
        // a pass that fuses its claimed pixels (WorkDev::unclaimed): only the listed slots get rays — a claimed pixel's
        // are formed where they are shaded (k_shade<0, .., DENSE, CLAIMED>), and nothing reads the padding slots' records
        const bool listed = !LIVE && wk.unclaimed != nullptr;
        const uint32_t units = listed ? *wk.unclaimed_count : wk.n_pad;
        for (uint32_t unit = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
             unit < units; unit += waves) {
            const uint32_t s_idx = listed ? wk.unclaimed[unit] : unit;
            const uint32_t pid_base = s_idx * wk.samples;
            if (s_idx < wk.n_active) {
                const uint32_t lp = wk.active[s_idx];
                const uint32_t pixel = global_pixel(fr, lp);
                const PixelKey pk = rng_pixel_key(fr.seed, pixel);
                // (the step bits are drawn at all only where a kernel reads them: fr.camera_bits / LIVE)
                const bool lights = (LIVE || fr.camera_bits) && pixel_may_reach_a_light(sc, fr, pixel);
                const uint32_t cur = px.cursor[lp];  // (sample_index, with the cursor fetched once)
                const uint32_t k0 = cur & ~kCursorStrided, kstep = (cur & kCursorStrided) ? fr.quarter : 1u;
                // LISTS: the pixel's list record, one scalar fetch (an empty list: the pixel's rays walk, k_trace_w<0>)
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                [[maybe_unused]] u32x4 lrec = {kClaimNone, kClaimNone, kClaimNone, kClaimNone};
                if constexpr (LISTS) lrec = ((const __attribute__((address_space(4))) u32x4 *)(uintptr_t)wk.claim_lists)[lp];
                for (uint32_t ch = 0; ch < chunks; ++ch) {
                    const uint32_t j = ch * 64u + lane;
                    const uint32_t k = (fr.lead != 0 && j >= fr.lead) ? (j - fr.lead + 1u) * fr.quarter : k0 + j * kstep;
                    bool live = false;
                    float dx = 0.f, dy = 0.f, dz = 0.f;
                    uint32_t depth = 0xFFFFFFFFu;
                    if (k < fr.kmax) {
                        Rng rng;
                        if (LIVE && !lights) {
                            // no ray of this pixel can meet a light: whether the path is live is decided by its draws
                            // alone — the stream keyed, the two jitter draws skipped, the step's three numbers drawn —
                            // and the ray itself is formed later, for the live paths only (k_raygen_live)
                            rng_init_keyed(rng, pk, k);
                            (void)rng_next(rng);
                            (void)rng_next(rng);
                            live = step_bits<false>(sc, fr.r2scale, rng, 0, fr.px, fr.py, fr.pz, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f, false) != 3u;
                        } else {
                            primary_ray_keyed(fr, pixel, pk, k, rng, dx, dy, dz);
                            if (LIVE) live = !step_is_dead<false>(sc, fr.r2scale, rng, 0, fr.px, fr.py, fr.pz, dx, dy, dz, 1.f, 1.f, 1.f);
                            else depth = fr.camera_bits ? step_bits<false>(sc, fr.r2scale, rng, 0, fr.px, fr.py, fr.pz, dx, dy, dz, 1.f, 1.f, 1.f, lights) : 0u;
                        }
                    }
                    if (!LIVE) ((float4 *)pa.rayA)[pid_base + j] = make_float4(dx, dy, dz, __uint_as_float(depth));
                    if (LIVE) {
                        const unsigned long long bits = __builtin_amdgcn_ballot_w64(live);
                        if (lane == 0) wk.live_mask[(pid_base >> 6) + ch] = bits, wk.live_cnt[(pid_base >> 6) + ch] = (uint32_t)__popcll(bits);
                    }
                    if constexpr (LISTS) {
                        if (lrec.x != kClaimNone) {  // (wave-uniform)
                            // the member records are read at wave-uniform addresses of the frame's constant triangle
                            // table: through the scalar cache, as the CLAIMED form of k_shade<0> takes its claimed triangle
                            const float *ctris = (const float *)(const __attribute__((address_space(4))) float *)(uintptr_t)wk.cam_tris;
                            const bool has = depth != 0xFFFFFFFFu;  // the slot has a sample
                            float t = 0.f;
                            uint32_t m = 0;
                            const bool settled = has && pc_list_settle(ctris, lrec.x, lrec.y, lrec.z, lrec.w, dx, dy, dz, t, m);
                            if (settled) ((float2 *)pa.hit)[pid_base + j] = make_float2(t, __int_as_float((int)m));
                            n_listed += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(settled));
                            // the stragglers' path ids: one ballot, and one atomic per chunk that has any
                            const bool strag = has && !settled;
                            const unsigned long long sm = __builtin_amdgcn_ballot_w64(strag);
                            if (sm != 0) {
                                uint32_t base = 0;
                                if (lane == 0) base = atomicAdd(wk.qids.counts, (uint32_t)__popcll(sm));
                                base = __builtin_amdgcn_readfirstlane(base);
                                const uint32_t at = base + (uint32_t)__popcll(sm & ((1ull << lane) - 1ull));
                                // (the list holds every path id of a pass: `at` stays below its end; an entry that would
                                // not is reported instead of written, as k_trace_w's fallback_append reports one)
                                if (strag && at < wk.qids.sub_capacity) wk.qids.ids[at] = pid_base + j;
                                else if (strag) atomicAdd(&wk.list_ctr->overflow, 1ull);
                            }
                        }
                    }
                }
            } else {
                // padding slots of the pass: marked like sample slots past a pixel's last sample
                for (uint32_t ch = 0; ch < chunks; ++ch) {
                    if (!LIVE) ((float4 *)pa.rayA)[pid_base + ch * 64u + lane] = make_float4(0.f, 0.f, 0.f, __uint_as_float(0xFFFFFFFFu));
                    if (LIVE && lane == 0) wk.live_mask[(pid_base >> 6) + ch] = 0ull, wk.live_cnt[(pid_base >> 6) + ch] = 0u;
                }
            }
        }
        if constexpr (LISTS) {
            if (lane == 0 && n_listed) atomicAdd(&wk.list_ctr->listed, (unsigned long long)n_listed);
        }
        return;
    }
    // (n_pad, and with it total, is a multiple of 64: a wave's 64 lanes hold 64 consecutive path ids and run the body together)
    for (uint32_t pid = blockIdx.x * blockDim.x + threadIdx.x; pid < total; pid += gridDim.x * blockDim.x) {
        uint32_t j, s_idx;
        if (wk.pixel_major) s_idx = fast_div(pid, wk.div_samples), j = pid - s_idx * wk.samples;
        else j = pid / wk.n_pad, s_idx = pid - j * wk.n_pad;
        uint32_t pid2, pixel, k;
        float dx = 0.f, dy = 0.f, dz = 0.f;
        uint32_t depth = 0xFFFFFFFFu;
        bool live = false;
        if (s_idx < wk.n_active && primary_item(fr, wk, px, j, s_idx, pid2, pixel, k)) {
            Rng rng;
            primary_ray(fr, pixel, k, rng, dx, dy, dz);
            if (LIVE) live = !step_is_dead<false>(sc, fr.r2scale, rng, 0, fr.px, fr.py, fr.pz, dx, dy, dz, 1.f, 1.f, 1.f);
            else depth = fr.camera_bits ? step_bits<false>(sc, fr.r2scale, rng, 0, fr.px, fr.py, fr.pz, dx, dy, dz, 1.f, 1.f, 1.f) : 0u;
        }
        // camera rays share the origin (FrameDev): one 16-byte record in rayA — direction, and a word that is ~0 for a
        // slot without a sample (past the pixel's last one, or padding), else the step's step_bits
        if (!LIVE) ((float4 *)pa.rayA)[pid] = make_float4(dx, dy, dz, __uint_as_float(depth));
        if (LIVE) {
            const unsigned long long bits = __builtin_amdgcn_ballot_w64(live);
            if ((threadIdx.x & 63u) == 0) wk.live_mask[pid >> 6] = bits, wk.live_cnt[pid >> 6] = (uint32_t)__popcll(bits);
        }
    }
}

// the rays of the live camera paths, in list order: rayA[i] belongs to path live_ids[i]
__global__ void __launch_bounds__(256)
k_raygen_live(SceneDev sc, FrameDev fr, WorkDev wk, PixelStateDev px, PathArrays pa) {
    const uint32_t n = *wk.live_count;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t pid = wk.live_ids[i];
        uint32_t j, s_idx;
        if (wk.pixel_major) s_idx = fast_div(pid, wk.div_samples), j = pid - s_idx * wk.samples;
        else j = pid / wk.n_pad, s_idx = pid - j * wk.n_pad;
        uint32_t pid2, pixel, k;
        float dx = 0.f, dy = 0.f, dz = 0.f;
        uint32_t depth = 0xFFFFFFFFu;
        if (primary_item(fr, wk, px, j, s_idx, pid2, pixel, k)) {  // (always: the path was found live from the same item)
            Rng rng;
            primary_ray(fr, pixel, k, rng, dx, dy, dz);
            depth = fr.camera_bits ? step_bits<false>(sc, fr.r2scale, rng, 0, fr.px, fr.py, fr.pz, dx, dy, dz, 1.f, 1.f, 1.f) : 0u;
        }
        ((float4 *)pa.rayA)[i] = make_float4(dx, dy, dz, __uint_as_float(depth));
    }
}

// VMX_SAMPLING_ELIDE_DEAD: the n live camera paths of a pass are split into 8 bands of whole waves, one per work source
__device__ __forceinline__ uint32_t live_band(uint32_t n) { return ((n + 511u) / 512u) * 64u; }

// ---------------------------------------------------------------------------
// k_trace_q — the first form of the split wavefront's persistent traversal kernel
// (BVH::getIntersection only, bvh.cpp:47-145), now the instrumented build (visit
// counters, vmx_opts.collect_counters) and an A/B reference for k_trace_w below.
// Lane state is one ray; lanes refill themselves from the work source.
// Writes hit[pid] = (t, leaf slot).
//   SRC 0: camera rays written by k_raygen (direction in rayA, the frame's origin)
//   SRC 1: bounce rays of the queued path ids, read from rayA/rayB
// ---------------------------------------------------------------------------
template <bool COUNT, int SRC>
__global__ void __launch_bounds__(256, VMX_TRACE_WAVES_PER_SIMD)
k_trace_q(SceneDev sc, FrameDev fr, WorkDev wk, PixelStateDev px, PathArrays pa, DevCounters *ctr) {
    extern __shared__ uint2 lds_stack[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int lds_entries = (int)wk.lds_entries;
    uint2 *stk = lds_stack + (size_t)wave * (lds_entries + 1) * 64 + lane;
    uint2 *ovf = (uint2 *)wk.overflow_stack +
                 ((size_t)(blockIdx.x * (blockDim.x >> 6) + wave) * wk.overflow_entries) * 64 + lane;
    // camera rays (SRC 0) read the per-frame origin-relative copies written by k_camera_tables
    const float4 *__restrict__ inner = SRC == 0 ? (const float4 *)wk.cam_inner : (const float4 *)sc.inner;
    const float4 *__restrict__ tris = SRC == 0 ? (const float4 *)wk.cam_tris : (const float4 *)sc.tris;
    float2 *__restrict__ hit_out = (float2 *)pa.hit;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const uint32_t kReserve = wk.reserve;
    constexpr int kActionsPerCheck = 8;  // traversal actions between two scheduling checks
    const uint32_t nsrc = wk.nsrc, refill_min = wk.refill_min;
    const uint32_t band_slots = wk.band_slots, band_items = wk.band_items;
    const uint32_t root_ref = sc.root_ref;

    // wave-uniform scheduling state (kept in SGPRs through readfirstlane)
    uint32_t src = blockIdx.x % nsrc, res_lo = 0, res_hi = 0, tried = 0;
    bool exhausted = false;
    // lane state: one ray
    bool has = false, exact = false, counted = false;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
    float ix = 0.f, iy = 0.f, iz = 0.f, best = 0.f, cur_near = 0.f;
    int slot = -1, sp = 0;
    uint32_t cur = 0, pid = 0;
    Cnt cn = {0, 0};

    for (;;) {
        // ---- refill idle lanes -------------------------------------------------------
        const unsigned long long idle = __builtin_amdgcn_ballot_w64(!has);
        if (idle != 0 && !exhausted && ((uint32_t)__popcll(idle) >= refill_min || idle == ~0ull)) {
            for (;;) {
                if (res_lo == res_hi) {
                    const uint32_t lim = SRC == 0 ? band_items : min(wk.qids.counts[src * 32], wk.qids.sub_capacity);
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&wk.heads[src * 32], kReserve);
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (base >= lim) {
                        src = (src + 1 == nsrc) ? 0 : src + 1;
                        if (++tried == nsrc) {
                            exhausted = true;
                            break;
                        }
                        continue;
                    }
                    tried = 0;
                    res_lo = base;
                    res_hi = min(base + kReserve, lim);
                }
                const unsigned long long want = __builtin_amdgcn_ballot_w64(!has);
                if (want == 0) break;
                const uint32_t avail = res_hi - res_lo;
                const uint32_t rank = (uint32_t)__popcll(want & lt_mask);
                const bool take = !has && rank < avail;
                const uint32_t item = res_lo + rank;
                res_lo = __builtin_amdgcn_readfirstlane(res_lo + min((uint32_t)__popcll(want), avail));
                if (take) {
                    bool valid = true;
                    if (SRC == 0) {
                        // band-local item -> path id; the ray was written by k_raygen
                        uint32_t j, s_idx;
                        if (wk.pixel_major) {
                            const uint32_t sl = fast_div(item, wk.div_samples);
                            j = item - sl * wk.samples, s_idx = src * band_slots + sl;
                        } else {
                            j = item / band_slots, s_idx = src * band_slots + (item - j * band_slots);
                        }
                        valid = s_idx < wk.n_active;
                        pid = path_id(wk, j, s_idx);
                    } else {
                        pid = wk.qids.ids[(size_t)src * wk.qids.sub_capacity + item];
                    }
                    if (valid) {
                        uint32_t depth;
                        if (SRC == 0) {  // camera ray: (direction, flag word), origin from the frame
                            const float4 a = ((const float4 *)pa.rayA)[pid];
                            ox = fr.px, oy = fr.py, oz = fr.pz, dx = a.x, dy = a.y, dz = a.z;
                            depth = __float_as_uint(a.w) == 0xFFFFFFFFu ? 0xFFFFFFFFu : 0u;  // (else: step_bits)
                        } else {
                            const float4 a = ((const float4 *)pa.state)[(size_t)pid * 4], b = ((const float4 *)pa.state)[(size_t)pid * 4 + 1];
                            ox = a.x, oy = a.y, oz = a.z, dx = a.w, dy = b.x, dz = b.y;
                            depth = __float_as_uint(b.z);
                        }
                        valid = depth != 0xFFFFFFFFu;  // k_raygen marks sample slots past the pixel's last sample
                        counted = (depth == 0u) || finite3(dx, dy, dz);
                    }
                    if (valid) {
                        has = true;
                        ix = 1.0f / dx, iy = 1.0f / dy, iz = 1.0f / dz;  // Ray.h:10
                        exact = !(finite3(ix, iy, iz) && finite3(ox, oy, oz));
                        best = 999999999.f;  // bvh.cpp:48
                        slot = -1;
                        sp = 0;
                        cur = root_ref;
                        cur_near = -9999999.f;  // bvh.cpp:59
                    }
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(has) == 0) break;
        // ---- traversal actions --------------------------------------------------------------
        // every iteration runs the one-triangle step for the lanes at a leaf and the inner-node step
        // for the others (a vote between the two was measured and is no faster)
        for (int act = 0; act < kActionsPerCheck; ++act) {
            const bool at_leaf = has && (cur & kLeafBit) != 0;
            if (__builtin_amdgcn_ballot_w64(has) == 0) break;
            bool need_next = false, carry = false;
            if (at_leaf) {
                float dist;
                bool hit;
                if (SRC == 0) {
                    const uint32_t ti = (cur & kLeafStartMask) * 4;
                    const float4 a = tris[ti], b = tris[ti + 1], c = tris[ti + 2], e = tris[ti + 3];
                    hit = tri_test_cam(a, b, c, e.x, dx, dy, dz, dist);
                } else {
                    const uint32_t ti = (cur & kLeafStartMask) * 3;
                    const float4 a = tris[ti], b = tris[ti + 1], c = tris[ti + 2];
                    hit = tri_test(a, b, c.x, ox, oy, oz, dx, dy, dz, dist);
                }
                if (COUNT && counted) cn.tris++;
                if (hit && dist < best) {  // strict <: first tested wins ties (bvh.cpp:90)
                    best = dist;
                    slot = (int)(cur & kLeafStartMask);
                }
                const uint32_t left = ((cur >> kLeafCountShift) & 31u) - 1u;
                need_next = left == 0;
                if (!need_next) cur = kLeafBit | (left << kLeafCountShift) | ((cur & kLeafStartMask) + 1u);
            }
            if (has && !at_leaf) {
                // The kernel is bound by the vector-memory pipe (4 x 1 KiB per wave and node visit).
                // Camera rays of one 8x8 tile mostly walk the same nodes: when every lane of this
                // step is at the same node, the record is fetched once through the scalar cache.
                float4 q0, q1, q2, q3;
                const uint32_t cur0 = __builtin_amdgcn_readfirstlane(cur);
                if (SRC == 0 && __builtin_amdgcn_ballot_w64(cur != cur0) == 0) {
                    // constant address space + wave-uniform address -> s_load_dwordx16
                    typedef float f32x4 __attribute__((ext_vector_type(4)));
                    typedef const __attribute__((address_space(4))) f32x4 *scalar_ptr;
                    const scalar_ptr rec = (scalar_ptr)(uintptr_t)(inner + (size_t)cur0 * 4);
                    const f32x4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                    q0 = make_float4(r0.x, r0.y, r0.z, r0.w);
                    q1 = make_float4(r1.x, r1.y, r1.z, r1.w);
                    q2 = make_float4(r2.x, r2.y, r2.z, r2.w);
                    q3 = make_float4(r3.x, r3.y, r3.z, r3.w);
                } else {
                    q0 = inner[cur * 4], q1 = inner[cur * 4 + 1], q2 = inner[cur * 4 + 2], q3 = inner[cur * 4 + 3];
                }
                if (COUNT && counted) cn.inner++;
                float tn0, tn1;
                bool h0, h1;
                if (SRC == 0) {
                    if (exact) {
                        h0 = box_exact_rel(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, ix, iy, iz, tn0);
                        h1 = box_exact_rel(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, ix, iy, iz, tn1);
                    } else {
                        h0 = box_fast_rel(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, ix, iy, iz, tn0);
                        h1 = box_fast_rel(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, ix, iy, iz, tn1);
                    }
                } else if (exact) {
                    h0 = box_exact(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, ox, oy, oz, ix, iy, iz, tn0);
                    h1 = box_exact(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, ox, oy, oz, ix, iy, iz, tn1);
                } else {
                    h0 = box_fast(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, ox, oy, oz, ix, iy, iz, tn0);
                    h1 = box_fast(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, ox, oy, oz, ix, iy, iz, tn1);
                }
                const uint32_t lref = __float_as_uint(q3.x), rref = __float_as_uint(q3.y);
                // bvh.cpp:103-132 without branches: both hit -> the strictly closer right child (else the
                // left) is next and the other one is pushed; one hit -> that child is next
                const bool both = h0 && h1;
                const bool go_right = both ? (tn1 < tn0) : h1;
                if (both) {
                    stack_push(stk, ovf, lds_entries, sp,
                               make_uint2(go_right ? lref : rref, __float_as_uint(go_right ? tn0 : tn1)));
                    ++sp;
                }
                cur = go_right ? rref : lref;
                cur_near = go_right ? tn1 : tn0;
                carry = h0 || h1;
                need_next = true;
            }
            if (need_next) {
                if (carry && cur_near > best) carry = false;  // bvh.cpp:69
                while (!carry) {
                    if (sp == 0) {
                        hit_out[pid] = make_float2(best, __int_as_float(slot));
                        has = false;
                        break;
                    }
                    --sp;
                    const uint2 e = stack_pop(stk, ovf, lds_entries, sp);
                    if (!(__uint_as_float(e.y) > best)) {
                        cur = e.x;
                        cur_near = __uint_as_float(e.y);
                        carry = true;
                    }
                }
            }
        }
    }
    if (COUNT) {
        const uint32_t iv = wave_sum(cn.inner), tt = wave_sum(cn.tris);
        if (lane == 0) {
            const int st = SRC == 0 ? 0 : 1;
            if (iv) atomicAdd(&ctr->stage[st].inner_visits, (unsigned long long)iv);
            if (tt) atomicAdd(&ctr->stage[st].tri_tests, (unsigned long long)tt);
        }
    }
}


// ---------------------------------------------------------------------------
// k_trace_w — k_trace_q's production form (no counters), written for the
// limit the SQ counters show this loop runs at: instruction delivery.  One
// traversal step of the first form executed ~62 VALU + ~47 SALU + ~12 branch
// instructions, and the instruction cache two CUs share was busy ~100 % of the
// kernel's cycles (SQC_ICACHE_BUSY_CYCLES; profiles/).  This form issues fewer of them:
//   * lane state is the node reference alone (idle = kIdle, "must pop" = kPop, bit 31 = leaf):
//     no has/carry/need_next lane masks to merge with SALU triples at every join;
//   * stack level 0 holds a bottom entry (ref kBottom, near = -inf): the pop loop is a
//     single do-while on `near > best` and a finished ray falls out of it;
//   * the NaN-exact box form is chosen per wave (a wave with any such ray runs the
//     exact form for all its lanes — both forms agree on finite data), not per lane;
//   * the min/max network of a box is one asm block (no hazard nops between the
//     pieces) and a scalar-fetched node record is multiplied straight from SGPRs;
//   * the all-lanes-idle test is made once per 8 steps, not every step.
// Each ray still performs exactly the reference's sequence of tests (bvh.cpp:47-145).
// ---------------------------------------------------------------------------
#ifdef VMX_STEP_PROFILE
#define VMX_DESCENT_COUNT "s_add_u32 %[done], %[done], 1\n\ts_nop 0\n\t"  // nodes done, for tools/step_profile.py
#else
#define VMX_DESCENT_COUNT "s_nop 1\n\t"  // the product does not count them: a scalar instruction is an issue slot
#endif
// ---------------------------------------------------------------------------
// uniform_descent — camera rays: the stretch of a traversal in which all traversing lanes of a wave are at
// the same inner node and take the same child, as one assembly loop.
//
// k_trace_w<0> is bound by instruction issue: on gfx950 a SIMD issues about one instruction per 2.2
// cycles whatever its kind — scalar ALU instructions do not overlap with vector ones — and a taken
// branch costs about three instructions (tools/sload_probe.hip, profiles/r02_sload_probe.txt); its
// counters add up to exactly that ((SQ_INSTS_VALU + SQ_INSTS_SALU) x 2.15 cycles = the kernel's SIMD
// cycles).  64 samples of one pixel walk the tree together, and the compiled step spends ~63
// instructions and two taken branches on such a node (lane dispatch, uniformity test, exec-masked push,
// lane masks merged with scalar ops) where the arithmetic is 16.  One iteration here is 39 instructions
// and the back edge:
//   * the 12 products and two max3/min3 pairs straight from the scalar-fetched record of the wave's
//     octant copy (near planes first, as the OCT route of the general step);
//   * a missed child gets the entry distance +inf, so "the right child is strictly closer, or the only
//     one hit" is one compare, near/far are a min and a max, and `near > t` (bvh.cpp:69) prunes a missed
//     child like a far one;
//   * the other child is stored above the stack top by every lane (no exec mask) and counts as an entry
//     (sp + 1) only where its distance is finite, i.e. where both children were hit (a child hit at +inf
//     is treated as missed: the reference would pop it again unvisited, `inf > t`);
//   * the next node is chosen on the scalar unit (s_cselect) and its record fetch issued at once.
// Round 3: when EVERY lane prunes at a node (both children missed, or beyond the hit so far — a wave's 64 samples of
// one pixel mostly agree on that too) the pop is done here as well, uniformly (label 5): 12 % of the kernel's
// wave-steps were whole waves leaving the loop only to pop and come back (tools/step_profile.py).
// While the lanes agree, none of them prunes and the next node is an inner node, the loop needs no
// per-lane node reference, no exec masking and no refill test (no lane can finish here).  When lanes
// disagree or one of them prunes, the node is finished per lane (same values, lane selects) and the
// general step goes on from there; a leaf, or a lane whose next push would leave the LDS levels, ends the
// loop as well.  Every ray performs exactly the tests of the general step, in the same order.
//   in: trav = the traversing lanes, scur = the inner node they all are at, sp < lds_entries in each of them
//   out: cur (per lane: next node, leaf or kPop), sp; returns the number of nodes done (diagnostic build; else 0)
// The record lives in s[36:51] (an inline-asm operand cannot be a 16-register tuple).
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t uniform_descent(int &sp, uint32_t &cur, float ix, float iy, float iz, float &best,
                                                    int &slot, float dx, float dy, float dz, uint32_t stk_lds,
                                                    const char *base, uint32_t tri_delta, uint32_t scur, int lds_entries,
                                                    unsigned long long trav) {
    float t0, t1, t2, n0, tf, n1, near, far;
    uint32_t va, oth, soff, soth, sidx, cnt, done = 0;
    unsigned long long tmp, pop;
    asm volatile(
        "s_mov_b64 exec, %[trav]\n\t"
        "s_lshl_b32 %[soff], %[scur], 6\n\t"
        "s_load_dwordx16 s[36:51], %[base], %[soff]\n"
        "1:\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_mul_f32_e32 %[t0], s36, %[ix]\n\t"
        "v_mul_f32_e32 %[t1], s37, %[iy]\n\t"
        "v_mul_f32_e32 %[t2], s38, %[iz]\n\t"
        "v_max3_f32 %[n0], %[t0], %[t1], %[t2]\n\t"
        "v_mul_f32_e32 %[t0], s39, %[ix]\n\t"
        "v_mul_f32_e32 %[t1], s40, %[iy]\n\t"
        "v_mul_f32_e32 %[t2], s41, %[iz]\n\t"
        "v_min3_f32 %[tf], %[t0], %[t1], %[t2]\n\t"
        "v_cmp_le_f32_e32 vcc, %[n0], %[tf]\n\t"              // left child hit (bbox.cpp:82)
        "v_mul_f32_e32 %[t0], s42, %[ix]\n\t"
        "v_mul_f32_e32 %[t1], s43, %[iy]\n\t"
        "v_mul_f32_e32 %[t2], s44, %[iz]\n\t"
        "v_cndmask_b32_e32 %[n0], %[inf], %[n0], vcc\n\t"  // its entry distance, +inf if missed
        "v_max3_f32 %[n1], %[t0], %[t1], %[t2]\n\t"
        "v_mul_f32_e32 %[t0], s45, %[ix]\n\t"
        "v_mul_f32_e32 %[t1], s46, %[iy]\n\t"
        "v_mul_f32_e32 %[t2], s47, %[iz]\n\t"
        "v_min3_f32 %[tf], %[t0], %[t1], %[t2]\n\t"
        "v_cmp_le_f32_e32 vcc, %[n1], %[tf]\n\t"              // right child hit
        VMX_DESCENT_COUNT  // (two wait states between the compare and the select on its mask either way)
        "v_cndmask_b32_e32 %[n1], %[inf], %[n1], vcc\n\t"
        "v_cmp_lt_f32_e32 vcc, %[n1], %[n0]\n\t"              // go right: strictly closer, or the only one hit (bvh.cpp:106)
        "v_min_f32_e32 %[near], %[n0], %[n1]\n\t"
        "v_max_f32_e32 %[far], %[n0], %[n1]\n\t"
        "v_cmp_gt_f32_e64 %[pop], %[near], %[best]\n\t"       // the child taken is pruned, or none was hit (bvh.cpp:69)
        "s_cmp_eq_u64 vcc, 0\n\t"                             // every lane goes left?
        "s_cselect_b32 %[scur], s48, s49\n\t"
        "s_cselect_b32 %[soth], s49, s48\n\t"
        "s_cselect_b64 %[tmp], exec, vcc\n\t"
        "s_andn2_b64 %[tmp], %[tmp], %[pop]\n\t"
        "s_cmp_eq_u64 %[tmp], exec\n\t"                       // all lanes the same way and none prunes
        "s_cbranch_scc0 2f\n\t"
        "v_mov_b32_e32 %[oth], %[soth]\n\t"
        "v_lshl_add_u32 %[va], %[sp], 9, %[stk]\n\t"
        "ds_write2_b32 %[va], %[oth], %[far] offset1:1\n\t"   // the other child, above the top
        "v_cmp_gt_f32_e32 vcc, %[inf], %[far]\n\t"        // ... an entry where both children were hit
        "s_lshl_b32 %[soff], %[scur], 6\n\t"
        "s_bitcmp1_b32 %[scur], 31\n\t"                       // the child taken is a leaf?
        "v_addc_co_u32_e32 %[sp], vcc, 0, %[sp], vcc\n\t"
        "s_cbranch_scc1 9f\n\t"
        "s_load_dwordx16 s[36:51], %[base], %[soff]\n\t"
        "v_cmp_le_i32_e32 vcc, %[lds], %[sp]\n\t"             // a lane whose next push would leave the LDS levels?
        "s_cbranch_vccz 1b\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"                            // nothing may land in s[36:51] after the block
        "s_branch 3f\n"
        // ---- the lanes part ways here, or some of them prune
        "2:\n\t"
        "s_cmp_eq_u64 %[pop], exec\n\t"                     // EVERY lane prunes (the common case: both children missed, or
        "s_cbranch_scc1 5f\n\t"                            // beyond the hit so far): pop here, uniformly, as long as that works
        // finish this node per lane (bvh.cpp:103-132)
        "v_mov_b32_e32 %[t0], s48\n\t"
        "v_mov_b32_e32 %[t1], s49\n\t"
        "v_cndmask_b32_e32 %[oth], %[t1], %[t0], vcc\n\t"     // stored: go right ? left : right
        "v_cndmask_b32_e32 %[t2], %[t0], %[t1], vcc\n\t"      // taken
        "v_lshl_add_u32 %[va], %[sp], 9, %[stk]\n\t"
        "ds_write2_b32 %[va], %[oth], %[far] offset1:1\n\t"
        "v_mov_b32_e32 %[t0], 0x7ffffffd\n\t"
        "v_cmp_gt_f32_e32 vcc, %[inf], %[far]\n\t"
        "v_cndmask_b32_e64 %[cur], %[t2], %[t0], %[pop]\n\t"  // kPop where the lane prunes
        "s_nop 0\n\t"
        "v_addc_co_u32_e32 %[sp], vcc, 0, %[sp], vcc\n\t"
        "s_branch 4f\n"
        // ---- uniform pop (bvh.cpp:61-70).  The child taken is pruned in every lane, so the other child — never nearer —
        // would be popped and pruned at once: it is not pushed at all.  Each lane reads ITS entry below the top; the wave
        // goes on together while all lanes skip it (near > t), or all take it and it is the same inner node for all of
        // them (back into the loop) or the same leaf (out, at that leaf).  Anything else — lanes disagree, the bottom
        // entry (the ray is done) — leaves sp untouched and hands every lane to the general step as "must pop".
        "5:\n\t"
        "v_add_u32_e32 %[t0], -1, %[sp]\n\t"
        "v_lshl_add_u32 %[va], %[t0], 9, %[stk]\n\t"
        "ds_read_b32 %[t1], %[va]\n\t"                      // node reference of the entry
        "ds_read_b32 %[t2], %[va] offset:4\n\t"             // its entry distance
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_cmp_gt_f32_e32 vcc, %[t2], %[best]\n\t"          // lanes that skip it
        "s_cbranch_vccz 6f\n\t"
        "s_cmp_eq_u64 vcc, exec\n\t"
        "s_cbranch_scc0 7f\n\t"                            // some skip, some take: per lane from here
        "v_mov_b32_e32 %[sp], %[t0]\n\t"                    // all skip: next entry
        "s_branch 5b\n"
        "6:\n\t"
        "v_readfirstlane_b32 %[soth], %[t1]\n\t"
        "s_nop 1\n\t"
        "v_cmp_ne_u32_e32 vcc, %[soth], %[t1]\n\t"
        "s_cbranch_vccnz 7f\n\t"                           // not the same entry in every lane
        "s_cmp_ge_u32 %[soth], 0x7ffffffd\n\t"              // leaf (bit 31) or bottom entry: not an inner node
        "s_cbranch_scc1 8f\n\t"
        "v_mov_b32_e32 %[sp], %[t0]\n\t"
        "s_mov_b32 %[scur], %[soth]\n\t"
        "s_lshl_b32 %[soff], %[scur], 6\n\t"
        "s_load_dwordx16 s[36:51], %[base], %[soff]\n\t"
        "s_branch 1b\n"
        "8:\n\t"
        "s_bitcmp1_b32 %[soth], 31\n\t"
        "s_cbranch_scc0 7f\n\t"                            // the bottom entry: the general step finishes the rays
        "v_mov_b32_e32 %[sp], %[t0]\n\t"
        "s_mov_b32 %[scur], %[soth]\n"
        // ---- uniform leaf (triangle.cpp:4-54 on the camera-relative records of k_camera_tables): every traversing lane
        // tests every triangle of the leaf, the record comes through the scalar cache into s[36:51]
        //   s36-38 e1   s39-41 e2   s42-44 tvec = o - v0   s45-47 qvec = cross(tvec, e1)   s48 dot(e2, qvec)
        // same operations in the same order as the general step (tri_test_cam is the C++ statement of this arithmetic);
        // then the uniform pop above
        "9:\n\t"
        "s_and_b32 %[sidx], %[scur], 0x3ffffff\n\t"         // leaf slot of the first triangle
        "s_bfe_u32 %[cnt], %[scur], 0x5001a\n\t"            // triangles in the leaf (5 bits at 26)
        "s_lshl_b32 %[soff], %[sidx], 6\n\t"
        "s_add_u32 %[soff], %[soff], %[tdelta]\n\t"
        "s_load_dwordx16 s[36:51], %[base], %[soff]\n"
        "10:\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_mul_f32_e32 %[t0], s41, %[dy]\n\t"               // pvec = cross(d, e2)
        "v_mul_f32_e32 %[t1], s40, %[dz]\n\t"
        "v_sub_f32_e32 %[n0], %[t0], %[t1]\n\t"
        "v_mul_f32_e32 %[t0], s39, %[dz]\n\t"
        "v_mul_f32_e32 %[t1], s41, %[dx]\n\t"
        "v_sub_f32_e32 %[tf], %[t0], %[t1]\n\t"
        "v_mul_f32_e32 %[t0], s40, %[dx]\n\t"
        "v_mul_f32_e32 %[t1], s39, %[dy]\n\t"
        "v_sub_f32_e32 %[n1], %[t0], %[t1]\n\t"
        "v_mul_f32_e32 %[t0], s36, %[n0]\n\t"               // det = dot(e1, pvec)
        "v_mul_f32_e32 %[t1], s37, %[tf]\n\t"
        "v_add_f32_e32 %[t0], %[t0], %[t1]\n\t"
        "v_mul_f32_e32 %[t1], s38, %[n1]\n\t"
        "v_add_f32_e32 %[near], %[t0], %[t1]\n\t"
        "v_div_scale_f32 %[t0], %[pop], %[near], %[near], 1.0\n\t"   // inv_det = 1 / det, correctly rounded
        "v_rcp_f32_e32 %[t1], %[t0]\n\t"
        "v_div_scale_f32 %[t2], vcc, 1.0, %[near], 1.0\n\t"
        "v_fma_f32 %[far], -%[t0], %[t1], 1.0\n\t"
        "v_fmac_f32_e32 %[t1], %[far], %[t1]\n\t"
        "v_mul_f32_e32 %[far], %[t2], %[t1]\n\t"
        "v_fma_f32 %[oth], -%[t0], %[far], %[t2]\n\t"
        "v_fmac_f32_e32 %[far], %[oth], %[t1]\n\t"
        "v_fma_f32 %[t0], -%[t0], %[far], %[t2]\n\t"
        "v_div_fmas_f32 %[t0], %[t0], %[t1], %[far]\n\t"
        "v_div_fixup_f32 %[t0], %[t0], %[near], 1.0\n\t"
        "v_mul_f32_e32 %[t1], s42, %[n0]\n\t"               // u = dot(tvec, pvec) * inv_det
        "v_mul_f32_e32 %[t2], s43, %[tf]\n\t"
        "v_add_f32_e32 %[t1], %[t1], %[t2]\n\t"
        "v_mul_f32_e32 %[t2], s44, %[n1]\n\t"
        "v_add_f32_e32 %[t1], %[t1], %[t2]\n\t"
        "v_mul_f32_e32 %[n0], %[t1], %[t0]\n\t"
        "v_mul_f32_e32 %[t1], s45, %[dx]\n\t"               // v = dot(d, qvec) * inv_det
        "v_mul_f32_e32 %[t2], s46, %[dy]\n\t"
        "v_add_f32_e32 %[t1], %[t1], %[t2]\n\t"
        "v_mul_f32_e32 %[t2], s47, %[dz]\n\t"
        "v_add_f32_e32 %[t1], %[t1], %[t2]\n\t"
        "v_mul_f32_e32 %[tf], %[t1], %[t0]\n\t"
        "v_mul_f32_e32 %[n1], s48, %[t0]\n\t"               // t = dot(e2, qvec) * inv_det
        "v_add_f32_e32 %[t1], %[n0], %[tf]\n\t"             // u + v
        "v_and_b32_e32 %[t2], 0x7fffffff, %[near]\n\t"      // |det|
        // the next triangle's record can be on its way while this one is judged
        "s_cmp_lg_u32 %[cnt], 1\n\t"
        "s_cbranch_scc0 11f\n\t"
        "s_add_u32 %[soff], %[soff], 64\n\t"
        "s_load_dwordx16 s[36:51], %[base], %[soff]\n"
        "11:\n\t"
        "s_mov_b64 %[tmp], exec\n\t"
        "v_cmpx_nge_f32_e32 vcc, 0x322bcc77, %[t2]\n\t"     // not (|det| <= float(1e-8))           triangle.cpp:25
        "v_cmpx_ngt_f32_e32 vcc, 0, %[n0]\n\t"              // not (u < 0)                          :34
        "v_cmpx_nlt_f32_e32 vcc, 1.0, %[n0]\n\t"            // not (u > 1)
        "v_cmpx_ngt_f32_e32 vcc, 0, %[tf]\n\t"              // not (v < 0)                          :40
        "v_cmpx_nlt_f32_e32 vcc, 1.0, %[t1]\n\t"            // not (u + v > 1)
        "v_cmpx_lt_f32_e32 vcc, 0, %[n1]\n\t"               // t > 0                                :44
        "v_cmpx_lt_f32_e32 vcc, %[n1], %[best]\n\t"         // strictly nearer: the first tested wins ties (bvh.cpp:90)
        "v_mov_b32_e32 %[best], %[n1]\n\t"
        "v_mov_b32_e32 %[slot], %[sidx]\n\t"
        "s_mov_b64 exec, %[tmp]\n\t"
        "s_add_u32 %[sidx], %[sidx], 1\n\t"
        "s_sub_u32 %[cnt], %[cnt], 1\n\t"
        "s_cmp_lg_u32 %[cnt], 0\n\t"
        "s_cbranch_scc1 10b\n\t"
        "s_branch 5b\n"
        "7:\n\t"
        "v_mov_b32_e32 %[cur], 0x7ffffffd\n\t"              // kPop
        "s_branch 4f\n"
        "3:\n\t"
        "v_mov_b32_e32 %[cur], %[scur]\n"
        "4:\n\t"
        "s_mov_b64 exec, -1"
        : [sp] "+v"(sp), [cur] "+v"(cur), [best] "+v"(best), [slot] "+v"(slot), [scur] "+s"(scur), [done] "+s"(done),
          [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [n0] "=&v"(n0), [tf] "=&v"(tf), [n1] "=&v"(n1),
          [near] "=&v"(near), [far] "=&v"(far), [va] "=&v"(va), [oth] "=&v"(oth), [soff] "=&s"(soff), [soth] "=&s"(soth),
          [sidx] "=&s"(sidx), [cnt] "=&s"(cnt), [tmp] "=&s"(tmp), [pop] "=&s"(pop)
        : [ix] "v"(ix), [iy] "v"(iy), [iz] "v"(iz), [dx] "v"(dx), [dy] "v"(dy), [dz] "v"(dz), [stk] "v"(stk_lds),
          [base] "s"(base), [tdelta] "s"(tri_delta), [lds] "s"(lds_entries), [trav] "s"(trav), [inf] "v"(__builtin_inff())
        : "vcc", "scc", "memory", "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47",
          "s48", "s49", "s50", "s51");
    return done;
}

#ifdef VMX_STEP_PROFILE
#include "vmx_step_profile.inc"
#else
#define VMX_PROF_STEP(EX, OC) step(EX, OC)
#endif

// LIVE (SRC 0, VMX_SAMPLING_ELIDE_DEAD): the work is the dense list of live camera paths — ray and hit record of list
// entry i sit at rayA[i] / hit[i] — cut into 8 bands of whole waves (live_band)
// SORT (classified output, DESIGN_HISTORY.md 5.1): instead of a hit record per ray, the finished rays of a wave are sorted on the
// spot when the wave refills.  A ray whose Radiance step is the path's last one by the path's own draws (the bits that
// came with the ray) and that cannot meet a light sphere needs nothing more: it is counted here and forgotten.  The
// others get a 32-byte record (direction, flag word | t, leaf slot, position) appended to a dense list — the wave
// reserves 256 entries at a time with one atomic, fills them to the last one, and pads the tail of its last chunk with
// position = ~0 when it ends — which k_shade reads front to back.
// GUIDE (SRC 1, a reference-tree scene with a valid guide; guide_walk.h): the rays walk the GUIDE's records (gd.base,
// gd.tri_off, gd.root_ref) with the prune on near > cut = best (1 + kGwKappa) and keep `second`.  A finished ray is held
// until the next refill, as SORT holds it; there the rule runs for the wave's finished lanes together (one 48-byte record
// fetch per ray): a settled ray takes the winner's REFERENCE slot from its record and goes where it goes today (hit_out,
// or sort_finished's decision and record); a fallback ray's path id is appended to gd.fb_ids — one atomic per wave and
// refill that has any, the count stays on the device — and the existing instantiation traces that list over the
// reference tree in a second launch.  Rays with non-finite inputs or an origin beyond the scene's |coordinates| are
// appended at refill without a walk, so the NaN-exact box form never meets the guide.
constexpr uint32_t kOutChunk = 256;
// VISITS (GUIDE; k_trace_w_visits, the debug entry vmx_guide_trace_visits only): every lane counts the inner records and
// the triangle tests of its ray's guide walk and leaves them in visits_out[pid] when the walk ends; the product kernels
// carry no counters.  (The kernel's text is vmx_trace_w.inc, included once per kernel.)
#define VMX_TRACE_W_VISITS 0
#include "vmx_trace_w.inc"
#undef VMX_TRACE_W_VISITS
#define VMX_TRACE_W_VISITS 1
#include "vmx_trace_w.inc"
#undef VMX_TRACE_W_VISITS

// ---------------------------------------------------------------------------
// k_shade — the wide shading kernel of the split wavefront: the part of
// MeshEngine::RayCast after the BVH query (triangle normal, sphere table,
// meshEngine.cpp:365-508) and one iteration of Radiance's loop
// (pathtracer.cpp:36-196), one lane per path, then wave-ballot compaction of
// the surviving path ids.
//   SRC 0: depth-0 steps; the camera ray and the RNG stream are regenerated
//          from (pixel, sample) instead of being stored by the trace kernel
//   SRC 1: queued path ids; ray, RNG and accumulated colour come from the arrays
// ---------------------------------------------------------------------------
#ifndef VMX_SHADE_WPS
#define VMX_SHADE_WPS 7  // waves per SIMD k_shade is compiled for (<= 72 VGPRs): left to itself hipcc takes 100 (5 waves) since the
                        // cosf/sinf path came in; k_shade<0> 14.6 ms at 5-6 waves (the cap at 6 spills into the hot path), 13.1 at 7, 13.4 at 8
#endif
// FROMQ: 0 every path of the generation; 1 the ordered list of positions k_shade_ends + launch_live_compact left
// (wk.flat_ids); 2 the records k_trace_w<.., SORT> appended (wk.out_rec: ray, hit and position in one place)
// CLAIMED (dense form, a pass that fuses its claimed pixels): the work is the ordered list of the pass's CLAIMED slots
// (wk.shade_slots, *wk.shade_count — as the plain dense form walks the unclaimed ones); the kernel forms each ray itself, as k_raygen does, and settles its BVH query by the pixel's claim —
// neither rayA nor hit holds anything for these pixels.  The pass's other slots go through the plain dense form, over
// the list of the unclaimed slots.  (One kernel with a wave-uniform branch was built first: 72 VGPRs, occupancy 7, but
// 76 -> 108 bytes of scratch for every pixel, claimed or not — DESIGN.md §9.)
template <int SRC, bool TEX, bool ELIDE = false, int FROMQ = 0, bool DENSE = false, bool CLAIMED = false>
__global__ void __launch_bounds__(256, VMX_SHADE_WPS)
k_shade(SceneDev sc, FrameDev fr, WorkDev wk, PixelStateDev px, PathArrays pa, IdQueue qout, uint32_t max_chunks,
        DevCounters *ctr) {
    const float2 *__restrict__ hits = (const float2 *)pa.hit;
    float4 *__restrict__ rad = (float4 *)pa.rad;
    __shared__ float4 s_geom[kLdsSpheres];
    __shared__ float4 s_cam_op[kLdsSpheres];  // SRC 0: (centre - camera position, squared length), same for every path
    // the dense camera form, one row per wave: the wave's pixel's sphere bounds and their minimum (pixel_sphere_bound);
    // its first sample index, the step between its samples and the pixel half of its stream key
    __shared__ float s_lmax[4][kLdsSpheres + 1];
    __shared__ uint32_t s_pix[4][6];
    if (threadIdx.x < min(sc.nspheres, kLdsSpheres)) {
        const SphereDev &q = sc.spheres[threadIdx.x];
        s_geom[threadIdx.x] = make_float4(q.cx, q.cy, q.cz, q.rad2);
        const float opx = q.cx - fr.px, opy = q.cy - fr.py, opz = q.cz - fr.pz;
        s_cam_op[threadIdx.x] = make_float4(opx, opy, opz, dot3(opx, opy, opz, opx, opy, opz));
    }
    __syncthreads();
    Tally tl = {{0, 0}, {0, 0}, {0, 0}};
    // FROMQ (two-phase shading): the work is the ordered list k_shade_ends + launch_live_compact left — the positions
    // of the paths whose step does not end by its draws alone (wk.flat_ids, *wk.flat_count).  A position is an index
    // into rayA / hit for camera paths (`src`), a place in the id queue for bounce paths
    uint32_t items = (SRC == 0 ? (wk.samples * wk.n_pad + blockDim.x - 1) / blockDim.x : max_chunks * kSubQueues);
    uint32_t flat_n = 0;
    if (FROMQ == 1) flat_n = *wk.flat_count, items = (flat_n + blockDim.x - 1) / blockDim.x;
    if (FROMQ == 2) flat_n = min(*wk.out_count, wk.out_capacity), items = (flat_n + blockDim.x - 1) / blockDim.x;
    // VMX_SAMPLING_ELIDE_DEAD: the pass's live camera paths only; ray and hit record sit at the list position `src`
    constexpr bool listed = SRC == 0 && ELIDE;
    uint32_t live_n = 0;
    if (listed) {
        live_n = *wk.live_count;
        if (FROMQ == 0) items = (live_n + blockDim.x - 1) / blockDim.x;
    }
    // The dense camera form (every path of the pass, pixel-major ids, a multiple of 64 samples): a wave's 64 paths are 64
    // samples of ONE pixel, and a wave takes a whole PIXEL per iteration, as k_raygen does — active[slot], the pixel's
    // cursor, the pixel half of the stream key and the pixel's sphere bounds (pixel_sphere_bound, lane i = sphere i)
    // once, then the pixel's chunks of 64 samples.  (rayA / hit of a chunk depend on the indices alone, but loading them
    // ahead of that chain holds five registers across the set-up: measured, the kernel then spills its generator state
    // inside the loop and loses the whole gain — profiles/pixel_sphere_bounds.txt — so they are loaded where they are used.)
    // Path ids, the rad_mask word per 64 ids, the sub-queue of an id ((pid >> 8) % kSubQueues) and the tallies are
    // those of the block-item loop, which every other form keeps (one unit = one block item of 256 positions).
    static_assert(!DENSE || (SRC == 0 && FROMQ == 0 && !ELIDE), "the dense form is the plain camera pass");
    static_assert(!CLAIMED || DENSE, "claimed pixels are fused in the dense form only");
    constexpr bool dense = DENSE;  // (launch_shade: wk.pixel_major && wk.samples % 64 == 0)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t chunks = dense ? wk.samples >> 6 : 1u;
    uint32_t n_fused = 0;  // (wave-uniform) camera paths of claimed pixels whose ray was formed and tested here
    uint32_t unit = blockIdx.x, unit_step = gridDim.x, units = items;
    if (dense) {
        unit = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
        // (a pass that fuses its claimed pixels: the listed slots — the unclaimed ones here, the claimed ones in the CLAIMED form)
        unit_step = gridDim.x * (blockDim.x >> 6), units = wk.shade_slots ? *wk.shade_count : wk.n_pad;
    }
    for (; unit < units; unit += unit_step) {
        const uint32_t slot = DENSE ? (wk.shade_slots ? wk.shade_slots[unit] : unit) : unit;
        const bool px_active = dense && slot < wk.n_active;
        uint32_t px_claim = kClaimNone, px_pixel = 0;  // CLAIMED: the pixel's claim and its global index, for the chunks below
        if (px_active) {
            const uint32_t lp = wk.active[slot];
            const uint32_t pixel = global_pixel(fr, lp);
            if (CLAIMED) px_claim = wk.claims[lp], px_pixel = pixel;
            const PixelKey pk = rng_pixel_key(fr.seed, pixel);
            const uint32_t cur = px.cursor[lp];  // (sample_index, with the cursor fetched once)
            // (the terms that depend on the frame or on the lane's sphere alone are formed here, per pixel, on purpose: kept
            // in registers across the loop they would push the shading's own state out to scratch)
            FilmDev fm = {fr.width, fr.height, fr.sensor_x, fr.sensor_y, fr.film_dist};
            uint32_t si = lane;
            asm volatile("" : "+s"(fm.width), "+s"(fm.height), "+s"(fm.sensor_x), "+s"(fm.sensor_y), "+s"(fm.film_dist), "+v"(si));
            si &= kLdsSpheres - 1u;
            const PixelCone cn = pixel_cone(fr, fm, pixel);
            const float4 q = s_cam_op[si];
            const float lm = si < sc.nspheres ? pixel_sphere_bound(cn, q.x, q.y, q.z, q.w, s_geom[si].w) : kInf;
            float lmin = kInf;
            for (uint32_t i = 0; i < sc.nspheres; ++i)
                lmin = fminf(lmin, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lm), (int)i)));
            // parked in the wave's LDS row, not in registers: the kernel sits at its register budget (VMX_SHADE_WPS)
            if (lane < kLdsSpheres) s_lmax[wave][lane] = lm;
            if (lane == 0) {
                s_lmax[wave][kLdsSpheres] = lmin;
                s_pix[wave][0] = cur & ~kCursorStrided, s_pix[wave][1] = (cur & kCursorStrided) ? fr.quarter : 1u;
                s_pix[wave][2] = (uint32_t)pk.a, s_pix[wave][3] = (uint32_t)(pk.a >> 32);
                s_pix[wave][4] = (uint32_t)pk.b, s_pix[wave][5] = (uint32_t)(pk.b >> 32);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        for (uint32_t ch = 0; ch < chunks; ++ch) {
            const uint32_t pos0 = dense ? slot * wk.samples + ch * 64u + lane : unit * blockDim.x + threadIdx.x;
            const uint32_t item = dense ? pos0 >> 8 : unit;  // the block item of these positions (blocks are 256 wide)
            bool run;
            uint32_t pid = 0, src = 0;
            float2 hrec = make_float2(0.f, 0.f);  // FROMQ 2: the hit record came with the list entry
            Path P;
            if (SRC == 0) {
                src = pid = pos0;
                float4 rec0 = make_float4(0.f, 0.f, 0.f, 0.f), rec1 = rec0;
                if (FROMQ == 1) {
                    src = pid = src < flat_n ? wk.flat_ids[src] : 0xFFFFFFFFu;
                    if (listed) live_n = 0xFFFFFFFFu;  // (a listed position is a valid one)
                }
                if (FROMQ == 2) {  // (direction, flag word)(t, leaf slot, position, -); position ~0: padding of a chunk
                    const bool in = src < flat_n;
                    if (in) rec0 = ((const float4 *)wk.out_rec)[(size_t)src * 2], rec1 = ((const float4 *)wk.out_rec)[(size_t)src * 2 + 1];
                    src = pid = in ? __float_as_uint(rec1.z) : 0xFFFFFFFFu;
                    hrec = make_float2(rec1.x, rec1.y);
                    if (listed) live_n = 0xFFFFFFFFu;
                }
                if (listed) pid = src < live_n ? wk.live_ids[src] : 0xFFFFFFFFu;  // (no such path: j >= samples below)
                uint32_t pixel = 0, k = 0, pid2;
                if (dense) {  // (sample_index of the pixel's sample j, from the cursor fetched above)
                    const uint32_t j = ch * 64u + lane;
                    if (px_active) k = (fr.lead != 0 && j >= fr.lead) ? (j - fr.lead + 1u) * fr.quarter : s_pix[wave][0] + j * s_pix[wave][1];
                    run = px_active && k < fr.kmax;
                } else {
                    uint32_t j, s_idx;
                    if (wk.pixel_major) s_idx = fast_div(pid, wk.div_samples), j = pid - s_idx * wk.samples;
                    else j = pid / wk.n_pad, s_idx = pid - j * wk.n_pad;
                    run = j < wk.samples && s_idx < wk.n_pad && primary_item(fr, wk, px, j, s_idx, pid2, pixel, k);
                }
                if (CLAIMED) {
                    // a claimed pixel of a fused pass: the ray is formed here as k_raygen forms it (same function, same
                    // translation unit: bit-equal), which leaves the stream past its two jitter draws, and the pixel's
                    // claim settles its BVH query as the refill branch of k_trace_w<0> does — the claimed triangle's own
                    // test on its camera-relative record (wave-uniform: through the scalar cache), or no hit
                    n_fused += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(run));
                    if (run) {
                        PixelKey pk;
                        pk.a = (uint64_t)s_pix[wave][2] | ((uint64_t)s_pix[wave][3] << 32);
                        pk.b = (uint64_t)s_pix[wave][4] | ((uint64_t)s_pix[wave][5] << 32);
                        P.ox = fr.px, P.oy = fr.py, P.oz = fr.pz, P.depth = 0;
                        primary_ray_keyed(fr, px_pixel, pk, k, P.rng, P.dx, P.dy, P.dz);
                        float best = 999999999.f;
                        int leaf = -1;
                        if (px_claim < kClaimMiss) {  // a slot claim (a listed pixel has a claim: never kClaimNone)
                            typedef float f32x4 __attribute__((ext_vector_type(4)));
                            typedef const __attribute__((address_space(4))) f32x4 *scalar_ptr;
                            const uint32_t claim = (uint32_t)__builtin_amdgcn_readfirstlane((int)px_claim);
                            const scalar_ptr rec = (scalar_ptr)((uintptr_t)wk.cam_tris + (size_t)claim * 64u);
                            const f32x4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                            float dist;
                            if (tri_test_cam(make_float4(r0.x, r0.y, r0.z, r0.w), make_float4(r1.x, r1.y, r1.z, r1.w),
                                             make_float4(r2.x, r2.y, r2.z, r2.w), r3.x, P.dx, P.dy, P.dz, dist) && dist < best)
                                best = dist, leaf = (int)claim;
                        }
                        hrec = make_float2(best, __int_as_float(leaf));
                        P.ar = P.ag = P.ab = 0.f;
                        P.aw = -100.f;  // pathtracer.cpp:29
                        P.tr = P.tg = P.tb = P.tw = 1.f;  // :30
                    }
                } else if (run) {
                    // the ray comes from k_raygen; the stream is re-keyed and its two jitter draws skipped
                    const float4 a = FROMQ == 2 ? rec0 : ((const float4 *)pa.rayA)[src];
                    P.ox = fr.px, P.oy = fr.py, P.oz = fr.pz, P.dx = a.x, P.dy = a.y, P.dz = a.z, P.depth = 0;
                    if (dense) {  // the pixel half of the key: once per pixel
                        PixelKey pk;
                        pk.a = (uint64_t)s_pix[wave][2] | ((uint64_t)s_pix[wave][3] << 32);
                        pk.b = (uint64_t)s_pix[wave][4] | ((uint64_t)s_pix[wave][5] << 32);
                        rng_init_keyed(P.rng, pk, k);
                    } else {
                        rng_init(P.rng, fr.seed, pixel, k);
                    }
                    (void)rng_next(P.rng);
                    (void)rng_next(P.rng);
                    P.ar = P.ag = P.ab = 0.f;
                    P.aw = -100.f;  // pathtracer.cpp:29
                    P.tr = P.tg = P.tb = P.tw = 1.f;  // :30
                }
            } else {
                uint32_t sub = item % kSubQueues, chunk = item / kSubQueues;
                uint32_t pos = chunk * blockDim.x + threadIdx.x;
                if (FROMQ == 1) {  // a listed position = (block item of k_shade_ends) * 256 + lane
                    const uint32_t at = item * blockDim.x + threadIdx.x;
                    run = at < flat_n;
                    const uint32_t p = run ? wk.flat_ids[at] : 0u;
                    sub = (p >> 8) % kSubQueues, chunk = (p >> 8) / kSubQueues, pos = chunk * 256u + (p & 255u);
                } else if (FROMQ == 2) {  // (t, leaf slot, path id, -); path id ~0: padding of a chunk
                    const uint32_t at = item * blockDim.x + threadIdx.x;
                    float4 r = make_float4(0.f, 0.f, __uint_as_float(0xFFFFFFFFu), 0.f);
                    if (at < flat_n) r = ((const float4 *)wk.out_rec)[at];
                    pid = __float_as_uint(r.z);
                    hrec = make_float2(r.x, r.y);
                    run = pid != 0xFFFFFFFFu;
                } else {
                    run = pos < min(wk.qids.counts[sub * 32], wk.qids.sub_capacity);
                }
                if (run) {
                    if (FROMQ != 2) pid = wk.qids.ids[(size_t)sub * wk.qids.sub_capacity + pos];
                    path_load_arrays<TEX, false>(pa, pid, P);  // (accumColour: below, only where the step changes it)
                }
            }
            StepFlags fl = {false, false, false};
            uint32_t depth0 = 0;
            int st = kPathEnded;
            ShadeMid mid;
            CastResult c;
            if (run) {
                P.dest = pid;
                depth0 = P.depth == 0 ? 1u : 0u;
                fl.was_ray = depth0 ? true : finite3(P.dx, P.dy, P.dz);
                const float2 h = (FROMQ == 2 || CLAIMED) ? hrec : hits[SRC == 0 ? src : pid];
                // (the pixel's sphere bounds: the dense camera form only — elsewhere lmax_min < 0, every sphere is evaluated)
                cast_finish<true, SRC == 0, DENSE>(sc, P.ox, P.oy, P.oz, P.dx, P.dy, P.dz, h.x, __float_as_int(h.y), c,
                                                                             s_geom, s_cam_op, s_lmax[wave], dense);
                // A bounce step changes accumColour only by += accumRadiance * hitColour (pathtracer.cpp:43) — nothing when no
                // light coloured the hit (x + t * 0 == x for finite t; the sums are never -0) — and, at depth 0 (explicit rays
                // of vmx_radiance), by its fourth component (:44-47).  Six steps in seven change nothing: their path's
                // 16 bytes of a 64-byte line are neither fetched nor written back (a third of this kernel's HBM traffic).
                bool touch = SRC == 0, had = true;
                if (SRC != 0) {
                    touch = P.depth == 0 || c.cr != 0.f || c.cg != 0.f || c.cb != 0.f;
                    if (TEX) touch = touch || !(finite3(P.tr, P.tg, P.tb) && fabsf(P.tw) < kInf);
                    if (touch) {
                        had = rad_has(pa, pid);
                        const float4 acc = rad_fetch(pa, pid, had);
                        P.ar = acc.x, P.ag = acc.y, P.ab = acc.z, P.aw = acc.w;
                    }
                }
                st = path_shade_begin<TEX>(sc, fr.r2scale, P, c, fl, mid);
                if (SRC != 0) {
                    if (touch) rad_commit(pa, pid, make_float4(P.ar, P.ag, P.ab, P.aw), had);
                } else if (!pa.rad_mask) {
                    rad[pid] = make_float4(P.ar, P.ag, P.ab, P.aw);
                }
            }
            bool alive = st == kPathNextRay;
            // (gathering the block's ~10 % of angles in LDS to evaluate cos/sin in full waves was measured:
            // the three barriers it needs cost what it saves)
            if (st == kPathNeedsTrig) {
                float sn, cs;
                shade_trig(mid, fr.libm_double, cs, sn);
                alive = path_shade_end(P, c, fl, mid, cs, sn);
            }
            if (ELIDE && alive &&
                step_is_dead<TEX>(sc, fr.r2scale, P.rng, P.depth, P.ox, P.oy, P.oz, P.dx, P.dy, P.dz, P.tr, P.tg, P.tb))
                alive = false, fl.continues = false;  // VMX_SAMPLING_ELIDE_DEAD: the next ray cannot change the path's colour
            if (alive) {
                uint32_t bits = 0;
                if (fr.bounce_bits) bits = step_bits<TEX>(sc, fr.r2scale, P.rng, P.depth, P.ox, P.oy, P.oz, P.dx, P.dy, P.dz, P.tr, P.tg, P.tb);
                ray_store(pa, pid, P, bits);
                rng_store(pa, pid, P.rng);
                if (TEX) ((float4 *)pa.thr)[pid] = make_float4(P.tr, P.tg, P.tb, P.tw);
            }
            if (SRC == 0 && pa.rad_mask) {
                // camera paths: most end at their first hit with accumColour.rgb == 0 (no light sphere hit): nothing to store
                // for them, k_resolve adds +0 (x + 0 == x bit for bit; the sums are never -0).  A wave's 64 paths are one
                // aligned word of the mask (path ids of an item are consecutive, 256 per block)
                // (a path that goes on black stores nothing either: the step that colours it later sets its bit, rad_commit)
                const bool need = run && (P.ar != 0.f || P.ag != 0.f || P.ab != 0.f);
                if (need) rad[pid] = make_float4(P.ar, P.ag, P.ab, P.aw);
                if (listed || FROMQ != 0) {  // the mask was cleared for the pass / written by k_shade_ends; neighbours share words
                    if (need) atomicOr(&pa.rad_mask[pid >> 6], 1ull << (pid & 63u));
                } else {
                    // (a pass that fuses its claimed pixels walks lists of slots below n_active: the words of its padding slots
                    // keep what an earlier pass left, which nothing reads — k_resolve takes the slots below n_active only)
                    const unsigned long long word = __builtin_amdgcn_ballot_w64(need);
                    if (lane == 0) pa.rad_mask[pos0 >> 6] = word;
                }
            }
            tally_add(tl, fl, run, depth0);
            id_append(qout, item % kSubQueues, alive, pid);
        }
    }
    const Cnt none = {0, 0};
    tally_flush<false>(ctr, tl, none, none);
    if (CLAIMED && lane == 0 && n_fused) atomicAdd(&ctr->fused, (unsigned long long)n_fused);
}

// ---------------------------------------------------------------------------
// k_shade_ends — first phase of the two-phase shading of a frame's split passes.  Under the reference's sampling four
// Radiance steps in five are the path's last one because of the path's own draws (Russian roulette :56; r2 = 10 U > 1,
// :156 / :170, where the hit's material flag — "the BVH hit a triangle", meshEngine.cpp:370 — picks the draw).  All
// such a step does is accumColour += accumRadiance * hitColour (:43): neither the hit's normal, nor its uv, nor the
// nearest distance is ever read.  And hitColour is decided by the sphere table's entries up to the last light
// (SceneDev::emit_prefix; `testHit < nearestHit` in table order, meshEngine.cpp:377-420).  This kernel takes every
// path of the generation, finishes those steps with exactly that — no attribute gather, no interpolation, 2 sphere
// tests instead of 8 with the reference's table — and marks the others (one bit per position; launch_live_compact
// makes the ordered list of them) for k_shade, which then runs in dense waves.  Same colours, same counters.
// (k_shade alone does the same work with four lanes in five idle behind the branch: 13.1 ms against 3.9 + 4 here
// for the 530.8 M camera paths of the bench frame.)
//   SRC 0: camera paths; the two "ends" bits come with the ray record (k_raygen: step_bits)
//   SRC 1: queued bounce paths; the draws are read off a copy of the path's stream
//   LISTED (SRC 0, VMX_SAMPLING_ELIDE_DEAD): the pass's live-path list instead of all its path ids
// ---------------------------------------------------------------------------
template <int SRC, bool TEX, bool LISTED>
__global__ void __launch_bounds__(256)
k_shade_ends(SceneDev sc, FrameDev fr, WorkDev wk, PathArrays pa, unsigned long long *__restrict__ full_mask,
             unsigned int *__restrict__ full_cnt, uint32_t max_chunks, DevCounters *ctr) {
    const float2 *__restrict__ hits = (const float2 *)pa.hit;
    float4 *__restrict__ rad = (float4 *)pa.rad;
    __shared__ float4 s_geom[kLdsSpheres];
    __shared__ float4 s_cam_op[kLdsSpheres];
    __shared__ float4 s_col[kLdsSpheres];  // (colour, emits)
    const uint32_t nlight = min(sc.emit_prefix, kLdsSpheres);
    if (threadIdx.x < nlight) {
        const SphereDev &q = sc.spheres[threadIdx.x];
        s_geom[threadIdx.x] = make_float4(q.cx, q.cy, q.cz, q.rad2);
        const float opx = q.cx - fr.px, opy = q.cy - fr.py, opz = q.cz - fr.pz;
        s_cam_op[threadIdx.x] = make_float4(opx, opy, opz, dot3(opx, opy, opz, opx, opy, opz));
        s_col[threadIdx.x] = make_float4(q.colr, q.colg, q.colb, (q.flags & 1u) ? 1.f : 0.f);
    }
    __syncthreads();
    Tally tl = {{0, 0}, {0, 0}, {0, 0}};
    uint32_t items = SRC == 0 ? (wk.samples * wk.n_pad + blockDim.x - 1) / blockDim.x : max_chunks * kSubQueues;
    uint32_t live_n = 0;
    if (LISTED) live_n = *wk.live_count, items = (live_n + blockDim.x - 1) / blockDim.x;
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        bool run, ends = false, material = false;
        uint32_t pid = 0, src = 0, depth = 0;
        float ox = fr.px, oy = fr.py, oz = fr.pz, dx = 0.f, dy = 0.f, dz = 0.f, best = 0.f;
        float tr = 1.f, tg = 1.f, tb = 1.f;
        if (SRC == 0) {
            src = pid = item * blockDim.x + threadIdx.x;
            run = LISTED ? src < live_n : src < wk.samples * wk.n_pad;
            if (run) {
                if (LISTED) pid = wk.live_ids[src];
                const float4 a = ((const float4 *)pa.rayA)[src];
                const uint32_t bits = __float_as_uint(a.w);
                run = bits != 0xFFFFFFFFu;  // a slot without a sample
                const float2 h = hits[src];
                dx = a.x, dy = a.y, dz = a.z, best = h.x;
                material = __float_as_int(h.y) >= 0;
                ends = ((material ? bits : bits >> 1) & 1u) != 0;
            }
        } else {
            const uint32_t sub = item % kSubQueues, chunk = item / kSubQueues;
            const uint32_t pos = chunk * blockDim.x + threadIdx.x;
            run = pos < min(wk.qids.counts[sub * 32], wk.qids.sub_capacity);
            if (run) {
                src = pid = wk.qids.ids[(size_t)sub * wk.qids.sub_capacity + pos];
                Path P;
                ray_load(pa, pid, P);
                Rng r;
                rng_load(pa, pid, r);
                ox = P.ox, oy = P.oy, oz = P.oz, dx = P.dx, dy = P.dy, dz = P.dz, depth = P.depth;
                const float2 h = hits[pid];
                best = h.x;
                material = __float_as_int(h.y) >= 0;
                // the draws of this step, in path_shade_begin's order
                bool rr_end = false;
                if (depth + 1u > 5u) {
                    const double rr = rng_u01(r);
                    rr_end = rr > (double)0.95f || depth + 1u > 1000u;
                }
                if (material) {
                    const double a = rng_u01(r);
                    (void)rng_next(r);
                    const double c = rng_u01(r);
                    ends = !(a >= 0.96) && (1.0f - (float)((double)fr.r2scale * c)) < 0.0f;
                } else {
                    (void)rng_next(r);
                    const double b = rng_u01(r);
                    ends = (1.0 - (double)fr.r2scale * b) < 0.0;
                }
                ends = ends || rr_end;
                if (TEX) {
                    const float4 th = ((const float4 *)pa.thr)[pid];
                    tr = th.x, tg = th.y, tb = th.z;
                    if (!finite3(tr, tg, tb)) ends = false;  // inf * 0: leave the step to k_shade
                }
            }
        }
        const bool fin = run && ends;
        // hitColour of the ending steps: the sphere table up to its last light, `testHit > 0 && testHit < nearestHit` in order
        float cr = 0.f, cg = 0.f, cb = 0.f;
        if (__builtin_amdgcn_ballot_w64(fin) != 0) {
            float nearest = material ? best : kInf;
            for (uint32_t i = 0; i < nlight; ++i) {
                float th;
                if (SRC == 0) {
                    const float4 q = s_cam_op[i];
                    th = sphere_hit_op(q.x, q.y, q.z, q.w, s_geom[i].w, dx, dy, dz, nearest);
                } else {
                    th = sphere_hit(ox, oy, oz, dx, dy, dz, s_geom[i], nearest);
                }
                if (fin && th > 0.f && th < nearest) {
                    nearest = th;
                    const float4 col = s_col[i];
                    if (col.w != 0.f) cr = col.x, cg = col.y, cb = col.z;
                }
            }
        }
        const bool lit = fin && (cr != 0.f || cg != 0.f || cb != 0.f);
        if (SRC == 0) {
            // accumColour = 0 + 1 * hitColour; stored only where it is not zero (PathArrays::rad_mask)
            if (lit) rad[pid] = make_float4(0.f + tr * cr, 0.f + tg * cg, 0.f + tb * cb, -100.f);
            if (LISTED) {  // the mask was cleared for the pass
                if (lit) atomicOr(&pa.rad_mask[pid >> 6], 1ull << (pid & 63u));
            } else {       // this wave's 64 path ids are one word; k_shade ORs the bits of its paths in afterwards
                const unsigned long long word = __builtin_amdgcn_ballot_w64(lit);
                if ((threadIdx.x & 63u) == 0 && src < wk.samples * wk.n_pad) pa.rad_mask[src >> 6] = word;
            }
        } else if (lit) {
            const bool had = rad_has(pa, pid);
            float4 acc = rad_fetch(pa, pid, had);
            if (TEX) acc.x = acc.x + tr * cr, acc.y = acc.y + tg * cg, acc.z = acc.z + tb * cb;
            else acc.x = acc.x + cr, acc.y = acc.y + cg, acc.z = acc.z + cb;
            rad_commit(pa, pid, acc, had);
        }
        StepFlags fl = {false, false, false};
        fl.was_ray = depth == 0u ? true : finite3(dx, dy, dz);
        fl.tri_hit = material;
        tally_add(tl, fl, fin, depth == 0u ? 1u : 0u);
        // the others: one word of bits per wave (position = block item * 256 + lane), compacted in order afterwards
        const unsigned long long full = __builtin_amdgcn_ballot_w64(run && !ends);
        if ((threadIdx.x & 63u) == 0) {
            const uint32_t w = item * (blockDim.x >> 6) + (threadIdx.x >> 6);
            full_mask[w] = full, full_cnt[w] = (uint32_t)__popcll(full);
        }
    }
    const Cnt none = {0, 0};
    tally_flush<false>(ctr, tl, none, none);
}

// explicit camera rays for vmx_radiance (split wavefront): path i keyed (seed, i, 0), jitter draws skipped
__global__ void k_radiance_init_ids(const float *__restrict__ o, const float *__restrict__ d, uint32_t n,
                                    uint64_t seed, PathArrays pa, IdQueue qout) {
    for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
        const uint32_t i = base + threadIdx.x;
        const bool run = i < n;
        if (run) {
            Path P;
            rng_init(P.rng, seed, i, 0);
            (void)rng_next(P.rng);
            (void)rng_next(P.rng);
            P.ox = o[i * 3], P.oy = o[i * 3 + 1], P.oz = o[i * 3 + 2];
            P.dx = d[i * 3], P.dy = d[i * 3 + 1], P.dz = d[i * 3 + 2];
            P.depth = 0;
            ray_store(pa, i, P);
            rng_store(pa, i, P.rng);
            ((float4 *)pa.rad)[i] = make_float4(0.f, 0.f, 0.f, -100.f);
            if (pa.thr) ((float4 *)pa.thr)[i] = make_float4(1.f, 1.f, 1.f, 1.f);
        }
        id_append(qout, (base / blockDim.x) % kSubQueues, run, i);
    }
}

// the pixel write (pathtracer.cpp:318-324) from a pixel's sums and sample count: what k_resolve stores for a finished
// pixel and k_preview (vmx_preview.inc) shows for an unfinished one
__device__ __forceinline__ void resolved_pixel(const float4 &acc, uint32_t n, float *o5) {
    const float fn = (float)n;  // accum / nTotalSamples (uint -> float)
    // std::max(std::min(x, 1.f), 0.f) (pathtracer.cpp:318-320): std::min(a, b) is (b < a) ? b : a, so a NaN mean —
    // an infinite throughput times a black hit, possible with a texture that holds an infinity — stays NaN
    // (fminf / fmaxf would return the other operand: found by tools/fuzz_parity.py's random textures, round 3)
    const float mx = acc.x / fn, my = acc.y / fn, mz = acc.z / fn;
    const float cx = 1.f < mx ? 1.f : mx, cy = 1.f < my ? 1.f : my, cz = 1.f < mz ? 1.f : mz;
    o5[0] = cx < 0.f ? 0.f : cx;
    o5[1] = cy < 0.f ? 0.f : cy;
    o5[2] = cz < 0.f ? 0.f : cz;
    o5[3] = 1.f;
    o5[4] = fn;
}

// per-pixel accumulation in sample order + early stop + pixel write (pathtracer.cpp:282-324)
// MOMENTS (a vmx_progressive handle begun with VMX_PROGRESSIVE_MOMENTS): accum.w carries the sum of the squared luminance of
// the samples taken, folded right after the colour — a path the radiance mask marks as not stored adds an exact +0 there
// too.  <false> is the kernel as it was.
template <bool MOMENTS>
__global__ void k_resolve(FrameDev fr, const unsigned int *__restrict__ active, uint32_t n_active,
                          uint32_t n_pad, uint32_t samples, uint32_t pixel_major, const float4 *__restrict__ rad,
                          const unsigned long long *__restrict__ rad_mask, PixelStateDev px,
                          unsigned int *__restrict__ next_active, unsigned int *next_count,
                          float *__restrict__ out, DevCounters *ctr) {
    __shared__ unsigned int s_keep, s_base, s_taken, s_disc, s_done, s_brk;
    if (threadIdx.x == 0) s_keep = 0, s_taken = 0, s_disc = 0, s_done = 0, s_brk = 0;
    __syncthreads();
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    uint32_t lp = 0, taken = 0, disc = 0, done = 0, brk = 0;
    if (slot < n_active) {
        lp = active[slot];
        float4 acc = ((float4 *)px.accum)[lp];
        uint32_t n = px.count[lp];
        const uint32_t craw = px.cursor[lp];
        const uint32_t cursor = craw & ~kCursorStrided;
        // strided: this pass's paths are the first samples of the following strata (sample_index)
        const bool strided = (craw & kCursorStrided) != 0;
        const uint32_t stride = strided ? fr.quarter : 1u;
        uint32_t next = cursor + samples * stride;
        bool flag = strided;  // still in a run of early stops unless a sample says otherwise
        // samples are taken strictly in order (float sums, early stop), but their loads need not
        // wait for each other: fetch 8 at a time (pixel-major: one 128-byte line per lane)
        constexpr uint32_t kChunk = 8;
        const size_t total = (size_t)n_pad * samples;
        bool stop = false;
        for (uint32_t j0 = 0; j0 < samples && !stop; j0 += kChunk) {
            float4 buf[kChunk];
            // rad_mask (split pipeline, pixel-major ids): one bit per path says whether its radiance was stored at all;
            // the others ended black at their first hit and count as an exact zero
            unsigned long long w0 = ~0ull, w1 = ~0ull;
            const size_t pid0 = (size_t)slot * samples + j0;
            if (rad_mask) {
                w0 = rad_mask[pid0 >> 6];
                w1 = rad_mask[min(pid0 + kChunk - 1, total - 1) >> 6];
            }
#pragma unroll
            for (uint32_t i = 0; i < kChunk; ++i) {
                const uint32_t j = j0 + i;
                size_t idx = pixel_major ? (size_t)slot * samples + j : (size_t)j * n_pad + slot;
                bool stored = true;
                if (j >= samples || idx >= total) idx = (size_t)slot, stored = false;  // any valid address; value unused
                if (rad_mask) {
                    const size_t pid = pid0 + i;
                    stored = stored && ((((pid >> 6) == (pid0 >> 6) ? w0 : w1) >> (pid & 63)) & 1ull) != 0;
                }
                buf[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (stored) buf[i] = rad[idx];
            }
#pragma unroll
            for (uint32_t i = 0; i < kChunk; ++i) {
                const uint32_t j = j0 + i;
                const bool lead_tail = fr.lead != 0 && j >= fr.lead;  // a following stratum's first sample
                const uint32_t k = lead_tail ? (j - fr.lead + 1u) * fr.quarter : cursor + j * stride;
                if (stop || j >= samples || k >= fr.kmax) {
                    stop = true;
                    continue;
                }
                const float4 s = buf[i];
                ++n;  // :249
                acc.x = acc.x + s.x;  // :283
                acc.y = acc.y + s.y;
                acc.z = acc.z + s.z;
                if (MOMENTS) {
                    const float l = luminance(s.x, s.y, s.z);
                    acc.w = acc.w + l * l;
                }
                ++taken;
                bool early = false;
                if (fr.early_stop && n > fr.nmin) {  // n > sqrt(spp), :292
                    const float fn = (float)n, fn1 = (float)(n + 1);
                    const float ex = acc.x / fn - (acc.x + s.x) / fn1;
                    const float ey = acc.y / fn - (acc.y + s.y) / fn1;
                    const float ez = acc.z / fn - (acc.z + s.z) / fn1;
                    early = fabsf(sqrtf(dot3(ex, ey, ez, ex, ey, ez))) < 0.00001f;
                }
                // number of this pass's paths that come after sample j
                uint32_t later = samples - 1u - j;
                if (fr.lead != 0) {
                    const uint32_t strata_after = fr.kmax / fr.quarter - 1u;
                    const uint32_t valid = fr.lead + (samples - fr.lead < strata_after ? samples - fr.lead : strata_after);
                    later = valid - 1u - j;
                } else if (cursor + (samples - 1u) * stride >= fr.kmax) {
                    later = (fr.kmax - 1u - k) / stride;
                }
                const bool strided_now = strided || lead_tail;
                const bool lead_last = fr.lead != 0 && j + 1u == fr.lead;  // the first sample the rule can stop
                if (early) {
                    brk = 1;
                    next = (k / fr.quarter + 1u) * fr.quarter;  // break the innermost loop only
                    flag = true;
                    // consecutive samples that follow in this pass are not taken — except that a lead
                    // pass goes on with the next strata's first samples, which are exactly what is due
                    if (!strided_now && !lead_last) {
                        disc = later;
                        stop = true;
                    }
                } else if (strided_now || lead_last) {
                    // this stratum goes on with sample k + 1; the later strata were not due yet
                    next = k + 1u;
                    flag = false;
                    disc = later;
                    stop = true;
                }
            }
        }
        if (next >= fr.kmax) {
            resolved_pixel(acc, n, out + (size_t)lp * 5);
            done = 1;
        } else {
            keep = true;
        }
        ((float4 *)px.accum)[lp] = acc;
        px.count[lp] = n;
        px.cursor[lp] = next | ((flag && next < fr.kmax) ? kCursorStrided : 0u);
    }
    // block-aggregated append to the next active list
    uint32_t my = 0;
    if (keep) my = atomicAdd(&s_keep, 1u);
    if (taken) atomicAdd(&s_taken, taken);
    if (disc) atomicAdd(&s_disc, disc);
    if (done) atomicAdd(&s_done, 1u);
    if (brk) atomicAdd(&s_brk, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        s_base = s_keep ? atomicAdd(next_count, s_keep) : 0u;
        if (s_brk) atomicAdd(next_count + 1, s_brk);
        if (s_taken) atomicAdd(&ctr->samples, (unsigned long long)s_taken);
        if (s_disc) atomicAdd(&ctr->discarded, (unsigned long long)s_disc);
        if (s_done) atomicAdd(&ctr->pixels_done, (unsigned long long)s_done);
    }
    __syncthreads();
    if (keep) next_active[s_base + my] = lp;
}

// ---------------------------------------------------------------------------
// k_bruteforce / k_bruteforce_long — BruteForceTracer::Render (core/integrators/integrators.cpp:9-186), the
// engine's default integrator: the reference's sample loop — jittered camera ray (:65-81), RayCast, N.L against
// the point light (:83-88), normal perturbation by boundTextures[0] (:98-106), the mirror probe (:119-137),
// albedo (:141-156), the convergence break (:166-172) — and the pixel write (:176-183).  Jitters come from the
// stream keyed (seed, pixel, sample) (the reference shares one unsynchronised std::mt19937, :30), so a sample is
// a function of (pixel, sample index) alone (bf_sample) and only the running sums and the break are sequential
// (bf_fold).  Most pixels break after 3 samples, a few run to the last one: with one lane per pixel those few
// set the frame time (186 ms at 256 spp, of which 25 ms is work).  So k_bruteforce (one lane per pixel, 8x8-pixel
// tiles: coherent waves) takes the first kBfShort samples of every pixel and hands the pixels that have not
// broken by then — with their sums — to k_bruteforce_long, where a WAVE takes a pixel: its 64 lanes evaluate 64
// consecutive samples at once, lane 0 folds them in order, and the samples past the break are dropped.
// ---------------------------------------------------------------------------
struct BfSample {
    float cx, cy, cz, dist;
    uint32_t flags;  // 1: the camera ray hit something, 2: a triangle, 4: the mirror probe was a ray (finite direction)
};
struct BfState {
    float ax, ay, az, aw;  // accum
    float lx, ly, lz, lw;  // lastSampleColour
    float dist;            // hitDistance of the last sample
    uint32_t n;            // samples taken
    uint32_t prim, sec, hits;
};
constexpr uint32_t kBfShort = 8;

__device__ __forceinline__ BfSample bf_sample(const SceneDev &sc, const FrameDev &fr, uint32_t p, uint32_t sample,
                                              uint2 *stk, uint2 *ovf, int lds_entries, Cnt &cnt) {
    BfSample r = {0.f, 0.f, 0.f, 0.f, 0u};
    Rng rng;
    rng_init(rng, fr.seed, p, sample);
    const float jx = rng_jitter(rng), jy = rng_jitter(rng);
    const float hX = (float)((((double)((float)(p % fr.width) + jx) - 0.25) / (double)fr.width) * 2.0 - 1.0);   // :65
    const float hY = (float)((((double)((float)(p / fr.width) + jy) - 0.25) / (double)fr.height) * 2.0 - 1.0);  // :66
    const float bx = (float)((double)(hX * fr.sensor_x) * 0.5), by = (float)((double)(hY * fr.sensor_y) * 0.5);  // :73-74
    const float gx = bx, gy = -by, gz = -fr.film_dist;  // :76
    float dx = (fr.m[0] * gx + fr.m[3] * gy) + (fr.m[6] * gz + 0.0f);  // :79, GLM mat4*vec4 order
    float dy = (fr.m[1] * gx + fr.m[4] * gy) + (fr.m[7] * gz + 0.0f);
    float dz = (fr.m[2] * gx + fr.m[5] * gy) + (fr.m[8] * gz + 0.0f);
    normalize3(dx, dy, dz);  // :81 (w == 1)
    CastResult c;
    ray_cast<false>(sc, fr.px, fr.py, fr.pz, dx, dy, dz, stk, c, cnt, ovf, lds_entries);
    r.dist = c.nearest;  // *pHitDistance (meshEngine.cpp:507)
    if (c.nearest < kInf) {
        r.flags = 1u | (c.slot >= 0 ? 2u : 0u);
        const float hx = fr.px + (dx * c.nearest), hy = fr.py + (dy * c.nearest), hz = fr.pz + (dz * c.nearest);
        float nx = c.nx, ny = c.ny, nz = c.nz;
        float Lx = 500.f - hx, Ly = 1100.f - hy, Lz = 2000.f - hz;  // :16,83
        normalize3(Lx, Ly, Lz);                                     // :84
        float unx = nx, uny = ny, unz = nz;
        normalize3(unx, uny, unz);
        float vNDL = dot3(Lx, Ly, Lz, unx, uny, unz);  // :88
        if (sc.tex) {                                   // :98-106
            const float4 t = tex_sample(sc, c.uvx, c.uvy);
            nx = nx + t.x, ny = ny + t.y, nz = nz + t.z;
            unx = nx, uny = ny, unz = nz;
            normalize3(unx, uny, unz);
            vNDL = dot3(Lx, Ly, Lz, unx, uny, unz);
        }
        // :119  -L - 2.f * N * dot(N, -L)
        const float mLx = -Lx, mLy = -Ly, mLz = -Lz;
        const float k = dot3(nx, ny, nz, mLx, mLy, mLz);
        const float sx = mLx - (2.f * nx) * k, sy = mLy - (2.f * ny) * k, sz = mLz - (2.f * nz) * k;
        if (finite3(sx, sy, sz)) r.flags |= 4u;
        // :121 — the probe's RayCast is only asked WHETHER it hit (:133).  RayCast returns nearest < INFINITY
        // (meshEngine.cpp:508), which is true iff the BVH query hit or some sphere of the table gave 0 < t < inf
        // (:378 with nearest still infinite) — whatever the order.  The spheres are asked first: inside the reference's
        // room (six 5e7-radius wall spheres) every probe with a finite direction hits one, and the BVH traversal —
        // half of this integrator's rays, the incoherent half — is only run for the probes that hit no sphere.
        bool probe_hit = false;
        for (uint32_t i = 0; i < sc.nspheres && !probe_hit; ++i) {
            const SphereDev &q = sc.spheres[i];
            const float th = sphere_hit(hx, hy, hz, sx, sy, sz, make_float4(q.cx, q.cy, q.cz, q.rad2), kInf);
            probe_hit = th > 0.f && th < kInf;
        }
        if (!probe_hit) {
            float best2;
            int slot2;
            bvh_nearest<false>(sc, hx, hy, hz, sx, sy, sz, stk, best2, slot2, cnt, ovf, lds_entries);
            probe_hit = slot2 >= 0;
        }
        if (!probe_hit) {                                            // :133-137
            vNDL = vNDL * 0.9f;
            vNDL = vNDL + 0.1f;
        }
        if (sc.tex1) {  // :141-147
            const float4 t = tex_sample_of(sc.tex1, sc.tex1_w, sc.tex1_h, sc.tex1_c, c.uvx, c.uvy);
            r.cx = t.x * vNDL, r.cy = t.y * vNDL, r.cz = t.z * vNDL;
        } else {  // :148-156
            r.cx = 0.890196078f * vNDL, r.cy = 0.258823529f * vNDL, r.cz = 0.203921569f * vNDL;
        }
    }
    return r;
}

// the sequential part of the sample loop (:59,158-173) for one sample; true = the convergence break fired
__device__ __forceinline__ bool bf_fold(BfState &st, const BfSample &r, uint32_t flags) {
    ++st.n;
    ++st.prim;
    st.dist = r.dist;
    if (r.flags & 1u) {
        if (r.flags & 2u) ++st.hits;
        if (r.flags & 4u) ++st.sec;
        st.ax = st.ax + r.cx, st.ay = st.ay + r.cy, st.az = st.az + r.cz, st.aw = st.aw + 1.0f;  // :158 (cw = 1)
    }
    const float fn = (float)st.n;
    if (st.n > 2) {  // :167-172
        st.lx = st.lx - st.ax / fn, st.ly = st.ly - st.ay / fn, st.lz = st.lz - st.az / fn, st.lw = st.lw - st.aw / fn;
        const float sum = ((st.lx + st.ly) + st.lz) + st.lw;
        float mag;
        if (flags & 1u) {  // VMX_BF_ABS_INT: abs(int), the float truncated to int first
            const double tr = trunc((double)sum);
            mag = (tr >= -2147483648.0 && tr <= 2147483647.0) ? (float)abs((int)tr) : 0.f;
        } else {
            mag = fabsf(sum);
        }
        if (mag < 0.001f) return true;
    }
    st.lx = st.ax / fn, st.ly = st.ay / fn, st.lz = st.az / fn, st.lw = st.aw / fn;  // :173
    return false;
}

__device__ __forceinline__ void bf_write_pixel(const BfState &st, float *__restrict__ out, uint32_t lp) {
    const float fn = (float)st.n;
    float *o5 = out + (size_t)lp * 5;  // :176-183
    o5[0] = sel_max(sel_min(st.ax / fn, 1.f), 0.f);  // std::max(std::min(x, 1.f), 0.f), NaN and all
    o5[1] = sel_max(sel_min(st.ay / fn, 1.f), 0.f);
    o5[2] = sel_max(sel_min(st.az / fn, 1.f), 0.f);
    o5[3] = st.aw / fn;
    o5[4] = st.dist;
}

// a pixel handed from k_bruteforce to k_bruteforce_long: 16 dwords
struct BfLong {
    uint32_t lp, n;
    float ax, ay, az, aw, lx, ly, lz, lw, dist;
    uint32_t pad[5];
};

__global__ void __launch_bounds__(256)
k_bruteforce(SceneDev sc, FrameDev fr, const unsigned int *__restrict__ order, uint32_t npix, uint32_t flags,
             float *__restrict__ out, DevCounters *ctr, BfLong *__restrict__ longs, unsigned int *long_count,
             uint32_t lds_levels, uint32_t overflow_entries, void *overflow_stack) {
    // (stack: lds_levels per lane in LDS, deeper entries in the global slab, as in the traversal kernels — the
    // whole stack in LDS leaves room for 3 waves per SIMD)
    extern __shared__ uint2 lds_stack[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int lds_entries = (int)lds_levels;
    uint2 *stk = lds_stack + (size_t)wave * (lds_levels + 1) * 64 + lane;
    uint2 *ovf = (uint2 *)overflow_stack + ((size_t)(blockIdx.x * (blockDim.x >> 6) + wave) * overflow_entries) * 64 + lane;
    Cnt cnt = {0, 0};
    uint32_t n_prim = 0, n_sec = 0, n_hits = 0, n_samples = 0;
    const uint32_t cap = min(fr.spp, kBfShort);
    for (uint32_t base = blockIdx.x * blockDim.x; base < npix; base += gridDim.x * blockDim.x) {
        const uint32_t i = base + threadIdx.x;
        if (i >= npix) continue;
        const uint32_t lp = order[i];
        const uint32_t p = global_pixel(fr, lp);
        BfState st = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0u, 0u, 0u, 0u};
        bool broke = false;
        for (uint32_t sample = 0; sample < cap && !broke; ++sample)  // :59
            broke = bf_fold(st, bf_sample(sc, fr, p, sample, stk, ovf, lds_entries, cnt), flags);
        n_prim += st.prim, n_sec += st.sec, n_hits += st.hits;
        if (broke || st.n >= fr.spp) {
            n_samples += st.n;
            bf_write_pixel(st, out, lp);
        } else {  // not converged yet: a wave of k_bruteforce_long goes on from here
            const uint32_t at = atomicAdd(long_count, 1u);
            BfLong rec = {lp, st.n, st.ax, st.ay, st.az, st.aw, st.lx, st.ly, st.lz, st.lw, st.dist, {0, 0, 0, 0, 0}};
            longs[at] = rec;
        }
    }
    const uint32_t wp = wave_sum(n_prim), ws = wave_sum(n_sec), wh = wave_sum(n_hits), wn = wave_sum(n_samples);
    if (lane == 0) {
        if (wp) atomicAdd(&ctr->stage[0].rays, (unsigned long long)wp);
        if (ws) atomicAdd(&ctr->stage[1].rays, (unsigned long long)ws);
        if (wh) atomicAdd(&ctr->stage[0].tri_hits, (unsigned long long)wh);
        if (wn) atomicAdd(&ctr->samples, (unsigned long long)wn);
    }
}

__global__ void __launch_bounds__(256)
k_bruteforce_long(SceneDev sc, FrameDev fr, uint32_t flags, float *__restrict__ out, DevCounters *ctr,
                  const BfLong *__restrict__ longs, const unsigned int *long_count, uint32_t lds_levels,
                  uint32_t overflow_entries, void *overflow_stack) {
    extern __shared__ uint2 lds_stack[];
    __shared__ BfSample s_res[4][64];
    __shared__ uint32_t s_stop[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int lds_entries = (int)lds_levels;
    uint2 *stk = lds_stack + (size_t)wave * (lds_levels + 1) * 64 + lane;
    uint2 *ovf = (uint2 *)overflow_stack + ((size_t)(blockIdx.x * (blockDim.x >> 6) + wave) * overflow_entries) * 64 + lane;
    Cnt cnt = {0, 0};
    const uint32_t total = *long_count, waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t e = blockIdx.x * (blockDim.x >> 6) + wave; e < total; e += waves) {
        const BfLong rec = longs[e];
        const uint32_t p = global_pixel(fr, rec.lp);
        BfState st = {rec.ax, rec.ay, rec.az, rec.aw, rec.lx, rec.ly, rec.lz, rec.lw, rec.dist, rec.n, 0u, 0u, 0u};
        uint32_t next = rec.n;  // the next sample index (= samples taken so far)
        bool broke = false;
        while (!broke && next < fr.spp) {
            const uint32_t count = min(64u, fr.spp - next);
            if (lane < count) s_res[wave][lane] = bf_sample(sc, fr, p, next + lane, stk, ovf, lds_entries, cnt);
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            if (lane == 0) {
                uint32_t j = 0;
                for (; j < count && !broke; ++j) broke = bf_fold(st, s_res[wave][j], flags);
                s_stop[wave] = broke ? 1u : 0u;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            broke = s_stop[wave] != 0u;
            next += count;
        }
        if (lane == 0) {
            bf_write_pixel(st, out, rec.lp);
            if (st.prim) atomicAdd(&ctr->stage[0].rays, (unsigned long long)st.prim);
            if (st.sec) atomicAdd(&ctr->stage[1].rays, (unsigned long long)st.sec);
            if (st.hits) atomicAdd(&ctr->stage[0].tri_hits, (unsigned long long)st.hits);
            atomicAdd(&ctr->samples, (unsigned long long)st.n);
        }
    }
}


__global__ void k_assemble(const float *__restrict__ gathered, uint64_t rank_stride, uint32_t width,
                           uint32_t height, uint32_t stripe_rows, uint32_t world, float *__restrict__ frame) {
    const uint64_t total = (uint64_t)width * height * 5;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t)(i / ((uint64_t)width * 5));
        const uint64_t in_row = i - (uint64_t)row * width * 5;
        const uint32_t gs = row / stripe_rows, r = row - gs * stripe_rows;
        const uint32_t rank = gs % world, ls = gs / world;
        const uint64_t lrow = (uint64_t)ls * stripe_rows + r;
        frame[i] = gathered[rank * rank_stride + lrow * width * 5 + in_row];
    }
}

// Camera::saveFrame's conversion (camera.cpp:159-162) of one pixel: floor(x*255) -> u8
__device__ __forceinline__ uchar4 quantized_pixel(const float *f) {
    uchar4 o;
    o.x = (unsigned char)floorf(f[0] * 255.0f);
    o.y = (unsigned char)floorf(f[1] * 255.0f);
    o.z = (unsigned char)floorf(f[2] * 255.0f);
    o.w = (unsigned char)floorf(f[3] * 255.0f);
    return o;
}

// Camera::saveFrame's conversion loop (camera.cpp:159-163): floor(x*255) -> u8, depth plane
__global__ void k_quantize(const float *__restrict__ frame, uint64_t npix, uchar4 *__restrict__ rgba8,
                           float *__restrict__ depth) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (uint64_t)gridDim.x * blockDim.x) {
        const float *f = frame + p * 5;
        rgba8[p] = quantized_pixel(f);
        if (depth) depth[p] = f[4];
    }
}

inline int launch_status() { return (int)hipGetLastError(); }

}  // namespace

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
int launch_trace(const SceneDev &sc, const float *o, const float *d, uint32_t n, int32_t *tri_id, float *t,
                 DevCounters *counters, bool count, LaunchCfg cfg, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (count)
        hipLaunchKernelGGL(k_trace<true>, dim3(cfg.grid), dim3(cfg.block), cfg.lds_bytes, s, sc, o, d, n, tri_id, t,
                           counters);
    else
        hipLaunchKernelGGL(k_trace<false>, dim3(cfg.grid), dim3(cfg.block), cfg.lds_bytes, s, sc, o, d, n, tri_id, t,
                           counters);
    return launch_status();
}

int launch_raycast(const SceneDev &sc, const float *o, const float *d, uint32_t n, void *out, LaunchCfg cfg,
                   void *stream) {
    hipLaunchKernelGGL(k_raycast, dim3(cfg.grid), dim3(cfg.block), cfg.lds_bytes, (hipStream_t)stream, sc, o, d, n,
                       (float4 *)out);
    return launch_status();
}

int launch_primary_ids(const SceneDev &sc, const FrameDev &fr, uint32_t k, int32_t *tri_id, float *t, LaunchCfg cfg,
                       void *stream) {
    hipLaunchKernelGGL(k_primary_ids, dim3(cfg.grid), dim3(cfg.block), cfg.lds_bytes, (hipStream_t)stream, sc, fr, k,
                       tri_id, t);
    return launch_status();
}

int launch_trig(const float *x, uint32_t n, float *cs, float *sn, void *stream) {
    hipLaunchKernelGGL(k_trig, dim3(std::min<uint32_t>((n + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream, x, n, cs, sn);
    return launch_status();
}

int launch_init_pixels(PixelStateDev px, uint32_t npix, void *stream) {
    hipLaunchKernelGGL(k_init_pixels, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream, px, npix);
    return launch_status();
}

int launch_zero_u32(unsigned int *p, uint32_t n, void *stream) {
    hipLaunchKernelGGL(k_zero_u32, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, p, n);
    return launch_status();
}

int launch_paths(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PixelStateDev px, void *rad,
                 DevCounters *counters, bool count, LaunchCfg cfg, void *stream, const GuidePathsDev *guide) {
    hipStream_t s = (hipStream_t)stream;
    dim3 g(cfg.grid), b(cfg.block);
#define VMX_GO(C, T) \
    hipLaunchKernelGGL((k_paths<C, 0, T>), g, b, cfg.lds_bytes, s, sc, fr, wk, px, (float4 *)rad, pa, counters)
    PathArrays pa{};
    if (guide && guide->off && !count) {
        if (sc.tex) hipLaunchKernelGGL((k_paths<false, 0, true, GuidePathsDev>), g, b, cfg.lds_bytes, s, sc, fr, wk, px, (float4 *)rad, pa, counters, *guide);
        else hipLaunchKernelGGL((k_paths<false, 0, false, GuidePathsDev>), g, b, cfg.lds_bytes, s, sc, fr, wk, px, (float4 *)rad, pa, counters, *guide);
    } else if (sc.tex) {
        if (count) VMX_GO(true, true);
        else VMX_GO(false, true);
    } else {
        if (count) VMX_GO(true, false);
        else VMX_GO(false, false);
    }
#undef VMX_GO
    return launch_status();
}

int launch_tail(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PathArrays pa, DevCounters *counters,
                bool count, LaunchCfg cfg, void *stream, const GuidePathsDev *guide) {
    hipStream_t s = (hipStream_t)stream;
    dim3 g(cfg.grid), b(cfg.block);
    PixelStateDev px{nullptr, nullptr, nullptr};
#define VMX_GO(C, T) \
    hipLaunchKernelGGL((k_paths<C, 2, T>), g, b, cfg.lds_bytes, s, sc, fr, wk, px, (float4 *)pa.rad, pa, counters)
    if (guide && guide->off && !count) {
        if (sc.tex) hipLaunchKernelGGL((k_paths<false, 2, true, GuidePathsDev>), g, b, cfg.lds_bytes, s, sc, fr, wk, px, (float4 *)pa.rad, pa, counters, *guide);
        else hipLaunchKernelGGL((k_paths<false, 2, false, GuidePathsDev>), g, b, cfg.lds_bytes, s, sc, fr, wk, px, (float4 *)pa.rad, pa, counters, *guide);
    } else if (sc.tex) {
        if (count) VMX_GO(true, true);
        else VMX_GO(false, true);
    } else {
        if (count) VMX_GO(true, false);
        else VMX_GO(false, false);
    }
#undef VMX_GO
    return launch_status();
}

int launch_camera_tables(const SceneDev &sc, uint32_t n_inner, float ox, float oy, float oz, void *cam_inner,
                         void *cam_tris, uint32_t cus, void *stream) {
    const uint32_t total = n_inner + sc.ntris;
    const uint32_t grid = strided_grid((total + 255) / 256, cus, 16);
    hipLaunchKernelGGL(k_camera_tables, dim3(grid), dim3(256), 0, (hipStream_t)stream, sc, n_inner, ox, oy, oz,
                       (float4 *)cam_inner, (float4 *)cam_tris);
    return launch_status();
}

int launch_raygen(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PixelStateDev px, PathArrays pa, uint32_t cus, void *stream) {
    const uint64_t total = (uint64_t)wk.samples * wk.n_pad;
    const uint32_t grid = strided_grid((total + 255) / 256, cus, 32);
    if (wk.live_mask) hipLaunchKernelGGL(k_raygen<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, sc, fr, wk, px, pa);
    else if (wk.unclaimed && wk.claim_lists && wk.qids.ids) {
        // a fused pass of a run with list claims (render_pass): the form that settles the listed pixels' rays itself
        if (!wk.pixel_major || (wk.samples & 63u) != 0 || !wk.cam_tris || !wk.list_ctr || !wk.qids.counts) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL((k_raygen<0, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, sc, fr, wk, px, pa);
    } else hipLaunchKernelGGL(k_raygen<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, sc, fr, wk, px, pa);
    return launch_status();
}

int launch_walk_words(const unsigned int *active, uint32_t n_active, uint32_t n_pad, const unsigned int *claims,
                      const unsigned int *lists, unsigned long long *mask, unsigned int *cnt, uint32_t cus, void *stream) {
    const uint32_t grid = strided_grid((n_pad + 255) / 256, cus, 16);
    hipLaunchKernelGGL(k_walk_words, dim3(grid), dim3(256), 0, (hipStream_t)stream, active, n_active, n_pad, claims, lists, mask, cnt);
    return launch_status();
}

int launch_pixel_claims(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, unsigned int *claims, unsigned int *lists, unsigned int *n_claimed,
                        unsigned long long *pend_mask, unsigned int *pend_cnt, LaunchCfg cfg, void *stream) {
    if (lists && (!pend_mask || !pend_cnt)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pixel_claims, dim3(cfg.grid), dim3(cfg.block), cfg.lds_bytes, (hipStream_t)stream, sc, fr,
                       (const float *)wk.cam_inner, (const float *)wk.cam_tris, claims, lists, n_claimed, pend_mask, pend_cnt,
                       wk.lds_entries, wk.overflow_entries, wk.overflow_stack);
    return launch_status();
}

int launch_pixel_lists(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, const unsigned int *entries, const unsigned int *count,
                       unsigned int *head, unsigned int *lists, LaunchCfg cfg, void *stream) {
    hipLaunchKernelGGL(k_pixel_lists, dim3(cfg.grid), dim3(cfg.block), cfg.lds_bytes, (hipStream_t)stream, sc, fr,
                       (const float *)wk.cam_inner, (const float *)wk.cam_tris, entries, count, head, lists, wk.lds_entries,
                       wk.overflow_entries, wk.overflow_stack);
    return launch_status();
}

int query_pixel_claims_blocks_per_cu(uint32_t block, uint32_t lds_bytes, int *blocks) {
    return (int)hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, k_pixel_claims, (int)block, lds_bytes);
}

int query_pixel_lists_blocks_per_cu(uint32_t block, uint32_t lds_bytes, int *blocks) {
    return (int)hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, k_pixel_lists, (int)block, lds_bytes);
}

int launch_unclaimed_words(const unsigned int *active, uint32_t n_active, uint32_t n_pad, const unsigned int *claims,
                           unsigned long long *mask, unsigned int *cnt, uint32_t cus, void *stream) {
    const uint32_t grid = strided_grid((n_pad + 255) / 256, cus, 16);
    hipLaunchKernelGGL(k_unclaimed_words, dim3(grid), dim3(256), 0, (hipStream_t)stream, active, n_active, n_pad, claims, mask, cnt);
    return launch_status();
}

int launch_raygen_live(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PixelStateDev px, PathArrays pa, uint32_t cus, void *stream) {
    // the list's length is known on the device only: a grid for a third of the pass's paths, striding over the rest
    const uint64_t total = ((uint64_t)wk.samples * wk.n_pad + 2) / 3;
    const uint32_t grid = strided_grid((total + 255) / 256, cus, 32);
    hipLaunchKernelGGL(k_raygen_live, dim3(grid), dim3(256), 0, (hipStream_t)stream, sc, fr, wk, px, pa);
    return launch_status();
}

// The instantiation that traces a pass: the production form k_trace_w (sorted: k_trace_w<.., SORT>; live: the
// ELIDE_DEAD list form of the camera kernel), with counters the first form k_trace_q (same tests per ray).
// launch_trace_q launches what these name and query_trace_q_blocks_per_cu sizes the persistent grid and the record-list
// padding from its occupancy: the figure is by construction that of the kernel launched.
using TraceWKernel = void (*)(SceneDev, FrameDev, WorkDev, PathArrays, GuideDev);
using TraceQKernel = void (*)(SceneDev, FrameDev, WorkDev, PixelStateDev, PathArrays, DevCounters *);
static TraceWKernel trace_w_kernel(bool from_queue, bool sorted, bool live, bool guide) {
    if (from_queue) {
        if (guide) {  // bounce rays over the scene's guide tree (guide_walk.h)
            if (sorted) return k_trace_w<1, false, true, true>;
            return k_trace_w<1, false, false, true>;
        }
        if (sorted) return k_trace_w<1, false, true>;
        return k_trace_w<1>;
    }
    if (sorted) {
        if (live) return k_trace_w<0, true, true>;
        return k_trace_w<0, false, true>;
    }
    if (live) return k_trace_w<0, true>;
    return k_trace_w<0>;
}
static TraceQKernel trace_q_kernel(bool from_queue) {
    if (from_queue) return k_trace_q<true, 1>;
    return k_trace_q<true, 0>;
}

int launch_trace_q(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PixelStateDev px, PathArrays pa,
                   DevCounters *counters, bool count, bool from_queue, LaunchCfg cfg, void *stream, const GuideDev *guide,
                   unsigned int *visits) {
    hipStream_t s = (hipStream_t)stream;
    dim3 g(cfg.grid), b(cfg.block);
    const bool guided = guide && guide->base && from_queue && !count;
    if (visits) {  // the debug entry's counting form of k_trace_w<1, false, false, true>: hit records only
        if (!guided || wk.out_rec) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(k_trace_w_visits, g, b, cfg.lds_bytes, s, sc, fr, wk, pa, *guide, (uint2 *)visits);
        return launch_status();
    }
    GuideDev gd{};
    if (guided) gd = *guide;
    if (count) hipLaunchKernelGGL(trace_q_kernel(from_queue), g, b, cfg.lds_bytes, s, sc, fr, wk, px, pa, counters);
    else hipLaunchKernelGGL(trace_w_kernel(from_queue, wk.out_rec != nullptr, wk.live_ids != nullptr, guided), g, b, cfg.lds_bytes, s, sc, fr, wk, pa, gd);
    return launch_status();
}

int query_trace_q_blocks_per_cu(uint32_t block, uint32_t lds_bytes, bool count, bool from_queue, bool sorted, bool live, int *blocks,
                                bool guide) {
    int a = 0;
    const hipError_t e = count ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, trace_q_kernel(from_queue), (int)block, lds_bytes)
                               : hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, trace_w_kernel(from_queue, sorted, live, guide && from_queue), (int)block, lds_bytes);
    if (blocks) *blocks = a;
    return (int)e;
}

// from_queue: bounce paths (wk.qids), else the camera paths of the pass.  wk.flat_ids: the second phase after
// launch_shade_ends + launch_live_compact — only the listed positions.
int launch_shade(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PixelStateDev px, PathArrays pa,
                 IdQueue qout, uint32_t max_chunks, DevCounters *counters, bool from_queue, uint32_t cus, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const bool flat = wk.flat_ids != nullptr || wk.out_rec != nullptr;  // a list whose length is known on the device only -> a full grid
    // 7 blocks per CU are resident (VMX_SHADE_WPS); more blocks only add end-of-block counter atomics, which a small pass
    // feels (early-stop frame, first pass: 1.70 ms with 4096 blocks, 1.05 with 1792; the bench frame's 530.8 M paths: no change)
    // (per compute unit of the scene: 256 * VMX_SHADE_WPS blocks on the device these figures are from)
    const uint32_t shade_grid = std::max(cus, 1u) * VMX_SHADE_WPS;
    // (k_shade<0>'s dense form: a wave per pixel, four pixels per block and iteration)
    const bool dense = !from_queue && !flat && !wk.live_ids && wk.pixel_major && (wk.samples & 63u) == 0;
    const uint64_t items = flat ? shade_grid
                                : (from_queue ? (uint64_t)max_chunks * kSubQueues
                                              : (dense ? ((uint64_t)wk.n_pad + 3) / 4 : ((uint64_t)wk.samples * wk.n_pad + 255) / 256));
    uint32_t grid = (uint32_t)std::min<uint64_t>(items, shade_grid);
    if (grid == 0) grid = 1;
#define VMX_GO(S, T, E, Q, D)                                                                                                    \
    do {  /* (wk.fused: the dense form's CLAIMED instantiation, over the pass's claimed slots) */                                \
        if (D && wk.fused) hipLaunchKernelGGL((k_shade<S, T, E, Q, D, D>), dim3(grid), dim3(256), 0, s, sc, fr, wk, px, pa, qout, max_chunks, counters); \
        else hipLaunchKernelGGL((k_shade<S, T, E, Q, D>), dim3(grid), dim3(256), 0, s, sc, fr, wk, px, pa, qout, max_chunks, counters); \
    } while (0)
#define VMX_GO_T(S, E, Q, ...)                       \
    do {                                             \
        if (sc.tex) VMX_GO(S, true, E, Q, (false __VA_ARGS__)); \
        else VMX_GO(S, false, E, Q, (false __VA_ARGS__));     \
    } while (0)
    // camera paths are shaded from the live list exactly when render_impl built one (wk.live_ids)
    const bool elide = from_queue ? fr.elide_dead != 0 : wk.live_ids != nullptr;
    if (from_queue) {
        if (wk.out_rec) { if (elide) VMX_GO_T(1, true, 2); else VMX_GO_T(1, false, 2); }
        else if (flat) { if (elide) VMX_GO_T(1, true, 1); else VMX_GO_T(1, false, 1); }
        else { if (elide) VMX_GO_T(1, true, 0); else VMX_GO_T(1, false, 0); }
    } else if (wk.out_rec) {
        if (elide) VMX_GO_T(0, true, 2);
        else VMX_GO_T(0, false, 2);
    } else if (flat) {
        if (elide) VMX_GO_T(0, true, 1);
        else VMX_GO_T(0, false, 1);
    } else {
        if (elide) VMX_GO_T(0, true, 0);
        else if (dense) VMX_GO_T(0, false, 0, || true);
        else VMX_GO_T(0, false, 0);
    }
#undef VMX_GO_T
#undef VMX_GO
    return launch_status();
}

// first phase of the two-phase shading (k_shade_ends): finishes the steps that end by their draws alone, queues the
// others' positions in full_mask / full_cnt (one word per wave of 64 positions) for launch_live_compact + launch_shade
int launch_shade_ends(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PathArrays pa, unsigned long long *full_mask,
                      unsigned int *full_cnt, uint32_t max_chunks, DevCounters *counters, bool from_queue, uint32_t cus, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const uint64_t items = from_queue ? (uint64_t)max_chunks * kSubQueues : ((uint64_t)wk.samples * wk.n_pad + 255) / 256;
    const uint32_t grid = strided_grid(items, cus, 8);  // 8 waves per SIMD resident; see launch_shade
#define VMX_GO(S, T, L) \
    hipLaunchKernelGGL((k_shade_ends<S, T, L>), dim3(grid), dim3(256), 0, s, sc, fr, wk, pa, full_mask, full_cnt, max_chunks, counters)
    if (from_queue) {
        if (sc.tex) VMX_GO(1, true, false);
        else VMX_GO(1, false, false);
    } else if (wk.live_ids) {
        if (sc.tex) VMX_GO(0, true, true);
        else VMX_GO(0, false, true);
    } else {
        if (sc.tex) VMX_GO(0, true, false);
        else VMX_GO(0, false, false);
    }
#undef VMX_GO
    return launch_status();
}

int launch_radiance_init_ids(const float *o, const float *d, uint32_t n, uint64_t seed, PathArrays pa, IdQueue qout,
                             uint32_t cus, void *stream) {
    const uint32_t grid = strided_grid(((uint64_t)n + 255) / 256, cus, 16);
    hipLaunchKernelGGL(k_radiance_init_ids, dim3(grid), dim3(256), 0, (hipStream_t)stream, o, d, n, seed, pa, qout);
    return launch_status();
}

int query_paths_blocks_per_cu(uint32_t block, uint32_t lds_bytes, bool count, int *blocks, bool guide) {
    int a = 0, b = 0;
    hipError_t e;
    if (guide && !count) {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_paths<false, 0, true, GuidePathsDev>, (int)block, lds_bytes);
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_paths<false, 2, true, GuidePathsDev>, (int)block, lds_bytes);
    } else if (count) {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_paths<true, 0, true>, (int)block, lds_bytes);
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_paths<true, 2, true>, (int)block, lds_bytes);
    } else {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_paths<false, 0, true>, (int)block, lds_bytes);
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_paths<false, 2, true>, (int)block, lds_bytes);
    }
    if (blocks) *blocks = a < b ? a : b;
    return (int)e;
}

int launch_resolve(const FrameDev &fr, const unsigned int *active, uint32_t n_active, uint32_t samples,
                   bool pixel_major, const void *rad, const unsigned long long *rad_mask, PixelStateDev px, unsigned int *next_active,
                   unsigned int *next_count, float *out_rgbaz, DevCounters *counters, void *stream, bool moments) {
    const uint32_t n_pad = (n_active + 63u) & ~63u;
    hipLaunchKernelGGL(moments ? k_resolve<true> : k_resolve<false>, dim3((n_active + 255) / 256), dim3(256), 0, (hipStream_t)stream, fr, active,
                       n_active, n_pad, samples, pixel_major ? 1u : 0u, (const float4 *)rad, pixel_major ? rad_mask : nullptr, px, next_active,
                       next_count, out_rgbaz, counters);
    return launch_status();
}

int launch_bruteforce(const SceneDev &sc, const FrameDev &fr, const unsigned int *order, uint32_t npix, uint32_t flags,
                      float *out, DevCounters *counters, void *longs, unsigned int *long_count, const WorkDev &stack,
                      LaunchCfg cfg, void *stream) {
    hipLaunchKernelGGL(k_bruteforce, dim3(cfg.grid), dim3(cfg.block), cfg.lds_bytes, (hipStream_t)stream, sc, fr, order,
                       npix, flags, out, counters, (BfLong *)longs, long_count, stack.lds_entries, stack.overflow_entries,
                       stack.overflow_stack);
    return launch_status();
}
// the pixels k_bruteforce handed over (*long_count of them, known to the host as `count`): one wave each
int launch_bruteforce_long(const SceneDev &sc, const FrameDev &fr, uint32_t flags, float *out, DevCounters *counters,
                           const void *longs, const unsigned int *long_count, uint32_t count, const WorkDev &stack,
                           LaunchCfg cfg, void *stream) {
    const uint32_t blocks = std::min<uint32_t>(cfg.grid, (count + (cfg.block / 64) - 1) / (cfg.block / 64));
    hipLaunchKernelGGL(k_bruteforce_long, dim3(std::max(blocks, 1u)), dim3(cfg.block), cfg.lds_bytes, (hipStream_t)stream, sc, fr,
                       flags, out, counters, (const BfLong *)longs, long_count, stack.lds_entries, stack.overflow_entries,
                       stack.overflow_stack);
    return launch_status();
}

int launch_assemble(const float *gathered, uint64_t rank_stride_floats, uint32_t width, uint32_t height,
                    uint32_t stripe_rows, uint32_t world, float *frame, void *stream) {
    hipLaunchKernelGGL(k_assemble, dim3(2048), dim3(256), 0, (hipStream_t)stream, gathered, rank_stride_floats, width,
                       height, stripe_rows, world, frame);
    return launch_status();
}

int launch_quantize(const float *frame, uint64_t npix, void *rgba8, float *depth, void *stream) {
    uint32_t grid = (uint32_t)std::min<uint64_t>((npix + 255) / 256, 8192);
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL(k_quantize, dim3(grid), dim3(256), 0, (hipStream_t)stream, frame, npix, (uchar4 *)rgba8, depth);
    return launch_status();
}

// device ray queries of explicit batches: k_query<MODE> + launch_query
#include "vmx_query.inc"

// the albedo plane of a camera: k_query's camera mode + k_albedo_finish
#include "vmx_albedo.inc"

// in-place geometry updates: record rewrite and per-level refit
#include "vmx_update.inc"

// progressive rendering: the displayable frame of unfinished per-pixel state
#include "vmx_preview.inc"

// what the image-space passes below share: the 32 x 8 tile, the guide's tap terms, the launch
#include "vmx_image.inc"
// G-buffer-guided a-trous filter of frames and previews
#include "vmx_filter.inc"
// G-buffer-guided upsampling: a low frame reconstructed under a full-size guide
#include "vmx_upsample.inc"

// temporal accumulation: reprojected history blended with each new frame
#include "vmx_temporal.inc"
// adaptive temporal accumulation: the reprojection alone, then the window test that cuts stale history before the blend
#include "vmx_adaptive.inc"
// variance-guided denoising: the variance of a moments accumulator and the filter it steers
#include "vmx_variance.inc"
// adaptive sampling of a progressive handle: list compaction, the per-pixel error of the mean and the selection map
#include "vmx_sampling.inc"
// motion records for refitted geometry: where each pixel's surface point was before an update
#include "vmx_motion.inc"
// ... and for pixels on an analytic sphere that vmx_scene_set_spheres moved
#include "vmx_motion_spheres.inc"
// emissive triangles: the derived table the light-sampling integrator samples
#include "vmx_emitters.inc"
// light sampling: the path integrator with next-event estimation
#include "vmx_nee.inc"

#ifdef VMX_AB_KERNELS
// first-generation kernels (pipeline forms 2, 3): only in the A/B library of `make ab`, never in the product
#include "vmx_kernels_ab.inc"
#include "vmx_trace_pool.inc"
#endif

}  // namespace vmx
