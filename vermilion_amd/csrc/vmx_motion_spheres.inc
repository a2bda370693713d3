// vmx_motion_spheres.inc — motion records for pixels that lie on a moved analytic sphere: where each such pixel's surface
// point was before vmx_scene_set_spheres replaced the table (vmx_motion_spheres_device), in vmx_motion.inc's record layout
// so that the call composes after vmx_motion_device or stands alone.  Included by vmx_kernels.hip beside vmx_motion.inc.
// The arithmetic is stated in include/vermilion_hip.h and restated in tests/sphere_motion_spec.py; with -ffp-contract=off
// every operation below rounds once, in the order written, `/` and sqrtf are correctly rounded and denormals are kept:
// bit for bit the restatement.
//
//   k_motion_spheres  one lane per record, read as three float4s; two float4 stores.  The two tables come by value (at
//             most 16 entries each: 784 bytes of kernel arguments) and are read with the loop's uniform index only — the
//             sphere a lane accepts is carried in registers by selects, so no lane indexes the arguments on its own.
//             Which sphere a record lies on is decided as cast_finish decides it: sphere_hit, with its single-precision
//             shortcuts, on the normalised direction from the common origin, in table order, `th > 0 && th < nearest`.
//             A record that is not on a moved sphere leaves as motion_in's record, or as (location, 0, normal, 0).
__global__ void __launch_bounds__(256) k_motion_spheres(const float4 *__restrict__ rayhit, uint32_t n, const SphereMotionDev tb,
                                                        const float4 *motion_in, float4 *out) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const float4 *r = rayhit + (size_t)p * 4;  // (location, distance) (normal, tri_id) (uv, tri_t, flags) (colour, pad)
    const float4 ra = r[0], rb = r[1], rc = r[2];
    const int id = (int)__float_as_uint(rb.w);
    // the complement of k_motion's `on`, without its ntris bound: a hit that does not lie on its triangle lies on a sphere
    const bool sphere = (__float_as_uint(rc.w) & 1u) != 0 && !(id >= 0 && ra.w == rc.z);
    float4 o0 = make_float4(ra.x, ra.y, ra.z, 0.f), o1 = make_float4(rb.x, rb.y, rb.z, 0.f);
    if (motion_in) {  // (uniform; may be `out` itself: a lane reads its own record before it writes it)
        o0 = motion_in[(size_t)p * 2];
        o1 = motion_in[(size_t)p * 2 + 1];
    }
    if (sphere) {
        float dx = ra.x - tb.ox, dy = ra.y - tb.oy, dz = ra.z - tb.oz;
        normalize3(dx, dy, dz);
        const bool fin = motion_finite(dx) && motion_finite(dy) && motion_finite(dz);
        float nearest = kInf;
        bool moved = false;
        float cx = 0.f, cy = 0.f, cz = 0.f, rn = 0.f;   // the accepted sphere now: centre, radius
        float qx = 0.f, qy = 0.f, qz = 0.f, rp = 0.f;   // ... and before
        float mx = 0.f, my = 0.f, mz = 0.f, sg = 0.f;   // ... its normal_centre and sign before
        for (uint32_t i = 0; i < tb.nspheres; ++i) {
            const float sx = tb.now[i][0], sy = tb.now[i][1], sz = tb.now[i][2], rad = tb.now[i][3];
            const float th = sphere_hit(tb.ox, tb.oy, tb.oz, dx, dy, dz, make_float4(sx, sy, sz, rad * rad), nearest);
            if (fin && th > 0.f && th < nearest) {
                nearest = th;
                moved = ((tb.moved >> i) & 1u) != 0;
                cx = sx, cy = sy, cz = sz, rn = rad;
                qx = tb.prev[i][0], qy = tb.prev[i][1], qz = tb.prev[i][2], rp = tb.prev[i][3];
                mx = tb.nprev[i][0], my = tb.nprev[i][1], mz = tb.nprev[i][2], sg = tb.nprev[i][3];
            }
        }
        const float k = rp / rn;
        const float xh = qx + (ra.x - cx) * k, yh = qy + (ra.y - cy) * k, zh = qz + (ra.z - cz) * k;
        float nx = xh - mx, ny = yh - my, nz = zh - mz;
        normalize3(nx, ny, nz);
        nx = nx * sg, ny = ny * sg, nz = nz * sg;
        const bool nfin = motion_finite(nx) && motion_finite(ny) && motion_finite(nz);
        nx = nfin ? nx : rb.x, ny = nfin ? ny : rb.y, nz = nfin ? nz : rb.z;
        // (no accepted sphere: moved is false)
        const bool valid = moved && motion_finite(xh) && motion_finite(yh) && motion_finite(zh);
        o0 = valid ? make_float4(xh, yh, zh, __uint_as_float(kMotionMoved)) : o0;
        o1 = valid ? make_float4(nx, ny, nz, 0.f) : o1;
    }
    out[(size_t)p * 2] = o0;
    out[(size_t)p * 2 + 1] = o1;
}

int launch_motion_spheres(const void *rayhit, uint32_t n, const SphereMotionDev &tb, const void *motion_in, void *out,
                          void *stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_motion_spheres, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float4 *)rayhit, n, tb,
                       (const float4 *)motion_in, (float4 *)out);
    return launch_status();
}
