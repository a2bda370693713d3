// vmx_motion.inc — motion records for refitted geometry: where each pixel's surface point was before a geometry update
// (vmx_motion_device), what vmx_temporal_accumulate_motion_device reprojects with.  Included by vmx_kernels.hip (inside
// its namespace, beside vmx_temporal.inc).  The arithmetic is stated in include/vermilion_hip.h and restated in
// tests/motion_spec.py; with -ffp-contract=off every operation below rounds once, in the order written, `/` and sqrtf are
// correctly rounded and denormals are kept: bit for bit the restatement.
//
//   k_motion  one lane per record.  The record is read as three float4s (as k_filter_guide reads it) and the result
//             leaves as two float4 stores.  The triangle's vertices now and before, and its previous normals where given —
//             two or three gathers of 36 bytes by tri_id — are read only by a lane whose record lies on a triangle of the
//             arrays (`on`); every other rule is a select.  A record that is not on a moved triangle leaves as
//             (location, 0, normal, 0), the record's own bits.
__device__ __forceinline__ float motion_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

__device__ __forceinline__ bool motion_finite(float x) { return fabsf(x) < __builtin_inff(); }  // (false for NaN)

__global__ void __launch_bounds__(256) k_motion(const float4 *__restrict__ rayhit, uint32_t n, const float *__restrict__ pos_now,
                                                const float *__restrict__ pos_prev, const float *__restrict__ nrm_prev,
                                                uint32_t ntris, float4 *__restrict__ out) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const float4 *r = rayhit + (size_t)p * 4;  // (location, distance) (normal, tri_id) (uv, tri_t, flags) (colour, pad)
    const float4 ra = r[0], rb = r[1], rc = r[2];
    const int id = (int)__float_as_uint(rb.w);
    // (tri_id stays set when a sphere is nearer than the triangle: the location then lies on the sphere, the distances differ)
    const bool on = (__float_as_uint(rc.w) & 1u) != 0 && id >= 0 && (uint32_t)id < ntris && ra.w == rc.z;
    float4 o0 = make_float4(ra.x, ra.y, ra.z, 0.f), o1 = make_float4(rb.x, rb.y, rb.z, 0.f);
    if (on) {
        const size_t base = (size_t)id * 9;
        float a[9], q[9];
        bool moved = false;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            a[i] = pos_now[base + i], q[i] = pos_prev[base + i];
            moved = moved || __float_as_uint(a[i]) != __float_as_uint(q[i]);
        }
        const float e1x = a[3] - a[0], e1y = a[4] - a[1], e1z = a[5] - a[2];
        const float e2x = a[6] - a[0], e2y = a[7] - a[1], e2z = a[8] - a[2];
        const float epx = ra.x - a[0], epy = ra.y - a[1], epz = ra.z - a[2];
        const float d11 = motion_dot(e1x, e1y, e1z, e1x, e1y, e1z), d12 = motion_dot(e1x, e1y, e1z, e2x, e2y, e2z);
        const float d22 = motion_dot(e2x, e2y, e2z, e2x, e2y, e2z);
        const float dp1 = motion_dot(epx, epy, epz, e1x, e1y, e1z), dp2 = motion_dot(epx, epy, epz, e2x, e2y, e2z);
        const float den = d11 * d22 - d12 * d12;
        const float b1 = (d22 * dp1 - d12 * dp2) / den, b2 = (d11 * dp2 - d12 * dp1) / den;
        const float b0 = (1.f - b1) - b2;
        const float xh = (b0 * q[0] + b1 * q[3]) + b2 * q[6];
        const float yh = (b0 * q[1] + b1 * q[4]) + b2 * q[7];
        const float zh = (b0 * q[2] + b1 * q[5]) + b2 * q[8];
        const bool good = den > 0.f && motion_finite(xh) && motion_finite(yh) && motion_finite(zh);
        float nx = rb.x, ny = rb.y, nz = rb.z;
        if (nrm_prev) {  // (uniform)
            float m[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) m[i] = nrm_prev[base + i];
            const float mx = (b0 * m[0] + b1 * m[3]) + b2 * m[6];
            const float my = (b0 * m[1] + b1 * m[4]) + b2 * m[7];
            const float mz = (b0 * m[2] + b1 * m[5]) + b2 * m[8];
            const float s = 1.f / sqrtf(motion_dot(mx, my, mz, mx, my, mz));
            const float hx = -(mx * s), hy = -(my * s), hz = -(mz * s);  // (negated, as Triangle::getNormal negates)
            const bool fin = motion_finite(hx) && motion_finite(hy) && motion_finite(hz);
            nx = fin ? hx : nx, ny = fin ? hy : ny, nz = fin ? hz : nz;
        }
        const bool valid = moved && good;
        o0 = valid ? make_float4(xh, yh, zh, __uint_as_float(kMotionMoved)) : o0;
        o1 = valid ? make_float4(nx, ny, nz, 0.f) : o1;
    }
    out[(size_t)p * 2] = o0;
    out[(size_t)p * 2 + 1] = o1;
}

int launch_motion(const void *rayhit, uint32_t n, const float *pos_now, const float *pos_prev, const float *nrm_prev,
                  uint32_t ntris, void *out, void *stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_motion, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float4 *)rayhit, n, pos_now,
                       pos_prev, nrm_prev, ntris, (float4 *)out);
    return launch_status();
}
