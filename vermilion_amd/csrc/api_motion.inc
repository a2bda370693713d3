// api_motion.inc — part of vmx_api.cpp
extern "C" {

// ---- motion records for refitted geometry (k_motion: vmx_motion.inc) ---------------------------------------------------
int vmx_motion_device(const void *d_rayhit, uint32_t n, const void *d_pos_now, const void *d_pos_prev, const void *d_nrm_prev,
                      uint32_t ntris, void *d_out, int device, void *stream) {
    // checks that need no device, in vmx_temporal_accumulate_device's order so that each can be seen alone
    if (!d_rayhit) return fail(VMX_ERR_INVALID, "NULL d_rayhit");
    if (!d_pos_now) return fail(VMX_ERR_INVALID, "NULL d_pos_now");
    if (!d_pos_prev) return fail(VMX_ERR_INVALID, "NULL d_pos_prev");
    if (!d_out) return fail(VMX_ERR_INVALID, "NULL d_out");
    if (ntris == 0) return fail(VMX_ERR_INVALID, "ntris must be non-zero");
    if (((uintptr_t)d_rayhit | (uintptr_t)d_out) & 15u) return fail(VMX_ERR_INVALID, "d_rayhit and d_out must be 16-byte aligned");
    if (((uintptr_t)d_pos_now | (uintptr_t)d_pos_prev | (uintptr_t)d_nrm_prev) & 3u)
        return fail(VMX_ERR_INVALID, "d_pos_now, d_pos_prev and d_nrm_prev must be 4-byte aligned");
    if (n > 0x7fffffffu) return fail(VMX_ERR_INVALID, "n must be at most 2^31 - 1");
    // d_out, the one buffer the call writes, against each it reads
    if (meets_any(Span{d_out, (size_t)n * 32}, {{d_rayhit, (size_t)n * 64}, {d_pos_now, (size_t)ntris * 36}, {d_pos_prev, (size_t)ntris * 36},
                                                {d_nrm_prev, (size_t)ntris * 36}}))
        return fail(VMX_ERR_INVALID, "d_out overlaps d_rayhit, d_pos_now, d_pos_prev or d_nrm_prev");
    if (n == 0) return VMX_OK;
    if (int rc = device_checks(device)) return rc;
    if (int rc = check_device_ptrs(device, {{d_rayhit, "d_rayhit"}, {d_pos_now, "d_pos_now"}, {d_pos_prev, "d_pos_prev"},
                                            {d_nrm_prev, "d_nrm_prev"}, {d_out, "d_out"}}))
        return rc;
    LAUNCH_TRY(launch_motion(d_rayhit, n, (const float *)d_pos_now, (const float *)d_pos_prev, (const float *)d_nrm_prev, ntris,
                             d_out, stream));
    return VMX_OK;
}

// ---- motion records for pixels on a moved analytic sphere (k_motion_spheres: vmx_motion_spheres.inc) ---------------------
int vmx_motion_spheres_device(const void *d_rayhit, uint32_t n, const float origin[3], const vmx_sphere *spheres_now,
                              const vmx_sphere *spheres_prev, uint32_t nspheres, const void *d_motion_in, void *d_out,
                              void *stream) {
    // checks that need no device, in vmx_motion_device's order so that each can be seen alone
    if (!d_rayhit) return fail(VMX_ERR_INVALID, "NULL d_rayhit");
    if (!origin) return fail(VMX_ERR_INVALID, "NULL origin");
    if (nspheres > 0 && !spheres_now) return fail(VMX_ERR_INVALID, "NULL spheres_now");
    if (nspheres > 0 && !spheres_prev) return fail(VMX_ERR_INVALID, "NULL spheres_prev");
    if (!d_out) return fail(VMX_ERR_INVALID, "NULL d_out");
    if (nspheres > kMaxSpheres) return fail(VMX_ERR_INVALID, "more than 16 spheres");
    if (((uintptr_t)d_rayhit | (uintptr_t)d_motion_in | (uintptr_t)d_out) & 15u)
        return fail(VMX_ERR_INVALID, "d_rayhit, d_motion_in and d_out must be 16-byte aligned");
    if (n > 0x7fffffffu) return fail(VMX_ERR_INVALID, "n must be at most 2^31 - 1");
    // d_out, the one buffer the call writes, against each it reads; d_motion_in may be d_out itself (a lane reads its own
    // record before it writes it), and only that
    if (spans_meet(Span{d_out, (size_t)n * 32}, Span{d_rayhit, (size_t)n * 64}) ||
        (d_motion_in != d_out && spans_meet(Span{d_out, (size_t)n * 32}, Span{d_motion_in, (size_t)n * 32})))
        return fail(VMX_ERR_INVALID, "d_out overlaps d_rayhit or d_motion_in (d_out == d_motion_in, in place, is allowed)");
    if (n == 0) return VMX_OK;
    // the records' device is the call's: every pointer must be memory of it
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(VMX_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    hipPointerAttribute_t a;
    std::memset(&a, 0, sizeof(a));
    if (hipPointerGetAttributes(&a, d_rayhit) != hipSuccess) {
        (void)hipGetLastError();  // (an unknown pointer sets the thread's error state)
        return fail(VMX_ERR_INVALID, "d_rayhit is not device memory");
    }
    if (a.type != hipMemoryTypeDevice) return fail(VMX_ERR_INVALID, "d_rayhit is not device memory");
    const int device = a.device;
    if (int rc = device_checks(device)) return rc;
    if (int rc = check_device_ptrs(device, {{d_motion_in, "d_motion_in"}, {d_out, "d_out"}})) return rc;
    SphereMotionDev tb;
    std::memset(&tb, 0, sizeof(tb));
    tb.nspheres = nspheres;
    tb.ox = origin[0], tb.oy = origin[1], tb.oz = origin[2];
    for (uint32_t i = 0; i < nspheres; ++i) {
        const vmx_sphere &now = spheres_now[i], &prev = spheres_prev[i];
        const float sn = sphere_sign(now), sp = sphere_sign(prev);
        for (int k = 0; k < 3; ++k) tb.now[i][k] = now.centre[k], tb.prev[i][k] = prev.centre[k], tb.nprev[i][k] = prev.normal_centre[k];
        tb.now[i][3] = now.radius, tb.prev[i][3] = prev.radius, tb.nprev[i][3] = sp;
        // moved: centre, radius or normal_centre differ as bits, or the sign the kernels multiply by differs
        const bool moved = std::memcmp(now.centre, prev.centre, 12) != 0 || std::memcmp(&now.radius, &prev.radius, 4) != 0 ||
                           std::memcmp(now.normal_centre, prev.normal_centre, 12) != 0 || sn != sp;
        if (moved) tb.moved |= 1u << i;
    }
    LAUNCH_TRY(launch_motion_spheres(d_rayhit, n, tb, d_motion_in, d_out, stream));
    return VMX_OK;
}

} /* extern "C" */
