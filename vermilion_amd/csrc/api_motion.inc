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

} /* extern "C" */
