// api_upsample.inc — part of vmx_api.cpp
extern "C" {

// ---- G-buffer-guided upsampling (k_filter_guide: vmx_filter.inc, k_upsample: vmx_upsample.inc) --------------------------
struct VMX_OPAQUE vmx_upsample {
    int device = 0;
    uint32_t low_width = 0, low_height = 0, width = 0, height = 0;
    DevBuf<unsigned char> guide_low, guide_full;  // float4 (n.xyz, z) per pixel
    Fence done;  // recorded after each call's last kernel, waited on by the next: one call at a time uses the guides
    bool guides_set = false;
    std::mutex mu;
};

static const vmx_upsample_params kUpsampleDefaults = {5u, 0.1f, {0u, 0u, 0u, 0u, 0u, 0u}};

// NULL selects the defaults; anything out of range is refused before any launch
static int upsample_params(const vmx_upsample_params *in, vmx_upsample_params &out) {
    out = in ? *in : kUpsampleDefaults;
    if (!squarings_ok(out.normal_squarings)) return fail(VMX_ERR_INVALID, "vmx_upsample_params: normal_squarings must be 0..8");
    if (!finite_positive(out.sigma_depth)) return fail(VMX_ERR_INVALID, "vmx_upsample_params: sigma_depth must be finite and > 0");
    if (!reserved_zero(out.reserved)) return fail(VMX_ERR_INVALID, "vmx_upsample_params: reserved words must be 0");
    return VMX_OK;
}

int vmx_upsample_default_params(vmx_upsample_params *out) { return default_params(out, kUpsampleDefaults); }

int vmx_upsample_create(int device, uint32_t low_width, uint32_t low_height, uint32_t width, uint32_t height, vmx_upsample **out) {
    if (!out) return fail(VMX_ERR_INVALID, "NULL out");
    *out = nullptr;
    if (low_width == 0 || low_height == 0 || width == 0 || height == 0)
        return fail(VMX_ERR_INVALID, "image resolution must be non-zero");
    if (low_width > width || low_height > height)
        return fail(VMX_ERR_INVALID, "the low frame must not be larger than the full one (low_width <= width, low_height <= height)");
    if ((uint64_t)width > 4ull * low_width || (uint64_t)height > 4ull * low_height)
        return fail(VMX_ERR_INVALID, "the full frame must be at most 4 times the low one (width <= 4 * low_width, height <= 4 * low_height)");
    if (int rc = image_handle_checks(device, width, height)) return rc;  // (the low image is no larger)
    std::unique_ptr<vmx_upsample> u(new (std::nothrow) vmx_upsample);
    if (!u) return fail(VMX_ERR_NOMEM, "out of host memory");
    u->device = device, u->low_width = low_width, u->low_height = low_height, u->width = width, u->height = height;
    if (u->guide_low.ensure((size_t)low_width * low_height * 16) || u->guide_full.ensure((size_t)width * height * 16))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed for the upsampler's guides");
    *out = u.release();
    return VMX_OK;
}

int vmx_upsample_destroy(vmx_upsample *u) {
    if (!u) return fail(VMX_ERR_INVALID, "NULL handle");
    (void)hipSetDevice(u->device);
    (void)u->done.sync();  // the last call may still use the guides
    delete u;
    return VMX_OK;
}

int vmx_upsample_set_guides_device(vmx_upsample *u, const void *d_rayhit_low, const void *d_rayhit_full, void *stream) {
    if (!d_rayhit_low) return fail(VMX_ERR_INVALID, "NULL d_rayhit_low");
    if (!d_rayhit_full) return fail(VMX_ERR_INVALID, "NULL d_rayhit_full");
    if (((uintptr_t)d_rayhit_low | (uintptr_t)d_rayhit_full) & 15u)
        return fail(VMX_ERR_INVALID, "d_rayhit_low and d_rayhit_full must be 16-byte aligned");
    if (!u) return fail(VMX_ERR_INVALID, "NULL handle");
    std::lock_guard<std::mutex> lock(u->mu);
    HIP_TRY(hipSetDevice(u->device));
    if (int rc = check_device_ptrs(u->device, {{d_rayhit_low, "d_rayhit_low"}, {d_rayhit_full, "d_rayhit_full"}})) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = u->done.wait(s)) return rc;  // after the previous call on this handle
    LAUNCH_TRY(launch_filter_guide(d_rayhit_low, u->low_width * u->low_height, u->guide_low.p, s));
    LAUNCH_TRY(launch_filter_guide(d_rayhit_full, u->width * u->height, u->guide_full.p, s));
    u->guides_set = true;
    return u->done.record(s);
}

int vmx_upsample_apply_device(vmx_upsample *u, const void *d_low_rgbaz, void *d_out_rgbaz, void *d_rgba8,
                              const vmx_upsample_params *params, void *stream) {
    // checks that need no device, in this order so that each can be seen alone; the handle comes last
    if (!d_out_rgbaz && !d_rgba8) return fail(VMX_ERR_INVALID, "no output: d_out_rgbaz and d_rgba8 are both NULL");
    vmx_upsample_params prm;
    if (int rc = upsample_params(params, prm)) return rc;
    if (!d_low_rgbaz) return fail(VMX_ERR_INVALID, "NULL d_low_rgbaz");
    if (((uintptr_t)d_low_rgbaz | (uintptr_t)d_out_rgbaz | (uintptr_t)d_rgba8) & 3u)
        return fail(VMX_ERR_INVALID, "d_low_rgbaz, d_out_rgbaz and d_rgba8 must be 4-byte aligned");
    if (!u) return fail(VMX_ERR_INVALID, "NULL handle");
    std::lock_guard<std::mutex> lock(u->mu);
    {
        // every pair of {low, out, rgba8}: the sizes differ, so there is no in-place form
        const size_t nlow = (size_t)u->low_width * u->low_height, npix = (size_t)u->width * u->height;
        const Span low{d_low_rgbaz, nlow * 20}, out{d_out_rgbaz, npix * 20}, q8{d_rgba8, npix * 4};
        if (meets_any(low, {out, q8}) || spans_meet(out, q8)) return fail(VMX_ERR_INVALID, "d_low_rgbaz, d_out_rgbaz and d_rgba8 overlap");
    }
    if (!u->guides_set) return fail(VMX_ERR_INVALID, "no guides: call vmx_upsample_set_guides_device first");
    HIP_TRY(hipSetDevice(u->device));
    if (int rc = check_device_ptrs(u->device, {{d_low_rgbaz, "d_low_rgbaz"}, {d_out_rgbaz, "d_out_rgbaz"}, {d_rgba8, "d_rgba8"}})) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = u->done.wait(s)) return rc;  // after the previous call on this handle
    UpsamplePass a{};
    a.width = u->width, a.height = u->height, a.low_width = u->low_width, a.low_height = u->low_height;
    a.squarings = prm.normal_squarings, a.sigma_depth = prm.sigma_depth;
    a.guide_low = u->guide_low.p, a.guide_full = u->guide_full.p;
    a.low = (const float *)d_low_rgbaz, a.out_rgbaz = (float *)d_out_rgbaz, a.rgba8 = d_rgba8;
    LAUNCH_TRY(launch_upsample(a, s));
    return u->done.record(s);
}

} /* extern "C" */
