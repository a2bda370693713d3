// api_filter.inc — part of vmx_api.cpp
extern "C" {

// ---- G-buffer-guided a-trous filter (k_filter_guide, k_atrous: vmx_filter.inc) ------------------------------------------
struct VMX_OPAQUE vmx_filter {
    int device = 0;
    uint32_t width = 0, height = 0;
    DevBuf<unsigned char> guide;   // float4 (n.xyz, z) per pixel
    DevBuf<unsigned char> planes;  // two float4 colour planes, back to back (an in-place single iteration stages its
                                   // 20-byte pixels here instead)
    Fence done;  // recorded after each call's last kernel, waited on by the next: one call at a time uses the guide and the planes
    bool guide_set = false;
    std::mutex mu;
};

// a filter for width x height frames on `device`, the current device
static int filter_make(int device, uint32_t width, uint32_t height, std::unique_ptr<vmx_filter> &out) {
    std::unique_ptr<vmx_filter> f(new (std::nothrow) vmx_filter);
    if (!f) return fail(VMX_ERR_NOMEM, "out of host memory");
    f->device = device, f->width = width, f->height = height;
    const size_t npix = (size_t)width * height;
    if (f->guide.ensure(npix * 16) || f->planes.ensure(npix * 32)) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the filter's planes");
    out = std::move(f);
    return VMX_OK;
}

static const vmx_filter_params kFilterDefaults = {5u, 5u, 2.f, 0.1f, {0u, 0u, 0u, 0u}};

// NULL selects the defaults; anything out of range is refused before any launch
static int filter_params(const vmx_filter_params *in, vmx_filter_params &out) {
    out = in ? *in : kFilterDefaults;
    if (out.iterations < 1 || out.iterations > 10) return fail(VMX_ERR_INVALID, "vmx_filter_params: iterations must be 1..10");
    if (!squarings_ok(out.normal_squarings)) return fail(VMX_ERR_INVALID, "vmx_filter_params: normal_squarings must be 0..8");
    if (!finite_positive(out.sigma_colour)) return fail(VMX_ERR_INVALID, "vmx_filter_params: sigma_colour must be finite and > 0");
    if (!finite_positive(out.sigma_depth)) return fail(VMX_ERR_INVALID, "vmx_filter_params: sigma_depth must be finite and > 0");
    if (!reserved_zero(out.reserved)) return fail(VMX_ERR_INVALID, "vmx_filter_params: reserved words must be 0");
    return VMX_OK;
}

static int filter_guide_enqueue(vmx_filter *f, const void *d_rayhit, hipStream_t s) {
    if (int rc = f->done.wait(s)) return rc;  // after the previous call on this handle
    LAUNCH_TRY(launch_filter_guide(d_rayhit, f->width * f->height, f->guide.p, s));
    f->guide_set = true;
    return f->done.record(s);
}

// what a call may take besides the frame; NULL: the call is without it
struct FilterExtras {
    const void *albedo = nullptr;     // the demodulated call's plane (float4 per pixel)
    const float *variance = nullptr;  // the variance-guided call's (float per pixel) ...
    float sigma_luminance = 0.f;      // ... and its colour stop
};

// the iterations of one call on `s`; the caller holds f->mu and has checked arguments and pointers
static int filter_enqueue(vmx_filter *f, FilterSrc src, float *out, void *rgba8, const vmx_filter_params &prm, hipStream_t s,
                          const FilterExtras &extra) {
    if (int rc = f->done.wait(s)) return rc;  // after the previous call on this handle
    const size_t npix = (size_t)f->width * f->height;
    // one iteration in place would read neighbours another block has already replaced: it filters a copy of the frame
    // (a demodulated call's taps read the pre-pass's plane, and its last iteration only its own pixel of the frame)
    if (prm.iterations == 1 && src.frame && src.frame == out && !extra.albedo && !extra.variance) {
        HIP_TRY(hipMemcpyAsync(f->planes.p, src.frame, npix * 20, hipMemcpyDeviceToDevice, s));
        src.frame = (const float *)f->planes.p;
    }
    FilterPass a{};
    a.width = f->width, a.height = f->height;
    a.squarings = prm.normal_squarings;
    a.guide = f->guide.p;
    a.src = src;
    a.albedo = extra.albedo;
    unsigned char *plane[2] = {f->planes.p, f->planes.p + npix * 16};
    a.sl2 = extra.sigma_luminance * extra.sigma_luminance;
    if (extra.variance) {  // (frame [/ albedo], variance) into the plane iteration 0 reads
        a.out_plane = plane[1];
        LAUNCH_TRY(launch_variance_pack(a, extra.variance, s));
    } else if (extra.albedo) {  // frame / albedo into the plane iteration 0 reads, as if it were iteration -1's output
        a.out_plane = plane[1];
        LAUNCH_TRY(launch_demod_divide(a, s));
    }
    float sc = prm.sigma_colour;
    for (uint32_t it = 0; it < prm.iterations; ++it) {
        a.step = 1u << it;
        a.isc2 = 1.f / (sc * sc);
        a.kz = prm.sigma_depth * (float)a.step;
        sc = sc * 0.5f;
        a.first = it == 0 && !extra.albedo && !extra.variance, a.last = it + 1 == prm.iterations;
        a.in_plane = a.first ? nullptr : plane[(it + 1) & 1];
        a.out_plane = a.last ? nullptr : plane[it & 1];
        a.out_rgbaz = a.last ? out : nullptr;
        a.rgba8 = a.last ? rgba8 : nullptr;
        if (extra.variance)
            LAUNCH_TRY(launch_atrous_var(a, s));
        else
            LAUNCH_TRY(launch_atrous(a, s));
    }
    return f->done.record(s);
}

int vmx_filter_default_params(vmx_filter_params *out) { return default_params(out, kFilterDefaults); }

int vmx_filter_create(int device, uint32_t width, uint32_t height, vmx_filter **out) {
    if (!out) return fail(VMX_ERR_INVALID, "NULL out");
    *out = nullptr;
    if (int rc = image_handle_checks(device, width, height)) return rc;
    std::unique_ptr<vmx_filter> f;
    if (int rc = filter_make(device, width, height, f)) return rc;
    *out = f.release();
    return VMX_OK;
}

int vmx_filter_destroy(vmx_filter *f) {
    if (!f) return fail(VMX_ERR_INVALID, "NULL handle");
    (void)hipSetDevice(f->device);
    (void)f->done.sync();  // the last call may still use the planes
    delete f;
    return VMX_OK;
}

int vmx_filter_set_guide_device(vmx_filter *f, const void *d_rayhit, void *stream) {
    if (!d_rayhit) return fail(VMX_ERR_INVALID, "NULL d_rayhit");
    if ((uintptr_t)d_rayhit & 15u) return fail(VMX_ERR_INVALID, "d_rayhit must be 16-byte aligned");
    if (!f) return fail(VMX_ERR_INVALID, "NULL handle");
    std::lock_guard<std::mutex> lock(f->mu);
    HIP_TRY(hipSetDevice(f->device));
    if (int rc = check_device_ptr(d_rayhit, f->device, "d_rayhit")) return rc;
    return filter_guide_enqueue(f, d_rayhit, (hipStream_t)stream);
}

enum FilterCall { kFilterPlain, kFilterDemodulated, kFilterVariance };

// the three apply entries.  kFilterDemodulated needs extra.albedo, kFilterVariance extra.variance (its albedo may be NULL)
static int filter_apply(vmx_filter *f, FilterCall call, const void *d_in_rgbaz, const FilterExtras &extra, void *d_out_rgbaz,
                        void *d_rgba8, const vmx_filter_params *params, void *stream) {
    const void *d_albedo = extra.albedo, *d_variance = extra.variance;
    // checks that need no device, in this order so that each can be seen alone; the handle comes last
    vmx_filter_params prm;
    if (int rc = filter_params(params, prm)) return rc;
    if (call == kFilterVariance && !finite_positive(extra.sigma_luminance))
        return fail(VMX_ERR_INVALID, "sigma_luminance must be finite and > 0");
    if (!d_in_rgbaz) return fail(VMX_ERR_INVALID, "NULL d_in_rgbaz");
    if (call == kFilterVariance && !d_variance) return fail(VMX_ERR_INVALID, "NULL d_variance");
    if (call == kFilterDemodulated && !d_albedo) return fail(VMX_ERR_INVALID, "NULL d_albedo");
    if (!d_out_rgbaz && !d_rgba8) return fail(VMX_ERR_INVALID, "no output: d_out_rgbaz and d_rgba8 are both NULL");
    if (((uintptr_t)d_in_rgbaz | (uintptr_t)d_out_rgbaz | (uintptr_t)d_rgba8) & 3u)
        return fail(VMX_ERR_INVALID, "d_in_rgbaz, d_out_rgbaz and d_rgba8 must be 4-byte aligned");
    if ((uintptr_t)d_variance & 3u) return fail(VMX_ERR_INVALID, "d_variance must be 4-byte aligned");
    if ((uintptr_t)d_albedo & 15u) return fail(VMX_ERR_INVALID, "d_albedo must be 16-byte aligned");
    if (!f) return fail(VMX_ERR_INVALID, "NULL handle");
    std::lock_guard<std::mutex> lock(f->mu);
    {
        const size_t npix = (size_t)f->width * f->height;
        const Span in{d_in_rgbaz, npix * 20}, out{d_out_rgbaz, npix * 20}, q8{d_rgba8, npix * 4};
        // every pair of {in, out, rgba8} except in == out: in place is the one overlap a call may have
        if ((d_in_rgbaz != d_out_rgbaz && spans_meet(in, out)) || spans_meet(in, q8) || spans_meet(out, q8))
            return fail(VMX_ERR_INVALID, "d_in_rgbaz, d_out_rgbaz and d_rgba8 overlap (only d_out_rgbaz == d_in_rgbaz may)");
        // d_albedo against each output: the iteration that writes the result reads it
        if (meets_any(Span{d_albedo, npix * 16}, {out, q8})) return fail(VMX_ERR_INVALID, "d_albedo overlaps d_out_rgbaz or d_rgba8");
        // d_variance against each output: the pre-pass reads it before anything is written; still, it is an input
        if (meets_any(Span{d_variance, npix * 4}, {out, q8})) return fail(VMX_ERR_INVALID, "d_variance overlaps d_out_rgbaz or d_rgba8");
    }
    if (!f->guide_set) return fail(VMX_ERR_INVALID, "no guide: call vmx_filter_set_guide_device first");
    HIP_TRY(hipSetDevice(f->device));
    if (int rc = check_device_ptrs(f->device, {{d_in_rgbaz, "d_in_rgbaz"}, {d_albedo, "d_albedo"}, {d_out_rgbaz, "d_out_rgbaz"}, {d_rgba8, "d_rgba8"}, {d_variance, "d_variance"}})) return rc;
    FilterSrc src{};
    src.frame = (const float *)d_in_rgbaz;
    return filter_enqueue(f, src, (float *)d_out_rgbaz, d_rgba8, prm, (hipStream_t)stream, extra);
}

int vmx_filter_apply_device(vmx_filter *f, const void *d_in_rgbaz, void *d_out_rgbaz, void *d_rgba8,
                            const vmx_filter_params *params, void *stream) {
    return filter_apply(f, kFilterPlain, d_in_rgbaz, FilterExtras{}, d_out_rgbaz, d_rgba8, params, stream);
}

int vmx_filter_apply_demodulated_device(vmx_filter *f, const void *d_in_rgbaz, const void *d_albedo, void *d_out_rgbaz,
                                        void *d_rgba8, const vmx_filter_params *params, void *stream) {
    return filter_apply(f, kFilterDemodulated, d_in_rgbaz, FilterExtras{d_albedo}, d_out_rgbaz, d_rgba8, params, stream);
}

int vmx_filter_apply_variance_device(vmx_filter *f, const void *d_in_rgbaz, const void *d_variance, const void *d_albedo,
                                     void *d_out_rgbaz, void *d_rgba8, const vmx_filter_params *params, float sigma_luminance,
                                     void *stream) {
    return filter_apply(f, kFilterVariance, d_in_rgbaz, FilterExtras{d_albedo, (const float *)d_variance, sigma_luminance},
                        d_out_rgbaz, d_rgba8, params, stream);
}

} /* extern "C" */
