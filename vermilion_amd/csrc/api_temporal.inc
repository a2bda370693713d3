// api_temporal.inc — part of vmx_api.cpp
extern "C" {

// ---- temporal accumulation (k_temporal: vmx_temporal.inc) ---------------------------------------------------------------
struct VMX_OPAQUE vmx_temporal {
    int device = 0;
    uint32_t width = 0, height = 0;
    DevBuf<unsigned char> state[2];  // three float4 planes per buffer: (c_h.rgb, n_h) (n.xyz, z) (X.xyz, -)
    bool moments = false;            // VMX_TEMPORAL_MOMENTS: a fourth plane of float2 (m1, m2) follows them
    DevBuf<unsigned char> plane;     // vmx_temporal_accumulate_adaptive_device's reprojection plane, float4 (hh.rgb, nh) and with moments
                                     // float2 (g1, g2) per pixel: allocated by the first such call, never by any other
    int cur = 0;                     // the buffer the last call wrote
    bool has_history = false;        // false after create and reset: the next call is a first call
    TemporalCam hist_cam{};          // the last call's camera
    uint64_t frames = 0;             // calls since create or reset
    Fence done;  // recorded after each call's kernel, waited on by the next: a call reads the state the previous one wrote
    mutable std::mutex mu;
};

static const vmx_temporal_params kTemporalDefaults = {0.9f, 0.01f, 32.f, {0u, 0u, 0u, 0u, 0u}};

// NULL selects the defaults; anything out of range is refused before any launch
static int temporal_params(const vmx_temporal_params *in, vmx_temporal_params &out) {
    out = in ? *in : kTemporalDefaults;
    if (!(std::isfinite(out.normal_min) && out.normal_min >= -1.f && out.normal_min <= 1.f))
        return fail(VMX_ERR_INVALID, "vmx_temporal_params: normal_min must be finite and -1..1");
    if (!finite_positive(out.plane_tol)) return fail(VMX_ERR_INVALID, "vmx_temporal_params: plane_tol must be finite and > 0");
    if (!(std::isfinite(out.max_history) && out.max_history >= 1.f))
        return fail(VMX_ERR_INVALID, "vmx_temporal_params: max_history must be finite and >= 1");
    if (!reserved_zero(out.reserved)) return fail(VMX_ERR_INVALID, "vmx_temporal_params: reserved words must be 0");
    return VMX_OK;
}

int vmx_temporal_default_params(vmx_temporal_params *out) { return default_params(out, kTemporalDefaults); }

int vmx_temporal_create(int device, uint32_t width, uint32_t height, vmx_temporal **out) {
    return vmx_temporal_create_ex(device, width, height, 0u, out);
}

int vmx_temporal_create_ex(int device, uint32_t width, uint32_t height, uint32_t flags, vmx_temporal **out) {
    if (!out) return fail(VMX_ERR_INVALID, "NULL out");
    *out = nullptr;
    if (flags & ~VMX_TEMPORAL_MOMENTS) return fail(VMX_ERR_INVALID, "vmx_temporal_create_ex: unknown flags");
    if (int rc = image_handle_checks(device, width, height)) return rc;
    std::unique_ptr<vmx_temporal> t(new (std::nothrow) vmx_temporal);
    if (!t) return fail(VMX_ERR_NOMEM, "out of host memory");
    t->device = device, t->width = width, t->height = height;
    t->moments = (flags & VMX_TEMPORAL_MOMENTS) != 0;
    const size_t npix = (size_t)width * height, per_pixel = t->moments ? 56 : 48;
    if (t->state[0].ensure(npix * per_pixel) || t->state[1].ensure(npix * per_pixel))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed for the temporal state");
    *out = t.release();
    return VMX_OK;
}

int vmx_temporal_destroy(vmx_temporal *t) {
    if (!t) return fail(VMX_ERR_INVALID, "NULL handle");
    (void)hipSetDevice(t->device);
    (void)t->done.sync();  // the last call may still use the state
    delete t;
    return VMX_OK;
}

int vmx_temporal_reset(vmx_temporal *t, void *stream) {
    (void)stream;  // a first call reads none of the state: there is nothing to enqueue
    if (!t) return fail(VMX_ERR_INVALID, "NULL handle");
    std::lock_guard<std::mutex> lock(t->mu);
    t->has_history = false;
    t->frames = 0;
    return VMX_OK;
}

int vmx_temporal_frames(const vmx_temporal *t, uint64_t *frames_since_reset) {
    if (!frames_since_reset) return fail(VMX_ERR_INVALID, "NULL frames_since_reset");
    if (!t) return fail(VMX_ERR_INVALID, "NULL handle");
    std::lock_guard<std::mutex> lock(t->mu);
    *frames_since_reset = t->frames;
    return VMX_OK;
}

int vmx_temporal_accumulate_device(vmx_temporal *t, const vmx_camera *cam, const void *d_rayhit, const void *d_in_rgbaz,
                                   void *d_out_rgbaz, void *d_rgba8, void *d_history_len, const vmx_temporal_params *params,
                                   void *stream) {
    return vmx_temporal_accumulate_motion_device(t, cam, d_rayhit, nullptr, d_in_rgbaz, d_out_rgbaz, d_rgba8, d_history_len,
                                                 params, stream);
}

// what vmx_temporal_accumulate_variance_device takes besides the others' arguments
struct TemporalVariance {
    void *d_variance;  // an output
    const vmx_variance_params *params;
};

// what vmx_temporal_accumulate_adaptive_device takes besides the others' arguments
struct TemporalAdaptive {
    void *d_change;  // an output, or NULL
    const vmx_adaptive_params *params;
};

// the four accumulate entries; var: the variance entry's own arguments, NULL for the motion entries; ad: the adaptive
// entry's — it takes both kinds of handle, so `var` is then non-NULL and whether the call is a variance call is the
// handle's to say
static int temporal_accumulate(vmx_temporal *t, const vmx_camera *cam, const void *d_rayhit, const void *d_motion,
                               const void *d_in_rgbaz, void *d_out_rgbaz, void *d_rgba8, void *d_history_len,
                               const vmx_temporal_params *params, void *stream, const TemporalVariance *var,
                               const TemporalAdaptive *ad = nullptr) {
    const bool adaptive = ad != nullptr;
    bool variance = var != nullptr && !adaptive;
    void *d_variance = var ? var->d_variance : nullptr;
    void *d_change = ad ? ad->d_change : nullptr;
    // checks that need no device, in the filter's order so that each can be seen alone; the handle comes last
    vmx_temporal_params prm;
    if (int rc = temporal_params(params, prm)) return rc;
    vmx_variance_params vprm = kVarianceDefaults;
    if (var)
        if (int rc = variance_params(var->params, vprm)) return rc;
    vmx_adaptive_params aprm = kAdaptiveDefaults;
    if (adaptive)
        if (int rc = adaptive_params(ad->params, aprm)) return rc;
    if (!cam) return fail(VMX_ERR_INVALID, "NULL camera");
    if (!d_rayhit) return fail(VMX_ERR_INVALID, "NULL d_rayhit");
    if (!d_in_rgbaz) return fail(VMX_ERR_INVALID, "NULL d_in_rgbaz");
    if (variance && !d_variance) return fail(VMX_ERR_INVALID, "NULL d_variance");
    // (the adaptive call: a variance it was given counts as an output; whether it needs one is the handle's to say)
    if (!variance && !(adaptive && d_variance) && !d_out_rgbaz && !d_rgba8)
        return fail(VMX_ERR_INVALID, "no output: d_out_rgbaz and d_rgba8 are both NULL");
    if ((uintptr_t)d_rayhit & 15u) return fail(VMX_ERR_INVALID, "d_rayhit must be 16-byte aligned");
    if ((uintptr_t)d_motion & 15u) return fail(VMX_ERR_INVALID, "d_motion must be 16-byte aligned");
    if (((uintptr_t)d_in_rgbaz | (uintptr_t)d_out_rgbaz | (uintptr_t)d_rgba8 | (uintptr_t)d_history_len) & 3u)
        return fail(VMX_ERR_INVALID, "d_in_rgbaz, d_out_rgbaz, d_rgba8 and d_history_len must be 4-byte aligned");
    if ((uintptr_t)d_variance & 3u) return fail(VMX_ERR_INVALID, "d_variance must be 4-byte aligned");
    if ((uintptr_t)d_change & 3u) return fail(VMX_ERR_INVALID, "d_change must be 4-byte aligned");
    FrameDev fr;
    {
        const vmx_opts none{};  // (make_frame reads a camera's opts too: the defaults of a zeroed struct)
        if (int rc = make_frame(*cam, none, fr)) return rc;
    }
    if (!t) return fail(VMX_ERR_INVALID, "NULL handle");
    std::lock_guard<std::mutex> lock(t->mu);
    if (adaptive) {
        variance = t->moments;
        if (variance && !d_variance) return fail(VMX_ERR_INVALID, "NULL d_variance");
        if (!variance && (d_variance || var->params))
            return fail(VMX_ERR_INVALID, "the handle keeps no moments: d_variance and vparams must be NULL (or create it with "
                                         "vmx_temporal_create_ex(.., VMX_TEMPORAL_MOMENTS, ..))");
    }
    if (variance && !t->moments)
        return fail(VMX_ERR_INVALID, "the handle keeps no moments: create it with vmx_temporal_create_ex(.., VMX_TEMPORAL_MOMENTS, ..)");
    if (!variance && t->moments)
        return fail(VMX_ERR_INVALID, "a VMX_TEMPORAL_MOMENTS handle takes vmx_temporal_accumulate_variance_device only (this call would leave its moments stale)");
    if (fr.width != t->width || fr.height != t->height)
        return fail(VMX_ERR_INVALID, "cam->image_res is " + std::to_string(fr.width) + " x " + std::to_string(fr.height) +
                                         ", the handle's frames are " + std::to_string(t->width) + " x " + std::to_string(t->height));
    {
        const size_t npix = (size_t)t->width * t->height;
        const Span rayhit{d_rayhit, npix * 64}, motion{d_motion, npix * 32}, in{d_in_rgbaz, npix * 20}, out{d_out_rgbaz, npix * 20},
            q8{d_rgba8, npix * 4}, hist{d_history_len, npix * 4};
        // d_motion against each buffer the call writes (the motion records are read only, like d_rayhit)
        if (meets_any(motion, {out, q8, hist})) return fail(VMX_ERR_INVALID, "d_motion overlaps d_out_rgbaz, d_rgba8 or d_history_len");
        // every pair of {rayhit, in, out, rgba8, history_len} with a written one in it, except in == out: in place is
        // the one overlap a buffer the call writes may have
        if (meets_any(rayhit, {out, q8, hist}) || (d_in_rgbaz != d_out_rgbaz && spans_meet(in, out)) || meets_any(in, {q8, hist}) ||
            meets_any(out, {q8, hist}) || spans_meet(q8, hist))
            return fail(VMX_ERR_INVALID, "d_rayhit, d_in_rgbaz, d_out_rgbaz, d_rgba8 and d_history_len overlap (only d_out_rgbaz == d_in_rgbaz may)");
        // d_variance against every other buffer of the call
        if (meets_any(Span{d_variance, npix * 4}, {motion, rayhit, in, out, q8, hist}))
            return fail(VMX_ERR_INVALID, "d_variance overlaps another buffer of the call");
        // d_change against every other buffer of the call
        if (meets_any(Span{d_change, npix * 4}, {motion, rayhit, in, out, q8, hist, Span{d_variance, npix * 4}}))
            return fail(VMX_ERR_INVALID, "d_change overlaps another buffer of the call");
    }
    HIP_TRY(hipSetDevice(t->device));
    if (int rc = check_device_ptrs(t->device, {{d_rayhit, "d_rayhit"}, {d_in_rgbaz, "d_in_rgbaz"}, {d_out_rgbaz, "d_out_rgbaz"},
                                               {d_rgba8, "d_rgba8"}, {d_history_len, "d_history_len"}, {d_motion, "d_motion"},
                                               {d_variance, "d_variance"}, {d_change, "d_change"}}))
        return rc;
    // the one allocation after creation: the reprojection plane, by the first adaptive call (a failure leaves the handle
    // as it was)
    if (adaptive && !t->plane.p) {
        DevBuf<unsigned char> plane;
        if (plane.ensure((size_t)t->width * t->height * (t->moments ? 24 : 16)))
            return fail(VMX_ERR_NOMEM, "hipMalloc failed for the reprojection plane");
        t->plane = std::move(plane);
    }
    hipStream_t s = (hipStream_t)stream;
    if (int rc = t->done.wait(s)) return rc;  // after the previous call on this handle
    TemporalPass a{};
    a.width = t->width, a.height = t->height;
    std::memcpy(a.cam.m, fr.m, sizeof(a.cam.m));
    a.cam.px = fr.px, a.cam.py = fr.py, a.cam.pz = fr.pz;
    a.cam.film_dist = fr.film_dist, a.cam.sensor_x = fr.sensor_x, a.cam.sensor_y = fr.sensor_y;
    a.hist_cam = t->hist_cam;
    a.normal_min = prm.normal_min, a.tol2 = prm.plane_tol * prm.plane_tol, a.max_history = prm.max_history;
    a.rayhit = d_rayhit, a.in_rgbaz = (const float *)d_in_rgbaz;
    a.old_state = t->state[t->cur].p, a.new_state = t->state[t->cur ^ 1].p;
    a.out_rgbaz = (float *)d_out_rgbaz, a.rgba8 = d_rgba8, a.history_len = (float *)d_history_len;
    a.first = !t->has_history;
    a.motion = d_motion;
    a.moments = t->moments;
    if (adaptive && !a.first) {
        // k_temporal_gather and k_rectify; a call in place leaves the frame to k_adaptive_store (vmx_adaptive.inc)
        AdaptivePass ap{};
        ap.t = a;
        const bool in_place = d_out_rgbaz && d_out_rgbaz == d_in_rgbaz;
        if (in_place) ap.t.out_rgbaz = nullptr;
        ap.plane = t->plane.p, ap.change = (float *)d_change;
        ap.gamma2 = aprm.gamma * aprm.gamma;
        ap.min_support = aprm.min_support, ap.sigma_depth = aprm.sigma_depth, ap.squarings = aprm.normal_squarings;
        LAUNCH_TRY(launch_adaptive(ap, in_place ? (float *)d_out_rgbaz : nullptr, s));
    } else {
        // (a first call has no history to test: the existing call, and no pixel changed)
        if (adaptive && d_change) HIP_TRY(hipMemsetAsync(d_change, 0, (size_t)t->width * t->height * 4, s));
        LAUNCH_TRY(launch_temporal(a, s));
    }
    if (variance) {
        VariancePass v{};
        v.width = t->width, v.height = t->height;
        v.squarings = vprm.normal_squarings, v.min_history = vprm.min_history, v.sigma_depth = vprm.sigma_depth;
        v.state = a.new_state, v.variance = (float *)d_variance;
        LAUNCH_TRY(launch_variance(v, s));
    }
    if (int rc = t->done.record(s)) {
        // the next call could not be ordered after this kernel: wait for it here and leave the history as it was (the
        // kernel wrote the other buffer only)
        (void)hipStreamSynchronize(s);
        return rc;
    }
    t->cur ^= 1, t->has_history = true, t->hist_cam = a.cam, t->frames += 1;
    return VMX_OK;
}

int vmx_temporal_accumulate_motion_device(vmx_temporal *t, const vmx_camera *cam, const void *d_rayhit, const void *d_motion,
                                          const void *d_in_rgbaz, void *d_out_rgbaz, void *d_rgba8, void *d_history_len,
                                          const vmx_temporal_params *params, void *stream) {
    return temporal_accumulate(t, cam, d_rayhit, d_motion, d_in_rgbaz, d_out_rgbaz, d_rgba8, d_history_len, params, stream, nullptr);
}

int vmx_temporal_accumulate_variance_device(vmx_temporal *t, const vmx_camera *cam, const void *d_rayhit, const void *d_motion,
                                            const void *d_in_rgbaz, void *d_out_rgbaz, void *d_rgba8, void *d_history_len,
                                            void *d_variance, const vmx_temporal_params *params,
                                            const vmx_variance_params *vparams, void *stream) {
    const TemporalVariance var{d_variance, vparams};
    return temporal_accumulate(t, cam, d_rayhit, d_motion, d_in_rgbaz, d_out_rgbaz, d_rgba8, d_history_len, params, stream, &var);
}

int vmx_adaptive_default_params(vmx_adaptive_params *out) { return default_params(out, kAdaptiveDefaults); }

int vmx_temporal_accumulate_adaptive_device(vmx_temporal *t, const vmx_camera *cam, const void *d_rayhit, const void *d_motion,
                                            const void *d_in_rgbaz, void *d_out_rgbaz, void *d_rgba8, void *d_history_len,
                                            void *d_variance, void *d_change, const vmx_temporal_params *tparams,
                                            const vmx_variance_params *vparams, const vmx_adaptive_params *aparams, void *stream) {
    const TemporalVariance var{d_variance, vparams};
    const TemporalAdaptive ad{d_change, aparams};
    return temporal_accumulate(t, cam, d_rayhit, d_motion, d_in_rgbaz, d_out_rgbaz, d_rgba8, d_history_len, tparams, stream, &var,
                               &ad);
}

} /* extern "C" */
