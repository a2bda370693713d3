// api_albedo.inc — part of vmx_api.cpp
extern "C" {

// ---- the albedo plane of a camera (k_query's camera mode + k_albedo_finish: vmx_albedo.inc) ----------------------------
// samples first .. first + n - 1 of fr's pixels into `plane` on `s`; the caller holds sc->mu and has checked the arguments
// and the pointer.  A query like any other of the scene: same workspace, same events
static int albedo_enqueue(vmx_scene *sc, const FrameDev &fr, uint32_t first, uint32_t n, void *plane, hipStream_t s) {
    if (int rc = ensure_query_ws(sc)) return rc;
    auto &w = sc->qws;
    const uint32_t npix = fr.width * fr.height;
    if (w.albedo_rec.n < (size_t)npix * sizeof(vmx_rayhit)) {
        if (int rc = w.done.sync()) return rc;  // an earlier plane's kernels may still use the smaller scratch
        if (w.albedo_rec.ensure((size_t)npix * sizeof(vmx_rayhit))) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the albedo scratch");
    }
    QueryDev q;
    LaunchCfg cfg;
    query_shape(sc, kQueryCastCamera, false, npix, q, cfg);  // (per-lane fetch: launch_albedo_sample)
    if (int rc = query_begin(sc, s)) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        if (i) HIP_TRY(hipMemsetAsync(w.head.p, 0, sizeof(unsigned int), s));  // (query_begin reset it for the first)
        q.sample = first + i;
        LAUNCH_TRY(launch_albedo_sample(sc->dev, q, fr, w.albedo_rec.p, i == 0, i + 1 == n, n, plane, cfg, s));
    }
    return query_end(sc, s);
}

int vmx_albedo_camera_device(const vmx_scene *csc, const vmx_camera *cam, const vmx_opts *opts, uint32_t first_sample,
                             uint32_t nsamples, void *d_albedo, void *stream) {
    // vmx_raycast_camera_device's checks in its order, each seen alone; the scene comes last
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!cam || !opts) return fail(VMX_ERR_INVALID, "NULL camera or opts");
    if (!d_albedo) return fail(VMX_ERR_INVALID, "NULL d_albedo");
    if ((uintptr_t)d_albedo & 15u) return fail(VMX_ERR_INVALID, "d_albedo must be 16-byte aligned");
    FrameDev fr;
    if (int rc = make_frame(*cam, *opts, fr)) return rc;
    if (opts->world > 1) return fail(VMX_ERR_INVALID, "world > 1: the albedo plane covers the whole image only");
    if (nsamples == 0) return fail(VMX_ERR_INVALID, "nsamples must be at least 1");
    if ((uint64_t)first_sample + nsamples > fr.kmax) return fail(VMX_ERR_INVALID, "sample range out of range");
    if (!sc) return fail(VMX_ERR_INVALID, "NULL scene");
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (int rc = check_device_ptr(d_albedo, sc->device, "d_albedo")) return rc;
    return albedo_enqueue(sc, fr, first_sample, nsamples, d_albedo, stream ? (hipStream_t)stream : sc->stream);
}

} /* extern "C" */
