// api_progressive.inc — part of vmx_api.cpp
extern "C" {

// ---- progressive rendering: a frame in resumable runs of passes, previews of the unfinished state --------------------
struct VMX_OPAQUE vmx_progressive {
    vmx_scene *sc = nullptr;
    RenderJob job;
    PixelBufs pixels;
    DevBuf<float> frame;            // k_resolve's output: the finished pixels
    DevBuf<float> host_rgbaz;       // vmx_progressive_preview: device side of the host buffers, on first use
    DevBuf<unsigned char> host_rgba8;
    vmx_camera cam;                 // as begun: the filtered previews' guide is sample 0's camera ray of every pixel
    std::unique_ptr<vmx_filter> filter;  // vmx_progressive_preview_filtered*: created, and its guide built, on first use
    DevBuf<unsigned char> albedo;   // vmx_progressive_preview_demodulated*: the albedo plane (float4 per pixel) of samples
    uint32_t albedo_samples = 0;    // 0 .. albedo_samples - 1, built on first use (0: none yet)
    uint64_t generation = 0;        // the scene's when the handle began
    uint64_t samples = 0, passes = 0, steps = 0;
    bool failed = false;            // a step stopped half way: the schedule and the device state may disagree
    // adaptive sampling (api_sampling.inc).  From the first selected step on the handle is ragged (job.sched.ragged): `master` is
    // the list of its active pixels in the tile order of render_init_pixels, compacted in order after every step; a step
    // compacts it by its selection into the job's active list and runs the pass loop on that
    DevBuf<unsigned int> master[2];
    int cur_master = 0;
    uint32_t n_master = 0;
    DevBuf<unsigned long long> list_mask;   // one word of bits per 64 slots of the master list
    DevBuf<unsigned int> list_u32;          // [popcounts | their exclusive scan | the compacted list's length]
    DevBuf<unsigned char> list_tmp;         // scan scratch
    size_t list_words = 0, list_tmp_bytes = 0;
    DevBuf<unsigned char> select_map;       // vmx_progressive_step_adaptive's map, on first use
    // budgeted steps (light-sampled handles): vmx_progressive_step_budgeted's plane; the step's sample counts and their
    // exclusive scan (one entry per local pixel and one more each), the scan's scratch — all on first use
    DevBuf<unsigned int> budget_map, item_cnt, item_base;
    DevBuf<unsigned char> item_tmp;
    size_t item_tmp_bytes = 0;
};

// a step of a ragged handle (api_sampling.inc); d_select NULL: every active pixel
static int progressive_step_list(vmx_progressive *p, uint32_t samples, const unsigned char *d_select, vmx_stats *stats,
                                 uint32_t *selected, std::chrono::steady_clock::time_point t0);

int vmx_progressive_begin(vmx_scene *sc, const vmx_camera *cam, const vmx_opts *opts, void *stream, vmx_progressive **out) {
    return vmx_progressive_begin_ex(sc, cam, opts, 0, stream, out);
}

// nee: a light-sampled handle (vmx_progressive_begin_nee), whose passes run k_nee (RenderJob::nee); ranks: its rank form
// (vmx_progressive_begin_nee_rank), which accepts world > 1
static int progressive_begin(vmx_scene *sc, const vmx_camera *cam, const vmx_opts *opts, uint32_t flags, void *stream,
                             vmx_progressive **out, bool nee, bool ranks = false) {
    // checks that need no device, in this order so that each can be seen alone; the scene comes last
    if (!cam || !opts) return fail(VMX_ERR_INVALID, "NULL argument: cam or opts");
    if (!out) return fail(VMX_ERR_INVALID, "NULL out");
    if (flags & ~VMX_PROGRESSIVE_MOMENTS)
        return fail(VMX_ERR_INVALID, nee ? "vmx_progressive_begin_nee: unknown flag (0 or VMX_PROGRESSIVE_MOMENTS)"
                                         : "vmx_progressive_begin_ex: unknown flag (0 or VMX_PROGRESSIVE_MOMENTS)");
    if (nee)
        if (int rc = nee_check_opts(opts, ranks)) return rc;
    {
        FrameDev fr;
        if (int rc = make_frame(*cam, *opts, fr)) return rc;
    }
    if (!sc) return fail(VMX_ERR_INVALID, "NULL scene");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    std::unique_ptr<vmx_progressive> p(new (std::nothrow) vmx_progressive);
    if (!p) return fail(VMX_ERR_NOMEM, "out of host memory");
    p->sc = sc;
    p->cam = *cam;
    p->generation = sc->generation;
    int rc = render_setup(sc, cam, opts, &p->pixels, nullptr, stream ? (hipStream_t)stream : sc->stream, p->job);
    p->job.moments = (flags & VMX_PROGRESSIVE_MOMENTS) != 0;
    p->job.nee = nee;
    if (rc == VMX_OK && p->job.npix) {
        if (p->frame.ensure((size_t)p->job.npix * 5)) rc = fail(VMX_ERR_NOMEM, "hipMalloc failed for the frame buffer");
        p->job.d_out = p->frame.p;
        // the state a preview before the first step shows; after the scene's last update, like every pass
        if (rc == VMX_OK) rc = sc->upd.done.wait(p->job.s);
        if (rc == VMX_OK) rc = render_init_pixels(sc, p->job);
    }
    if (rc) {
        (void)hipStreamSynchronize(p->job.s);
        return rc;
    }
    sc->progressive_open++;
    *out = p.release();
    return VMX_OK;
}

int vmx_progressive_begin_ex(vmx_scene *sc, const vmx_camera *cam, const vmx_opts *opts, uint32_t flags, void *stream,
                             vmx_progressive **out) {
    return progressive_begin(sc, cam, opts, flags, stream, out, false);
}

int vmx_progressive_begin_nee(vmx_scene *sc, const vmx_camera *cam, const vmx_opts *opts, uint32_t flags, void *stream,
                              vmx_progressive **out) {
    return progressive_begin(sc, cam, opts, flags, stream, out, true);
}

int vmx_progressive_begin_nee_rank(vmx_scene *sc, const vmx_camera *cam, const vmx_opts *opts, uint32_t flags, void *stream,
                                   vmx_progressive **out) {
    return progressive_begin(sc, cam, opts, flags, stream, out, true, true);
}

int vmx_progressive_step(vmx_progressive *p, uint32_t samples, vmx_stats *stats) {
    if (!p) return fail(VMX_ERR_INVALID, "NULL handle");
    const auto t0 = std::chrono::steady_clock::now();
    vmx_scene *sc = p->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (p->generation != sc->generation) return fail(VMX_ERR_INVALID, "scene updated since vmx_progressive_begin");
    if (p->failed) return fail(VMX_ERR_INVALID, "an earlier step of this handle failed: end it and begin again");
    if (p->job.sched.ragged) return progressive_step_list(p, samples, nullptr, stats, nullptr, t0);
    vmx_stats st;
    std::memset(&st, 0, sizeof(st));
    if (p->job.n_active > 0) {
        const int rc = render_run(sc, p->job, samples, &st, t0);
        if (rc) {
            p->failed = true;
            (void)hipStreamSynchronize(p->job.s);
            return rc;
        }
        p->samples += st.samples, p->passes += st.passes, p->steps++;
    }
    if (stats) *stats = st;
    return VMX_OK;
}

int vmx_progressive_info_get(const vmx_progressive *p, vmx_progressive_info *out) {
    if (!p) return fail(VMX_ERR_INVALID, "NULL handle");
    if (!out) return fail(VMX_ERR_INVALID, "NULL out");
    std::lock_guard<std::mutex> lock(p->sc->mu);
    std::memset(out, 0, sizeof(*out));
    out->width = p->job.fr.width, out->rows = p->job.fr.local_rows, out->kmax = p->job.fr.kmax;
    out->pixels_active = p->job.n_active;
    out->samples = p->samples, out->passes = p->passes, out->steps = p->steps;
    return VMX_OK;
}

// argument checks of the previews that need no device (the handle last, so that each is seen alone)
static int preview_args(const vmx_progressive *p, const void *rgbaz, const void *rgba8) {
    if (!rgbaz && !rgba8) return fail(VMX_ERR_INVALID, "no output: rgbaz and rgba8 are both NULL");
    if (!p) return fail(VMX_ERR_INVALID, "NULL handle");
    return VMX_OK;
}

int vmx_progressive_preview_device(vmx_progressive *p, void *d_rgbaz, void *d_rgba8) {
    if (int rc = preview_args(p, d_rgbaz, d_rgba8)) return rc;
    if (((uintptr_t)d_rgbaz | (uintptr_t)d_rgba8) & 3u) return fail(VMX_ERR_INVALID, "d_rgbaz and d_rgba8 must be 4-byte aligned");
    vmx_scene *sc = p->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (int rc = check_device_ptrs(sc->device, {{d_rgbaz, "d_rgbaz"}, {d_rgba8, "d_rgba8"}})) return rc;
    const RenderJob &job = p->job;
    LAUNCH_TRY(launch_preview(PixelStateDev{p->pixels.accum.p, p->pixels.count.p, p->pixels.cursor.p}, job.npix, job.fr.kmax,
                              p->frame.p, (float *)d_rgbaz, d_rgba8, job.s));
    return VMX_OK;
}

int vmx_progressive_preview(vmx_progressive *p, float *rgbaz, unsigned char *rgba8) {
    if (int rc = preview_args(p, rgbaz, rgba8)) return rc;
    vmx_scene *sc = p->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    const RenderJob &job = p->job;
    const size_t npix = job.npix;
    if (npix == 0) return VMX_OK;
    if ((rgbaz && p->host_rgbaz.ensure(npix * 5)) || (rgba8 && p->host_rgba8.ensure(npix * 4)))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed for the preview buffers");
    LAUNCH_TRY(launch_preview(PixelStateDev{p->pixels.accum.p, p->pixels.count.p, p->pixels.cursor.p}, job.npix, job.fr.kmax,
                              p->frame.p, rgbaz ? p->host_rgbaz.p : nullptr, rgba8 ? p->host_rgba8.p : nullptr, job.s));
    if (rgbaz) HIP_TRY(hipMemcpyAsync(rgbaz, p->host_rgbaz.p, npix * 20, hipMemcpyDeviceToHost, job.s));
    if (rgba8) HIP_TRY(hipMemcpyAsync(rgba8, p->host_rgba8.p, npix * 4, hipMemcpyDeviceToHost, job.s));
    HIP_TRY(hipStreamSynchronize(job.s));
    return VMX_OK;
}

// first filtered preview of a handle: its filter, and the guide from sample 0's camera ray of every pixel (the code path
// of vmx_raycast_camera_device); blocks until the guide is built, because the G-buffer it is packed from is freed here
static int progressive_filter_ensure(vmx_progressive *p) {
    if (p->filter) return VMX_OK;
    vmx_scene *sc = p->sc;
    if (p->job.opts.world > 1) return fail(VMX_ERR_INVALID, "world > 1: a filtered preview is guided by the camera raycast (whole images only)");
    if (p->generation != sc->generation) return fail(VMX_ERR_INVALID, "scene updated since vmx_progressive_begin");
    FrameDev fr;
    if (int rc = make_frame(p->cam, p->job.opts, fr)) return rc;
    const uint32_t npix = fr.width * fr.height;
    std::unique_ptr<vmx_filter> f;
    if (int rc = filter_make(sc->device, fr.width, fr.height, f)) return rc;
    DevBuf<unsigned char> gbuf;
    int rc = gbuf.ensure((size_t)npix * sizeof(vmx_rayhit)) ? fail(VMX_ERR_NOMEM, "hipMalloc failed for the G-buffer") : VMX_OK;
    if (rc == VMX_OK) rc = raycast_enqueue(sc, true, true, nullptr, nullptr, npix, fr, 0, gbuf.p, p->job.s);
    if (rc == VMX_OK) rc = filter_guide_enqueue(f.get(), gbuf.p, p->job.s);
    const hipError_t e = hipStreamSynchronize(p->job.s);
    gbuf.release();  // (64 bytes per pixel, packed into the guide's 16: not kept for the handle's life)
    if (rc == VMX_OK && e != hipSuccess) rc = fail(VMX_ERR_HIP, std::string("vmx_progressive_preview_filtered: ") + hipGetErrorString(e));
    if (rc) return rc;
    p->filter = std::move(f);
    return VMX_OK;
}

// the handle's albedo plane: built on the first demodulated preview, and again when `samples` changes, from the handle's
// own camera and seed on its stream — under the guide's refusals
static int progressive_albedo_ensure(vmx_progressive *p, uint32_t samples) {
    if (p->albedo_samples == samples) return VMX_OK;
    vmx_scene *sc = p->sc;
    if (p->job.opts.world > 1) return fail(VMX_ERR_INVALID, "world > 1: a demodulated preview needs the camera's albedo plane (whole images only)");
    if (p->generation != sc->generation) return fail(VMX_ERR_INVALID, "scene updated since vmx_progressive_begin");
    FrameDev fr;
    if (int rc = make_frame(p->cam, p->job.opts, fr)) return rc;
    if (p->albedo.ensure((size_t)fr.width * fr.height * 16)) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the albedo plane");
    p->albedo_samples = 0;
    if (int rc = albedo_enqueue(sc, fr, 0, samples, p->albedo.p, p->job.s)) return rc;
    p->albedo_samples = samples;
    return VMX_OK;
}

// albedo_samples == 0: the plain filtered preview
static int progressive_filter_enqueue(vmx_progressive *p, float *d_rgbaz, void *d_rgba8, const vmx_filter_params &prm,
                                      uint32_t albedo_samples = 0) {
    if (int rc = progressive_filter_ensure(p)) return rc;
    if (albedo_samples)
        if (int rc = progressive_albedo_ensure(p, albedo_samples)) return rc;
    FilterSrc src{};
    src.px = PixelStateDev{p->pixels.accum.p, p->pixels.count.p, p->pixels.cursor.p};
    src.finished = p->frame.p;
    src.kmax = p->job.fr.kmax;
    std::lock_guard<std::mutex> lock(p->filter->mu);
    return filter_enqueue(p->filter.get(), src, d_rgbaz, d_rgba8, prm, p->job.s, FilterExtras{albedo_samples ? p->albedo.p : nullptr});
}

// demod: vmx_progressive_preview_demodulated_device, whose albedo_samples must be 1 .. kmax
static int progressive_preview_filtered_device(vmx_progressive *p, void *d_rgbaz, void *d_rgba8, const vmx_filter_params *params,
                                               bool demod, uint32_t albedo_samples) {
    vmx_filter_params prm;
    if (int rc = filter_params(params, prm)) return rc;
    if (int rc = preview_args(p, d_rgbaz, d_rgba8)) return rc;
    if (((uintptr_t)d_rgbaz | (uintptr_t)d_rgba8) & 3u) return fail(VMX_ERR_INVALID, "d_rgbaz and d_rgba8 must be 4-byte aligned");
    if (demod && (albedo_samples < 1 || albedo_samples > p->job.fr.kmax)) return fail(VMX_ERR_INVALID, "albedo_samples must be 1 .. 4 * (rays_per_pixel / 4)");
    vmx_scene *sc = p->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (int rc = check_device_ptrs(sc->device, {{d_rgbaz, "d_rgbaz"}, {d_rgba8, "d_rgba8"}})) return rc;
    if (spans_meet(Span{d_rgbaz, (size_t)p->job.npix * 20}, Span{d_rgba8, (size_t)p->job.npix * 4}))
        return fail(VMX_ERR_INVALID, "d_rgbaz and d_rgba8 overlap");
    return progressive_filter_enqueue(p, (float *)d_rgbaz, d_rgba8, prm, demod ? albedo_samples : 0);
}

int vmx_progressive_preview_filtered_device(vmx_progressive *p, void *d_rgbaz, void *d_rgba8, const vmx_filter_params *params) {
    return progressive_preview_filtered_device(p, d_rgbaz, d_rgba8, params, false, 0);
}

int vmx_progressive_preview_demodulated_device(vmx_progressive *p, void *d_rgbaz, void *d_rgba8, const vmx_filter_params *params,
                                               uint32_t albedo_samples) {
    return progressive_preview_filtered_device(p, d_rgbaz, d_rgba8, params, true, albedo_samples);
}

static int progressive_preview_filtered_host(vmx_progressive *p, float *rgbaz, unsigned char *rgba8, const vmx_filter_params *params,
                                             bool demod, uint32_t albedo_samples) {
    vmx_filter_params prm;
    if (int rc = filter_params(params, prm)) return rc;
    if (int rc = preview_args(p, rgbaz, rgba8)) return rc;
    if (demod && (albedo_samples < 1 || albedo_samples > p->job.fr.kmax)) return fail(VMX_ERR_INVALID, "albedo_samples must be 1 .. 4 * (rays_per_pixel / 4)");
    vmx_scene *sc = p->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    const RenderJob &job = p->job;
    const size_t npix = job.npix;
    if ((rgbaz && p->host_rgbaz.ensure(npix * 5)) || (rgba8 && p->host_rgba8.ensure(npix * 4)))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed for the preview buffers");
    if (int rc = progressive_filter_enqueue(p, rgbaz ? p->host_rgbaz.p : nullptr, rgba8 ? p->host_rgba8.p : nullptr, prm,
                                            demod ? albedo_samples : 0)) return rc;
    if (rgbaz) HIP_TRY(hipMemcpyAsync(rgbaz, p->host_rgbaz.p, npix * 20, hipMemcpyDeviceToHost, job.s));
    if (rgba8) HIP_TRY(hipMemcpyAsync(rgba8, p->host_rgba8.p, npix * 4, hipMemcpyDeviceToHost, job.s));
    HIP_TRY(hipStreamSynchronize(job.s));
    return VMX_OK;
}

int vmx_progressive_preview_filtered(vmx_progressive *p, float *rgbaz, unsigned char *rgba8, const vmx_filter_params *params) {
    return progressive_preview_filtered_host(p, rgbaz, rgba8, params, false, 0);
}

int vmx_progressive_preview_demodulated(vmx_progressive *p, float *rgbaz, unsigned char *rgba8, const vmx_filter_params *params,
                                        uint32_t albedo_samples) {
    return progressive_preview_filtered_host(p, rgbaz, rgba8, params, true, albedo_samples);
}

int vmx_progressive_end(vmx_progressive *p) {
    if (!p) return fail(VMX_ERR_INVALID, "NULL handle");
    vmx_scene *sc = p->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    (void)hipSetDevice(sc->device);
    (void)hipStreamSynchronize(p->job.s);  // a preview may still read the state
    delete p;
    sc->progressive_open--;
    return VMX_OK;
}

} /* extern "C" */
