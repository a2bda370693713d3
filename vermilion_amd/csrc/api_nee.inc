// api_nee.inc — part of vmx_api.cpp: the light-sampling integrator, vmx_render_nee*, their rank forms and vmx_radiance_nee* (k_nee, vmx_nee.inc)
extern "C" {
namespace {
int check_device_ptr(const void *p, int device, const char *what);  // api_query.inc
}
}

namespace {

// what the entries accept of a vmx_opts (include/vermilion_hip.h, "light sampling"); ranks: the entry renders a rank's
// stripes (the *_rank entries), so world > 1 passes here and make_frame checks the rank against it
int nee_check_opts(const vmx_opts *o, bool ranks = false) {
    if ((o->sampling & VMX_SAMPLING_MODE_MASK) > VMX_SAMPLING_CORRECTED ||
        (o->sampling & ~(VMX_SAMPLING_MODE_MASK | VMX_SAMPLING_LIBM_DOUBLE | VMX_SAMPLING_ELIDE_DEAD)))
        return fail(VMX_ERR_INVALID, "unknown sampling mode");
    if (o->sampling & VMX_SAMPLING_ELIDE_DEAD) return fail(VMX_ERR_INVALID, "light sampling: VMX_SAMPLING_ELIDE_DEAD does not apply");
    if ((o->sampling & VMX_SAMPLING_MODE_MASK) != VMX_SAMPLING_CORRECTED)
        return fail(VMX_ERR_INVALID, "light sampling: sampling must be VMX_SAMPLING_CORRECTED");
    if (o->early_stop) return fail(VMX_ERR_INVALID, "light sampling: early_stop is not supported");
    if (o->world > 1 && !ranks) return fail(VMX_ERR_INVALID, "light sampling: world > 1 is not supported");
    if (o->collect_counters) return fail(VMX_ERR_INVALID, "light sampling: collect_counters is not supported");
    if (o->reserved[0]) return fail(VMX_ERR_INVALID, "light sampling: reserved[0] must be 0");
    return VMX_OK;
}

// The derived table of the scene's emissive triangles (vmx_scene_set_emitters), current for a launch on `s`: rebuilt from
// the records the scene holds NOW when the generation moved since it was derived — an update rewrote or permuted them,
// a new table came — and then fenced, since the next launch may run on another stream.  sc->em.dev.n == 0: no table.
int nee_emitters(vmx_scene *sc, hipStream_t s) {
    auto &em = sc->em;
    const uint32_t n = (uint32_t)em.table.size();
    if (n == 0) {
        em.dev = EmitDev{};
        return VMX_OK;
    }
    if (em.built != sc->generation) {
        if (int rc = sc->upd.done.wait(s)) return rc;
        if (em.rec.ensure(n) || em.area.ensure(n) || em.weight.ensure(n) || em.cdf.ensure(n) || em.slot_em.ensure(sc->ntris) ||
            em.id_em.ensure(sc->ntris))
            return fail(VMX_ERR_NOMEM, "hipMalloc failed for the emitter table");
        em.dev = EmitDev{em.rec.p, em.area.p, em.weight.p, em.cdf.p, em.slot_em.p, n};
        LAUNCH_TRY(launch_emitter_table(sc->dev.tris, sc->ntris, em.ids.p, em.radiance.p, em.id_em.p, em.dev, s));
        if (int rc = em.done.record(s)) return rc;
        em.built = sc->generation;
        em.builds++;
    }
    return em.done.wait(s);
}

// the stack and the persistent grid of a k_nee launch over `items` work items on `s`; the scene's emitter table is made
// current first (sc->em.dev is what launch_nee then takes).  (budgeted defaults to false: api_render.inc declares it, for pass_nee)
int nee_launch_cfg(vmx_scene *sc, hipStream_t s, const Tuning &tn, uint64_t items, bool rays, WorkDev &wk, LaunchCfg &cfg,
                   bool budgeted) {
    if (int rc = nee_emitters(sc, s)) return rc;
    int blocks = 0;
    HIP_TRY((hipError_t)query_nee_blocks_per_cu(kPathsBlock, (kPathsBlock / 64) * (tn.lds_entries + 1) * 512, rays, &blocks, budgeted,
                                                sc->em.dev.n != 0));
    if (blocks < 1) return fail(VMX_ERR_HIP, "kernel does not fit on a CU (LDS stack too deep?)");
    cfg = paths_cfg(sc, tn.lds_entries, items, blocks);
    return bind_stack(sc, tn, tn.lds_entries, cfg.grid, items, wk);
}

// One frame: vmx_render's set-up and pass loop (render_run), whose passes run their paths in k_nee (RenderJob::nee) — the
// routine a light-sampled progressive handle steps through
int nee_render_impl(vmx_scene *sc, const vmx_camera *cam, const vmx_opts *opts, float *d_out, hipStream_t s, vmx_stats *stats) {
    const auto t0 = std::chrono::steady_clock::now();
    RenderJob job;
    int rc = render_setup(sc, cam, opts, &sc->ws.pixels, d_out, s, job);
    if (rc) return rc;
    job.nee = true;
    if (job.npix == 0) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return VMX_OK;
    }
    return render_run(sc, job, 0, stats, t0);
}

// vmx_render_nee_device and its rank form: the checks that need no device, the scene last
int nee_render_device_entry(const vmx_scene *csc, const vmx_camera *cam, const vmx_opts *opts, void *d_out, vmx_stats *stats,
                            void *stream, bool ranks) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!cam || !opts || !d_out) return fail(VMX_ERR_INVALID, "NULL argument");
    if (int rc = nee_check_opts(opts, ranks)) return rc;
    if (ranks) {  // (the rank against the world, with make_frame's other checks, before the scene: each can be seen alone)
        FrameDev fr;
        if (int rc = make_frame(*cam, *opts, fr)) return rc;
    }
    if (!sc) return fail(VMX_ERR_INVALID, "NULL scene");  // (last: the checks above need no scene)
    std::lock_guard<std::mutex> lock(sc->mu);
    int rc = bind_device(sc);
    if (rc) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : sc->stream;
    return nee_render_impl(sc, cam, opts, (float *)d_out, s, stats);
}

// vmx_render_nee and its rank form
int nee_render_host_entry(const vmx_scene *csc, const vmx_camera *cam, const vmx_opts *opts, float *out, vmx_stats *stats,
                          bool ranks) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!cam || !opts || !out) return fail(VMX_ERR_INVALID, "NULL argument");
    if (int rc = nee_check_opts(opts, ranks)) return rc;
    if (ranks) {
        FrameDev fr;
        if (int rc = make_frame(*cam, *opts, fr)) return rc;
    }
    if (!sc) return fail(VMX_ERR_INVALID, "NULL scene");
    std::lock_guard<std::mutex> lock(sc->mu);
    int rc = bind_device(sc);
    if (rc) return rc;
    FrameDev fr;
    rc = make_frame(*cam, *opts, fr);
    if (rc) return rc;
    const size_t nfloats = (size_t)fr.width * fr.local_rows * 5;  // (0: a rank that owns no row — nothing is copied)
    if (sc->ws.out.ensure(nfloats)) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the frame buffer");
    rc = nee_render_impl(sc, cam, opts, sc->ws.out.p, sc->stream, stats);
    if (rc) return rc;
    if (nfloats) HIP_TRY(hipMemcpy(out, sc->ws.out.p, nfloats * 4, hipMemcpyDeviceToHost));
    return VMX_OK;
}

// One batch of n rays in k_nee's ray form, device to device on `s`; blocks until it is done (the stats are the counters'
// read-back).  The caller holds sc->mu, has bound the device and has checked the pointers.
int radiance_nee_run(vmx_scene *sc, const float *d_o, const float *d_d, uint32_t n, const vmx_opts *opts, void *d_out4,
                     vmx_stats *stats, hipStream_t s, std::chrono::steady_clock::time_point t0) {
    Workspace &ws = sc->ws;
    int rc;
    if ((rc = sc->upd.done.wait(s))) return rc;
    const Tuning tn = make_tuning(sc, opts);
    FrameDev fr;
    std::memset(&fr, 0, sizeof(fr));
    fr.r2scale = 1.0f;
    fr.libm_double = (opts->sampling & VMX_SAMPLING_LIBM_DOUBLE) ? 1u : 0u;
    fr.seed = opts->seed;
    if (ws.heads.ensure(kSubQueues * 32) || ws.counters.ensure(1)) return fail(VMX_ERR_NOMEM, "hipMalloc failed");
    WorkDev wk = make_work(ws.heads.p, nullptr);
    LaunchCfg cfg;
    if ((rc = nee_launch_cfg(sc, s, tn, n, true, wk, cfg))) return rc;
    CallScope call{sc, s, t0};
    std::vector<TimedLaunch> timed;
    if ((rc = call.open()) || (rc = call.start()) || (rc = call.clear_counters())) return rc;
    HIP_TRY(hipMemsetAsync(ws.heads.p, 0, 4, s));
    if ((rc = timed_begin(ws, timed, s, 0, VMX_K_OTHER))) return rc;
    LAUNCH_TRY(launch_nee(sc->dev, fr, wk, PixelStateDev{nullptr, nullptr, nullptr}, d_o, d_d, n, d_out4, ws.counters.p, cfg, s, sc->em.dev));
    if ((rc = timed_end(timed, s))) return rc;
    rc = call.finish(timed, stats, 1, 1);
    if (rc == VMX_OK && stats) stats->samples = n;
    return rc;
}

}  // namespace

extern "C" {

int vmx_render_nee_device(const vmx_scene *csc, const vmx_camera *cam, const vmx_opts *opts, void *d_out_rgbaz, vmx_stats *stats,
                          void *stream) {
    return nee_render_device_entry(csc, cam, opts, d_out_rgbaz, stats, stream, false);
}

int vmx_render_nee(const vmx_scene *csc, const vmx_camera *cam, const vmx_opts *opts, float *out_rgbaz, vmx_stats *stats) {
    return nee_render_host_entry(csc, cam, opts, out_rgbaz, stats, false);
}

int vmx_render_nee_rank_device(const vmx_scene *csc, const vmx_camera *cam, const vmx_opts *opts, void *d_out_local,
                               vmx_stats *stats, void *stream) {
    return nee_render_device_entry(csc, cam, opts, d_out_local, stats, stream, true);
}

int vmx_render_nee_rank(const vmx_scene *csc, const vmx_camera *cam, const vmx_opts *opts, float *out_local, vmx_stats *stats) {
    return nee_render_host_entry(csc, cam, opts, out_local, stats, true);
}

int vmx_radiance_nee_device(const vmx_scene *csc, const void *d_origin, const void *d_dir, uint32_t n, const vmx_opts *opts,
                            void *d_out4, vmx_stats *stats, void *stream) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    // checks that need no device, in this order so that each can be seen alone; the scene comes last
    if (!d_origin || !d_dir || !opts || !d_out4) return fail(VMX_ERR_INVALID, "NULL argument");
    if (int rc = nee_check_opts(opts)) return rc;
    if (n == 0) return VMX_OK;  // (nothing to do, whatever the scene)
    if (((uintptr_t)d_origin | (uintptr_t)d_dir) & 3u) return fail(VMX_ERR_INVALID, "the rays must be 4-byte aligned");
    if ((uintptr_t)d_out4 & 15u) return fail(VMX_ERR_INVALID, "d_out4 must be 16-byte aligned");
    if (n > 0x7FFFFFFFu) return fail(VMX_ERR_INVALID, "more than 2^31 - 1 rays");
    {
        // the results are written while other rays are still read: [out, out + 16 n) must not meet either ray array
        const uintptr_t a = (uintptr_t)d_out4, b = a + (uintptr_t)n * 16;
        const uintptr_t ro[2] = {(uintptr_t)d_origin, (uintptr_t)d_dir};
        for (uintptr_t r : ro)
            if (r < b && a < r + (uintptr_t)n * 12) return fail(VMX_ERR_INVALID, "d_out4 overlaps the rays");
    }
    if (!sc) return fail(VMX_ERR_INVALID, "NULL scene");
    const auto t0 = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lock(sc->mu);
    int rc = bind_device(sc);
    if (rc) return rc;
    if ((rc = check_device_ptr(d_origin, sc->device, "origin")) || (rc = check_device_ptr(d_dir, sc->device, "dir")) ||
        (rc = check_device_ptr(d_out4, sc->device, "d_out4")))
        return rc;
    return radiance_nee_run(sc, (const float *)d_origin, (const float *)d_dir, n, opts, d_out4, stats,
                            stream ? (hipStream_t)stream : sc->stream, t0);
}

// upload, vmx_radiance_nee_device's routine, download
int vmx_radiance_nee(const vmx_scene *csc, const float *origin, const float *dir, uint32_t n, const vmx_opts *opts, float *out4,
                     vmx_stats *stats) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!origin || !dir || !opts || !out4) return fail(VMX_ERR_INVALID, "NULL argument");
    if (int rc = nee_check_opts(opts)) return rc;
    if (n == 0) return VMX_OK;  // (nothing to do, whatever the scene)
    if (!sc) return fail(VMX_ERR_INVALID, "NULL scene");
    const auto t0 = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lock(sc->mu);
    int rc = bind_device(sc);
    if (rc) return rc;
    Workspace &ws = sc->ws;
    hipStream_t s = sc->stream;
    DevBuf<float> d_o, d_d;
    if (d_o.ensure((size_t)n * 3) || d_d.ensure((size_t)n * 3) || ws.rad.ensure((size_t)n * 16))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed");
    auto body = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_o.p, origin, (size_t)n * 12, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_d.p, dir, (size_t)n * 12, hipMemcpyHostToDevice, s));
        if (int r = radiance_nee_run(sc, d_o.p, d_d.p, n, opts, ws.rad.p, stats, s, t0)) return r;
        HIP_TRY(hipMemcpy(out4, ws.rad.p, (size_t)n * 16, hipMemcpyDeviceToHost));
        return VMX_OK;
    };
    rc = body();
    if (rc) (void)hipStreamSynchronize(s);  // (what was enqueued may still use d_o / d_d, which are freed here)
    return rc;
}

}  // extern "C"
