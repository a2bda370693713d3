// api_bruteforce.inc — part of vmx_api.cpp: BruteForceTracer::Render on the device, vmx_render_bruteforce*
namespace {

// BruteForceTracer::Render (integrators.cpp:9-186) on the device
int bruteforce_impl(vmx_scene *sc, const vmx_camera *cam, const vmx_opts *opts, uint32_t flags, float *d_out,
                    hipStream_t s, vmx_stats *stats) {
    CallScope call{sc, s, std::chrono::steady_clock::now()};
    vmx_camera c = *cam;
    if (c.rays_per_pixel == 0 || c.rays_per_pixel > 65535)
        return fail(VMX_ERR_INVALID, "BruteForceTracer: rays_per_pixel must be 1..65535 (uint16_t sample counter, integrators.cpp:59)");
    if (flags & ~VMX_BF_ABS_INT) return fail(VMX_ERR_INVALID, "unknown BruteForceTracer flag");
    const uint32_t spp = c.rays_per_pixel;
    c.rays_per_pixel = std::max(spp, 4u);  // make_frame's PathTracer-only check (spp/4 strata) does not apply here
    vmx_opts o = *opts;
    o.sampling = VMX_SAMPLING_PARITY;
    FrameDev fr;
    int rc = make_frame(c, o, fr);
    if (rc) return rc;
    fr.spp = spp;
    if ((rc = sc->upd.done.wait(s))) return rc;
    Workspace &ws = sc->ws;
    const uint32_t W = fr.width, rows = fr.local_rows, npix = W * rows;
    if (npix == 0) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return VMX_OK;
    }
    // rad doubles as the list of pixels that go on past the first samples (64 bytes each, at most every pixel)
    if (ws.pixels.active[0].ensure(npix) || ws.counters.ensure(1) || ws.rad.ensure((size_t)npix * 64) || ws.next_count.ensure(32))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed for the render workspace");
    if (ws.order_w != W || ws.order_rows != rows) {
        tile_order(W, rows, ws.order);
        ws.order_w = W, ws.order_rows = rows;
    }
    std::vector<TimedLaunch> timed;
    if ((rc = call.open())) return rc;
    HIP_TRY(hipMemcpyAsync(ws.pixels.active[0].p, ws.order.data(), (size_t)npix * 4, hipMemcpyHostToDevice, s));
    if ((rc = call.clear_counters())) return rc;
    HIP_TRY(hipMemsetAsync(ws.next_count.p, 0, 4, s));
    if ((rc = call.start())) return rc;
    // stack as in the traversal kernels: a few levels per lane in LDS, the rest in the global slab (the whole stack
    // in LDS leaves room for 3 waves per SIMD: 28 -> 20 ms for the 16-spp frame)
    const Tuning tn = make_tuning(sc, &o);
    LaunchCfg cfg = paths_cfg(sc, tn.lds_entries, (uint64_t)npix, 5);
    WorkDev stack = make_work(nullptr, nullptr);
    rc = bind_stack(sc, tn, tn.lds_entries, cfg.grid, (uint64_t)npix, stack);
    if (rc) return rc;
    // (one event pair per kernel: the host reads the long-pixel count between the two, and that round trip is not
    // device time)
    if ((rc = timed_begin(ws, timed, s, 0, VMX_K_BRUTEFORCE))) return rc;
    LAUNCH_TRY(launch_bruteforce(sc->dev, fr, ws.pixels.active[0].p, npix, flags, d_out, ws.counters.p, ws.rad.p, ws.next_count.p,
                                 stack, cfg, s));
    if ((rc = timed_end(timed, s))) return rc;
    uint64_t launches = 1;
    unsigned int n_long = 0;  // pixels the break has not stopped within the first samples: a wave each from here
    HIP_TRY(hipMemcpyAsync(&n_long, ws.next_count.p, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (n_long != 0) {
        if ((rc = timed_begin(ws, timed, s, 0, VMX_K_BRUTEFORCE))) return rc;
        LAUNCH_TRY(launch_bruteforce_long(sc->dev, fr, flags, d_out, ws.counters.p, ws.rad.p, ws.next_count.p, n_long, stack, cfg, s));
        if ((rc = timed_end(timed, s))) return rc;
        launches++;
    }
    return call.finish(timed, stats, 1, launches);
}

}  // namespace

extern "C" {

int vmx_render_bruteforce_device(const vmx_scene *csc, const vmx_camera *cam, const vmx_opts *opts, uint32_t flags,
                                 void *d_out_rgbaz, void *stream, vmx_stats *stats) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!sc || !cam || !opts || !d_out_rgbaz) return fail(VMX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(sc->mu);
    int rc = bind_device(sc);
    if (rc) return rc;
    return bruteforce_impl(sc, cam, opts, flags, (float *)d_out_rgbaz, stream ? (hipStream_t)stream : sc->stream, stats);
}

int vmx_render_bruteforce(const vmx_scene *csc, const vmx_camera *cam, const vmx_opts *opts, uint32_t flags,
                          float *out_rgbaz, vmx_stats *stats) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!sc || !cam || !opts || !out_rgbaz) return fail(VMX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(sc->mu);
    int rc = bind_device(sc);
    if (rc) return rc;
    if (cam->image_res[0] == 0 || cam->image_res[1] == 0) return fail(VMX_ERR_INVALID, "image resolution must be non-zero");
    if (opts->world > 1 && opts->rank >= opts->world) return fail(VMX_ERR_INVALID, "rank must be < world");
    const uint32_t rows = local_rows_of(cam->image_res[1], opts->stripe_rows ? opts->stripe_rows : 16u,
                                        opts->world <= 1 ? 0u : opts->rank, opts->world <= 1 ? 1u : opts->world);
    const size_t nfloats = (size_t)cam->image_res[0] * rows * 5;
    if (nfloats == 0) return VMX_OK;
    if (sc->ws.out.ensure(nfloats)) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the frame buffer");
    rc = bruteforce_impl(sc, cam, opts, flags, sc->ws.out.p, sc->stream, stats);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_rgbaz, sc->ws.out.p, nfloats * 4, hipMemcpyDeviceToHost));
    return VMX_OK;
}

} /* extern "C" */
