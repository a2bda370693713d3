// api_multi.inc — part of vmx_api.cpp
struct ReplicaWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false, done = false, quit = false;
    void start() {
        th = std::thread([this]() {
            std::unique_lock<std::mutex> lk(mu);
            for (;;) {
                cv.wait(lk, [this]() { return has_job || quit; });
                if (quit) return;
                std::function<void()> j = std::move(job);
                has_job = false;
                lk.unlock();
                j();
                lk.lock();
                done = true;
                cv.notify_all();
            }
        });
    }
    void submit(std::function<void()> j) {
        std::lock_guard<std::mutex> lk(mu);
        job = std::move(j), has_job = true, done = false;
        cv.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [this]() { return done; });
    }
    void stop() {
        {
            std::lock_guard<std::mutex> lk(mu);
            quit = true;
            cv.notify_all();
        }
        if (th.joinable()) th.join();
    }
};

struct vmx_multi {
    std::vector<vmx_scene *> replica;  // one scene replica per entry of the device list (entries may repeat)
    std::vector<std::unique_ptr<ReplicaWorker>> worker;
    // how replica r's stripes reach the root: 2 same device, 1 direct peer copy (xGMI), 0 staged through the host
    std::vector<int> route;
    DevBuf<float> gathered, frame;     // on the root = replica[0]'s device
    std::mutex mu;
    // the exchange step of the last render, timed apart from the rendering (SURVEY 8e: "gather time separately"):
    // per replica the device time of its render and of its stripes' copy into the root's gather buffer (hipEvent pairs
    // on the replica's stream), the de-interleave kernel on the root, and the host's wall clock around all of it
    std::vector<double> render_ms, copy_ms;
    std::vector<hipEvent_t> copy_ev;   // two per replica, created on the replica's device by its worker
    hipEvent_t asm_ev[2] = {nullptr, nullptr};
    double assemble_ms = 0.0, wall_ms = 0.0;
};

namespace {

template <class RenderFn>
int multi_render(vmx_multi *m, const vmx_camera *cam, const vmx_opts *opts, float *out_host, void *d_out_root,
                 vmx_stats *stats, RenderFn render_one) {
    const uint32_t world = (uint32_t)m->replica.size();
    const uint32_t W = cam->image_res[0], H = cam->image_res[1];
    if (W == 0 || H == 0) return fail(VMX_ERR_INVALID, "image resolution must be non-zero");
    const uint32_t stripe = opts->stripe_rows ? opts->stripe_rows : 16u;
    uint32_t max_rows = 0;
    for (uint32_t r = 0; r < world; ++r) max_rows = std::max(max_rows, local_rows_of(H, stripe, r, world));
    const uint64_t stride = (uint64_t)max_rows * W * 5;  // floats per rank slot of the gather buffer
    vmx_scene *root = m->replica[0];
    HIP_TRY(hipSetDevice(root->device));
    if (m->gathered.ensure((size_t)stride * world) || m->frame.ensure((size_t)W * H * 5))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed for the gather buffer");

    // one host thread per replica: render its interleaved stripes into its own device buffer, then push
    // them into the root's gather buffer — a device-to-device copy (peer copy over xGMI when the replica
    // sits on another GPU: every peer has its own link to the root, SURVEY 8e; not a ring)
    std::vector<int> rc(world, VMX_OK);
    std::vector<std::string> msg(world);
    std::vector<vmx_stats> st(world);
    const auto wall0 = std::chrono::steady_clock::now();
    m->render_ms.assign(world, 0.0), m->copy_ms.assign(world, 0.0);
    m->copy_ev.resize((size_t)world * 2, nullptr);
    for (uint32_t r = 0; r < world; ++r) {
        m->worker[r]->submit([&, r]() {
            vmx_scene *sc = m->replica[r];
            vmx_opts o = *opts;
            o.rank = r, o.world = world, o.stripe_rows = stripe;
            std::lock_guard<std::mutex> lock(sc->mu);
            auto body = [&]() -> int {
                int e = bind_device(sc);
                if (e) return e;
                const size_t nfloats = (size_t)local_rows_of(H, stripe, r, world) * W * 5;
                if (nfloats == 0) return VMX_OK;
                if (sc->ws.out.ensure(nfloats)) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the frame buffer");
                e = render_one(sc, &o, sc->ws.out.p, &st[r]);
                if (e) return e;
                hipEvent_t *ev = &m->copy_ev[(size_t)r * 2];
                for (int k = 0; k < 2; ++k)
                    if (!ev[k]) HIP_TRY(hipEventCreate(&ev[k]));
                HIP_TRY(hipEventRecord(ev[0], sc->stream));
                HIP_TRY(hipMemcpyPeerAsync(m->gathered.p + (size_t)stride * r, root->device, sc->ws.out.p, sc->device,
                                           nfloats * 4, sc->stream));
                HIP_TRY(hipEventRecord(ev[1], sc->stream));
                HIP_TRY(hipStreamSynchronize(sc->stream));
                float ms = 0.f;
                HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
                m->copy_ms[r] = ms, m->render_ms[r] = st[r].ms_device;
                return VMX_OK;
            };
            std::memset(&st[r], 0, sizeof(vmx_stats));
            rc[r] = body();
            if (rc[r]) msg[r] = g_err;  // g_err is thread-local
        });
    }
    for (uint32_t r = 0; r < world; ++r) m->worker[r]->wait();
    for (uint32_t r = 0; r < world; ++r)
        if (rc[r]) return fail(rc[r], "device " + std::to_string(m->replica[r]->device) + ": " + msg[r]);

    HIP_TRY(hipSetDevice(root->device));
    float *d_frame = d_out_root ? (float *)d_out_root : m->frame.p;
    for (int k = 0; k < 2; ++k)
        if (!m->asm_ev[k]) HIP_TRY(hipEventCreate(&m->asm_ev[k]));
    HIP_TRY(hipEventRecord(m->asm_ev[0], root->stream));
    LAUNCH_TRY(launch_assemble(m->gathered.p, stride, W, H, stripe, world, d_frame, root->stream));
    HIP_TRY(hipEventRecord(m->asm_ev[1], root->stream));
    if (out_host) HIP_TRY(hipMemcpyAsync(out_host, d_frame, (size_t)W * H * 5 * 4, hipMemcpyDeviceToHost, root->stream));
    HIP_TRY(hipStreamSynchronize(root->stream));
    {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, m->asm_ev[0], m->asm_ev[1]));
        m->assemble_ms = ms;
        m->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        for (uint32_t r = 0; r < world; ++r) {
            const vmx_stats &a = st[r];
            stats->rays_primary += a.rays_primary, stats->rays_secondary += a.rays_secondary;
            stats->samples += a.samples, stats->samples_discarded += a.samples_discarded;
            stats->kernel_launches += a.kernel_launches;
            stats->passes = std::max(stats->passes, a.passes);
            stats->ms_total = std::max(stats->ms_total, a.ms_total);     // ranks run side by side: the slowest one
            stats->ms_device = std::max(stats->ms_device, a.ms_device);
            vmx_stage_stats *dst[3] = {&stats->primary, &stats->bounce, &stats->shade};
            const vmx_stage_stats *src[3] = {&a.primary, &a.bounce, &a.shade};
            for (int k = 0; k < 3; ++k) {
                dst[k]->rays += src[k]->rays, dst[k]->inner_visits += src[k]->inner_visits;
                dst[k]->tri_tests += src[k]->tri_tests, dst[k]->tri_hits += src[k]->tri_hits;
                dst[k]->continued += src[k]->continued, dst[k]->launches += src[k]->launches;
                dst[k]->ms = std::max(dst[k]->ms, src[k]->ms);
            }
        }
    }
    return VMX_OK;
}

}  // namespace

extern "C" {

int vmx_multi_create(const float *pos, const float *nrm, const float *uv, uint32_t ntris, const vmx_sphere *spheres,
                     uint32_t nspheres, uint32_t leaf_size, uint32_t builder, const int *devices, uint32_t ndevices,
                     vmx_multi **out) {
    if (!out) return fail(VMX_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!devices || ndevices == 0 || ndevices > 64) return fail(VMX_ERR_INVALID, "device list must hold 1..64 entries");
    vmx_scene *first = nullptr;
    int rc = vmx_scene_create_ex(pos, nrm, uv, ntris, spheres, nspheres, leaf_size, builder, devices[0], &first);
    if (rc) return rc;
    vmx_multi *m = new vmx_multi();
    m->replica.push_back(first);
    m->route.push_back(2);
    int ndev = 0;
    (void)hipGetDeviceCount(&ndev);
    for (uint32_t i = 1; i < ndevices; ++i) {
        if (devices[i] < 0 || devices[i] >= ndev) {
            vmx_multi_destroy(m);
            return fail(VMX_ERR_NO_DEVICE, "device ordinal out of range");
        }
        vmx_scene *sc = nullptr;
        if (first->device_built) {
            // a device-built tree is built again on every device (deterministic: same sort, same boxes)
            rc = vmx_scene_create_ex(pos, nrm, uv, ntris, spheres, nspheres, leaf_size, builder, devices[i], &sc);
            if (rc) {
                const std::string keep = g_err;
                vmx_multi_destroy(m);
                return fail(rc, keep);
            }
        } else {
            sc = new vmx_scene();  // replica: shares the host-side build, uploads to its own device
            sc->device = devices[i];
            sc->builder = first->builder;
            sc->ntris = first->ntris, sc->leaf_size = first->leaf_size;
            sc->bvh = first->bvh;
            sc->guide.host = first->guide.host, sc->guide.scene_max = first->guide.scene_max;
            sc->spheres = first->spheres;
            std::memcpy(sc->bounds_lo, first->bounds_lo, sizeof(sc->bounds_lo));
            std::memcpy(sc->bounds_hi, first->bounds_hi, sizeof(sc->bounds_hi));
            rc = scene_upload(sc);
            if (rc) {
                const std::string keep = g_err;
                vmx_scene_destroy(sc);
                vmx_multi_destroy(m);
                return fail(rc, keep);
            }
        }
        m->replica.push_back(sc);
        // direct peer copies into the root's gather buffer (xGMI); without peer access the runtime stages
        // the copy through the host, which is slower but still correct
        int route = 2;
        if (devices[i] != devices[0]) {
            route = 0;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, devices[i], devices[0]) == hipSuccess && can) {
                (void)hipSetDevice(devices[i]);
                const hipError_t e = hipDeviceEnablePeerAccess(devices[0], 0);
                // every non-success return (AlreadyEnabled included: a device listed twice, a second vmx_multi in the
                // process) stays behind as the thread's last error and would fail the next launch's status check
                if (e != hipSuccess) (void)hipGetLastError();
                if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) route = 1;
                else
                    std::fprintf(stderr, "vermilion_hip: peer access %d -> %d failed (%s): stripes of device %d are staged "
                                 "through the host\n", devices[i], devices[0], hipGetErrorString(e), devices[i]);
            } else {
                (void)hipGetLastError();
            }
        }
        m->route.push_back(route);
    }
    for (size_t i = 0; i < m->replica.size(); ++i) {
        m->worker.emplace_back(new ReplicaWorker());
        m->worker.back()->start();
    }
    *out = m;
    return VMX_OK;
}

int vmx_multi_destroy(vmx_multi *m) {
    if (!m) return VMX_OK;
    for (auto &w : m->worker) w->stop();
    for (size_t i = 0; i < m->copy_ev.size(); ++i)
        if (m->copy_ev[i]) {
            (void)hipSetDevice(m->replica[i / 2]->device);
            (void)hipEventDestroy(m->copy_ev[i]);
        }
    const int root = m->replica[0]->device;  // (a vmx_multi holds at least its first replica)
    for (vmx_scene *sc : m->replica) vmx_scene_destroy(sc);
    (void)hipSetDevice(root);
    for (int k = 0; k < 2; ++k)
        if (m->asm_ev[k]) (void)hipEventDestroy(m->asm_ev[k]);
    delete m;  // the gather buffer and the frame
    return VMX_OK;
}

uint32_t vmx_multi_world(const vmx_multi *m) { return m ? (uint32_t)m->replica.size() : 0u; }

int vmx_multi_routes(const vmx_multi *m, int *devices, int *routes) {
    if (!m) return fail(VMX_ERR_INVALID, "NULL argument");
    for (size_t i = 0; i < m->replica.size(); ++i) {
        if (devices) devices[i] = m->replica[i]->device;
        if (routes) routes[i] = m->route[i];
    }
    return VMX_OK;
}

int vmx_multi_timings(const vmx_multi *cm, vmx_multi_times *out, double *render_ms, double *copy_ms) {
    vmx_multi *m = const_cast<vmx_multi *>(cm);
    if (!m || !out) return fail(VMX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(m->mu);
    std::memset(out, 0, sizeof(*out));
    out->world = (uint32_t)m->replica.size();
    for (size_t r = 0; r < m->render_ms.size(); ++r) {
        out->slowest_render_ms = std::max(out->slowest_render_ms, m->render_ms[r]);
        out->gather_ms = std::max(out->gather_ms, m->copy_ms[r]);
        out->gather_sum_ms += m->copy_ms[r];
        if (render_ms) render_ms[r] = m->render_ms[r];
        if (copy_ms) copy_ms[r] = m->copy_ms[r];
    }
    out->assemble_ms = m->assemble_ms;
    out->wall_ms = m->wall_ms;
    return VMX_OK;
}

int vmx_multi_bind_texture(vmx_multi *m, const float *data, uint32_t width, uint32_t height, uint32_t channels) {
    if (!m) return fail(VMX_ERR_INVALID, "NULL argument");
    for (vmx_scene *sc : m->replica) {
        const int rc = vmx_scene_bind_texture(sc, data, width, height, channels);
        if (rc) return rc;
    }
    return VMX_OK;
}

int vmx_multi_render(vmx_multi *m, const vmx_camera *cam, const vmx_opts *opts, float *out_rgbaz, vmx_stats *stats) {
    if (!m || !cam || !opts || !out_rgbaz) return fail(VMX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(m->mu);
    return multi_render(m, cam, opts, out_rgbaz, nullptr, stats,
                        [&](vmx_scene *sc, const vmx_opts *o, float *d_out, vmx_stats *st) {
                            return render_impl(sc, cam, o, d_out, sc->stream, st);
                        });
}

int vmx_multi_render_device(vmx_multi *m, const vmx_camera *cam, const vmx_opts *opts, void *d_out_rgbaz,
                            vmx_stats *stats) {
    if (!m || !cam || !opts || !d_out_rgbaz) return fail(VMX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(m->mu);
    return multi_render(m, cam, opts, nullptr, d_out_rgbaz, stats,
                        [&](vmx_scene *sc, const vmx_opts *o, float *d_out, vmx_stats *st) {
                            return render_impl(sc, cam, o, d_out, sc->stream, st);
                        });
}

int vmx_multi_render_bruteforce(vmx_multi *m, const vmx_camera *cam, const vmx_opts *opts, uint32_t flags,
                                float *out_rgbaz, vmx_stats *stats) {
    if (!m || !cam || !opts || !out_rgbaz) return fail(VMX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(m->mu);
    return multi_render(m, cam, opts, out_rgbaz, nullptr, stats,
                        [&](vmx_scene *sc, const vmx_opts *o, float *d_out, vmx_stats *st) {
                            return bruteforce_impl(sc, cam, o, flags, d_out, sc->stream, st);
                        });
}

// Light sampling over the device list: every replica renders its stripes through the routine of vmx_render_nee_rank*
// (nee_render_impl).  The opts are checked as vmx_render_nee checks them — a caller's world > 1 is refused, the library
// sets rank and world — and the vmx_multi comes last, so that each refusal can be seen without a device.
static int multi_render_nee(vmx_multi *m, const vmx_camera *cam, const vmx_opts *opts, float *out_host, void *d_out_root,
                            vmx_stats *stats) {
    if (!cam || !opts || (!out_host && !d_out_root)) return fail(VMX_ERR_INVALID, "NULL argument");
    if (int rc = nee_check_opts(opts)) return rc;
    if (!m) return fail(VMX_ERR_INVALID, "NULL vmx_multi");
    std::lock_guard<std::mutex> lock(m->mu);
    return multi_render(m, cam, opts, out_host, d_out_root, stats,
                        [&](vmx_scene *sc, const vmx_opts *o, float *d_out, vmx_stats *st) {
                            return nee_render_impl(sc, cam, o, d_out, sc->stream, st);
                        });
}

int vmx_multi_render_nee(vmx_multi *m, const vmx_camera *cam, const vmx_opts *opts, float *out_rgbaz, vmx_stats *stats) {
    return multi_render_nee(m, cam, opts, out_rgbaz, nullptr, stats);
}

int vmx_multi_render_nee_device(vmx_multi *m, const vmx_camera *cam, const vmx_opts *opts, void *d_out_rgbaz, vmx_stats *stats) {
    return multi_render_nee(m, cam, opts, nullptr, d_out_rgbaz, stats);
}

} /* extern "C" */

extern "C" {

int vmx_assemble_device(const void *d_gathered, uint64_t rank_stride_floats, uint32_t width, uint32_t height,
                        uint32_t stripe_rows, uint32_t world, void *d_frame, int device, void *stream) {
    if (!d_gathered || !d_frame || width == 0 || height == 0 || world == 0)
        return fail(VMX_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(device));
    LAUNCH_TRY(launch_assemble((const float *)d_gathered, rank_stride_floats, width, height,
                               stripe_rows ? stripe_rows : 16u, world, (float *)d_frame, stream));
    if (!stream) HIP_TRY(hipDeviceSynchronize());
    return VMX_OK;
}

int vmx_quantize_device(const void *d_frame_rgbaz, uint64_t npixels, void *d_rgba8, void *d_depth, int device,
                        void *stream) {
    if (!d_frame_rgbaz || !d_rgba8) return fail(VMX_ERR_INVALID, "NULL argument");
    if (npixels == 0) return VMX_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(VMX_ERR_NO_DEVICE, "no such HIP device");
    HIP_TRY(hipSetDevice(device));
    LAUNCH_TRY(launch_quantize((const float *)d_frame_rgbaz, npixels, d_rgba8, (float *)d_depth, stream));
    if (!stream) HIP_TRY(hipDeviceSynchronize());
    return VMX_OK;
}

} /* extern "C" */
