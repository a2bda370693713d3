// api_query.inc — part of vmx_api.cpp
namespace {

// The staging of a host-pointer entry: device room for its arrays (none for a NULL one), the inputs copied in, the
// outputs copied back, and one synchronise before the buffers go.  The first HIP error is kept, skips what follows, and
// is reported under the entry's name.
struct Staging {
    struct Copy {
        void *host, *dev;
        size_t bytes;
    };
    hipStream_t s;
    const char *entry;
    hipError_t e = hipSuccess;
    bool nomem = false;
    std::vector<DevBuf<unsigned char>> bufs;
    std::vector<Copy> ins, outs;
    Staging(hipStream_t s_, const char *entry_) : s(s_), entry(entry_) {}
    void *add(std::vector<Copy> &list, const void *host, size_t bytes) {
        if (!host) return nullptr;
        bufs.emplace_back();
        if (bufs.back().ensure(bytes)) nomem = true;
        list.push_back({const_cast<void *>(host), bufs.back().p, bytes});
        return bufs.back().p;
    }
    template <class T>
    T *in(const T *host, size_t n) { return (T *)add(ins, host, n * sizeof(T)); }
    template <class T>
    T *out(T *host, size_t n) { return (T *)add(outs, host, n * sizeof(T)); }
    bool ok() const { return e == hipSuccess; }
    void copy_in() {
        for (const Copy &c : ins)
            if (ok()) e = hipMemcpyAsync(c.dev, c.host, c.bytes, hipMemcpyHostToDevice, s);
    }
    int finish() {
        for (const Copy &c : outs)
            if (ok()) e = hipMemcpyAsync(c.host, c.dev, c.bytes, hipMemcpyDeviceToHost, s);
        const hipError_t es = hipStreamSynchronize(s);  // (whatever failed: nothing in flight may outlive the buffers)
        if (ok()) e = es;
        if (!ok()) return fail(VMX_ERR_HIP, std::string(entry) + ": " + hipGetErrorString(e));
        return VMX_OK;
    }
};

}  // namespace

extern "C" {

int vmx_trace(const vmx_scene *csc, const float *origin, const float *dir, uint32_t n, int32_t *tri_id,
              float *t) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!sc || !origin || !dir || !tri_id || !t) return fail(VMX_ERR_INVALID, "NULL argument");
    if (n == 0) return VMX_OK;
    std::lock_guard<std::mutex> lock(sc->mu);
    int rc = bind_device(sc);
    if (rc) return rc;
    if ((rc = sc->upd.done.wait(sc->stream))) return rc;
    Staging st(sc->stream, "vmx_trace");
    const float *d_o = st.in(origin, (size_t)n * 3), *d_d = st.in(dir, (size_t)n * 3);
    int32_t *d_id = st.out(tri_id, n);
    float *d_t = st.out(t, n);
    if (st.nomem) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the ray batch");
    st.copy_in();
    if (st.ok()) {
        LaunchCfg cfg = trace_cfg(sc, (n + sc->block - 1) / sc->block, 4);
        st.e = (hipError_t)launch_trace(sc->dev, d_o, d_d, n, d_id, d_t, nullptr, false, cfg, st.s);
    }
    return st.finish();
}

int vmx_raycast(const vmx_scene *csc, const float *origin, const float *dir, uint32_t n, vmx_rayhit *out) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!sc || !origin || !dir || !out) return fail(VMX_ERR_INVALID, "NULL argument");
    if (n == 0) return VMX_OK;
    static_assert(sizeof(vmx_rayhit) == 64, "vmx_rayhit must be 64 bytes");
    std::lock_guard<std::mutex> lock(sc->mu);
    int rc = bind_device(sc);
    if (rc) return rc;
    if ((rc = sc->upd.done.wait(sc->stream))) return rc;
    Staging st(sc->stream, "vmx_raycast");
    const float *d_o = st.in(origin, (size_t)n * 3), *d_d = st.in(dir, (size_t)n * 3);
    vmx_rayhit *d_out = st.out(out, n);
    if (st.nomem) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the ray batch");
    st.copy_in();
    if (st.ok()) {
        LaunchCfg cfg = trace_cfg(sc, (n + sc->block - 1) / sc->block, 4);
        st.e = (hipError_t)launch_raycast(sc->dev, d_o, d_d, n, d_out, cfg, st.s);
    }
    return st.finish();
}

// ---- device ray queries (k_query, vmx_query.inc) -------------------------------------------------------
namespace {

constexpr uint32_t kQueryBlock = 256;
constexpr uint32_t kQueryModeMask = 0xFFu;

// argument checks that need no device: mode, rays, the output set (in this order, so that each can be seen alone)
int query_args(const vmx_scene *sc, uint32_t mode, const void *o, const void *d, uint32_t n, const void *tri_id,
               const void *t, const void *hit) {
    if ((mode & ~(kQueryModeMask | VMX_QUERY_FETCH_PER_LANE)) || (mode & kQueryModeMask) > VMX_QUERY_COLLISION)
        return fail(VMX_ERR_INVALID, "unknown query mode");
    if (n > 0 && (!o || !d)) return fail(VMX_ERR_INVALID, "NULL rays");
    if (n > 0 && !tri_id && !t && !hit) return fail(VMX_ERR_INVALID, "no output: tri_id, t and hit are all NULL");
    if ((mode & kQueryModeMask) == VMX_QUERY_ANY && (tri_id || t))
        return fail(VMX_ERR_INVALID, "VMX_QUERY_ANY returns hit only: tri_id and t must be NULL");
    if (!sc) return fail(VMX_ERR_INVALID, "NULL scene");
    return VMX_OK;
}

// `p` must be device memory of `device`: a host pointer handed to the kernel would fault the GPU
int check_device_ptr(const void *p, int device, const char *what) {
    if (!p) return VMX_OK;
    hipPointerAttribute_t a;
    std::memset(&a, 0, sizeof(a));
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // (an unknown pointer sets the thread's error state)
        return fail(VMX_ERR_INVALID, std::string(what) + " is not device memory");
    }
    if (a.type != hipMemoryTypeDevice) return fail(VMX_ERR_INVALID, std::string(what) + " is not device memory");
    if (a.device != device) return fail(VMX_ERR_INVALID, std::string(what) + " is memory of another device");
    return VMX_OK;
}

// the same for a call's pointers, in the order given
static int check_device_ptrs(int device, std::initializer_list<std::pair<const void *, const char *>> ptrs) {
    for (const auto &p : ptrs)
        if (int rc = check_device_ptr(p.first, device, p.second)) return rc;
    return VMX_OK;
}

// first query of a scene: launch shapes from the occupancy of each instantiation, work counter, overflow slab
int ensure_query_ws(vmx_scene *sc) {
    auto &q = sc->qws;
    if (q.stack_entries == sc->dev.stack_entries) return VMX_OK;  // (0 before the first query; a tree's is >= 2)
    // first query, or the tree's depth changed (VMX_UPDATE_REBUILD): the slab is sized again, once no query uses it
    if (int rc = q.done.sync()) return rc;
    // stack levels in LDS: the bounce kernel's 9 (make_tuning); deeper levels go to the slab
    q.lds_entries = std::min(sc->dev.stack_entries, 9u);
    q.overflow_entries = sc->dev.stack_entries + 1 > q.lds_entries ? sc->dev.stack_entries + 1 - q.lds_entries : 1u;
    const uint32_t lds = (kQueryBlock / 64) * (q.lds_entries + 1) * 512;
    uint32_t max_grid = 1;
    for (int pl = 0; pl < 2; ++pl)
        for (uint32_t m = 0; m < kQueryModes; ++m) {
            int b = 0;
            HIP_TRY((hipError_t)query_query_blocks_per_cu(kQueryBlock, lds, m, pl == 0, &b));
            q.grid[pl][m] = (uint32_t)sc->num_cus * (uint32_t)std::max(b, 1);
            max_grid = std::max(max_grid, q.grid[pl][m]);
        }
    if (q.head.ensure(32) || q.overflow_stack.ensure((size_t)max_grid * (kQueryBlock / 64) * q.overflow_entries * 64 * 8))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed for the query workspace");
    q.stack_entries = sc->dev.stack_entries;
    return VMX_OK;
}

// QueryDev (work source and stack, no rays or outputs) and launch shape of one query of n rays in mode m
void query_shape(const vmx_scene *sc, uint32_t m, bool quad, uint32_t n, QueryDev &q, LaunchCfg &cfg) {
    const auto &w = sc->qws;
    q = QueryDev{};
    q.n = n;
    q.head = w.head.p;
    q.lds_entries = w.lds_entries, q.overflow_entries = w.overflow_entries;
    q.overflow_stack = w.overflow_stack.p;
    // refill as soon as 8 lanes are idle: the bounce kernel's setting for incoherent rays (make_tuning)
    q.refill_min = 8;
    cfg.block = kQueryBlock;
    cfg.lds_bytes = (kQueryBlock / 64) * (w.lds_entries + 1) * 512;
    cfg.grid = (uint32_t)std::min<uint64_t>(w.grid[quad ? 0 : 1][m], std::max<uint64_t>(1, ((uint64_t)n + kQueryBlock - 1) / kQueryBlock));
    // reservation per atomic: WorkDev::reserve's rule (bind_stack)
    const uint64_t per_lane = n / ((uint64_t)cfg.grid * kQueryBlock);
    q.reserve = per_lane >= 256 ? 256u : (per_lane >= 64 ? 128u : 64u);
}

// a query's kernels on `s` run after the previous query (the workspace) and the last update, and reset the counter
int query_begin(vmx_scene *sc, hipStream_t s) {
    auto &w = sc->qws;
    if (int rc = w.done.wait(s)) return rc;
    if (int rc = sc->upd.done.wait(s)) return rc;
    HIP_TRY(hipMemsetAsync(w.head.p, 0, sizeof(unsigned int), s));
    return VMX_OK;
}

// after a query's last kernel: the next query and the next update wait for it
int query_end(vmx_scene *sc, hipStream_t s) { return sc->qws.done.record(s); }

// enqueues one query on `s`; the caller holds sc->mu and has checked the arguments
int query_enqueue(vmx_scene *sc, uint32_t mode, const float *o, const float *d, const float *tmax, uint32_t n,
                  int32_t *tri_id, float *t, uint8_t *hit, hipStream_t s) {
    if (int rc = ensure_query_ws(sc)) return rc;
    const uint32_t m = mode & kQueryModeMask;
    const bool quad = (mode & VMX_QUERY_FETCH_PER_LANE) == 0;
    QueryDev q;
    LaunchCfg cfg;
    query_shape(sc, m, quad, n, q, cfg);
    q.o = o, q.d = d, q.tmax = tmax;
    q.tri_id = tri_id, q.t = t, q.hit = hit;
    if (int rc = query_begin(sc, s)) return rc;
    LAUNCH_TRY(launch_query(sc->dev, q, m, quad, cfg, s));
    return query_end(sc, s);
}

// ---- MeshEngine::RayCast of device batches (k_query_cast + k_raycast_finish) ----------------------------------
// argument checks that need no device, in this order (each can be seen alone): flags, rays, output, count, the
// output's alignment and overlap with the rays; the NULL scene comes last (vmx_raycast_device_args / _camera_args)
int raycast_flags(uint32_t flags) {
    if (flags & ~VMX_QUERY_FETCH_PER_LANE) return fail(VMX_ERR_INVALID, "unknown raycast flags");
    return VMX_OK;
}

int raycast_out(const void *out) {
    if (!out) return fail(VMX_ERR_INVALID, "NULL d_out");
    if ((uintptr_t)out & 15u) return fail(VMX_ERR_INVALID, "d_out must be 16-byte aligned");
    return VMX_OK;
}

int raycast_args(const vmx_scene *sc, const void *o, const void *d, uint32_t n, const void *out, uint32_t flags) {
    if (int rc = raycast_flags(flags)) return rc;
    if (n > 0 && (!o || !d)) return fail(VMX_ERR_INVALID, "NULL rays");
    if (n > 0)
        if (int rc = raycast_out(out)) return rc;
    if (n > 0x7FFFFFFFu) return fail(VMX_ERR_INVALID, "more than 2^31 - 1 rays");
    if (n > 0) {
        // the records are written while the rays are still read: [out, out + 64 n) must not meet either ray array
        const uintptr_t a = (uintptr_t)out, b = a + (uintptr_t)n * sizeof(vmx_rayhit);
        const uintptr_t ro[2] = {(uintptr_t)o, (uintptr_t)d};
        for (uintptr_t r : ro)
            if (r < b && a < r + (uintptr_t)n * 12) return fail(VMX_ERR_INVALID, "d_out overlaps the rays");
    }
    if (!sc) return fail(VMX_ERR_INVALID, "NULL scene");
    return VMX_OK;
}

// flags, camera / opts, output, the frame (make_frame's checks), world, sample index; the NULL scene comes last
int raycast_camera_args(const vmx_scene *sc, const vmx_camera *cam, const vmx_opts *opts, uint32_t k, const void *out,
                        uint32_t flags, FrameDev &fr) {
    if (int rc = raycast_flags(flags)) return rc;
    if (!cam || !opts) return fail(VMX_ERR_INVALID, "NULL camera or opts");
    if (int rc = raycast_out(out)) return rc;
    if (int rc = make_frame(*cam, *opts, fr)) return rc;
    if (opts->world > 1) return fail(VMX_ERR_INVALID, "world > 1: the camera raycast returns the whole image only");
    if (k >= fr.kmax) return fail(VMX_ERR_INVALID, "sample index out of range");
    if (!sc) return fail(VMX_ERR_INVALID, "NULL scene");
    return VMX_OK;
}

// enqueues one raycast of n rays (camera: sample k's camera ray of every pixel of fr) on `s`; the caller holds sc->mu
// and has checked the arguments and pointers
int raycast_enqueue(vmx_scene *sc, bool camera, bool quad, const float *o, const float *d, uint32_t n, const FrameDev &fr,
                    uint32_t k, void *out, hipStream_t s) {
    if (int rc = ensure_query_ws(sc)) return rc;
    QueryDev q;
    LaunchCfg cfg;
    query_shape(sc, camera ? kQueryCastCamera : kQueryCastRays, quad, n, q, cfg);
    q.o = o, q.d = d, q.sample = k;
    // the finish kernel: one lane per ray, a few rays per lane at the largest sizes (its LDS table is staged per block)
    const uint32_t finish_grid = (uint32_t)std::min<uint64_t>(((uint64_t)n + 255) / 256, (uint64_t)std::max(sc->num_cus, 1) * 16);
    if (int rc = query_begin(sc, s)) return rc;
    LAUNCH_TRY(launch_raycast_query(sc->dev, q, fr, camera, quad, out, cfg, finish_grid, s));
    return query_end(sc, s);
}

}  // namespace

int vmx_query_device(const vmx_scene *csc, uint32_t mode, const void *d_origin, const void *d_dir, const void *d_tmax,
                     uint32_t n, void *d_tri_id, void *d_t, void *d_hit, void *stream) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (int rc = query_args(sc, mode, d_origin, d_dir, n, d_tri_id, d_t, d_hit)) return rc;
    if (n == 0) return VMX_OK;
    if (n > 0x7FFFFFFFu) return fail(VMX_ERR_INVALID, "more than 2^31 - 1 rays");
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (int rc = check_device_ptrs(sc->device, {{d_origin, "origin"}, {d_dir, "dir"}, {d_tmax, "tmax"}, {d_tri_id, "tri_id"}, {d_t, "t"}, {d_hit, "hit"}})) return rc;
    return query_enqueue(sc, mode, (const float *)d_origin, (const float *)d_dir, (const float *)d_tmax, n,
                         (int32_t *)d_tri_id, (float *)d_t, (uint8_t *)d_hit, stream ? (hipStream_t)stream : sc->stream);
}

int vmx_raycast_device(const vmx_scene *csc, const void *d_origin, const void *d_dir, uint32_t n, void *d_out,
                       uint32_t flags, void *stream) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (int rc = raycast_args(sc, d_origin, d_dir, n, d_out, flags)) return rc;
    if (n == 0) return VMX_OK;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (int rc = check_device_ptrs(sc->device, {{d_origin, "origin"}, {d_dir, "dir"}, {d_out, "d_out"}})) return rc;
    FrameDev fr;
    std::memset(&fr, 0, sizeof(fr));
    return raycast_enqueue(sc, false, (flags & VMX_QUERY_FETCH_PER_LANE) == 0, (const float *)d_origin,
                           (const float *)d_dir, n, fr, 0, d_out, stream ? (hipStream_t)stream : sc->stream);
}

int vmx_raycast_camera_device(const vmx_scene *csc, const vmx_camera *cam, const vmx_opts *opts, uint32_t k, void *d_out,
                              uint32_t flags, void *stream) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    FrameDev fr;
    if (int rc = raycast_camera_args(sc, cam, opts, k, d_out, flags, fr)) return rc;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (int rc = check_device_ptr(d_out, sc->device, "d_out")) return rc;
    return raycast_enqueue(sc, true, (flags & VMX_QUERY_FETCH_PER_LANE) == 0, nullptr, nullptr, fr.width * fr.height, fr,
                           k, d_out, stream ? (hipStream_t)stream : sc->stream);
}

int vmx_query(const vmx_scene *csc, uint32_t mode, const float *origin, const float *dir, const float *tmax, uint32_t n,
              int32_t *tri_id, float *t, uint8_t *hit) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (int rc = query_args(sc, mode, origin, dir, n, tri_id, t, hit)) return rc;
    if (n == 0) return VMX_OK;
    if (n > 0x7FFFFFFFu) return fail(VMX_ERR_INVALID, "more than 2^31 - 1 rays");
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    Staging st(sc->stream, "vmx_query");
    const float *d_o = st.in(origin, (size_t)n * 3), *d_d = st.in(dir, (size_t)n * 3), *d_tmax = st.in(tmax, n);
    int32_t *d_id = st.out(tri_id, n);
    float *d_t = st.out(t, n);
    uint8_t *d_hit = st.out(hit, n);
    if (st.nomem) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the ray batch");
    st.copy_in();
    if (!st.ok()) return st.finish();
    if (int rc = query_enqueue(sc, mode, d_o, d_d, d_tmax, n, d_id, d_t, d_hit, st.s)) {
        (void)hipStreamSynchronize(st.s);  // (part of it may be enqueued, and the buffers go)
        return rc;
    }
    return st.finish();
}

int vmx_primary_ids(const vmx_scene *csc, const vmx_camera *cam, const vmx_opts *opts, uint32_t k,
                    int32_t *tri_id, float *t) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!sc || !cam || !opts || !tri_id || !t) return fail(VMX_ERR_INVALID, "NULL argument");
    FrameDev fr;
    int rc = make_frame(*cam, *opts, fr);
    if (rc) return rc;
    if (k >= fr.kmax) return fail(VMX_ERR_INVALID, "sample index out of range");
    std::lock_guard<std::mutex> lock(sc->mu);
    rc = bind_device(sc);
    if (rc) return rc;
    if ((rc = sc->upd.done.wait(sc->stream))) return rc;
    const uint32_t n = fr.width * fr.height;
    Staging st(sc->stream, "vmx_primary_ids");
    int32_t *d_id = st.out(tri_id, n);
    float *d_t = st.out(t, n);
    if (st.nomem) return fail(VMX_ERR_NOMEM, "hipMalloc failed");
    LaunchCfg cfg = trace_cfg(sc, (n + sc->block - 1) / sc->block, 4);
    st.e = (hipError_t)launch_primary_ids(sc->dev, fr, k, d_id, d_t, cfg, st.s);
    return st.finish();
}

int vmx_radiance(const vmx_scene *csc, const float *origin, const float *dir, uint32_t n, const vmx_opts *opts,
                 float *out, vmx_stats *stats) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!sc || !origin || !dir || !opts || !out) return fail(VMX_ERR_INVALID, "NULL argument");
    if ((opts->sampling & VMX_SAMPLING_MODE_MASK) > VMX_SAMPLING_CORRECTED ||
        (opts->sampling & ~(VMX_SAMPLING_MODE_MASK | VMX_SAMPLING_LIBM_DOUBLE | VMX_SAMPLING_ELIDE_DEAD)))
        return fail(VMX_ERR_INVALID, "unknown sampling mode");
    // (kFormsRadiance, vmx_host.h: the bits of reserved[0] that select shading forms of vmx_render's split passes mean
    // nothing here and are accepted and ignored, as render_setup accepts them)
    Forms f;
    f.pipeline = opts->reserved[0] & kFormPipeline;
    if (f.pipeline > 4 || (opts->reserved[0] & ~kFormsRadiance)) return fail(VMX_ERR_INVALID, "unknown pipeline form");
    if (int rc = ab_check_forms(sc, f.pipeline)) return rc;
    if (n == 0) return VMX_OK;
    CallScope call{sc, sc->stream, std::chrono::steady_clock::now()};
    std::lock_guard<std::mutex> lock(sc->mu);
    int rc = bind_device(sc);
    if (rc) return rc;
    Workspace &ws = sc->ws;
    hipStream_t s = sc->stream;
    if ((rc = sc->upd.done.wait(s))) return rc;
    const bool count = f.count = opts->collect_counters != 0;
    const bool legacy = f.legacy = f.pipeline == 2 || f.pipeline == 3;  // first-generation kernels (A/B library)
    const Tuning tn = make_tuning(sc, opts);
    f.pool = ab_pool_bit(opts) && !count;  // the phase-pure probe (vmx_trace_pool.inc)
    FrameDev fr;
    std::memset(&fr, 0, sizeof(fr));
    fr.r2scale = (opts->sampling & VMX_SAMPLING_MODE_MASK) == VMX_SAMPLING_CORRECTED ? 1.0f : 10.0f;
    fr.libm_double = (opts->sampling & VMX_SAMPLING_LIBM_DOUBLE) ? 1u : 0u;
    fr.elide_dead = 0;
    PathArrays pa{};
    IdQueue qi[3];
    QueueDev q[2];
    int tb = 1, rb = 1, bb = 1;
    const uint32_t lds_paths = (kPathsBlock / 64) * (tn.lds_entries + 1) * 512;
    if (legacy) {
        rc = ab_radiance_setup(sc, n, count, q, &bb);
        if (rc) return rc;
    } else {
        rc = ensure_paths(sc, n, pa, qi);
        if (rc) return rc;
        HIP_TRY((hipError_t)query_trace_q_blocks_per_cu(kPathsBlock, (kPathsBlock / 64) * (tn.lds_bounce + 1) * 512, count, true,
                                                        false, false, &tb));
        HIP_TRY((hipError_t)query_paths_blocks_per_cu(kPathsBlock, lds_paths, count, &rb));
    }
    DevBuf<float> d_o, d_d;
    if (d_o.ensure((size_t)n * 3) || d_d.ensure((size_t)n * 3)) return fail(VMX_ERR_NOMEM, "hipMalloc failed");
    std::vector<TimedLaunch> timed;
    uint64_t launches = 0;
    if ((rc = call.open())) return rc;
    auto body = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_o.p, origin, (size_t)n * 12, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_d.p, dir, (size_t)n * 12, hipMemcpyHostToDevice, s));
        int r;
        if ((r = call.start()) || (r = call.clear_counters())) return r;
        if (legacy) {
            r = ab_radiance_enqueue(sc, fr, q, d_o.p, d_d.p, n, opts->seed, count, tn.tail_threshold, s, timed, launches, bb);
        } else {
            HIP_TRY(hipMemsetAsync(qi[0].counts, 0, kSubQueues * 32 * 4, s));
            LAUNCH_TRY(launch_radiance_init_ids(d_o.p, d_d.p, n, opts->seed, pa, qi[0], (uint32_t)sc->num_cus, s));
            launches += 2;
            r = run_ids(sc, fr, pa, qi, 0, ws.counters.p, f, tn, s, timed, launches, tb, rb);
        }
        if (r) return r;
        if ((r = call.stop())) return r;
        HIP_TRY(hipMemcpyAsync(out, ws.rad.p, (size_t)n * 16, hipMemcpyDeviceToHost, s));
        return call.finish(timed, stats, launches, 1);
    };
    rc = body();
    if (rc) (void)hipStreamSynchronize(s);  // (what was enqueued may still use d_o / d_d, which are freed here)
    if (rc == VMX_OK && stats) stats->samples = n;
    return rc;
}

int vmx_trig(const float *x, uint32_t n, float *cos_out, float *sin_out, int device) {
    if (!x || !cos_out || !sin_out) return fail(VMX_ERR_INVALID, "NULL argument");
    if (n == 0) return VMX_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(VMX_ERR_NO_DEVICE, "no such HIP device");
    HIP_TRY(hipSetDevice(device));
    Staging st(nullptr, "vmx_trig");  // (the device's default stream)
    const float *d_x = st.in(x, n);
    float *d_c = st.out(cos_out, n), *d_s = st.out(sin_out, n);
    if (st.nomem) return fail(VMX_ERR_NOMEM, "hipMalloc failed");
    st.copy_in();
    if (st.ok()) st.e = (hipError_t)launch_trig(d_x, n, d_c, d_s, nullptr);
    return st.finish();
}

} /* extern "C" */
