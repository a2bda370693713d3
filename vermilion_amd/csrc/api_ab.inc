// api_ab.inc — part of vmx_api.cpp: the host code that only the A/B library runs (make ab: the first-generation kernels of
// pipeline forms 2 and 3, the bounce reordering, the k_trace_pool probe, the VMX_AB_* environment reads), behind the ab_*
// hooks that the pass loop and vmx_radiance call.  The product gets the stubs at the end: they refuse what the library does
// not hold and do nothing otherwise.
namespace {

#ifdef VMX_AB_KERNELS

// forms 2 and 3: what the first-generation kernels cannot do
int ab_check_forms(const vmx_scene *sc, uint32_t pipeline) {
    if (sc->dev.tex && pipeline >= 2 && pipeline <= 3)
        return fail(VMX_ERR_INVALID, "the first-generation kernels (pipeline forms 2, 3) do not sample textures");
    return VMX_OK;
}

// vmx_opts.reserved[0] bit 10: the bounce generations of a pass through k_trace_pool
int ab_check_pool(const vmx_opts *) { return VMX_OK; }
bool ab_pool_bit(const vmx_opts *o) { return (o->reserved[0] & kFormPool) != 0; }

// cap on the bounce kernel's blocks per CU (how much of its time is latency hiding: profiles/r04_state_pool.txt)
int ab_bounce_blocks(int tbb) {
    if (const char *e = std::getenv("VMX_AB_BOUNCE_BLOCKS")) tbb = std::max(1, std::min(tbb, std::atoi(e)));
    return tbb;
}

int run_queue(vmx_scene *sc, const FrameDev &fr, QueueDev q[2], int cur, void *rad, DevCounters *ctr, bool count,
              uint32_t tail_threshold, hipStream_t s, std::vector<TimedLaunch> &timed, uint64_t &launches,
              int bounce_blocks) {
    for (;;) {
        uint64_t total;
        uint32_t largest;
        int rc = read_counts(sc, q[cur].counts, s, total, largest);
        if (rc) return rc;
        if (total == 0) break;
        const uint32_t max_chunks = (largest + sc->block - 1) / sc->block;
        const bool tail = total <= tail_threshold;
        LaunchCfg cfg = trace_cfg(sc, max_chunks * kSubQueues, bounce_blocks);
        if (!tail) LAUNCH_TRY(launch_zero_u32(q[cur ^ 1].counts, kSubQueues * 32, s));
        if ((rc = timed_begin(sc->ws, timed, s, 1, VMX_K_OTHER))) return rc;
        LAUNCH_TRY(launch_bounce(sc->dev, fr.r2scale, fr.libm_double, q[cur], max_chunks, q[cur ^ 1], rad, ctr, count, tail, false, cfg, s));
        if ((rc = timed_end(timed, s))) return rc;
        launches += tail ? 1 : 2;
        if (tail) break;
        cur ^= 1;
    }
    return VMX_OK;
}

int ensure_queues(vmx_scene *sc, uint32_t sub_capacity, QueueDev q[2]) {
    Workspace &ws = sc->ws;
    const size_t cap = (size_t)sub_capacity * kSubQueues;
    for (int i = 0; i < 2; ++i) {
        int e = ws.queue_planes[i].ensure(cap * kPathBytes);
        if (e) return fail(VMX_ERR_NOMEM, std::string("path queue: ") + hipGetErrorString((hipError_t)e));
    }
    int e = ws.queue_counts.ensure(2 * kSubQueues * 32);
    if (e) return fail(VMX_ERR_NOMEM, "queue counters");
    if (ws.heads.ensure(kSubQueues * 32)) return fail(VMX_ERR_NOMEM, "work heads");
    for (int i = 0; i < 2; ++i) {
        q[i].planes = ws.queue_planes[i].p;
        q[i].counts = ws.queue_counts.p + (size_t)i * kSubQueues * 32;
        q[i].capacity = (uint32_t)cap;
        q[i].sub_capacity = sub_capacity;
    }
    return VMX_OK;
}

int legacy_occupancy(const vmx_scene *sc, bool count, int *pb, int *bb) {
    HIP_TRY((hipError_t)query_blocks_per_cu(sc->block, (sc->block / 64) * sc->dev.stack_entries * 512, count, pb, bb));
    if (*pb < 1 || *bb < 1) return fail(VMX_ERR_HIP, "kernel does not fit on a CU (LDS stack too deep?)");
    return VMX_OK;
}

// render_bind of a frame in form 2 or 3: the two path queues and the kernels' blocks per CU
int ab_bind_legacy(vmx_scene *sc, RenderJob &job) {
    if (int rc = ensure_queues(sc, job.sub_cap, job.q)) return rc;
    return legacy_occupancy(sc, job.f.count, &job.pb, &job.bb);
}

// a pass of form 2 (k_primary, then k_bounce per generation) or 3 (k_primary follows every path to its end)
int ab_legacy_pass(vmx_scene *sc, RenderJob &job, const unsigned int *act_cur, uint32_t n_active, uint32_t S) {
    Workspace &ws = sc->ws;
    hipStream_t s = job.s;
    const bool mega = job.f.pipeline == 3;
    const uint32_t n_pad = (n_active + 63u) & ~63u;
    const uint32_t tiles8 = (((n_pad + sc->block - 1) / sc->block) + 7u) & ~7u;
    if (!mega) HIP_TRY(hipMemsetAsync(job.q[0].counts, 0, kSubQueues * 32 * 4, s));
    LaunchCfg cfg = trace_cfg(sc, tiles8 * S, job.pb);
    int rc = timed_begin(ws, job.timed, s, 0, VMX_K_OTHER);
    if (rc) return rc;
    LAUNCH_TRY(launch_primary(sc->dev, job.fr, act_cur, n_active, S, job.px, job.q[0], ws.rad.p, ws.counters.p, job.f.count, mega, cfg, s));
    if ((rc = timed_end(job.timed, s))) return rc;
    job.launches += 2;
    if (mega) return VMX_OK;
    return run_queue(sc, job.fr, job.q, 0, ws.rad.p, ws.counters.p, job.f.count, job.tn.tail_threshold, s, job.timed, job.launches, job.bb);
}

// vmx_radiance in form 2 or 3: the workspace, then the path starts and their generations
int ab_radiance_setup(vmx_scene *sc, uint32_t n, bool count, QueueDev q[2], int *bb) {
    Workspace &ws = sc->ws;
    const uint32_t blocks = (n + 255) / 256;
    const uint32_t sub_cap0 = (blocks / kSubQueues + 2) * 256;
    if (int rc = ensure_queues(sc, sub_cap0 + sub_cap0 / 4 + 4096, q)) return rc;
    if (ws.rad.ensure((size_t)n * 16) || ws.counters.ensure(1)) return fail(VMX_ERR_NOMEM, "hipMalloc failed");
    int pb = 1;
    HIP_TRY((hipError_t)query_blocks_per_cu(sc->block, (sc->block / 64) * sc->dev.stack_entries * 512, count, &pb, bb));
    return VMX_OK;
}

int ab_radiance_enqueue(vmx_scene *sc, const FrameDev &fr, QueueDev q[2], const float *d_o, const float *d_d, uint32_t n,
                        uint64_t seed, bool count, uint32_t tail_threshold, hipStream_t s, std::vector<TimedLaunch> &timed,
                        uint64_t &launches, int bb) {
    HIP_TRY(hipMemsetAsync(q[0].counts, 0, kSubQueues * 32 * 4, s));
    LAUNCH_TRY(launch_radiance_init(d_o, d_d, n, seed, q[0], s));
    launches += 2;
    return run_queue(sc, fr, q, 0, sc->ws.rad.p, sc->ws.counters.p, count, tail_threshold, s, timed, launches, bb);
}

// bounce reordering (vmx_opts.reserved[5]) of a generation that is not the last: the live ids by (origin cell,
// direction cell) of their next rays (path_sort.hip); the traversal, and with bit 20 the shading, then take the sorted list
int ab_reorder(vmx_scene *sc, const Tuning &tn, bool tail, const IdQueue &qcur, uint32_t largest, const uint32_t *per_queue,
               const PathArrays &pa, hipStream_t s, std::vector<TimedLaunch> &timed, WorkDev &wk, IdQueue &q_shade) {
    if (tail || !tn.sort_mode) return VMX_OK;
    Workspace &ws = sc->ws;
    const size_t qsize = (size_t)qcur.sub_capacity * kSubQueues;
    const size_t tmp_bytes = path_sort_tmp_bytes(largest);
    if (ws.sort_keys[0].ensure(qsize) || ws.sort_keys[1].ensure(qsize) || ws.ids_sorted.ensure(qsize) || ws.sort_tmp.ensure(tmp_bytes))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed for the path sort");
    if (sc->upd.bounds_stale) {  // after a device REFIT: the root's box, written by the refit
        float rb[6];
        HIP_TRY(hipMemcpyAsync(rb, sc->upd.root_box.p, sizeof(rb), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int a = 0; a < 3; ++a) sc->bounds_lo[a] = rb[a], sc->bounds_hi[a] = rb[3 + a];
        sc->upd.bounds_stale = false;
    }
    SortKeyCfg kc;
    for (int a = 0; a < 3; ++a) {
        kc.lo[a] = sc->bounds_lo[a];
        const float ext = sc->bounds_hi[a] - sc->bounds_lo[a];
        kc.inv[a] = ext > 0.f ? 1.0f / ext : 0.f;
    }
    kc.obits = tn.sort_mode & 15u, kc.dbits = (tn.sort_mode >> 4) & 15u;
    kc.dir_major = (tn.sort_mode >> 8) & 1u, kc.chunk_log2 = (tn.sort_mode >> 12) & 31u;
    if (kc.obits > 10 || kc.dbits > 8 || 3 * kc.obits + 2 * kc.dbits > 32)
        return fail(VMX_ERR_INVALID, "bounce reordering: key wider than 32 bits");
    int rc = timed_begin(ws, timed, s, -1, VMX_K_OTHER);
    if (rc) return rc;
    LAUNCH_TRY(path_sort_ids(qcur, per_queue, pa.state, kc, ws.sort_keys[0].p, ws.sort_keys[1].p, ws.ids_sorted.p, ws.sort_tmp.p, tmp_bytes, s));
    if ((rc = timed_end(timed, s))) return rc;
    wk.qids.ids = ws.ids_sorted.p;
    if ((tn.sort_mode >> 20) & 1u) q_shade.ids = ws.ids_sorted.p;
    return VMX_OK;
}

// the probe's traversal of one bounce generation of `total` rays: P ray slots per block of 256 threads
// (VMX_AB_POOL_SLOTS, default 512), L stack levels in LDS (VMX_AB_POOL_LEVELS, default 8), as many blocks per CU as the
// LDS admits
int ab_trace_pool(vmx_scene *sc, uint64_t total, WorkDev &wk, const PathArrays &pa, hipStream_t s) {
    Workspace &ws = sc->ws;
    uint32_t P = 512, Lv = 8, lds = 0;
    if (const char *e = std::getenv("VMX_AB_POOL_SLOTS")) P = (uint32_t)std::atoi(e);
    if (const char *e = std::getenv("VMX_AB_POOL_LEVELS")) Lv = (uint32_t)std::atoi(e);
    if (P < 64 || P > 16384 || Lv < 1 || Lv > 64) return fail(VMX_ERR_INVALID, "k_trace_pool: bad VMX_AB_POOL_SLOTS / _LEVELS");
    int pbl = 0;
    HIP_TRY((hipError_t)query_trace_pool(kPathsBlock, P, Lv, &lds, &pbl));
    if (pbl < 1) return fail(VMX_ERR_INVALID, "k_trace_pool does not fit on a CU with these slots / levels");
    if (const char *e = std::getenv("VMX_AB_POOL_BLOCKS")) pbl = std::max(1, std::min(pbl, std::atoi(e)));
    LaunchCfg pc;
    pc.block = kPathsBlock, pc.lds_bytes = lds;
    pc.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)sc->num_cus * pbl, (total + P - 1) / P));
    if (const char *e = std::getenv("VMX_AB_POOL_GRID")) pc.grid = (uint32_t)std::max(1, std::min((int)pc.grid, std::atoi(e)));
    wk.pool_slots = P, wk.lds_entries = Lv;
    wk.overflow_entries = sc->dev.stack_entries + 1 > Lv ? sc->dev.stack_entries + 1 - Lv : 1u;
    if (ws.overflow_stack.ensure((size_t)pc.grid * P * wk.overflow_entries * 8))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed for the overflow stack");
    wk.overflow_stack = ws.overflow_stack.p;
    wk.reserve = 256;
    LAUNCH_TRY(launch_trace_pool(sc->dev, wk, pa, pc, s));
    return VMX_OK;
}

#else

int ab_check_forms(const vmx_scene *, uint32_t pipeline) {
    if (pipeline >= 2 && pipeline <= 3)
        return fail(VMX_ERR_INVALID, "pipeline forms 2 and 3 (first-generation kernels) are only in the A/B library (make ab)");
    return VMX_OK;
}

int ab_check_pool(const vmx_opts *o) {
    if (o->reserved[0] & kFormPool)
        return fail(VMX_ERR_INVALID, "k_trace_pool (vmx_opts.reserved[0] bit 10) is a probe of the A/B library (make ab): "
                                     "profiles/r04_state_pool.txt");
    return VMX_OK;
}
bool ab_pool_bit(const vmx_opts *) { return false; }

int ab_bounce_blocks(int tbb) { return tbb; }

int ab_reorder(vmx_scene *, const Tuning &tn, bool, const IdQueue &, uint32_t, const uint32_t *, const PathArrays &, hipStream_t,
               std::vector<TimedLaunch> &, WorkDev &, IdQueue &) {
    if (tn.sort_mode)
        return fail(VMX_ERR_INVALID, "bounce reordering (vmx_opts.reserved[5]) is an experiment of the A/B library (make ab): "
                                     "it never paid for its sort, profiles/r03_bounce_sort.txt");
    return VMX_OK;
}

// (never reached: ab_check_forms has refused the forms, and ab_pool_bit leaves Tuning::pool off)
int ab_bind_legacy(vmx_scene *sc, RenderJob &job) { return ab_check_forms(sc, job.f.pipeline); }
int ab_legacy_pass(vmx_scene *sc, RenderJob &job, const unsigned int *, uint32_t, uint32_t) { return ab_check_forms(sc, job.f.pipeline); }
int ab_radiance_setup(vmx_scene *sc, uint32_t, bool, QueueDev *, int *) { return ab_check_forms(sc, 2); }
int ab_radiance_enqueue(vmx_scene *sc, const FrameDev &, QueueDev *, const float *, const float *, uint32_t, uint64_t, bool, uint32_t,
                        hipStream_t, std::vector<TimedLaunch> &, uint64_t &, int) {
    return ab_check_forms(sc, 2);
}
int ab_trace_pool(vmx_scene *, uint64_t, WorkDev &, const PathArrays &, hipStream_t) {
    return fail(VMX_ERR_INVALID, "k_trace_pool is a probe of the A/B library (make ab)");
}

#endif

}  // namespace
