// api_guide.inc — part of vmx_api.cpp: the guide tree on the host side — the guided bounce generation that run_ids enqueues,
// the fused kernels' GuidePathsDev, the counters' entries and the diagnostic vmx_guide_trace*
namespace {

// api_render.inc
Tuning make_tuning(const vmx_scene *sc, const vmx_opts *o);
LaunchCfg paths_cfg(const vmx_scene *sc, uint32_t entries, uint64_t items, int blocks_per_cu);
int bind_stack(vmx_scene *sc, const Tuning &tn, uint32_t entries, uint32_t grid, uint64_t items, WorkDev &wk, bool guided = false);
int ensure_paths(vmx_scene *sc, size_t nslots, PathArrays &pa, IdQueue q[3]);

// blocks per CU of the launch that traces a guided bounce generation's fallback list over the reference tree: the
// list is a fraction of a per cent of the generation where the guide is worth having, and every wave of the launch may
// leave the tail of one record chunk unused, which the record lists are padded for
constexpr uint32_t kGuideFallbackBlocks = 2;

// the scene's guide as the fused kernel's GUIDE forms read it (k_paths<.., GuidePathsDev>: the tail of run_ids, pass_fused),
// where the call's forms have the guide on, the guide is still valid and the call has its counters; else off = 0: the launch is
// the reference-tree instantiation.  A launch that is handed this must have its stack bound with guided = true.
GuidePathsDev guide_paths(const vmx_scene *sc, bool guide) {
    GuidePathsDev g{};
    const vmx_scene::Guide &sg = sc->guide;
    if (guide && sg.valid && sg.base && sg.off && sc->ws.guide_fused_ctr.p) {
        g.off = sg.off, g.tri_off = sg.off + sg.tri_off, g.root_ref = sg.root_ref;
        g.scene_max = sg.scene_max;
        g.ctr = sc->ws.guide_fused_ctr.p;
    }
    return g;
}

// ---- the guided bounce generation, in two halves ----------------------------------------------------------------------
// Over the guide tree first (guide_walk.h); then today's kernel once more, over the rays the per-ray rule did not settle:
// it reads the list's length on the device, appends to the same record list, and every ray is counted by the launch that
// settles it.  wk, cfg: the generation's work and grid, its stack bound with guided = true.  run_ids enqueues both halves
// as one timed interval; vmx_guide_trace reads the first one's answers back in between.
uint32_t guide_fb_capacity(const Workspace &ws) { return (uint32_t)std::min<size_t>(ws.guide_fb.n, 0xFFFFFFFFu); }

int guided_walk(vmx_scene *sc, const FrameDev &fr, const WorkDev &wk, PathArrays pa, DevCounters *ctr, bool count, LaunchCfg cfg,
                hipStream_t s, unsigned int *visits = nullptr) {
    Workspace &ws = sc->ws;
    GuideDev gd;
    gd.base = sc->guide.base, gd.tri_off = sc->guide.tri_off, gd.root_ref = sc->guide.root_ref;
    gd.scene_max = sc->guide.scene_max;
    gd.fb_capacity = guide_fb_capacity(ws);
    gd.fb_ids = ws.guide_fb.p, gd.fb_count = ws.guide_fb_count.p, gd.ctr = ws.guide_ctr.p, gd.overflow = ctr;
    HIP_TRY(hipMemsetAsync(ws.guide_fb_count.p, 0, 4, s));
    HIP_TRY(hipMemsetAsync(ws.guide_heads.p, 0, 4, s));
    LAUNCH_TRY(launch_trace_q(sc->dev, fr, wk, PixelStateDev{nullptr, nullptr, nullptr}, pa, ctr, count, true, cfg, s, &gd, visits));
    return VMX_OK;
}

// the second launch's grid (the record lists are padded for its waves too: ensure_paths, render_bind)
LaunchCfg guided_fallback_cfg(const vmx_scene *sc, LaunchCfg cfg) {
    cfg.grid = std::min<uint32_t>(cfg.grid, (uint32_t)sc->num_cus * kGuideFallbackBlocks);
    return cfg;
}

int guided_fallback(vmx_scene *sc, const FrameDev &fr, const WorkDev &wk, PathArrays pa, DevCounters *ctr, bool count, LaunchCfg cfg,
                    hipStream_t s) {
    Workspace &ws = sc->ws;
    WorkDev wf = wk;
    wf.heads = ws.guide_heads.p, wf.nsrc = 1;
    wf.qids.ids = ws.guide_fb.p, wf.qids.counts = ws.guide_fb_count.p, wf.qids.sub_capacity = guide_fb_capacity(ws);
    wf.reserve = 64;  // (the grid is no larger than cfg's: the overflow slab bound for the first launch holds this one's waves)
    LAUNCH_TRY(launch_trace_q(sc->dev, fr, wf, PixelStateDev{nullptr, nullptr, nullptr}, pa, ctr, count, true, guided_fallback_cfg(sc, cfg), s));
    return VMX_OK;
}

}  // namespace

extern "C" {

int vmx_guide_rays(const vmx_scene *csc, uint64_t *settled, uint64_t *fallback) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!sc || !settled || !fallback) return fail(VMX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(sc->mu);
    *settled = sc->guide_settled, *fallback = sc->guide_fallback;
    return VMX_OK;
}

int vmx_guide_fused_rays(const vmx_scene *csc, uint64_t *settled, uint64_t *fallback) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!sc || !settled || !fallback) return fail(VMX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(sc->mu);
    *settled = sc->guide_fused_settled, *fallback = sc->guide_fused_fallback;
    return VMX_OK;
}

int vmx_guide_list_entries(const vmx_scene *csc, uint64_t *entries) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!sc || !entries) return fail(VMX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(sc->mu);
    *entries = sc->guide_entries;
    return VMX_OK;
}

// The guided bounce generation over n explicit rays: guided_walk, as run_ids enqueues it, and (flags bit 1) guided_fallback
// over the list it left.  Where each ray ended is read back after either half and checked per ray.
// inner_visits / tri_tests (both or neither; hit records only): the launch is the kernel's counting form, and every ray's
// guide walk leaves its inner records and triangle tests there (0, 0 for a ray that never walked).
static int guide_trace_impl(const vmx_scene *csc, const float *origin, const float *dir, uint32_t n, const vmx_opts *opts,
                            uint32_t flags, uint32_t grid_blocks, uint8_t *settled, uint32_t *slot, float *t,
                            uint32_t *inner_visits, uint32_t *tri_tests) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!sc || !origin || !dir || !opts || !settled || !slot || !t) return fail(VMX_ERR_INVALID, "NULL argument");
    if (flags & ~3u) return fail(VMX_ERR_INVALID, "vmx_guide_trace: unknown flag");
    const bool visits = inner_visits != nullptr;
    if (visits && (flags & 1u)) return fail(VMX_ERR_INVALID, "vmx_guide_trace_visits: visits are counted with hit records only");
    if (opts->collect_counters) return fail(VMX_ERR_INVALID, "vmx_guide_trace: the counting build never walks the guide");
    const bool records = (flags & 1u) != 0, complete = (flags & 2u) != 0;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (!sc->guide.valid || !sc->guide.base)
        return fail(VMX_ERR_INVALID, "vmx_guide_trace: the scene has no valid guide (another builder, or vertices moved without a rebuild)");
    if (n == 0) return VMX_OK;
    int rc = bind_device(sc);
    if (rc) return rc;
    Workspace &ws = sc->ws;
    hipStream_t s = sc->stream;
    if ((rc = sc->upd.done.wait(s))) return rc;
    const Tuning tn = make_tuning(sc, opts);
    FrameDev fr;
    std::memset(&fr, 0, sizeof(fr));
    PathArrays pa{};
    IdQueue qi[3];
    if ((rc = ensure_paths(sc, n, pa, qi))) return rc;
    const uint32_t entries = tn.lds_bounce;
    int tb = 1;
    HIP_TRY((hipError_t)query_trace_q_blocks_per_cu(kPathsBlock, (kPathsBlock / 64) * (entries + 1) * 512, false, true, records,
                                                    false, &tb, true));
    if (tb < 1) return fail(VMX_ERR_HIP, "trace kernel does not fit on a CU");
    LaunchCfg cfg = paths_cfg(sc, entries, n, ab_bounce_blocks(tb));
    if (grid_blocks) cfg.grid = std::min(cfg.grid, grid_blocks);
    // every ray may need a record, and each wave of either launch leaves at most the tail of one chunk of 256 unused
    const size_t out_capacity = (size_t)n + ((size_t)cfg.grid + guided_fallback_cfg(sc, cfg).grid) * (kPathsBlock / 64) * 256 + 1024;
    if (out_capacity > 0xFFFFFFFFull) return fail(VMX_ERR_INVALID, "vmx_guide_trace: too many rays");
    if (ws.guide_ctr.ensure(2) || ws.guide_fb.ensure(n) || ws.guide_fb_count.ensure(32) || ws.guide_heads.ensure(32) ||
        (records && (ws.out_rec.ensure(out_capacity * 16) || ws.out_count.ensure(32))))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed for the guide tree's lists");
    DevBuf<float> d_o, d_d;
    DevBuf<unsigned int> d_visits;
    if (d_o.ensure((size_t)n * 3) || d_d.ensure((size_t)n * 3) || (visits && d_visits.ensure((size_t)n * 2)))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed");
    WorkDev wk = make_work(ws.heads.p, &tn);
    wk.nsrc = kSubQueues;
    wk.qids = qi[0];
    if ((rc = bind_stack(sc, tn, entries, cfg.grid, n, wk, true))) return rc;
    if (records) {
        wk.out_rec = ws.out_rec.p, wk.out_count = ws.out_count.p, wk.out_ctr = ws.counters.p, wk.out_capacity = (uint32_t)out_capacity;
        wk.keep_all = 1u;
    }
    CallScope call{sc, s, std::chrono::steady_clock::now()};  // (no events, no statistics: the counters only)
    // where the rays of one launch ended, by pid: hit[pid] (a word of ones where the launch wrote nothing) or the records
    // the launch appended, entries [rec_from, the list's length)
    std::vector<float> got(records ? 0 : (size_t)n * 2), rec;
    std::vector<uint32_t> times((size_t)n, 0u);
    unsigned int rec_from = 0;
    uint64_t beyond = 0;
    auto collect = [&](bool first) -> int {
        if (!records) {
            HIP_TRY(hipMemcpyAsync(got.data(), pa.hit, (size_t)n * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            for (uint32_t i = 0; i < n; ++i) {
                uint32_t tb_, sb_;
                std::memcpy(&tb_, &got[(size_t)i * 2], 4), std::memcpy(&sb_, &got[(size_t)i * 2 + 1], 4);
                if (tb_ == 0xFFFFFFFFu || (!first && settled[i])) continue;
                times[i]++, slot[i] = sb_, t[i] = got[(size_t)i * 2];
                if (first) settled[i] = 1;
            }
            return VMX_OK;
        }
        unsigned int len = 0;
        HIP_TRY(hipMemcpyAsync(&len, ws.out_count.p, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        len = (unsigned int)std::min<size_t>(len, out_capacity);
        rec.resize((size_t)(len - rec_from) * 4);
        if (len > rec_from) HIP_TRY(hipMemcpy(rec.data(), (const char *)ws.out_rec.p + (size_t)rec_from * 16, rec.size() * 4, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < rec.size() / 4; ++k) {
            uint32_t sb_, pid;
            std::memcpy(&sb_, &rec[k * 4 + 1], 4), std::memcpy(&pid, &rec[k * 4 + 2], 4);
            if (pid == 0xFFFFFFFFu) continue;  // the padded tail of a wave's last chunk
            if (pid >= n) {
                ++beyond;
                continue;
            }
            times[pid]++, slot[pid] = sb_, t[pid] = rec[k * 4];
            if (first) settled[pid] = 1;
        }
        rec_from = len;
        return VMX_OK;
    };
    auto body = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_o.p, origin, (size_t)n * 12, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_d.p, dir, (size_t)n * 12, hipMemcpyHostToDevice, s));
        if (int r = call.clear_counters()) return r;
        HIP_TRY(hipMemsetAsync(qi[0].counts, 0, kSubQueues * 32 * 4, s));
        LAUNCH_TRY(launch_radiance_init_ids(d_o.p, d_d.p, n, opts->seed, pa, qi[0], (uint32_t)sc->num_cus, s));
        HIP_TRY(hipMemsetAsync(pa.hit, 0xFF, (size_t)n * 8, s));
        HIP_TRY(hipMemsetAsync(ws.heads.p, 0, kSubQueues * 32 * 4, s));
        if (records) HIP_TRY(hipMemsetAsync(ws.out_count.p, 0, 4, s));
        if (visits) HIP_TRY(hipMemsetAsync(d_visits.p, 0, (size_t)n * 8, s));
        int r = guided_walk(sc, fr, wk, pa, ws.counters.p, false, cfg, s, visits ? d_visits.p : nullptr);
        if (r) return r;
        if (visits) {
            std::vector<unsigned int> hv((size_t)n * 2);
            HIP_TRY(hipMemcpyAsync(hv.data(), d_visits.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            for (uint32_t i = 0; i < n; ++i) inner_visits[i] = hv[(size_t)i * 2], tri_tests[i] = hv[(size_t)i * 2 + 1];
        }
        std::memset(settled, 0, n);
        for (uint32_t i = 0; i < n; ++i) slot[i] = 0xFFFFFFFFu, t[i] = 0.f;
        if ((r = collect(true))) return r;
        // exactly one of the two: a ray the launch settled is on no list, every other ray is on the fallback list once
        unsigned int fb_n = 0;
        unsigned long long ctr[2] = {0, 0};
        DevCounters h;
        HIP_TRY(hipMemcpy(&fb_n, ws.guide_fb_count.p, 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ctr, ws.guide_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&h, ws.counters.p, sizeof(h), hipMemcpyDeviceToHost));
        std::vector<unsigned int> fb(std::min<size_t>(fb_n, n));
        if (!fb.empty()) HIP_TRY(hipMemcpy(fb.data(), ws.guide_fb.p, fb.size() * 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> listed((size_t)n, 0u);
        uint64_t twice = 0, both = 0, neither = 0, again = 0, n_settled = 0;
        for (unsigned int pid : fb) {
            if (pid >= n) ++beyond;
            else if (listed[pid]++) ++twice;
        }
        for (uint32_t i = 0; i < n; ++i) {
            both += settled[i] && listed[i], neither += !settled[i] && !listed[i], again += times[i] > 1, n_settled += settled[i];
        }
        sc->guide_settled = ctr[0], sc->guide_fallback = ctr[1], sc->guide_entries = n;
        if (h.overflow || fb_n > n || twice || both || neither || again || beyond || ctr[0] != n_settled || ctr[1] != fb_n)
            return fail(VMX_ERR_HIP, "vmx_guide_trace: of " + std::to_string(n) + " rays " + std::to_string(both) +
                                         " are settled and on the fallback list, " + std::to_string(neither) + " are neither, " +
                                         std::to_string(twice) + " are listed more than once, " + std::to_string(again) +
                                         " were answered more than once, " + std::to_string(beyond) + " entries name no ray; the list holds " +
                                         std::to_string(fb_n) + " ids, " + std::to_string(h.overflow) + " did not fit; the kernel counted " +
                                         std::to_string(ctr[0]) + " settled + " + std::to_string(ctr[1]) + " fallback, the host " +
                                         std::to_string(n_settled) + " settled");
        if (!complete) return VMX_OK;
        if ((r = guided_fallback(sc, fr, wk, pa, ws.counters.p, false, cfg, s))) return r;
        std::fill(times.begin(), times.end(), 0u);
        if ((r = collect(false))) return r;
        HIP_TRY(hipMemcpy(&h, ws.counters.p, sizeof(h), hipMemcpyDeviceToHost));
        uint64_t wrong = 0;
        for (uint32_t i = 0; i < n; ++i) wrong += times[i] != (settled[i] ? 0u : 1u);
        if (wrong || beyond || h.overflow)
            return fail(VMX_ERR_HIP, "vmx_guide_trace: the launch over the fallback list answered " + std::to_string(wrong) + " of " +
                                         std::to_string(n) + " rays not exactly once (" + std::to_string(beyond) + " entries name no ray, " +
                                         std::to_string(h.overflow) + " did not fit)");
        return VMX_OK;
    };
    rc = body();
    if (rc) (void)hipStreamSynchronize(s);  // (what was enqueued may still use d_o / d_d, which are freed here)
    return rc;
}

int vmx_guide_trace(const vmx_scene *csc, const float *origin, const float *dir, uint32_t n, const vmx_opts *opts,
                    uint32_t flags, uint32_t grid_blocks, uint8_t *settled, uint32_t *slot, float *t) {
    return guide_trace_impl(csc, origin, dir, n, opts, flags, grid_blocks, settled, slot, t, nullptr, nullptr);
}

int vmx_guide_trace_visits(const vmx_scene *csc, const float *origin, const float *dir, uint32_t n, const vmx_opts *opts,
                           uint32_t flags, uint32_t grid_blocks, uint8_t *settled, uint32_t *slot, float *t,
                           uint32_t *inner_visits, uint32_t *tri_tests) {
    if (!inner_visits || !tri_tests) return fail(VMX_ERR_INVALID, "NULL argument");
    return guide_trace_impl(csc, origin, dir, n, opts, flags, grid_blocks, settled, slot, t, inner_visits, tri_tests);
}

} /* extern "C" */
