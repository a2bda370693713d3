// api_sampling.inc — part of vmx_api.cpp
extern "C" {

// ---- adaptive sampling: steps over a subset of a progressive handle's pixels, and the error that chooses it ----------
static const vmx_sampling_params kSamplingDefaults = {0.5f, 0.05f, 8u, 1u, {0u, 0u, 0u, 0u}};

static int sampling_params(const vmx_sampling_params *in, vmx_sampling_params &out) {
    out = in ? *in : kSamplingDefaults;
    if (!(std::isfinite(out.threshold) && out.threshold >= 0.f))
        return fail(VMX_ERR_INVALID, "vmx_sampling_params: threshold must be finite and >= 0");
    if (!finite_positive(out.floor)) return fail(VMX_ERR_INVALID, "vmx_sampling_params: floor must be finite and > 0");
    if (out.min_samples < 2) return fail(VMX_ERR_INVALID, "vmx_sampling_params: min_samples must be >= 2");
    if (out.radius > 3) return fail(VMX_ERR_INVALID, "vmx_sampling_params: radius must be 0..3");
    if (!reserved_zero(out.reserved)) return fail(VMX_ERR_INVALID, "vmx_sampling_params: reserved words must be 0");
    return VMX_OK;
}

int vmx_sampling_default_params(vmx_sampling_params *out) { return default_params(out, kSamplingDefaults); }

// the refusals that depend on how the handle was begun (no device needed)
static int selection_refusals(const vmx_progressive *p, bool selects, bool needs_moments) {
    if (selects && p->job.fr.early_stop)
        return fail(VMX_ERR_INVALID, "selected steps need a handle begun with opts.early_stop == 0: the early-stop schedule assumes that all "
                                     "pixels advance together, and the reference's rule is a different stopping rule");
    if (needs_moments && !p->job.moments)
        return fail(VMX_ERR_INVALID, "the handle keeps no second moment: begin it with vmx_progressive_begin_ex and VMX_PROGRESSIVE_MOMENTS");
    return VMX_OK;
}

static SamplingPass sampling_pass(const vmx_progressive *p, const vmx_sampling_params &prm) {
    SamplingPass a{};
    a.width = p->job.fr.width, a.height = p->job.fr.local_rows;
    a.kmax = p->job.fr.kmax, a.min_samples = prm.min_samples, a.radius = prm.radius;
    a.threshold = prm.threshold, a.floor = prm.floor;
    a.px = PixelStateDev{p->pixels.accum.p, p->pixels.count.p, p->pixels.cursor.p};
    return a;
}

// the pixels of src[0, n) that are unfinished and (select: selected), in order, to dst; *kept their number.  Blocks.
static int progressive_compact(vmx_progressive *p, const unsigned int *src, uint32_t n, const unsigned char *select, unsigned int *dst,
                               uint32_t *kept) {
    *kept = 0;
    if (n == 0) return VMX_OK;
    hipStream_t s = p->job.s;
    const uint32_t nwords = (n + 63u) / 64u;
    unsigned int *cnt = p->list_u32.p, *offs = cnt + p->list_words, *len = offs + p->list_words;
    LAUNCH_TRY(launch_list_words(src, n, select, p->pixels.cursor.p, p->job.fr.kmax, p->list_mask.p, cnt, s));
    HIP_TRY((hipError_t)launch_list_compact(p->list_mask.p, cnt, nwords, offs, src, dst, len, p->list_tmp.p, p->list_tmp_bytes, (uint32_t)p->sc->num_cus, s));
    unsigned int h = 0;
    HIP_TRY(hipMemcpyAsync(&h, len, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *kept = h;
    return VMX_OK;
}

// first selected step of a handle: its master list is the job's active list as it stands — the tile order of
// render_init_pixels, every pixel at the same count — and from here on the schedule is the ragged one
static int progressive_make_ragged(vmx_progressive *p) {
    RenderJob &job = p->job;
    const size_t npix = job.npix, words = (npix + 63) / 64;
    const size_t tmp = live_compact_tmp_bytes((uint32_t)words);
    if (p->master[0].ensure(npix) || p->master[1].ensure(npix) || p->list_mask.ensure(words + 8) || p->list_u32.ensure(2 * words + 16) ||
        p->list_tmp.ensure(tmp + 256))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed for the handle's pixel lists");
    p->list_words = words, p->list_tmp_bytes = tmp;
    if (job.n_active)
        HIP_TRY(hipMemcpyAsync(p->master[0].p, job.pixels->active[job.cur_list].p, (size_t)job.n_active * 4, hipMemcpyDeviceToDevice, job.s));
    p->cur_master = 0, p->n_master = job.n_active;
    job.sched.ragged = true;
    return VMX_OK;
}

// the caller holds the scene's lock, has bound its device and has checked the handle's generation and `failed`
static int progressive_step_list(vmx_progressive *p, uint32_t samples, const unsigned char *d_select, vmx_stats *stats,
                                 uint32_t *selected, std::chrono::steady_clock::time_point t0) {
    vmx_scene *sc = p->sc;
    RenderJob &job = p->job;
    vmx_stats st;
    std::memset(&st, 0, sizeof(st));
    if (job.npix == 0) {  // (a rank without rows)
        if (stats) *stats = st;
        if (selected) *selected = 0;
        return VMX_OK;
    }
    if (!job.sched.ragged)
        if (int rc = progressive_make_ragged(p)) return rc;
    uint32_t n_sel = 0;
    int rc = progressive_compact(p, p->master[p->cur_master].p, p->n_master, d_select, job.pixels->active[job.cur_list].p, &n_sel);
    if (rc == VMX_OK && n_sel > 0) {
        job.n_active = n_sel;
        rc = render_run(sc, job, samples, &st, t0);
        // the master list without the pixels this step completed, in order
        if (rc == VMX_OK) {
            uint32_t left = 0;
            rc = progressive_compact(p, p->master[p->cur_master].p, p->n_master, nullptr, p->master[p->cur_master ^ 1].p, &left);
            p->cur_master ^= 1, p->n_master = left;
        }
        if (rc == VMX_OK) p->samples += st.samples, p->passes += st.passes, p->steps++;
    }
    if (rc) {
        p->failed = true;
        (void)hipStreamSynchronize(job.s);
        (void)hipGetLastError();  // (a refused allocation stays the thread's last error: not the next launch's)
        return rc;
    }
    job.n_active = p->n_master;
    if (stats) *stats = st;
    if (selected) *selected = n_sel;
    return VMX_OK;
}

int vmx_progressive_state_device(vmx_progressive *p, void *d_sums, void *d_counts) {
    if (!d_sums && !d_counts) return fail(VMX_ERR_INVALID, "no output: d_sums and d_counts are both NULL");
    if (((uintptr_t)d_sums | (uintptr_t)d_counts) & 3u) return fail(VMX_ERR_INVALID, "d_sums and d_counts must be 4-byte aligned");
    // (buffers that meet in their first element overlap whatever the image's size: seen without a handle)
    if (spans_meet(Span{d_sums, 16}, Span{d_counts, 4})) return fail(VMX_ERR_INVALID, "d_sums and d_counts overlap");
    if (!p) return fail(VMX_ERR_INVALID, "NULL handle");
    vmx_scene *sc = p->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (int rc = check_device_ptrs(sc->device, {{d_sums, "d_sums"}, {d_counts, "d_counts"}})) return rc;
    const size_t npix = p->job.npix;
    if (spans_meet(Span{d_sums, npix * 16}, Span{d_counts, npix * 4})) return fail(VMX_ERR_INVALID, "d_sums and d_counts overlap");
    if (npix == 0) return VMX_OK;
    if (d_sums) HIP_TRY(hipMemcpyAsync(d_sums, p->pixels.accum.p, npix * 16, hipMemcpyDeviceToDevice, p->job.s));
    if (d_counts) HIP_TRY(hipMemcpyAsync(d_counts, p->pixels.count.p, npix * 4, hipMemcpyDeviceToDevice, p->job.s));
    return VMX_OK;
}

int vmx_progressive_step_selected_device(vmx_progressive *p, uint32_t samples, const void *d_select, vmx_stats *stats,
                                         uint32_t *selected) {
    if (!d_select) return fail(VMX_ERR_INVALID, "NULL d_select");
    if (!p) return fail(VMX_ERR_INVALID, "NULL handle");
    if (int rc = selection_refusals(p, true, false)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    vmx_scene *sc = p->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (int rc = check_device_ptrs(sc->device, {{d_select, "d_select"}})) return rc;
    if (p->generation != sc->generation) return fail(VMX_ERR_INVALID, "scene updated since vmx_progressive_begin");
    if (p->failed) return fail(VMX_ERR_INVALID, "an earlier step of this handle failed: end it and begin again");
    return progressive_step_list(p, samples, (const unsigned char *)d_select, stats, selected, t0);
}

int vmx_progressive_error_device(vmx_progressive *p, const vmx_sampling_params *params, void *d_error, void *d_variance) {
    vmx_sampling_params prm;
    if (int rc = sampling_params(params, prm)) return rc;
    if (!d_error && !d_variance) return fail(VMX_ERR_INVALID, "no output: d_error and d_variance are both NULL");
    if (((uintptr_t)d_error | (uintptr_t)d_variance) & 3u) return fail(VMX_ERR_INVALID, "d_error and d_variance must be 4-byte aligned");
    if (spans_meet(Span{d_error, 4}, Span{d_variance, 4})) return fail(VMX_ERR_INVALID, "d_error and d_variance overlap");
    if (!p) return fail(VMX_ERR_INVALID, "NULL handle");
    if (int rc = selection_refusals(p, false, true)) return rc;
    vmx_scene *sc = p->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (int rc = check_device_ptrs(sc->device, {{d_error, "d_error"}, {d_variance, "d_variance"}})) return rc;
    const size_t npix = p->job.npix;
    if (spans_meet(Span{d_error, npix * 4}, Span{d_variance, npix * 4})) return fail(VMX_ERR_INVALID, "d_error and d_variance overlap");
    LAUNCH_TRY(launch_sampling_error(sampling_pass(p, prm), (float *)d_error, (float *)d_variance, p->job.s));
    return VMX_OK;
}

int vmx_progressive_select_device(vmx_progressive *p, const vmx_sampling_params *params, void *d_select, void *d_count) {
    vmx_sampling_params prm;
    if (int rc = sampling_params(params, prm)) return rc;
    if (!d_select) return fail(VMX_ERR_INVALID, "NULL d_select");
    if ((uintptr_t)d_count & 3u) return fail(VMX_ERR_INVALID, "d_count must be 4-byte aligned");
    if (spans_meet(Span{d_select, 1}, Span{d_count, 4})) return fail(VMX_ERR_INVALID, "d_select and d_count overlap");
    if (!p) return fail(VMX_ERR_INVALID, "NULL handle");
    if (int rc = selection_refusals(p, true, true)) return rc;
    vmx_scene *sc = p->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (int rc = check_device_ptrs(sc->device, {{d_select, "d_select"}, {d_count, "d_count"}})) return rc;
    if (spans_meet(Span{d_select, (size_t)p->job.npix}, Span{d_count, 4})) return fail(VMX_ERR_INVALID, "d_select and d_count overlap");
    if (d_count) HIP_TRY(hipMemsetAsync(d_count, 0, 4, p->job.s));
    LAUNCH_TRY(launch_sampling_select(sampling_pass(p, prm), (unsigned char *)d_select, (unsigned int *)d_count, p->job.s));
    return VMX_OK;
}

int vmx_progressive_step_adaptive(vmx_progressive *p, uint32_t samples, const vmx_sampling_params *params, vmx_stats *stats,
                                  uint32_t *selected) {
    vmx_sampling_params prm;
    if (int rc = sampling_params(params, prm)) return rc;
    if (!p) return fail(VMX_ERR_INVALID, "NULL handle");
    if (int rc = selection_refusals(p, true, true)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    vmx_scene *sc = p->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (p->generation != sc->generation) return fail(VMX_ERR_INVALID, "scene updated since vmx_progressive_begin");
    if (p->failed) return fail(VMX_ERR_INVALID, "an earlier step of this handle failed: end it and begin again");
    if (p->job.npix == 0) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        if (selected) *selected = 0;
        return VMX_OK;
    }
    if (p->select_map.ensure(p->job.npix)) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the selection map");
    LAUNCH_TRY(launch_sampling_select(sampling_pass(p, prm), p->select_map.p, nullptr, p->job.s));
    return progressive_step_list(p, samples, p->select_map.p, stats, selected, t0);
}

// ---- budgeted steps: every pixel takes the number of samples its own error asks for, in one pass (light-sampled handles) ----
static const vmx_sampling_budget_params kBudgetDefaults = {{0.5f, 0.05f, 8u, 1u, {0u, 0u, 0u, 0u}}, 0u, {0u, 0u, 0u}};

static int budget_params(const vmx_sampling_budget_params *in, vmx_sampling_budget_params &out) {
    out = in ? *in : kBudgetDefaults;
    vmx_sampling_params sel;
    if (int rc = sampling_params(&out.select, sel)) return rc;
    if (!reserved_zero(out.reserved)) return fail(VMX_ERR_INVALID, "vmx_sampling_budget_params: reserved words must be 0");
    return VMX_OK;
}

int vmx_sampling_budget_default_params(vmx_sampling_budget_params *out) { return default_params(out, kBudgetDefaults); }

// how the handle was begun (no device needed)
static int budget_refusals(const vmx_progressive *p, bool needs_moments) {
    if (!p->job.nee)
        return fail(VMX_ERR_INVALID, "budgeted steps are built for light-sampled handles only: begin the handle with vmx_progressive_begin_nee");
    return selection_refusals(p, true, needs_moments);
}

static BudgetPass budget_pass(const vmx_progressive *p, const vmx_sampling_budget_params &prm) {
    BudgetPass b{};
    b.a = sampling_pass(p, prm.select);
    const uint32_t B = p->job.smax;
    b.cap = prm.max_step ? std::min(prm.max_step, B) : B;
    return b;
}

// One budgeted pass.  The caller holds the scene's lock, has bound its device and has checked the handle's generation and
// `failed`; d_budget is read until the call returns.
static int progressive_step_budget(vmx_progressive *p, const unsigned int *d_budget, vmx_stats *stats, uint32_t *selected,
                                   std::chrono::steady_clock::time_point t0) {
    vmx_scene *sc = p->sc;
    RenderJob &job = p->job;
    Workspace &ws = sc->ws;
    hipStream_t s = job.s;
    vmx_stats st;
    std::memset(&st, 0, sizeof(st));
    uint32_t n_sel = 0;
    auto body = [&]() -> int {
        if (job.npix == 0) return VMX_OK;
        if (!job.sched.ragged)
            if (int rc = progressive_make_ragged(p)) return rc;
        const uint32_t n_master = p->n_master;
        if (n_master == 0) return VMX_OK;
        const size_t tmp = item_base_tmp_bytes(job.npix);
        if (p->item_cnt.ensure((size_t)job.npix + 1) || p->item_base.ensure((size_t)job.npix + 1) || p->item_tmp.ensure(tmp + 256))
            return fail(VMX_ERR_NOMEM, "hipMalloc failed for the step's item bases");
        p->item_tmp_bytes = tmp;
        if (int rc = sc->upd.done.wait(s)) return rc;
        // the step's list: the master list compacted by "has a budget and is unfinished"; its sample counts and their scan;
        // the list's length and the items come back in one round trip
        unsigned int *act = job.pixels->active[job.cur_list].p, *act_next = job.pixels->active[job.cur_list ^ 1].p;
        const unsigned int *master = p->master[p->cur_master].p;
        const uint32_t nwords = (n_master + 63u) / 64u;
        unsigned int *cnt = p->list_u32.p, *offs = cnt + p->list_words, *len = offs + p->list_words;
        LAUNCH_TRY(launch_list_words_budget(master, n_master, d_budget, p->pixels.cursor.p, job.fr.kmax, p->list_mask.p, cnt, s));
        HIP_TRY((hipError_t)launch_list_compact(p->list_mask.p, cnt, nwords, offs, master, act, len, p->list_tmp.p, p->list_tmp_bytes, (uint32_t)sc->num_cus, s));
        HIP_TRY((hipError_t)launch_item_base(act, len, n_master, d_budget, p->pixels.cursor.p, job.fr.kmax, job.smax, p->item_cnt.p,
                                             p->item_base.p, p->item_tmp.p, p->item_tmp_bytes, s));
        unsigned int h[2] = {0, 0};  // [0] the list's length, [1] the pass's items
        HIP_TRY(hipMemcpyAsync(&h[0], len, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&h[1], p->item_base.p + n_master, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        n_sel = h[0];
        const uint32_t items = h[1];
        if (n_sel == 0) return VMX_OK;
        if (n_sel > n_master || items < n_sel || (uint64_t)items > (uint64_t)job.n_pad_max * job.smax)
            return fail(VMX_ERR_HIP, "budgeted step: the item scan does not fit the pass's workspace");
        // the pass: k_nee over the items, k_resolve_budget over the list
        CallScope call{sc, s, t0};
        job.timed.clear();
        job.passes = 0;
        if (int rc = call.open()) return rc;
        if (int rc = call.start()) return rc;
        if (int rc = render_bind(sc, job, 0)) return rc;
        if (int rc = call.clear_counters()) return rc;
        WorkDev wk = make_work(ws.heads.p, nullptr);
        wk.active = act;
        wk.n_active = n_sel, wk.n_pad = (n_sel + 63u) & ~63u, wk.samples = 1, wk.div_samples = make_fastdiv(1);
        wk.pixel_major = 1;
        wk.flat_ids = p->item_base.p;
        LaunchCfg cfg;
        if (int rc = nee_launch_cfg(sc, s, job.tn, items, false, wk, cfg, true)) return rc;
        HIP_TRY(hipMemsetAsync(ws.heads.p, 0, 4, s));
        if (int rc = timed_begin(ws, job.timed, s, 0, VMX_K_OTHER)) return rc;
        LAUNCH_TRY(launch_nee(sc->dev, job.fr, wk, job.px, nullptr, nullptr, items, ws.rad.p, ws.counters.p, cfg, s, sc->em.dev));
        if (int rc = timed_end(job.timed, s)) return rc;
        HIP_TRY(hipMemsetAsync(ws.next_count.p, 0, 8, s));
        if (int rc = timed_begin(ws, job.timed, s, -1, VMX_K_RESOLVE)) return rc;
        LAUNCH_TRY(launch_resolve_budget(job.fr, act, n_sel, p->item_base.p, ws.rad.p, job.px, act_next, ws.next_count.p, job.d_out,
                                         ws.counters.p, s, job.moments));
        if (int rc = timed_end(job.timed, s)) return rc;
        job.launches += 2;
        job.passes = 1;
        job.frame_passes++;
        int rc = call.finish(job.timed, &st, job.launches, job.passes);
        job.launches = 0;
        if (rc) return rc;
        // the master list without the pixels this step completed, in order
        uint32_t left = 0;
        if ((rc = progressive_compact(p, p->master[p->cur_master].p, p->n_master, nullptr, p->master[p->cur_master ^ 1].p, &left))) return rc;
        p->cur_master ^= 1, p->n_master = left;
        p->samples += st.samples, p->passes += st.passes, p->steps++;
        return VMX_OK;
    };
    if (int rc = body()) {
        p->failed = true;
        (void)hipStreamSynchronize(s);
        (void)hipGetLastError();
        return rc;
    }
    if (job.sched.ragged) job.n_active = p->n_master;
    if (stats) *stats = st;
    if (selected) *selected = n_sel;
    return VMX_OK;
}

int vmx_progressive_budget_device(vmx_progressive *p, const vmx_sampling_budget_params *params, void *d_budget, void *d_total) {
    vmx_sampling_budget_params prm;
    if (int rc = budget_params(params, prm)) return rc;
    if (!d_budget) return fail(VMX_ERR_INVALID, "NULL d_budget");
    if ((uintptr_t)d_budget & 3u) return fail(VMX_ERR_INVALID, "d_budget must be 4-byte aligned");
    if ((uintptr_t)d_total & 7u) return fail(VMX_ERR_INVALID, "d_total must be 8-byte aligned");
    if (spans_meet(Span{d_budget, 4}, Span{d_total, 8})) return fail(VMX_ERR_INVALID, "d_budget and d_total overlap");
    if (!p) return fail(VMX_ERR_INVALID, "NULL handle");
    if (int rc = budget_refusals(p, true)) return rc;
    vmx_scene *sc = p->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (int rc = check_device_ptrs(sc->device, {{d_budget, "d_budget"}, {d_total, "d_total"}})) return rc;
    if (spans_meet(Span{d_budget, (size_t)p->job.npix * 4}, Span{d_total, 8})) return fail(VMX_ERR_INVALID, "d_budget and d_total overlap");
    if (d_total) HIP_TRY(hipMemsetAsync(d_total, 0, 8, p->job.s));
    LAUNCH_TRY(launch_sampling_budget(budget_pass(p, prm), (unsigned int *)d_budget, (unsigned long long *)d_total, p->job.s));
    return VMX_OK;
}

int vmx_progressive_step_budget_device(vmx_progressive *p, const void *d_budget, vmx_stats *stats, uint32_t *selected) {
    if (!d_budget) return fail(VMX_ERR_INVALID, "NULL d_budget");
    if ((uintptr_t)d_budget & 3u) return fail(VMX_ERR_INVALID, "d_budget must be 4-byte aligned");
    if (!p) return fail(VMX_ERR_INVALID, "NULL handle");
    if (int rc = budget_refusals(p, false)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    vmx_scene *sc = p->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (int rc = check_device_ptrs(sc->device, {{d_budget, "d_budget"}})) return rc;
    if (p->generation != sc->generation) return fail(VMX_ERR_INVALID, "scene updated since vmx_progressive_begin");
    if (p->failed) return fail(VMX_ERR_INVALID, "an earlier step of this handle failed: end it and begin again");
    return progressive_step_budget(p, (const unsigned int *)d_budget, stats, selected, t0);
}

int vmx_progressive_step_budgeted(vmx_progressive *p, const vmx_sampling_budget_params *params, vmx_stats *stats, uint32_t *selected) {
    vmx_sampling_budget_params prm;
    if (int rc = budget_params(params, prm)) return rc;
    if (!p) return fail(VMX_ERR_INVALID, "NULL handle");
    if (int rc = budget_refusals(p, true)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    vmx_scene *sc = p->sc;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (p->generation != sc->generation) return fail(VMX_ERR_INVALID, "scene updated since vmx_progressive_begin");
    if (p->failed) return fail(VMX_ERR_INVALID, "an earlier step of this handle failed: end it and begin again");
    if (p->job.npix == 0) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        if (selected) *selected = 0;
        return VMX_OK;
    }
    if (p->budget_map.ensure(p->job.npix)) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the budget plane");
    LAUNCH_TRY(launch_sampling_budget(budget_pass(p, prm), p->budget_map.p, nullptr, p->job.s));
    return progressive_step_budget(p, p->budget_map.p, stats, selected, t0);
}

} /* extern "C" */
