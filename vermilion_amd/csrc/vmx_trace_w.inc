// vmx_trace_w.inc — the body of k_trace_w (vmx_kernels.hip, which describes it), included twice: as the template
// kernel k_trace_w<SRC, LIVE, SORT, GUIDE>, and (VMX_TRACE_W_VISITS) as k_trace_w_visits, the counting form of
// k_trace_w<1, false, false, true> behind the debug entry vmx_guide_trace_visits.  Two kernels from one text, not one
// kernel that calls a shared function and not a fifth template parameter: either changes the product kernels'
// instruction streams or symbols (tools/isa_compare.py).
#if VMX_TRACE_W_VISITS
__global__ void __launch_bounds__(256, VMX_TRACE_WAVES_PER_SIMD) __attribute__((amdgpu_num_sgpr(VMX_TRACE_SGPRS)))
k_trace_w_visits(SceneDev sc, FrameDev fr, WorkDev wk, PathArrays pa, GuideDev gd, uint2 *visits_out) {
    constexpr int SRC = 1;
    constexpr bool LIVE = false, SORT = false, GUIDE = true, VISITS = true;
#else
template <int SRC, bool LIVE = false, bool SORT = false, bool GUIDE = false>
__global__ void __launch_bounds__(256, VMX_TRACE_WAVES_PER_SIMD) __attribute__((amdgpu_num_sgpr(VMX_TRACE_SGPRS)))
k_trace_w(SceneDev sc, FrameDev fr, WorkDev wk, PathArrays pa, GuideDev gd) {
    constexpr bool VISITS = false;
#endif
    static_assert(!GUIDE || (SRC == 1 && !LIVE), "the guide is for bounce rays");
    static_assert(!VISITS || GUIDE, "visits are counted on the guide walk");
    [[maybe_unused]] uint32_t n_inner = 0, n_tris = 0;  // VISITS: of the ray this lane holds
    extern __shared__ uint2 lds_stack[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int lds_entries = (int)wk.lds_entries;
#ifdef VMX_STEP_PROFILE
    __shared__ unsigned long long s_prof[4][10][2];
    if (lane < 20) s_prof[wave][lane >> 1][lane & 1] = 0;
    unsigned long long prof_t = __builtin_readcyclecounter();
    if (lane == 0) atomicMin(&g_wave_span[SRC][0], (unsigned long long)wall_clock64());
#endif
    uint2 *stk = lds_stack + (size_t)wave * (lds_entries + 1) * 64 + lane;
    uint2 *ovf = (uint2 *)wk.overflow_stack +
                 ((size_t)(blockIdx.x * (blockDim.x >> 6) + wave) * wk.overflow_entries) * 64 + lane;
    const float4 *__restrict__ inner = SRC == 0 ? (const float4 *)wk.cam_inner : (GUIDE ? (const float4 *)gd.base : (const float4 *)sc.inner);
    const float4 *__restrict__ tris = SRC == 0 ? (const float4 *)wk.cam_tris : (const float4 *)sc.tris;
    float2 *__restrict__ hit_out = (float2 *)pa.hit;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const uint32_t kReserve = wk.reserve;
    const uint32_t nsrc = wk.nsrc, refill_min = wk.refill_min;
    const uint32_t band_slots = wk.band_slots, band_items = wk.band_items;
    const uint32_t root_ref = GUIDE ? gd.root_ref : sc.root_ref;
    const uint32_t tri_off = GUIDE ? gd.tri_off : sc.tri_off;
    // GUIDE: the prune bound and the smallest accepted distance of any triangle but the nearest (guide_walk.h); `slot` is
    // the winner's slot in the GUIDE until the rule has run
    float cut = 0.f, second = 0.f;
    uint32_t n_settled = 0, n_fallback = 0;  // (wave-uniform)

    uint32_t src = blockIdx.x % nsrc, res_lo = 0, res_hi = 0, tried = 0;
    bool exhausted = false;
    bool exact = false;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
    float ix = 0.f, iy = 0.f, iz = 0.f, best = 0.f;
    int slot = -1, sp = 0;
    uint32_t cur = kIdle, pid = 0;
    // SORT: the ray's flag word; bit 31 set while the lane holds a finished ray that has not been sorted yet
    uint32_t rflags = 0;
    uint32_t out_lo = 0, out_hi = 0, n_rays = 0, n_hits = 0;  // (wave-uniform) reserved list entries; rays / triangle hits settled here
    uint32_t n_listed = 0;  // (wave-uniform) camera rays settled by a list claim
    // camera rays: direction octant of the wave's rays if they all share it (else 8): selects the
    // per-octant copy of the node table (k_camera_tables) for wave-uniform steps
    uint32_t wave_octant = 8;
    stk[0] = make_uint2(kBottom, 0xFF800000u);  // bottom entry; pushes start at level 1, so it stays

    // SORT: settle the finished rays the wave's lanes hold (wave-uniform code: called before a refill and at the end)
    auto sort_finished = [&]() {
        const bool fin = (rflags >> 31) != 0;
        const bool material = slot >= 0;
        // ends by its draws (bit 0 / 1 by the material flag) and no light sphere in reach (bit 2): nothing to shade
        // (wk.keep_all: nothing is settled here — every ray gets its record and its full RayCast in k_shade)
        const bool done = !wk.keep_all && fin && (((material ? rflags : rflags >> 1) & 1u) != 0) && (rflags & 4u) == 0;
        // (a bounce "ray" with a non-finite direction is traced like the others but is not counted as a ray: tally_add)
        const bool counted = SRC == 0 || finite3(dx, dy, dz);
        n_rays += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(done && counted));
        n_hits += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(done && counted && material));
        const bool todo = fin && !done;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(todo);
        const uint32_t n = (uint32_t)__popcll(m);
        float4 *__restrict__ rec = (float4 *)wk.out_rec;
        if (n != 0) {
            constexpr uint32_t kRec = SRC == 0 ? 2 : 1;  // float4s per entry; the last one holds (t, leaf slot, position, -)
            // the entries fill the wave's chunk to its end and go on in a new one: nothing is left unused but the tail of
            // the wave's last chunk (padded at the end), so the list never holds more than rays + 255 per wave
            const uint32_t rem = out_hi - out_lo, rank = (uint32_t)__popcll(m & lt_mask);
            uint32_t at = out_lo + rank;
            if (n > rem) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(wk.out_count, kOutChunk);
                base = __builtin_amdgcn_readfirstlane(base);
                if (rank >= rem) at = base + (rank - rem);
                out_lo = base + (n - rem);
                out_hi = base + kOutChunk;
            } else {
                out_lo += n;
            }
            // (the list is sized for every path of the pass + one chunk per wave, so `at` cannot reach its end; an entry
            // that would is dropped and reported instead of written — never a store past the allocation)
            if (todo && at < wk.out_capacity) {
                if (SRC == 0) rec[(size_t)at * kRec] = make_float4(dx, dy, dz, __uint_as_float(rflags & 7u));  // (bounce paths: ray and stream are in state[pid])
                rec[(size_t)at * kRec + (kRec - 1)] = make_float4(best, __int_as_float(slot), __uint_as_float(pid), 0.f);
            } else if (todo) {
                atomicAdd(&wk.out_ctr->overflow, 1ull);
            }
        }
        rflags &= 0x7FFFFFFFu;
    };
    // GUIDE: the path ids of the lanes with `fb` go to the fallback list (wave-uniform code)
    auto fallback_append = [&](bool fb) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(fb);
        if (m == 0) return;
        const uint32_t n = (uint32_t)__popcll(m);
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(gd.fb_count, n);
        base = __builtin_amdgcn_readfirstlane(base);
        const uint32_t at = base + (uint32_t)__popcll(m & lt_mask);
        // (the list holds every path id of the pass, and a path is appended once per launch: `at` stays below its end; an
        // entry that would not is reported instead of written, as sort_finished reports a record)
        if (fb && at < gd.fb_capacity) gd.fb_ids[at] = pid;
        else if (fb) atomicAdd(&gd.overflow->overflow, 1ull);
        n_fallback += n;
    };
    // GUIDE: the rule (gw_settle) for the finished rays the wave's lanes hold, before sort_finished / the hit records
    auto guide_finished = [&]() {
        const bool fin = (rflags >> 31) != 0;
        bool fb = false;
        if (fin) {
            const bool have = slot >= 0;
            float r[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            int ref_slot = -1;
            if (have) {
                const float4 *rec = (const float4 *)((const char *)inner + (tri_off + (uint32_t)slot * 48u));
                const float4 a = rec[0], b = rec[1], c = rec[2];
                r[0] = a.x, r[1] = a.y, r[2] = a.z, r[3] = a.w, r[4] = b.x, r[5] = b.y, r[6] = b.z, r[7] = b.w, r[8] = c.x;
                ref_slot = __float_as_int(c.z);  // TriRecord::pad[0]: the triangle's leaf slot in the reference tree
            }
            const float o[3] = {ox, oy, oz}, d[3] = {dx, dy, dz}, inv[3] = {ix, iy, iz};
            if (gw_settle(have, r, best, second, o, d, inv, gd.scene_max)) slot = ref_slot;
            else fb = true;
        }
        n_settled += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(fin && !fb));
        fallback_append(fb);
        if (fb) rflags &= 0x7FFFFFFFu;  // the second launch settles it
        if (!SORT) {
            if (fin && !fb) hit_out[pid] = make_float2(best, __int_as_float(slot));
            rflags &= 0x7FFFFFFFu;
        }
    };

    // One traversal step of every active lane.  The NaN-exact box form runs only while one of the
    // wave's rays needs it.
    // base of the node table the wave-uniform steps of this batch read: the wave's octant copy if its
    // rays share an octant (OCT), else the plain copy; records are addressed by a 32-bit byte offset
    const char *uni_base = (const char *)inner;
    auto push = [&](uint2 e) {
        stack_push(stk, ovf, lds_entries, sp, e);
        ++sp;
    };
    auto step = [&](auto exact_tag, auto oct_tag) {
        constexpr bool EXACT = decltype(exact_tag)::value;  // NaN-exact box form
        constexpr bool OCT = decltype(oct_tag)::value;      // uniform steps read near-plane-first records
        if constexpr (SRC == 1) {
            // ---- bounce rays: ONE fetch phase per step.  Incoherent rays put inner-node lanes and leaf lanes in
            // the same wave at every step; fetched separately (node loads, wait, box math; triangle loads, wait,
            // triangle math) a wave-step pays two dependent memory round trips, and this kernel is bound by that
            // latency (SQ_WAIT_ANY 67 % of its wave cycles, 5 waves per SIMD; profiles/).  Inner records and
            // triangle records live in one allocation (SceneDev::tri_off), so every traversing lane forms a
            // 32-bit byte offset to ITS record, all of them load 56 bytes in one set of four loads, and the wave
            // waits once.  Same tests per ray in the same order (bvh.cpp:47-145).
            const bool leaf = (int)cur < 0;
            float4 q0, q1, q2, q3;
            // byte offset of this lane's record (0 while the lane is not traversing)
            // (round 3: the same transposition through LDS — 4 ds_write_b128 + 4 ds_read_b128 instead of the 32 DPP
            // selects — was measured in the kernel as well: its 4 KB of staging per wave cost waves or LDS stack levels,
            // 50.5 ms for the bounce stage against 42.9; profiles/r03_lds_transpose.txt, tools/ta_probe.hip)
            quad_fetch_record((const char *)inner,
                              cur == kIdle ? 0u : (leaf ? tri_off + (cur & kLeafStartMask) * 48u : (cur << 6)),
                              lane, q0, q1, q2, q3);
            if (cur != kIdle) {
                if (!leaf) {
                    float tn0, tf0, tn1, tf1;
                    child_boxes<EXACT>(q0, q1, q2, ox, oy, oz, ix, iy, iz, tn0, tf0, tn1, tf1);
                    if (VISITS) ++n_inner;
                    if (GUIDE)
                        cur = choose_child_cull(tn0, tf0, tn1, tf1, __float_as_uint(q3.x), __float_as_uint(q3.y),
                                                __float_as_uint(q3.z), __float_as_uint(q3.w), cut, push);
                    else cur = choose_child(tn0, tf0, tn1, tf1, __float_as_uint(q3.x), __float_as_uint(q3.y), best, push);
                } else {
                    // one triangle of the leaf (triangle.cpp:4-54)
                    if (VISITS) ++n_tris;
                    float dist;
                    const bool hit = tri_test(q0, q1, q2.x, ox, oy, oz, dx, dy, dz, dist);
                    if (hit && dist < best) {  // strict <: first tested wins ties (bvh.cpp:90)
                        if (GUIDE) second = best, cut = dist * kGwCut;
                        best = dist;
                        slot = (int)(cur & kLeafStartMask);
                    } else if (GUIDE && hit) {
                        second = fminf(second, dist);
                    }
                    cur = leaf_advance(cur);
                }
            }
        } else {
            // ---- camera rays: inner references are the values below kPop, leaf references have bit 31
            if (cur < kPop) {
                // ---- inner node: both children boxes (bbox.cpp:70-83), nearer child first (bvh.cpp:103-132)
                float tn0, tf0, tn1, tf1;
                uint32_t lref, rref;
                const uint32_t cur0 = __builtin_amdgcn_readfirstlane(cur);
                if (!EXACT && __builtin_amdgcn_ballot_w64(cur != cur0) == 0) {
                    // every lane of this step is at the same node: one fetch through the scalar cache,
                    // and the products take the record straight from SGPRs
                    typedef float f32x4 __attribute__((ext_vector_type(4)));
                    typedef const __attribute__((address_space(4))) f32x4 *scalar_ptr;
                    const scalar_ptr rec = (scalar_ptr)(uintptr_t)(uni_base + (uint32_t)(cur0 << 6));
                    const f32x4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
                    if (OCT) {  // near planes first in this octant's copy: no min/max pairs
                        tn0 = vmax3(r0.x * ix, r0.y * iy, r0.z * iz);
                        tf0 = vmin3(r0.w * ix, r1.x * iy, r1.y * iz);
                        tn1 = vmax3(r1.z * ix, r1.w * iy, r2.x * iz);
                        tf1 = vmin3(r2.y * ix, r2.z * iy, r2.w * iz);
                    } else {
                        box_net(r0.x * ix, r0.y * iy, r0.z * iz, r0.w * ix, r1.x * iy, r1.y * iz, tn0, tf0);
                        box_net(r1.z * ix, r1.w * iy, r2.x * iz, r2.y * ix, r2.z * iy, r2.w * iz, tn1, tf1);
                    }
                    lref = __float_as_uint(r3.x), rref = __float_as_uint(r3.y);
                } else {
                    // (32-bit byte offset from a scalar base: the record tables are < 4 GB, and an index scaled in 64 bits
                    // costs two 64-bit VALU operations per fetch)
                    const float4 *rec = (const float4 *)((const char *)inner + (uint32_t)(cur << 6));
                    const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2];
                    const float2 q3 = *(const float2 *)(rec + 3);
                    child_boxes_rel<EXACT>(q0, q1, q2, ix, iy, iz, tn0, tf0, tn1, tf1);
                    lref = __float_as_uint(q3.x), rref = __float_as_uint(q3.y);
                }
                // (the lane-mask form of the choice: the &&/|| form is evaluated partly under temporary exec masks here)
                cur = choose_child_masks(tn0, tf0, tn1, tf1, lref, rref, best, push);
            } else if ((int)cur < 0) {
                // ---- one triangle of the leaf (triangle.cpp:4-54) from its camera-relative record
                const uint32_t ti = (cur & kLeafStartMask) * 4;
                const float4 a = tris[ti], b = tris[ti + 1], c = tris[ti + 2];
                const float cd = ((const float *)tris)[ti * 4 + 12];
                float dist;
                const bool hit = tri_test_cam(a, b, c, cd, dx, dy, dz, dist);
                if (hit && dist < best) {  // strict <: first tested wins ties (bvh.cpp:90)
                    best = dist;
                    slot = (int)(cur & kLeafStartMask);
                }
                cur = leaf_advance(cur);
            }
        }
        if (cur == kPop) {
            cur = pop_to_next(stk, ovf, lds_entries, sp, GUIDE ? cut : best);
            if (cur == kBottom) {
#if VMX_TRACE_W_VISITS
                visits_out[pid] = make_uint2(n_inner, n_tris);
#endif
                if (SORT || GUIDE) rflags |= 0x80000000u;  // settled at the next refill (the lane keeps t, slot, direction until then)
                else hit_out[pid] = make_float2(best, __int_as_float(slot));
                cur = kIdle;
            }
        }
    };

    for (;;) {
        // ---- refill idle lanes -------------------------------------------------------
        const unsigned long long idle = __builtin_amdgcn_ballot_w64(cur == kIdle);
        if (idle != 0 && !exhausted && ((uint32_t)__popcll(idle) >= refill_min || idle == ~0ull)) {
            if (GUIDE) guide_finished();
            if (SORT) sort_finished();
            for (;;) {
                if (res_lo == res_hi) {
                    uint32_t lim = SRC == 0 ? band_items : min(wk.qids.counts[src * 32], wk.qids.sub_capacity);
                    if (LIVE) {  // (scalar loads, once per reservation)
                        const uint32_t n = *wk.live_count, seg = live_band(n);
                        lim = min(seg, n - min(n, src * seg));
                    }
                    if (SRC == 0 && !LIVE && !SORT && wk.unclaimed) {  // the pass's listed slots, in bands of the ordered list
                        // (wk.qids.ids: the last source is the straggler list k_raygen<0, true> left, path ids in any order)
                        const uint32_t nband = wk.qids.ids ? nsrc - 1u : nsrc;
                        const uint32_t n = *wk.unclaimed_count, seg = (n + nband - 1u) / nband;
                        lim = src == nband ? min(wk.qids.counts[0], wk.qids.sub_capacity) : min(seg, n - min(n, src * seg)) * wk.samples;
                    }
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&wk.heads[src * 32], kReserve);
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (base >= lim) {
                        src = (src + 1 == nsrc) ? 0 : src + 1;
                        if (++tried == nsrc) {
                            exhausted = true;
                            break;
                        }
                        continue;
                    }
                    tried = 0;
                    res_lo = base;
                    res_hi = min(base + kReserve, lim);
                }
                const unsigned long long want = __builtin_amdgcn_ballot_w64(cur == kIdle);
                if (want == 0) break;
                const uint32_t avail = res_hi - res_lo;
                const uint32_t rank = (uint32_t)__popcll(want & lt_mask);
                const bool take = cur == kIdle && rank < avail;
                const uint32_t item = res_lo + rank;
                res_lo = __builtin_amdgcn_readfirstlane(res_lo + min((uint32_t)__popcll(want), avail));
                bool listed = false;  // this lane's ray was settled by its pixel's list
                bool unwalked = false;  // GUIDE: this lane's ray goes to the fallback list as it is
                if (take) {
                    bool valid = true;
                    uint32_t claim = kClaimNone;  // (camera rays: the pixel's claim, pixel_claim.h)
                    uint4 lrec = make_uint4(kClaimNone, kClaimNone, kClaimNone, kClaimNone);  // ... and its list
                    if (LIVE) {
                        pid = src * live_band(*wk.live_count) + item;  // list position
                    } else if (SRC == 0) {
                        uint32_t j, s_idx;
                        bool straggler = false;  // (wave-uniform) a path id of the straggler list: a ray of a listed pixel that its list did not settle
                        if (!SORT && wk.unclaimed) {  // (a fused pass is pixel-major) band-local item -> (list entry, sample)
                            const uint32_t nband = wk.qids.ids ? nsrc - 1u : nsrc;
                            if (src == nband) {
                                straggler = true, j = 0, s_idx = 0;
                            } else {
                                const uint32_t sl = fast_div(item, wk.div_samples), n = *wk.unclaimed_count;
                                j = item - sl * wk.samples, s_idx = wk.unclaimed[src * ((n + nband - 1u) / nband) + sl];
                            }
                        } else if (wk.pixel_major) {
                            const uint32_t sl = fast_div(item, wk.div_samples);
                            j = item - sl * wk.samples, s_idx = src * band_slots + sl;
                        } else {
                            j = item / band_slots, s_idx = src * band_slots + (item - j * band_slots);
                        }
                        if (!SORT && straggler) {
                            pid = wk.qids.ids[item];  // (its pixel is active and unclaimed, and its list has had its say)
                        } else {
                            valid = s_idx < wk.n_active;
                            pid = path_id(wk, j, s_idx);
                            if (wk.claims && valid) claim = wk.claims[wk.active[s_idx]];
                            // (a fused pass hands no claims on — its listed slots have none — and no lists either where
                            // k_raygen<0, true> has run the rule: then the listed slots are the walk slots)
                            if (wk.claim_lists && valid && claim == kClaimNone) lrec = ((const uint4 *)wk.claim_lists)[wk.active[s_idx]];
                        }
                    } else {
                        pid = wk.qids.ids[(size_t)src * wk.qids.sub_capacity + item];
                    }
                    if (valid) {
                        if (SRC == 0) {  // camera ray: (direction, flag word), origin from the frame
                            const float4 a = ((const float4 *)pa.rayA)[pid];
                            ox = fr.px, oy = fr.py, oz = fr.pz, dx = a.x, dy = a.y, dz = a.z;
                            valid = __float_as_uint(a.w) != 0xFFFFFFFFu;  // sample slot past the pixel's last sample
                            if (SORT && valid) rflags = __float_as_uint(a.w) & 7u;
                        } else {
                            const float4 a = ((const float4 *)pa.state)[(size_t)pid * 4], b = ((const float4 *)pa.state)[(size_t)pid * 4 + 1];
                            ox = a.x, oy = a.y, oz = a.z, dx = a.w, dy = b.x, dz = b.y;
                            valid = __float_as_uint(b.z) != 0xFFFFFFFFu;
                            if (SORT && valid) rflags = __float_as_uint(b.w) & 7u;  // k_shade: step_bits of this step
                        }
                    }
                    if (SRC == 0 && !LIVE && valid && claim != kClaimNone) {
                        // the pixel's claim settles this ray's BVH query: the claimed triangle's own test (the t the walk
                        // would have found, bit for bit), or no hit; the lane stays idle and takes the next item
                        best = 999999999.f, slot = -1;
                        if (claim != kClaimMiss) {
                            const float4 a = tris[claim * 4], b = tris[claim * 4 + 1], c = tris[claim * 4 + 2];
                            const float cd = ((const float *)tris)[claim * 16 + 12];
                            float dist;
                            if (tri_test_cam(a, b, c, cd, dx, dy, dz, dist) && dist < best) best = dist, slot = (int)claim;
                        }
                        if (SORT) rflags |= 0x80000000u;  // settled below, before the lane takes another item
                        else hit_out[pid] = make_float2(best, __int_as_float(slot));
                        valid = false;
                    }
                    if (SRC == 0 && !LIVE && valid && lrec.x != kClaimNone) {
                        // the pixel's list: the ray's own test on its two to four members settles it where the nearest one
                        // is clear of the others and of its box's faces (pc_list_settle); else the ray walks
                        float t;
                        uint32_t m;
                        if (pc_list_settle((const float *)tris, lrec.x, lrec.y, lrec.z, lrec.w, dx, dy, dz, t, m)) {
                            best = t, slot = (int)m;
                            if (SORT) rflags |= 0x80000000u;
                            else hit_out[pid] = make_float2(best, __int_as_float(slot));
                            valid = false, listed = true;
                        }
                    }
                    if (valid) {
                        ray_start(dx, dy, dz, root_ref, 999999999.f, ix, iy, iz, best, slot, sp, cur);
                        exact = !(finite3(ix, iy, iz) && finite3(ox, oy, oz));
                        if (GUIDE) {
                            cut = best * kGwCut, second = 3.0e38f;
                            exact = false;
                            if (VISITS) n_inner = n_tris = 0;
                            if (!gw_ray_ok(ox, oy, oz, dx, dy, dz, ix, iy, iz, gd.scene_max)) cur = kIdle, unwalked = true;
                        }
                    }
                }
                if (GUIDE) fallback_append(unwalked);
                if (SRC == 0 && !LIVE && wk.claim_lists) n_listed += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(listed));
                if (SRC == 0 && !LIVE && SORT && wk.claims) {
                    if (__builtin_amdgcn_ballot_w64((rflags >> 31) != 0) != 0) sort_finished();
                }
            }
        }
        const unsigned long long active = __builtin_amdgcn_ballot_w64(cur != kIdle);
#ifdef VMX_STEP_PROFILE
        {
            const unsigned long long now = __builtin_readcyclecounter();
            if (lane == 0) {
                s_prof[wave][5][0] += now - prof_t;
                s_prof[wave][5][1] += 1;
            }
        }
#endif
        if (active == 0) break;
        if (SRC == 0) {
            const uint32_t oct = (__float_as_uint(ix) >> 31) | ((__float_as_uint(iy) >> 31) << 1) |
                                 ((__float_as_uint(iz) >> 31) << 2);
            const uint32_t o0 = (uint32_t)__builtin_amdgcn_readlane((int)oct, (int)__ffsll((long long)active) - 1);
            wave_octant = __builtin_amdgcn_ballot_w64(cur != kIdle && oct != o0) == 0 ? o0 : 8u;
        }
        if (!GUIDE && __builtin_amdgcn_ballot_w64(exact && cur != kIdle) != 0) {
#pragma unroll 1
            for (int act = 0; act < 8; ++act) VMX_PROF_STEP(std::true_type{}, std::false_type{});
        } else if (SRC == 0 && wave_octant < 8) {
            uni_base = (const char *)inner + (size_t)wave_octant * wk.cam_n_inner * 64;
            // (16 steps per batch here: these waves refill only when all 64 lanes are done; measured 8 / 16 / 32)
#pragma unroll 1
            for (int act = 0; act < VMX_CAM_BATCH; ++act) {
                // all 64 lanes at the same inner node: the assembly loop takes the wave down the tree while that
                // holds (uniform_descent), the general step goes on from where it stopped
                const unsigned long long trav = __builtin_amdgcn_ballot_w64(cur != kIdle);
                if (trav == 0) break;  // every ray of the wave is done: on to the refill (these waves refill all 64 lanes at once)
                {
                    const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)__ffsll((long long)trav) - 1);
                    if (c0 < kPop && __builtin_amdgcn_ballot_w64(cur != kIdle && (cur != c0 || sp >= lds_entries)) == 0)
                    {
#ifdef VMX_STEP_PROFILE
                        const unsigned long long t0_ = __builtin_readcyclecounter();
#endif
                        const uint32_t done = uniform_descent(sp, cur, ix, iy, iz, best, slot, dx, dy, dz, (uint32_t)(uintptr_t)stk,
                                                              uni_base, (uint32_t)((const char *)tris - uni_base), c0, lds_entries,
                                                              trav);
#ifdef VMX_STEP_PROFILE
                        act += (int)done;
#else
                        (void)done;
                        act += 4;  // about what a descent takes (4.7 nodes on the bench frame); the batch only paces the refill test
#endif
#ifdef VMX_STEP_PROFILE
                        if (lane == 0) {
                            s_prof[wave][7][0] += __builtin_readcyclecounter() - t0_;
                            s_prof[wave][7][1] += done;
                            s_prof[wave][8][1] += 1;  // entries
                            s_prof[wave][8][0] += (unsigned long long)__popcll(trav);  // traversing lanes at entry
                        }
#endif
                    }
                }
                VMX_PROF_STEP(std::false_type{}, std::true_type{});
            }
        } else {
            uni_base = (const char *)inner;
#pragma unroll 1
            for (int act = 0; act < 8; ++act) VMX_PROF_STEP(std::false_type{}, std::false_type{});
        }
#ifdef VMX_STEP_PROFILE
        prof_t = __builtin_readcyclecounter();
#endif
    }
    if (SRC == 0 && !LIVE && lane == 0 && n_listed) atomicAdd(&wk.list_ctr->listed, (unsigned long long)n_listed);
    if (GUIDE) {
        guide_finished();
        if (lane == 0) {
            if (n_settled) atomicAdd(&gd.ctr[0], (unsigned long long)n_settled);
            if (n_fallback) atomicAdd(&gd.ctr[1], (unsigned long long)n_fallback);
        }
    }
    if (SORT) {
        sort_finished();
        float4 *__restrict__ rec = (float4 *)wk.out_rec;
        constexpr uint32_t kRec = SRC == 0 ? 2 : 1;
        for (uint32_t i = out_lo + lane; i < min(out_hi, wk.out_capacity); i += 64u) rec[(size_t)i * kRec + (kRec - 1)] = make_float4(0.f, 0.f, __uint_as_float(0xFFFFFFFFu), 0.f);
        if (lane == 0) {
            if (n_rays) atomicAdd(&wk.out_ctr->stage[SRC].rays, (unsigned long long)n_rays);
            if (n_hits) atomicAdd(&wk.out_ctr->stage[SRC].tri_hits, (unsigned long long)n_hits);
        }
    }
#ifdef VMX_STEP_PROFILE
    if (lane < 20) atomicAdd(&g_step_prof[SRC][lane >> 1][lane & 1], s_prof[wave][lane >> 1][lane & 1]);
    if (lane == 0) {
        const unsigned long long now = (unsigned long long)wall_clock64();
        atomicMax(&g_wave_span[SRC][1], now);
        atomicAdd(&g_wave_span[SRC][2], now);
        atomicAdd(&g_wave_span[SRC][3], 1ull);
    }
#endif
}
