// vmx_trace_pool.inc — A/B library only (make ab): the phase-pure bounce traversal VERDICT r3 item 1 asked to be
// MEASURED, as a probe on the real scene and the real rays.  Not in the product; profiles/r04_state_pool.txt has the
// numbers and why it stays out.
//
// k_trace_w<1> pays ~325 issue slots per wave-step, in which 82 % of the lane-steps need only the two-box block and 18 %
// only the Moeller-Trumbore block (99.6 % of its wave-steps hold inner-node AND leaf lanes).  Here a wave holds ONE
// phase: the state of a ray lives in LDS by slot, not in a lane —
//     sA[slot] = (o.xyz, best)   sB[slot] = (1/d.xyz, node reference)   sC[slot] = (d.xyz, leaf slot of the hit)
//     sD[slot] = (path id, stack depth)   stk[level][slot] = (node reference, entry distance), deeper levels in HBM
// — and three slot lists per block (at an inner node / at a leaf / finished or empty) feed the waves: a wave takes 64
// slots of one list, runs that phase's block only (inner: both child boxes, push, descend; leaf: one triangle;
// finished: write the hit record, load the next ray), pops where the reference pops (bvh.cpp:61-70), and appends each
// slot to the list of its new state (ballot + popcount + one LDS atomic per wave and list).  Per-ray test order
// (bvh.cpp:47-145) is untouched: hit records are bit-identical to k_trace_w<1>'s (tests/test_gpu_properties.py).
//
// The lists are double-buffered per ROUND, with one workgroup barrier per round: every slot of the block is advanced
// once per round (a wave takes chunks wave, wave + NW, ... of the round's lists).  That is the simplest correct form of
// the hand-over; what it measures does not depend on it — the issue slots per lane-step of phase-pure steps with the
// state in LDS (rocprofv3 SQ_INSTS_VALU / SQ_INSTS_SALU over the lane-steps this kernel counts itself) and the LDS
// bytes per ray that bound its residency.  A short last chunk of the leaf / finished lists is carried over to the next
// round while the block still has inner-node work, so that those phases run in full waves too.
constexpr uint32_t kPoolPhases = 3;  // 0 inner, 1 leaf, 2 finished / empty
__device__ unsigned long long g_pool_stats[16];  // [ph*2] wave-steps, [ph*2+1] lane-steps; [6] rounds; [7] carried slots; [8] blocks
extern "C" int vmx_debug_pool_stats(unsigned long long *out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pool_stats), sizeof(g_pool_stats)) != hipSuccess) return -1;
    if (reset) {
        static unsigned long long zero[16];
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_pool_stats), zero, sizeof(zero)) != hipSuccess) return -1;
    }
    return 0;
}

__global__ void __launch_bounds__(256, 3)
k_trace_pool(SceneDev sc, WorkDev wk, PathArrays pa) {
    extern __shared__ float4 pool_lds[];
    __shared__ uint32_t s_cnt[3][4];  // three rotating sets of list lengths: read (round r), appended (r + 1), cleared (r + 2)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const uint32_t P = wk.pool_slots;
    const int L = (int)wk.lds_entries;
    float4 *sA = pool_lds, *sB = sA + P, *sC = sB + P;
    uint2 *sD = (uint2 *)(sC + P);
    uint2 *stk = sD + P;                                        // [L][P]
    uint32_t *lists = (uint32_t *)(stk + (size_t)L * P);        // [3 sets][3 phases][P]
    uint2 *ovf = (uint2 *)wk.overflow_stack + (size_t)blockIdx.x * P * wk.overflow_entries;  // [slot][level - L]
    const char *rec_base = (const char *)sc.inner;
    float2 *__restrict__ hit_out = (float2 *)pa.hit;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    const uint32_t nsrc = wk.nsrc, root_ref = sc.root_ref;
    uint32_t src = blockIdx.x % nsrc, tried = 0;
    bool exhausted = false;
    unsigned long long st_steps[3] = {0, 0, 0}, st_lanes[3] = {0, 0, 0}, st_carried = 0, st_rounds = 0, st_started = 0, st_written = 0, st_invalid = 0;

    // every slot starts empty, in the finished list of set 0
    for (uint32_t s = threadIdx.x; s < P; s += blockDim.x) {
        sD[s] = make_uint2(kNone, 0u);
        lists[(0 * kPoolPhases + 2) * P + s] = s;
    }
    if (threadIdx.x < 12) s_cnt[threadIdx.x >> 2][threadIdx.x & 3u] = 0;
    __syncthreads();
    if (threadIdx.x == 0) s_cnt[0][2] = P;
    __syncthreads();

    auto append = [&](uint32_t set, uint32_t ph, bool yes, uint32_t slot) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(yes);
        if (m == 0) return;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&s_cnt[set][ph], (uint32_t)__popcll(m));
        base = __builtin_amdgcn_readfirstlane(base);
        if (yes) lists[(set * kPoolPhases + ph) * P + base + (uint32_t)__popcll(m & lt_mask)] = slot;
    };
    // pop until an entry passes `near > t` (bvh.cpp:69); an empty stack ends the ray.  Returns the new node reference,
    // kNone when the ray is done
    auto pop = [&](uint32_t slot, int &sp, float best) -> uint32_t {
        uint32_t ref = kNone;
        while (sp > 0) {
            --sp;
            const uint2 e = sp < L ? stk[(size_t)sp * P + slot] : ovf[(size_t)slot * wk.overflow_entries + (sp - L)];
            if (!(__uint_as_float(e.y) > best)) {
                ref = e.x;
                break;
            }
        }
        return ref;
    };

    for (uint32_t round = 0;; ++round) {
        const uint32_t rd = round % 3u, wr = (round + 1u) % 3u, cl = (round + 2u) % 3u;
        const uint32_t n0 = s_cnt[rd][0], n1 = s_cnt[rd][1], n2 = s_cnt[rd][2];
        if (n0 + n1 + n2 == 0) break;  // (read after the barrier: the same in every wave)
        if (threadIdx.x < 4) s_cnt[cl][threadIdx.x] = 0;
        ++st_rounds;
        const uint32_t c0 = (n0 + 63u) >> 6, c1 = (n1 + 63u) >> 6, c2 = (n2 + 63u) >> 6;
        for (uint32_t c = wave; c < c0 + c1 + c2; c += nw) {
            const uint32_t ph = c < c0 ? 0u : (c < c0 + c1 ? 1u : 2u);
            const uint32_t ci = ph == 0 ? c : (ph == 1 ? c - c0 : c - c0 - c1);
            const uint32_t n = ph == 0 ? n0 : (ph == 1 ? n1 : n2);
            const uint32_t at = ci * 64u + lane;
            const bool have = at < n;
            const uint32_t slot = have ? lists[(rd * kPoolPhases + ph) * P + at] : 0u;
            const uint32_t filled = min(64u, n - ci * 64u);
            // a short last chunk of the leaf / finished list waits for company while the block has inner-node work
            // (finished slots: only while new rays are left to take — else they would circulate for nothing)
            if (ph != 0 && filled < 48u && n0 != 0 && (ph == 1 || !exhausted)) {
                append(wr, ph, have, slot);
                st_carried += filled;
                continue;
            }
            st_steps[ph] += 1, st_lanes[ph] += filled;
            if (ph == 0) {
                // ---- inner node: both child boxes (bbox.cpp:70-83), nearer child first (bvh.cpp:103-132)
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
                uint2 d = make_uint2(0u, 0u);
                if (have) a = sA[slot], b = sB[slot], d = sD[slot];
                const uint32_t cur = __float_as_uint(b.w);
                float4 q0, q1, q2, q3;
                quad_fetch_record(rec_base, have ? (cur << 6) : 0u, lane, q0, q1, q2, q3);
                if (have) {
                    const float ox = a.x, oy = a.y, oz = a.z, best = a.w, ix = b.x, iy = b.y, iz = b.z;
                    int sp = (int)d.y;
                    float tn0, tf0, tn1, tf1;
                    if (!(finite3(ix, iy, iz) && finite3(ox, oy, oz))) child_boxes<true>(q0, q1, q2, ox, oy, oz, ix, iy, iz, tn0, tf0, tn1, tf1);
                    else child_boxes<false>(q0, q1, q2, ox, oy, oz, ix, iy, iz, tn0, tf0, tn1, tf1);
                    uint32_t nxt = choose_child(tn0, tf0, tn1, tf1, __float_as_uint(q3.x), __float_as_uint(q3.y), best, [&](uint2 e) {
                        if (sp < L) stk[(size_t)sp * P + slot] = e;
                        else ovf[(size_t)slot * wk.overflow_entries + (sp - L)] = e;
                        ++sp;
                    });
                    if (nxt == kPop) nxt = pop(slot, sp, best);
                    ((float *)&sB[slot])[3] = __uint_as_float(nxt);
                    ((uint32_t *)&sD[slot])[1] = (uint32_t)sp;
                    const bool done = nxt == kNone;
                    const bool leaf = !done && (int)nxt < 0;
                    append(wr, 0, !done && !leaf, slot);
                    append(wr, 1, leaf, slot);
                    append(wr, 2, done, slot);
                } else {
                    append(wr, 0, false, 0), append(wr, 1, false, 0), append(wr, 2, false, 0);
                }
            } else if (ph == 1) {
                // ---- one triangle of the leaf (triangle.cpp:4-54); the reference itself carries the progress
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f), cc = a;
                uint32_t cur = 0;
                uint2 d = make_uint2(0u, 0u);
                if (have) a = sA[slot], cc = sC[slot], cur = __float_as_uint(((const float *)&sB[slot])[3]), d = sD[slot];
                float4 q0, q1, q2, q3;
                quad_fetch_record(rec_base, have ? sc.tri_off + (cur & kLeafStartMask) * 48u : 0u, lane, q0, q1, q2, q3);
                if (have) {
                    const float ox = a.x, oy = a.y, oz = a.z, dx = cc.x, dy = cc.y, dz = cc.z;
                    float best = a.w;
                    int sp = (int)d.y;
                    float dist;
                    const bool hit = tri_test(q0, q1, q2.x, ox, oy, oz, dx, dy, dz, dist);
                    if (hit && dist < best) {  // strict <: first tested wins ties (bvh.cpp:90)
                        best = dist;
                        ((float *)&sA[slot])[3] = best;
                        ((float *)&sC[slot])[3] = __int_as_float((int)(cur & kLeafStartMask));
                    }
                    uint32_t nxt = leaf_advance(cur);
                    if (nxt == kPop) nxt = pop(slot, sp, best);
                    ((float *)&sB[slot])[3] = __uint_as_float(nxt);
                    ((uint32_t *)&sD[slot])[1] = (uint32_t)sp;
                    const bool done = nxt == kNone;
                    const bool leaf = !done && (int)nxt < 0;
                    append(wr, 0, !done && !leaf, slot);
                    append(wr, 1, leaf, slot);
                    append(wr, 2, done, slot);
                } else {
                    append(wr, 0, false, 0), append(wr, 1, false, 0), append(wr, 2, false, 0);
                }
            } else {
                // ---- finished (or still empty) slots: write the hit record, take the next ray of the generation
                if (have) {
                    const uint32_t old = sD[slot].x;
                    if (old != kNone) hit_out[old] = make_float2(sA[slot].w, sC[slot].w);
                    st_written += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(old != kNone));
                }
                // (a wave reserves exactly the ids its chunk's slots take: slots move between waves here, so a larger
                // reservation kept by the wave — k_trace_w's 256 — could be left unconsumed when the block runs dry)
                bool got = false;
                uint32_t pid = kNone;
                while (!exhausted) {
                    const unsigned long long want = __builtin_amdgcn_ballot_w64(have && !got);
                    if (want == 0) break;
                    const uint32_t nwant = (uint32_t)__popcll(want);
                    const uint32_t lim = min(wk.qids.counts[src * 32], wk.qids.sub_capacity);
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&wk.heads[src * 32], nwant);
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (base >= lim) {
                        src = (src + 1 == nsrc) ? 0 : src + 1;
                        if (++tried == nsrc) exhausted = true;
                        continue;
                    }
                    tried = 0;
                    const uint32_t avail = lim - base;
                    const uint32_t rank = (uint32_t)__popcll(want & lt_mask);
                    if (have && !got && rank < avail) {
                        got = true;
                        pid = wk.qids.ids[(size_t)src * wk.qids.sub_capacity + base + rank];
                    }
                }
                bool started = false;
                if (got) {
                    const float4 a = ((const float4 *)pa.state)[(size_t)pid * 4], b = ((const float4 *)pa.state)[(size_t)pid * 4 + 1];
                    if (__float_as_uint(b.z) != 0xFFFFFFFFu) {
                        const float ox = a.x, oy = a.y, oz = a.z, dx = a.w, dy = b.x, dz = b.y;
                        sA[slot] = make_float4(ox, oy, oz, 999999999.f);                                      // bvh.cpp:48
                        sB[slot] = make_float4(1.0f / dx, 1.0f / dy, 1.0f / dz, __uint_as_float(root_ref));  // Ray.h:10
                        sC[slot] = make_float4(dx, dy, dz, __int_as_float(-1));
                        sD[slot] = make_uint2(pid, 0u);
                        started = true;
                    }
                }
                st_started += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(started));
                st_invalid += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(got && !started));
                if (have && !started) sD[slot] = make_uint2(kNone, 0u);
                // (root_ref of a scene that is one leaf has bit 31: the ray starts in the leaf list)
                append(wr, (int)root_ref < 0 ? 1u : 0u, started, slot);
                // a slot that got no ray stays in the finished list while rays may still come (another sub-queue)
                append(wr, 2, have && !started && !exhausted, slot);
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        for (int p = 0; p < 3; ++p) {
            atomicAdd(&g_pool_stats[p * 2], st_steps[p]);
            atomicAdd(&g_pool_stats[p * 2 + 1], st_lanes[p]);
        }
        atomicAdd(&g_pool_stats[7], st_carried);
        atomicAdd(&g_pool_stats[9], st_started), atomicAdd(&g_pool_stats[10], st_written), atomicAdd(&g_pool_stats[11], st_invalid);
        if (wave == 0) atomicAdd(&g_pool_stats[6], st_rounds), atomicAdd(&g_pool_stats[8], 1ull);
    }
}

// LDS bytes of a block of k_trace_pool with P slots and L stack levels
static size_t pool_lds_bytes(uint32_t P, uint32_t L) { return (size_t)P * (48 + 8 + 8 * (size_t)L) + (size_t)3 * kPoolPhases * P * 4; }

int launch_trace_pool(const SceneDev &sc, const WorkDev &wk, PathArrays pa, LaunchCfg cfg, void *stream) {
    hipLaunchKernelGGL(k_trace_pool, dim3(cfg.grid), dim3(cfg.block), cfg.lds_bytes, (hipStream_t)stream, sc, wk, pa);
    return launch_status();
}
int query_trace_pool(uint32_t block, uint32_t P, uint32_t L, uint32_t *lds_bytes, int *blocks) {
    const size_t lds = pool_lds_bytes(P, L);
    if (lds_bytes) *lds_bytes = (uint32_t)lds;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)k_trace_pool, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    int a = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_trace_pool, (int)block, lds);
    if (blocks) *blocks = a;
    return (int)e;
}
