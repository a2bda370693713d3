// vmx_query.inc — k_query: device ray queries of explicit ray batches (vmx_query_device / vmx_query).
// Included by vmx_kernels.hip (inside its namespace) so that it uses box_net / box_net_exact, stack_push / stack_pop,
// quad_fetch_record and SceneDev exactly as the bounce traversal k_trace_w<1> does.
//
// Three modes, one traversal (BVH::getIntersection, bvh.cpp:47-145):
//   NEAREST   (occlusion == false)  `best` starts at L = min(tmax, 999999999.f) instead of 999999999.f (bvh.cpp:48)
//   ANY       (occlusion == true, bvh.cpp:83-86)  the first triangle accepted with dist < L ends the ray
//   COLLISION (MeshEngine::RayCastCollision, meshEngine.cpp:196-206)  NEAREST, then hit = t > 1e-3 (double) = t >= 1e-3f
//
// Why NEAREST with a bound is the reference's answer cut at L: the traversal below is the reference's step for step
// (same box tests, same near-first order, same strict `<` on triangle distances, same `near > best` pruning), only
// `best` starts lower.  Let (id_ref, t_ref) be the unbounded result.  If every box on the path to the winning triangle
// is entered at near <= L, none of them is pruned by the lower start, the nodes are visited in the same order, and
// every triangle the bounded run accepts is one the unbounded run accepts at the same point of the same order — so
// ties resolve identically and the result is (id_ref, t_ref) when t_ref < L.  If t_ref >= L, no triangle has dist < L
// among those the unbounded run tests (it would have taken it), nor among the others (they lie in boxes it pruned at
// near > best >= t_ref >= L, which the bounded run prunes too): a miss with t = L.  The premise is exact arithmetic's
// near <= t_ref; in float a box's slab near can lie a few ulps above the Moeller-Trumbore t of a triangle on its face,
// so for L within those ulps above t_ref the bounded query may report a miss (at L = nextafter(t_ref): 0.3 % of random
// rays on cornell8, 1.2 % on sponza260k; tests/test_gpu_query.py: check_window).  A bound 0.1 % above t_ref is exact.
//
// Schedule: persistent waves that reserve chunks of ray indices with one atomic on a device counter (WorkDev::reserve:
// 256 / 128 / 64 by the launch's items per lane) and refill idle lanes from the reservation as soon as refill_min of
// them are idle — any-hit lanes finish early, and a wave no longer waits on its longest ray as in k_trace.  The stack
// is k_trace_w's: lane-strided LDS levels [0, lds_entries) with the bottom entry (near = -inf) at level 0, deeper
// levels in the per-wave HBM slab.
constexpr uint32_t kQueryNearest = 0, kQueryAny = 1, kQueryCollision = 2;  // VMX_QUERY_* of vermilion_hip.h

// QUAD: record fetch of k_trace_w<1> (quad-cooperative + DPP transpose, the default); else per-lane 64-B loads as in
// bvh_nearest (VMX_QUERY_FETCH_PER_LANE)
template <uint32_t MODE, bool QUAD>
__global__ void __launch_bounds__(256, VMX_TRACE_WAVES_PER_SIMD)
k_query(SceneDev sc, QueryDev q) {
    extern __shared__ uint2 lds_stack[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int lds_entries = (int)q.lds_entries;
    uint2 *stk = lds_stack + (size_t)wave * (lds_entries + 1) * 64 + lane;
    uint2 *ovf = (uint2 *)q.overflow_stack + ((size_t)(blockIdx.x * (blockDim.x >> 6) + wave) * q.overflow_entries) * 64 + lane;
    const char *rec_base = (const char *)sc.inner;
    const float4 *__restrict__ tris = (const float4 *)sc.tris;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    constexpr uint32_t kIdle = 0x7FFFFFFFu, kBottom = 0x7FFFFFFEu, kPop = 0x7FFFFFFDu;  // never valid inner indices
    const uint32_t n = q.n, kReserve = q.reserve, refill_min = q.refill_min, root_ref = sc.root_ref;

    uint32_t res_lo = 0, res_hi = 0;
    bool exhausted = false;
    bool exact = false;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
    float ix = 0.f, iy = 0.f, iz = 0.f, best = 0.f;
    int slot = -1, sp = 0;
    uint32_t cur = kIdle, ray = 0;
    stk[0] = make_uint2(kBottom, 0xFF800000u);  // bottom entry; pushes start at level 1, so it stays

    // results of ray `i` (t = best: L on a miss)
    auto write_out = [&](uint32_t i, int s, float t) {
        if (MODE != kQueryAny) {
            if (q.tri_id) q.tri_id[i] = s >= 0 ? (int32_t)__float_as_uint(tris[(uint32_t)s * 3 + 2].y) : -1;
            if (q.t) q.t[i] = t;
        }
        if (q.hit) {
            // COLLISION: `ii.t > 1e-3` compares the float t with the double 1e-3 (meshEngine.cpp:202); in float that
            // is t >= 1e-3f, as 1e-3f = 0.0010000000474974513 lies above the double and the float below it does not
            const bool h = MODE == kQueryCollision ? (s >= 0 && t >= 1e-3f) : s >= 0;
            q.hit[i] = h ? 1 : 0;
        }
    };

    auto step = [&](auto exact_tag) {
        constexpr bool EXACT = decltype(exact_tag)::value;  // NaN-exact box form (bbox.cpp:70-83 compare-select)
        const bool leaf = (int)cur < 0;
        float4 q0, q1, q2, q3;
        // one fetch phase for inner-node lanes and leaf lanes: a 32-bit byte offset into the one record allocation
        // (SceneDev::tri_off), 64 bytes from it (the allocation is padded for a triangle record's 48)
        const uint32_t off = cur == kIdle ? 0u : (leaf ? sc.tri_off + (cur & kLeafStartMask) * 48u : (cur << 6));
        if (QUAD) {
            quad_fetch_record(rec_base, off, lane, q0, q1, q2, q3);
        } else {
            const float4 *rec = (const float4 *)(rec_base + off);
            q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
        }
        if (cur != kIdle) {
            if (!leaf) {
                // ---- inner node: both child boxes (bbox.cpp:70-83), nearer child first (bvh.cpp:103-132)
                const float a0 = (q0.x - ox) * ix, a1 = (q0.y - oy) * iy, a2 = (q0.z - oz) * iz;
                const float a3 = (q0.w - ox) * ix, a4 = (q1.x - oy) * iy, a5 = (q1.y - oz) * iz;
                const float b0 = (q1.z - ox) * ix, b1 = (q1.w - oy) * iy, b2 = (q2.x - oz) * iz;
                const float b3 = (q2.y - ox) * ix, b4 = (q2.z - oy) * iy, b5 = (q2.w - oz) * iz;
                float tn0, tf0, tn1, tf1;
                if (EXACT) {
                    box_net_exact(a0, a1, a2, a3, a4, a5, tn0, tf0);
                    box_net_exact(b0, b1, b2, b3, b4, b5, tn1, tf1);
                } else {
                    box_net(a0, a1, a2, a3, a4, a5, tn0, tf0);
                    box_net(b0, b1, b2, b3, b4, b5, tn1, tf1);
                }
                const uint32_t lref = __float_as_uint(q3.x), rref = __float_as_uint(q3.y);
                const bool h0 = tn0 <= tf0, h1 = tn1 <= tf1;
                const bool both = h0 && h1;
                const bool go_right = h1 && (!h0 || tn1 < tn0);  // both: the strictly closer right child; one: that child
                if (both) {
                    const uint2 e = make_uint2(go_right ? lref : rref, __float_as_uint(go_right ? tn0 : tn1));
                    stack_push(stk, ovf, lds_entries, sp, e);  // farther first (bvh.cpp:120)
                    ++sp;
                }
                const float near = go_right ? tn1 : tn0;
                // no child hit, or the child taken directly fails `near > t` (bvh.cpp:69): pop
                cur = (!(h0 || h1) || near > best) ? kPop : (go_right ? rref : lref);
            } else {
                // ---- one triangle of the leaf (triangle.cpp:4-54): q0 = (v0, e1.x) q1 = (e1.yz, e2.xy) q2.x = e2.z
                const float e1x = q0.w, e1y = q1.x, e1z = q1.y, e2x = q1.z, e2y = q1.w, e2z = q2.x;
                float pvx, pvy, pvz;
                cross3(dx, dy, dz, e2x, e2y, e2z, pvx, pvy, pvz);
                const float det = dot3(e1x, e1y, e1z, pvx, pvy, pvz);
                const float inv_det = 1.0f / det;
                const float tx = ox - q0.x, ty = oy - q0.y, tz = oz - q0.z;
                const float u = dot3(tx, ty, tz, pvx, pvy, pvz) * inv_det;
                float qx, qy, qz;
                cross3(tx, ty, tz, e1x, e1y, e1z, qx, qy, qz);
                const float v = dot3(dx, dy, dz, qx, qy, qz) * inv_det;
                const float dist = dot3(e2x, e2y, e2z, qx, qy, qz) * inv_det;
                const bool parallel = fabsf(det) <= 9.99999993922529e-09f;
                const bool u_out = (u < 0.0f) || (u > 1.0f);
                const bool v_out = (v < 0.0f) || (u + v > 1.0f);
                const bool hit = !parallel && !u_out && !v_out && (dist > 0.0f);
                const bool last = ((cur >> kLeafCountShift) & 31u) == 1u;
                if (hit && dist < best) {  // strict <: first tested wins ties (bvh.cpp:90)
                    slot = (int)(cur & kLeafStartMask);
                    if (MODE == kQueryAny) {
                        cur = kBottom;  // any hit below the bound is good enough (bvh.cpp:83-86); `best` stays L
                    } else {
                        best = dist;
                    }
                }
                // next triangle: start + 1, count - 1; after the last one the lane pops
                if (MODE != kQueryAny || cur != kBottom) cur = last ? kPop : cur + (1u - (1u << kLeafCountShift));
            }
        }
        if (cur == kPop) {
            // pop until an entry passes `near > t` (bvh.cpp:69); level 0 holds the bottom entry
            // (near = -inf), which always passes and ends the ray
            uint2 e;
            do {
                --sp;
                e = stack_pop(stk, ovf, lds_entries, sp);
            } while (__uint_as_float(e.y) > best);
            cur = e.x;
        }
        if (cur == kBottom) {
            write_out(ray, slot, best);
            cur = kIdle;
        }
    };

    for (;;) {
        // ---- refill idle lanes (k_trace_w's scheme with one work source: ray indices [0, n)) -----------------
        const unsigned long long idle = __builtin_amdgcn_ballot_w64(cur == kIdle);
        if (idle != 0 && !exhausted && ((uint32_t)__popcll(idle) >= refill_min || idle == ~0ull)) {
            for (;;) {
                if (res_lo == res_hi) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(q.head, kReserve);
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (base >= n) {
                        exhausted = true;
                        break;
                    }
                    res_lo = base;
                    res_hi = min(base + kReserve, n);  // (n <= 2^31 and base < n: no wrap)
                }
                const unsigned long long want = __builtin_amdgcn_ballot_w64(cur == kIdle);
                if (want == 0) break;
                const uint32_t avail = res_hi - res_lo;
                const uint32_t rank = (uint32_t)__popcll(want & lt_mask);
                const bool take = cur == kIdle && rank < avail;
                const uint32_t item = res_lo + rank;
                res_lo = __builtin_amdgcn_readfirstlane(res_lo + min((uint32_t)__popcll(want), avail));
                if (take) {
                    const size_t i3 = (size_t)item * 3;
                    ox = q.o[i3], oy = q.o[i3 + 1], oz = q.o[i3 + 2];
                    dx = q.d[i3], dy = q.d[i3 + 1], dz = q.d[i3 + 2];
                    float lim = 999999999.f;  // bvh.cpp:48
                    bool valid = true;
                    if (q.tmax) {
                        const float tm = q.tmax[item];
                        valid = tm > 0.0f;  // !(tmax > 0), NaN included: a miss, not traversed
                        lim = valid ? fminf(tm, 999999999.f) : tm;
                    }
                    if (valid) {
                        ray = item;
                        ix = 1.0f / dx, iy = 1.0f / dy, iz = 1.0f / dz;  // Ray.h:10
                        exact = !(finite3(ix, iy, iz) && finite3(ox, oy, oz));
                        best = lim;
                        slot = -1;
                        sp = 1;
                        cur = root_ref;  // its near value, -9999999 (bvh.cpp:59), passes `near > t` for any L > 0
                    } else {
                        write_out(item, -1, lim);  // the lane stays idle and takes the next item
                    }
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(cur != kIdle) == 0) break;
        if (__builtin_amdgcn_ballot_w64(exact && cur != kIdle) != 0) {
#pragma unroll 1
            for (int act = 0; act < 8; ++act) step(std::true_type{});
        } else {
#pragma unroll 1
            for (int act = 0; act < 8; ++act) step(std::false_type{});
        }
    }
}

int launch_query(const SceneDev &sc, const QueryDev &q, uint32_t mode, bool quad, LaunchCfg cfg, void *stream) {
    const dim3 g(cfg.grid), b(cfg.block);
    hipStream_t s = (hipStream_t)stream;
#define VMX_Q(M)                                                                                   \
    if (quad) hipLaunchKernelGGL((k_query<M, true>), g, b, cfg.lds_bytes, s, sc, q);              \
    else hipLaunchKernelGGL((k_query<M, false>), g, b, cfg.lds_bytes, s, sc, q);
    if (mode == kQueryAny) {
        VMX_Q(kQueryAny)
    } else if (mode == kQueryCollision) {
        VMX_Q(kQueryCollision)
    } else {
        VMX_Q(kQueryNearest)
    }
#undef VMX_Q
    return launch_status();
}

// occupancy of the exact instantiation launch_query selects
int query_query_blocks_per_cu(uint32_t block, uint32_t lds_bytes, uint32_t mode, bool quad, int *blocks) {
    int a = 0;
    hipError_t e;
#define VMX_OCC(K) hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, K, (int)block, lds_bytes)
    if (mode == kQueryAny) e = quad ? VMX_OCC((k_query<kQueryAny, true>)) : VMX_OCC((k_query<kQueryAny, false>));
    else if (mode == kQueryCollision) e = quad ? VMX_OCC((k_query<kQueryCollision, true>)) : VMX_OCC((k_query<kQueryCollision, false>));
    else e = quad ? VMX_OCC((k_query<kQueryNearest, true>)) : VMX_OCC((k_query<kQueryNearest, false>));
#undef VMX_OCC
    if (blocks) *blocks = a;
    return (int)e;
}
