// vmx_query.inc — k_query: device ray queries of explicit ray batches (vmx_query_device / vmx_query).
// Included by vmx_kernels.hip (inside its namespace): its step is made of that file's traversal primitives — tri_test,
// leaf_advance, child_boxes, choose_child, pop_to_next, ray_start — with quad_fetch_record and the stack_push / stack_pop
// stack, the same functions the bounce traversal k_trace_w<1> calls.
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
// Internal modes of vmx_raycast_device / vmx_raycast_camera_device (no ABI name): NEAREST with L = 999999999.f — the
// (best, slot) of bvh_nearest — over the rays of q.o / q.d (CAST_RAYS) or over sample q.sample's camera ray of pixel
// `item` (CAST_CAMERA: primary_ray, origin = the camera).  A finished ray's (best, slot) goes into the caller's own
// vmx_rayhit record (tri_t, pad words), which k_raycast_finish then completes: no scratch that grows with n.
// (kQueryCastRays = 3, kQueryCastCamera = 4: vmx_kernels.h)

// what the cast modes add to k_query's arguments: the camera (kQueryCastCamera) and the caller's vmx_rayhit records
struct QueryCast {
    FrameDev fr;
    float *rec;  // [n * 16] words
};
__device__ __forceinline__ const QueryCast &query_cast(const QueryCast &c) { return c; }

// QUAD: record fetch of k_trace_w<1> (quad-cooperative + DPP transpose, the default); else per-lane 64-B loads as in
// bvh_nearest (VMX_QUERY_FETCH_PER_LANE).  Cast: one QueryCast for the cast modes, nothing for the others (whose
// kernels keep the two-argument form)
template <uint32_t MODE, bool QUAD, typename... Cast>
__global__ void __launch_bounds__(256, VMX_TRACE_WAVES_PER_SIMD)
k_query(SceneDev sc, QueryDev q, Cast... cast) {
    constexpr bool CAST = MODE >= kQueryCastRays;
    static_assert(CAST == (sizeof...(Cast) == 1), "the cast modes and only they take a QueryCast");
    extern __shared__ uint2 lds_stack[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int lds_entries = (int)q.lds_entries;
    uint2 *stk = lds_stack + (size_t)wave * (lds_entries + 1) * 64 + lane;
    uint2 *ovf = (uint2 *)q.overflow_stack + ((size_t)(blockIdx.x * (blockDim.x >> 6) + wave) * q.overflow_entries) * 64 + lane;
    const char *rec_base = (const char *)sc.inner;
    const float4 *__restrict__ tris = (const float4 *)sc.tris;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
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
        if constexpr (CAST) {  // vmx_rayhit words 10 (tri_t) and 15 (pad): k_raycast_finish reads them back
            float *rec = query_cast(cast...).rec;
            rec[(size_t)i * 16 + 10] = t;
            rec[(size_t)i * 16 + 15] = __int_as_float(s);
            return;
        }
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
                float tn0, tf0, tn1, tf1;
                child_boxes<EXACT>(q0, q1, q2, ox, oy, oz, ix, iy, iz, tn0, tf0, tn1, tf1);
                cur = choose_child(tn0, tf0, tn1, tf1, __float_as_uint(q3.x), __float_as_uint(q3.y), best, [&](uint2 e) {
                    stack_push(stk, ovf, lds_entries, sp, e);
                    ++sp;
                });
            } else {
                // ---- one triangle of the leaf (triangle.cpp:4-54)
                float dist;
                const bool hit = tri_test(q0, q1, q2.x, ox, oy, oz, dx, dy, dz, dist);
                const uint32_t at = cur;
                if (hit && dist < best) {  // strict <: first tested wins ties (bvh.cpp:90)
                    slot = (int)(cur & kLeafStartMask);
                    if (MODE == kQueryAny) {
                        cur = kBottom;  // any hit below the bound is good enough (bvh.cpp:83-86); `best` stays L
                    } else {
                        best = dist;
                    }
                }
                if (MODE != kQueryAny || cur != kBottom) cur = leaf_advance(at);
            }
        }
        if (cur == kPop) cur = pop_to_next(stk, ovf, lds_entries, sp, best);
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
                    if constexpr (MODE == kQueryCastCamera) {  // the ray k_raygen / k_primary_ids form for (pixel, sample)
                        const FrameDev &fr = query_cast(cast...).fr;
                        Rng rng;
                        ox = fr.px, oy = fr.py, oz = fr.pz;
                        primary_ray(fr, item, q.sample, rng, dx, dy, dz);
                    } else {
                        const size_t i3 = (size_t)item * 3;
                        ox = q.o[i3], oy = q.o[i3 + 1], oz = q.o[i3 + 2];
                        dx = q.d[i3], dy = q.d[i3 + 1], dz = q.d[i3 + 2];
                    }
                    float lim = 999999999.f;  // bvh.cpp:48
                    bool valid = true;
                    if (!CAST && q.tmax) {
                        const float tm = q.tmax[item];
                        valid = tm > 0.0f;  // !(tmax > 0), NaN included: a miss, not traversed
                        lim = valid ? fminf(tm, 999999999.f) : tm;
                    }
                    if (valid) {
                        ray = item;
                        ray_start(dx, dy, dz, root_ref, lim, ix, iy, iz, best, slot, sp, cur);
                        exact = !(finite3(ix, iy, iz) && finite3(ox, oy, oz));
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

// MeshEngine::RayCast after the BVH query (meshEngine.cpp:365-508) for the (best, slot) k_query<3 / 4> left in each
// record: one lane per ray, dense, grid-stride.  The sphere table is staged in LDS as k_shade does; SRC 1 (camera
// rays: the ray is formed again by primary_ray, origin = the camera) also stages (centre - camera, |op|^2), which is
// what sphere_hit computes from the same floats for that origin (k_shade<0>).  Writes the whole 64-byte vmx_rayhit in
// k_raycast's order: location, distance | normal, tri_id | uv, tri_t, flags | colour, pad = 0.
template <int SRC>
__global__ void __launch_bounds__(256)
k_raycast_finish(SceneDev sc, FrameDev fr, const float *__restrict__ o, const float *__restrict__ d, uint32_t n,
                 uint32_t k, float4 *out) {
    __shared__ float4 s_geom[kLdsSpheres];
    __shared__ float4 s_cam_op[kLdsSpheres];
    if (threadIdx.x < min(sc.nspheres, kLdsSpheres)) {
        const SphereDev &q = sc.spheres[threadIdx.x];
        s_geom[threadIdx.x] = make_float4(q.cx, q.cy, q.cz, q.rad2);
        if (SRC == 1) {
            const float opx = q.cx - fr.px, opy = q.cy - fr.py, opz = q.cz - fr.pz;
            s_cam_op[threadIdx.x] = make_float4(opx, opy, opz, dot3(opx, opy, opz, opx, opy, opz));
        }
    }
    __syncthreads();
    const float4 *__restrict__ tris = (const float4 *)sc.tris;
    const float *rec = (const float *)out;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float ox, oy, oz, dx, dy, dz;
        if (SRC == 1) {
            Rng rng;
            ox = fr.px, oy = fr.py, oz = fr.pz;
            primary_ray(fr, i, k, rng, dx, dy, dz);
        } else {
            const size_t i3 = (size_t)i * 3;
            ox = o[i3], oy = o[i3 + 1], oz = o[i3 + 2];
            dx = d[i3], dy = d[i3 + 1], dz = d[i3 + 2];
        }
        const float best = rec[(size_t)i * 16 + 10];
        const int slot = __float_as_int(rec[(size_t)i * 16 + 15]);
        CastResult c;
        cast_finish<true, SRC == 1>(sc, ox, oy, oz, dx, dy, dz, best, slot, c, s_geom, s_cam_op);
        const int32_t id = c.slot >= 0 ? (int32_t)__float_as_uint(tris[c.slot * 3 + 2].y) : -1;
        const uint32_t flags = ((c.nearest < kInf) ? 1u : 0u) | (c.material ? 2u : 0u);
        out[(size_t)i * 4] = make_float4(ox + (dx * c.nearest), oy + (dy * c.nearest), oz + (dz * c.nearest), c.nearest);
        out[(size_t)i * 4 + 1] = make_float4(c.nx, c.ny, c.nz, __int_as_float(id));
        out[(size_t)i * 4 + 2] = make_float4(c.uvx, c.uvy, c.tri_t, __uint_as_float(flags));
        out[(size_t)i * 4 + 3] = make_float4(c.cr, c.cg, c.cb, 0.f);
    }
}

// The instantiation of a (mode, fetch form): launch_query / launch_raycast_query launch it and
// query_query_blocks_per_cu reports its occupancy, so the grid is sized from the kernel that runs.
using QueryKernel = void (*)(SceneDev, QueryDev);
using QueryCastKernel = void (*)(SceneDev, QueryDev, QueryCast);
static QueryKernel query_kernel(uint32_t mode, bool quad) {
    if (mode == kQueryAny) {
        if (quad) return k_query<kQueryAny, true>;
        return k_query<kQueryAny, false>;
    }
    if (mode == kQueryCollision) {
        if (quad) return k_query<kQueryCollision, true>;
        return k_query<kQueryCollision, false>;
    }
    if (quad) return k_query<kQueryNearest, true>;
    return k_query<kQueryNearest, false>;
}
static QueryCastKernel query_cast_kernel(bool camera, bool quad) {
    if (camera) {
        if (quad) return k_query<kQueryCastCamera, true, QueryCast>;
        return k_query<kQueryCastCamera, false, QueryCast>;
    }
    if (quad) return k_query<kQueryCastRays, true, QueryCast>;
    return k_query<kQueryCastRays, false, QueryCast>;
}

int launch_query(const SceneDev &sc, const QueryDev &q, uint32_t mode, bool quad, LaunchCfg cfg, void *stream) {
    hipLaunchKernelGGL(query_kernel(mode, quad), dim3(cfg.grid), dim3(cfg.block), cfg.lds_bytes, (hipStream_t)stream, sc, q);
    return launch_status();
}

int query_query_blocks_per_cu(uint32_t block, uint32_t lds_bytes, uint32_t mode, bool quad, int *blocks) {
    int a = 0;
    const bool cast = mode == kQueryCastRays || mode == kQueryCastCamera;
    const hipError_t e = cast ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, query_cast_kernel(mode == kQueryCastCamera, quad), (int)block, lds_bytes)
                              : hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, query_kernel(mode, quad), (int)block, lds_bytes);
    if (blocks) *blocks = a;
    return (int)e;
}

int launch_raycast_query(const SceneDev &sc, const QueryDev &q, const FrameDev &fr, bool camera, bool quad, void *out,
                         LaunchCfg cfg, uint32_t finish_grid, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const QueryCast c = {fr, (float *)out};
    hipLaunchKernelGGL(query_cast_kernel(camera, quad), dim3(cfg.grid), dim3(cfg.block), cfg.lds_bytes, s, sc, q, c);
    if (int e = launch_status()) return e;
    if (camera)
        hipLaunchKernelGGL(k_raycast_finish<1>, dim3(finish_grid), dim3(256), 0, s, sc, fr, nullptr, nullptr, q.n,
                           q.sample, (float4 *)out);
    else
        hipLaunchKernelGGL(k_raycast_finish<0>, dim3(finish_grid), dim3(256), 0, s, sc, fr, q.o, q.d, q.n, 0u,
                           (float4 *)out);
    return launch_status();
}
