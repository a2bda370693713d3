// vmx_nee.inc — part of vmx_kernels.hip: the light-sampling integrator (vmx_render_nee*, vmx_radiance_nee).
//
// Radiance (pathtracer.cpp:21-198) under r2 = U with next-event estimation: after every diffuse step one direction per
// VMX_SPHERE_EMIT sphere is drawn uniformly inside the cone the sphere subtends from the new origin, a full RayCast goes
// along it and its hitColour is added with the weight cos / pi * solid angle; the step that follows then does not add
// the emission it hits (`lit`), so every light path is counted once.  The arithmetic is stated in include/vermilion_hip.h
// and restated in tests/nee_spec.py, which the kernel matches bit for bit; DESIGN.md "Light sampling" has the argument.
//
// One persistent kernel, a path per lane, per-lane refill.  A lane's next ray is either its path's ray or a pending shadow
// ray — both start at P.o, the shadow ray along (sx, sy, sz) — and every iteration traverses whichever is next: one
// bvh_nearest / cast_finish call site for both, per lane as k_bruteforce runs them (LDS stack levels + the global slab).
// What a finished ray means is decided after the cast: a shadow ray adds its colour, a path ray takes Radiance's step; a
// diffuse step then opens the emitter loop (`em` = the next table index to sample), which runs one emitter at a time
// between casts, so the draws stay in the order the definition consumes them.

constexpr uint32_t kNeeNoLoop = 0xFFFFFFFFu;

// emitter i seen from x: axis a = normalize(c - x) and q = 1 - cos(theta_max) in double, from the float32 op, C = op.op
// and rad * rad that sphere_hit forms.  q = s2 / (1 + sqrt(1 - s2)), s2 = r^2 / C: 1 - sqrt(1 - s2) without the
// cancellation (in float32 it loses 0.4 % for a 3.5-unit sphere 500 units away)
__device__ __forceinline__ void nee_cone(float4 g, float ox, float oy, float oz, float &ax, float &ay, float &az, double &q) {
    ax = g.x - ox, ay = g.y - oy, az = g.z - oz;
    const float C = dot3(ax, ay, az, ax, ay, az);
    const double s2 = (double)g.w / (double)C;
    q = s2 / (1.0 + sqrt(1.0 - s2));
    normalize3(ax, ay, az);
}

// SRC 0: camera paths — item = path id = slot * samples + j of the pass's active pixels (pixel-major, as k_paths numbers
//        them for k_resolve); SRC 1: explicit rays o / d — item i on stream (seed, i, 0), jitter draws skipped;
//        SRC 2: a budgeted step's camera paths — slot s of the step's list owns the items [base[s], base[s + 1]) of the
//        exclusive scan wk.flat_ids (n_active + 1 entries, strictly increasing: every listed pixel takes a sample), item
//        i is sample j = i - base[s] of its pixel; a lane finds s by bisection when it takes the item (log2 of the list's
//        length dependent 4-byte loads per path of some 55 rays), and rad[i] is where k_resolve_budget looks for it
// TEX: accumRadiance is carried (a texture is bound); else it stays (1, 1, 1, 1)
template <int SRC, bool TEX>
__global__ void __launch_bounds__(256)
k_nee(SceneDev sc, FrameDev fr, WorkDev wk, PixelStateDev px, const float *__restrict__ ray_o, const float *__restrict__ ray_d,
      uint32_t n_items, float4 *__restrict__ rad, DevCounters *ctr) {
    extern __shared__ uint2 lds_stack[];
    __shared__ float4 s_geom[kLdsSpheres];  // spheres' (centre, rad*rad): read by every RayCast and every cone
    __shared__ uint32_t s_emit;             // bit i: sphere i is an emitter
    if (threadIdx.x < min(sc.nspheres, kLdsSpheres)) {
        const SphereDev &q = sc.spheres[threadIdx.x];
        s_geom[threadIdx.x] = make_float4(q.cx, q.cy, q.cz, q.rad2);
    }
    if (threadIdx.x == 0) {
        uint32_t m = 0;
        for (uint32_t i = 0; i < min(sc.nspheres, kLdsSpheres); ++i) m |= (sc.spheres[i].flags & 1u) << i;
        s_emit = m;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int lds_entries = (int)wk.lds_entries;
    uint2 *stk = lds_stack + (size_t)wave * (wk.lds_entries + 1) * 64 + lane;
    uint2 *ovf = (uint2 *)wk.overflow_stack + ((size_t)(blockIdx.x * (blockDim.x >> 6) + wave) * wk.overflow_entries) * 64 + lane;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const uint32_t emask = s_emit, nsph = min(sc.nspheres, kLdsSpheres);
    const SampCfg cfg = {1.0f, fr.libm_double, 0u};

    uint32_t res_lo = 0, res_hi = 0;  // wave-uniform: the reserved items
    bool exhausted = false;
    bool has = false, shadow = false, lit = false, bounce_ok = false;
    Path P;
    float wx = 0.f, wy = 0.f, wz = 0.f;  // the flipped normal of the diffuse step whose emitter loop is open
    float sx = 0.f, sy = 0.f, sz = 0.f, wt = 0.f;  // the pending shadow ray's direction and weight
    uint32_t em = kNeeNoLoop;
    uint32_t n_prim = 0, n_sec = 0;
    Cnt cnt = {0, 0};

    for (;;) {
        // ---- refill idle lanes -------------------------------------------------------------------------------------
        if (!exhausted && __builtin_amdgcn_ballot_w64(!has) != 0) {
            for (;;) {
                if (res_lo == res_hi) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(wk.heads, wk.reserve);
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (base >= n_items) {
                        exhausted = true;
                        break;
                    }
                    res_lo = base;
                    res_hi = min(base + wk.reserve, n_items);
                }
                const unsigned long long want = __builtin_amdgcn_ballot_w64(!has);
                if (want == 0) break;
                const uint32_t avail = res_hi - res_lo;
                const uint32_t rank = (uint32_t)__popcll(want & lt_mask);
                const bool take = !has && rank < avail;
                const uint32_t item = res_lo + rank;
                res_lo += min((uint32_t)__popcll(want), avail);
                if (take) {
                    bool valid = true;
                    if (SRC == 0) {
                        const uint32_t sl = fast_div(item, wk.div_samples), j = item - sl * wk.samples;
                        valid = sl < wk.n_active;
                        if (valid) {
                            const uint32_t lp = wk.active[sl];
                            const uint32_t k = sample_index(fr, px, lp, j);
                            valid = k < fr.kmax;
                            if (valid) {
                                primary_ray(fr, global_pixel(fr, lp), k, P.rng, P.dx, P.dy, P.dz);
                                P.ox = fr.px, P.oy = fr.py, P.oz = fr.pz;
                            }
                        }
                    } else if (SRC == 2) {
                        const unsigned int *__restrict__ base = wk.flat_ids;
                        uint32_t lo = 0, hi = wk.n_active;  // base[lo] <= item < base[hi]
                        while (hi - lo > 1u) {
                            const uint32_t mid = lo + ((hi - lo) >> 1);
                            if (base[mid] <= item) lo = mid;
                            else hi = mid;
                        }
                        const uint32_t lp = wk.active[lo];
                        const uint32_t k = sample_index(fr, px, lp, item - base[lo]);
                        valid = k < fr.kmax;
                        if (valid) {
                            primary_ray(fr, global_pixel(fr, lp), k, P.rng, P.dx, P.dy, P.dz);
                            P.ox = fr.px, P.oy = fr.py, P.oz = fr.pz;
                        }
                    } else {
                        rng_init(P.rng, fr.seed, item, 0);
                        (void)rng_next(P.rng);
                        (void)rng_next(P.rng);
                        P.ox = ray_o[(size_t)item * 3], P.oy = ray_o[(size_t)item * 3 + 1], P.oz = ray_o[(size_t)item * 3 + 2];
                        P.dx = ray_d[(size_t)item * 3], P.dy = ray_d[(size_t)item * 3 + 1], P.dz = ray_d[(size_t)item * 3 + 2];
                    }
                    if (valid) {
                        P.ar = P.ag = P.ab = 0.f;
                        P.aw = -100.f;                    // pathtracer.cpp:29
                        P.tr = P.tg = P.tb = P.tw = 1.f;  // :30
                        P.depth = 0;
                        P.dest = item;
                        has = true, shadow = false, lit = false, em = kNeeNoLoop;
                        ++n_prim;
                    }
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(has) == 0) break;

        // ---- the lane's next ray: RayCast ----------------------------------------------------------------------------
        const float dx = shadow ? sx : P.dx, dy = shadow ? sy : P.dy, dz = shadow ? sz : P.dz;
        CastResult c;
        if (has) {
            float best;
            int slot;
            bvh_nearest<false>(sc, P.ox, P.oy, P.oz, dx, dy, dz, stk, best, slot, cnt, ovf, lds_entries);
            cast_finish<true, false>(sc, P.ox, P.oy, P.oz, dx, dy, dz, best, slot, c, s_geom);
        }

        // ---- what the finished ray means -------------------------------------------------------------------------------
        if (has) {
            if (shadow) {
                // accumColour.rgb += accumRadiance.rgb * hitColour * weight (a miss leaves hitColour black)
                if (TEX) {
                    P.ar = P.ar + (P.tr * c.cr) * wt;
                    P.ag = P.ag + (P.tg * c.cg) * wt;
                    P.ab = P.ab + (P.tb * c.cb) * wt;
                } else {
                    P.ar = P.ar + c.cr * wt;
                    P.ag = P.ag + c.cg * wt;
                    P.ab = P.ab + c.cb * wt;
                }
                shadow = false;
            } else {
                // Radiance's step.  A lit path does not add what it hits: the step's sum is taken back (depth 0 is never lit,
                // so the distance that step stores in the fourth component stays)
                const float kr = P.ar, kg = P.ag, kb = P.ab, kw = P.aw;
                const float idx = P.dx, idy = P.dy, idz = P.dz;
                StepFlags fl = {false, false, false};
                ShadeMid m;
                const int st = path_shade_begin<TEX>(sc, cfg.r2scale, P, c, fl, m);
                if (lit) P.ar = kr, P.ag = kg, P.ab = kb, P.aw = kw;
                if (st == kPathEnded) {
                    rad[P.dest] = make_float4(P.ar, P.ag, P.ab, P.aw);
                    has = false;
                } else if (st == kPathNextRay) {  // the specular arm
                    lit = false;
                    if (finite3(P.dx, P.dy, P.dz)) ++n_sec;
                } else {  // a diffuse arm: the bounce ray goes into P, then the emitter loop opens at the new origin
                    const bool facing = dot3(c.nx, c.ny, c.nz, idx, idy, idz) < 0.f;
                    wx = facing ? c.nx : c.nx * -1.f, wy = facing ? c.ny : c.ny * -1.f, wz = facing ? c.nz : c.nz * -1.f;
                    float cs, sn;
                    shade_trig(m, cfg.libm_double, cs, sn);
                    bounce_ok = path_shade_end(P, c, fl, m, cs, sn);
                    // inside or on an emitter: no light draws, and the next step adds what it hits
                    bool inside = false;
                    for (uint32_t i = 0; i < nsph; ++i) {
                        if (!((emask >> i) & 1u)) continue;
                        const float4 g = s_geom[i];
                        const float opx = g.x - P.ox, opy = g.y - P.oy, opz = g.z - P.oz;
                        if (dot3(opx, opy, opz, opx, opy, opz) <= g.w) inside = true;
                    }
                    lit = !inside;
                    em = inside ? nsph : 0u;
                }
            }
        }
        // ---- the emitter loop, up to its next shadow ray ---------------------------------------------------------------
        if (has && em != kNeeNoLoop) {
            for (; em < nsph && !shadow; ++em) {
                if (!((emask >> em) & 1u)) continue;
                const double xi1 = rng_u01(P.rng), xi2 = rng_u01(P.rng);
                float ax, ay, az;
                double q;
                nee_cone(s_geom[em], P.ox, P.oy, P.oz, ax, ay, az, q);
                const double z = xi1 * q;
                const float ct = (float)(1.0 - z), sth = (float)sqrt(z * (2.0 - z));
                ShadeMid pm;
                pm.angle_f = (float)(6.283185307179586 * xi2);
                pm.angle = (double)pm.angle_f;
                float cs, sn;
                shade_trig(pm, cfg.libm_double, cs, sn);
                const bool use_y = (double)fabsf(ax) > .1;
                float ux, uy, uz, vx, vy, vz;
                cross3(use_y ? 0.f : 1.f, use_y ? 1.f : 0.f, 0.f, ax, ay, az, ux, uy, uz);
                normalize3(ux, uy, uz);
                cross3(ax, ay, az, ux, uy, uz, vx, vy, vz);
                float ox_ = (ux * cs * sth + vx * sn * sth) + ax * ct;
                float oy_ = (uy * cs * sth + vy * sn * sth) + ay * ct;
                float oz_ = (uz * cs * sth + vz * sn * sth) + az * ct;
                normalize3(ox_, oy_, oz_);
                // a direction inside the cone of an earlier emitter belongs to that emitter's sample
                bool keep = true;
                for (uint32_t j = 0; j < em; ++j) {
                    if (!((emask >> j) & 1u)) continue;
                    float bx, by, bz;
                    double qj;
                    nee_cone(s_geom[j], P.ox, P.oy, P.oz, bx, by, bz, qj);
                    const float ex = ox_ - bx, ey = oy_ - by, ez = oz_ - bz;
                    if (0.5 * (double)dot3(ex, ey, ez, ex, ey, ez) <= qj) keep = false;
                }
                const float dw = dot3(wx, wy, wz, ox_, oy_, oz_);
                if (dw <= 0.f) keep = false;
                if (keep) {
                    sx = ox_, sy = oy_, sz = oz_;
                    wt = (float)((double)dw / 3.141592653589793 * (6.283185307179586 * q));
                    shadow = true;
                    ++n_sec;
                }
            }
            if (!shadow) {  // the loop is through: on with the bounce ray
                em = kNeeNoLoop;
                if (!bounce_ok) {
                    rad[P.dest] = make_float4(P.ar, P.ag, P.ab, P.aw);
                    has = false;
                } else if (finite3(P.dx, P.dy, P.dz)) {
                    ++n_sec;
                }
            }
        }
    }
    const uint32_t wp = wave_sum(n_prim), ws = wave_sum(n_sec);
    if (lane == 0) {
        if (wp) atomicAdd(&ctr->stage[0].rays, (unsigned long long)wp);
        if (ws) atomicAdd(&ctr->stage[1].rays, (unsigned long long)ws);
    }
}

// wk: heads (one counter, zeroed), reserve, the stack fields; camera paths (rays == NULL): active, n_active, samples,
// div_samples, `items` = padded slots * samples; explicit rays: o / d, `items` rays; a budgeted step (rays == NULL,
// wk.flat_ids the item bases): active, n_active, `items` = base[n_active]
int launch_nee(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PixelStateDev px, const float *o, const float *d,
               uint32_t items, void *rad, DevCounters *counters, LaunchCfg cfg, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    dim3 g(cfg.grid), b(cfg.block);
#define VMX_GO(S, T) hipLaunchKernelGGL((k_nee<S, T>), g, b, cfg.lds_bytes, s, sc, fr, wk, px, o, d, items, (float4 *)rad, counters)
    if (o) {
        if (sc.tex) VMX_GO(1, true);
        else VMX_GO(1, false);
    } else if (wk.flat_ids) {
        if (sc.tex) VMX_GO(2, true);
        else VMX_GO(2, false);
    } else {
        if (sc.tex) VMX_GO(0, true);
        else VMX_GO(0, false);
    }
#undef VMX_GO
    return launch_status();
}

int query_nee_blocks_per_cu(uint32_t block, uint32_t lds_bytes, bool rays, int *blocks, bool budgeted) {
    int a = 0, b = 0;
    hipError_t e;
    if (budgeted) {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_nee<2, true>, (int)block, lds_bytes);
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_nee<2, false>, (int)block, lds_bytes);
    } else if (rays) {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_nee<1, true>, (int)block, lds_bytes);
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_nee<1, false>, (int)block, lds_bytes);
    } else {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_nee<0, true>, (int)block, lds_bytes);
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_nee<0, false>, (int)block, lds_bytes);
    }
    if (blocks) *blocks = a < b ? a : b;
    return (int)e;
}

// A budgeted step's fold (vmx_progressive_step_budget_device): slot s of the step's list folds rad[base[s] + j], j < base[s + 1]
// - base[s], in order — k_resolve's statements for a taken sample: ++n, the three colour adds, the l*l fold — advances
// count and cursor, writes the pixels that finished and appends the others to the next list.  No early stop (light
// sampling refuses it), so the cursor is a plain sample index and every listed sample is taken.
template <bool MOMENTS>
__global__ void __launch_bounds__(256)
k_resolve_budget(FrameDev fr, const unsigned int *__restrict__ active, uint32_t n_active, const unsigned int *__restrict__ base,
                 const float4 *__restrict__ rad, PixelStateDev px, unsigned int *__restrict__ next_active, unsigned int *next_count,
                 float *__restrict__ out, DevCounters *ctr) {
    __shared__ unsigned int s_keep, s_base, s_taken, s_done;
    if (threadIdx.x == 0) s_keep = 0, s_taken = 0, s_done = 0;
    __syncthreads();
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    uint32_t lp = 0, taken = 0, done = 0;
    if (slot < n_active) {
        lp = active[slot];
        float4 acc = ((float4 *)px.accum)[lp];
        uint32_t n = px.count[lp];
        const uint32_t cursor = px.cursor[lp];
        const uint32_t b0 = base[slot];
        uint32_t cnt = base[slot + 1] - b0;
        cnt = min(cnt, cursor < fr.kmax ? fr.kmax - cursor : 0u);  // (the scan's counts are clamped so already)
        for (uint32_t j = 0; j < cnt; ++j) {
            const float4 s = rad[b0 + j];
            ++n;
            acc.x = acc.x + s.x;
            acc.y = acc.y + s.y;
            acc.z = acc.z + s.z;
            if (MOMENTS) {
                const float l = luminance(s.x, s.y, s.z);
                acc.w = acc.w + l * l;
            }
        }
        taken = cnt;
        const uint32_t next = cursor + cnt;
        if (next >= fr.kmax) {
            resolved_pixel(acc, n, out + (size_t)lp * 5);
            done = 1;
        } else {
            keep = true;
        }
        ((float4 *)px.accum)[lp] = acc;
        px.count[lp] = n;
        px.cursor[lp] = next;
    }
    uint32_t my = 0;
    if (keep) my = atomicAdd(&s_keep, 1u);
    if (taken) atomicAdd(&s_taken, taken);
    if (done) atomicAdd(&s_done, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        s_base = s_keep ? atomicAdd(next_count, s_keep) : 0u;
        if (s_taken) atomicAdd(&ctr->samples, (unsigned long long)s_taken);
        if (s_done) atomicAdd(&ctr->pixels_done, (unsigned long long)s_done);
    }
    __syncthreads();
    if (keep) next_active[s_base + my] = lp;
}

int launch_resolve_budget(const FrameDev &fr, const unsigned int *active, uint32_t n_active, const unsigned int *base, const void *rad,
                          PixelStateDev px, unsigned int *next_active, unsigned int *next_count, float *out_rgbaz, DevCounters *counters,
                          void *stream, bool moments) {
    if (n_active == 0) return 0;
    hipLaunchKernelGGL(moments ? k_resolve_budget<true> : k_resolve_budget<false>, dim3((n_active + 255) / 256), dim3(256), 0,
                       (hipStream_t)stream, fr, active, n_active, base, (const float4 *)rad, px, next_active, next_count, out_rgbaz, counters);
    return launch_status();
}
