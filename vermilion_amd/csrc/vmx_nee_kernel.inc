// vmx_nee_kernel.inc — part of vmx_nee.inc: the light-sampling kernel, once per VMX_NEE_MESH.
//
// SRC 0: camera paths — item = path id = slot * samples + j of the pass's active pixels (pixel-major, as k_paths numbers
//        them for k_resolve); SRC 1: explicit rays o / d — item i on stream (seed, i, 0), jitter draws skipped;
//        SRC 2: a budgeted step's camera paths — slot s of the step's list owns the items [base[s], base[s + 1]) of the
//        exclusive scan wk.flat_ids (n_active + 1 entries, strictly increasing: every listed pixel takes a sample), item
//        i is sample j = i - base[s] of its pixel; a lane finds s by bisection when it takes the item (log2 of the list's
//        length dependent 4-byte loads per path of some 55 rays), and rad[i] is where k_resolve_budget looks for it
// TEX: accumRadiance is carried (a texture is bound); else it stays (1, 1, 1, 1)
// MESH: the scene has a table of emissive triangles (ed.n > 0; include/vermilion_hip.h, "emissive triangles").  Every cast
//       whose returned hit is emitter e's triangle takes radiance_e for its hitColour (one 4-byte load of slot_em per
//       triangle hit), and the emitter loop gets one more step, em == nsph: one area sample of the table, chosen by
//       bisection over cdf.  hit_em / step_em / sh_em: the emitter of the cast's returned hit, of the open step's own hit
//       (self-exclusion) and of the pending area shadow ray (-1: a cone's), so there is still one traversal call site.
//       This file is included twice by vmx_nee.inc: VMX_NEE_MESH 0 is k_nee<SRC, TEX>, which keeps its name and its
//       arguments, so that a scene without a table runs the kernel it always ran, instruction for instruction
//       (profiles/nee_mesh_isa.txt: a trailing argument alone moves the hidden arguments behind it); VMX_NEE_MESH 1 is
//       k_nee_mesh<SRC, TEX>, which takes the table
#if VMX_NEE_MESH
#define VMX_NEE_KERNEL k_nee_mesh
#define VMX_NEE_TABLE_ARG , EmitDev ed
#else
#define VMX_NEE_KERNEL k_nee
#define VMX_NEE_TABLE_ARG
#endif
template <int SRC, bool TEX>
__global__ void __launch_bounds__(256)
VMX_NEE_KERNEL(SceneDev sc, FrameDev fr, WorkDev wk, PixelStateDev px, const float *__restrict__ ray_o, const float *__restrict__ ray_d,
               uint32_t n_items, float4 *__restrict__ rad, DevCounters *ctr VMX_NEE_TABLE_ARG) {
    constexpr bool MESH = VMX_NEE_MESH != 0;
#if !VMX_NEE_MESH
    const EmitDev ed = {};  // (never read: every use is under `if (MESH)`)
#endif
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
    int step_em = -1, sh_em = -1;  // MESH only
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
        int hit_em = -1;
        if (MESH) {  // the returned hit is the BVH's triangle (no sphere came nearer) and that triangle emits
            if (has && c.slot >= 0 && c.nearest == c.tri_t) {
                hit_em = ed.slot_em[c.slot];
                if (hit_em >= 0) {
                    const EmitRecord &r = ed.rec[hit_em];
                    c.cr = r.rad[0], c.cg = r.rad[1], c.cb = r.rad[2];
                }
            }
        }

        // ---- what the finished ray means -------------------------------------------------------------------------------
        if (has) {
            if (shadow) {
                // accumColour.rgb += accumRadiance.rgb * hitColour * weight (a miss leaves hitColour black); an area
                // sample counts only where its own triangle is the returned hit
                if (MESH && sh_em >= 0 && hit_em != sh_em) {
                } else if (TEX) {
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
                if (MESH) step_em = hit_em;
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
                    em = inside ? nsph + (MESH ? 1u : 0u) : 0u;
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
                    if (MESH) sh_em = -1;
                    ++n_sec;
                }
            }
            if (MESH && em == nsph && !shadow) {  // the area sample of the emissive triangles, after the last sphere
                em = nsph + 1u;
                const double W = ed.cdf[ed.n - 1u];
                if (!(W == 0.0)) {
                    const double xi0 = rng_u01(P.rng), xi1 = rng_u01(P.rng), xi2 = rng_u01(P.rng);
                    const double u = xi0 * W;
                    uint32_t lo = 0, hi = ed.n - 1u;  // the smallest e with cdf[e] > u, clamped to n - 1
                    while (lo < hi) {
                        const uint32_t mid = lo + ((hi - lo) >> 1);
                        if (ed.cdf[mid] > u) hi = mid;
                        else lo = mid + 1u;
                    }
                    const double we = ed.weight[lo], area = ed.area[lo];
                    const EmitRecord &r = ed.rec[lo];
                    const double e1x = (double)r.e1[0], e1y = (double)r.e1[1], e1z = (double)r.e1[2];
                    const double e2x = (double)r.e2[0], e2y = (double)r.e2[1], e2z = (double)r.e2[2];
                    const double s = sqrt(xi1), b1 = s * (1.0 - xi2), b2 = s * xi2;
                    const double ddx = (((double)r.v0[0] + b1 * e1x) + b2 * e2x) - (double)P.ox;
                    const double ddy = (((double)r.v0[1] + b1 * e1y) + b2 * e2y) - (double)P.oy;
                    const double ddz = (((double)r.v0[2] + b1 * e1z) + b2 * e2z) - (double)P.oz;
                    const double d2 = (ddx * ddx + ddy * ddy) + ddz * ddz;
                    const double inv = 1.0 / sqrt(d2);
                    const double odx = ddx * inv, ody = ddy * inv, odz = ddz * inv;
                    const double nx = e1y * e2z - e2y * e1z, ny = e1z * e2x - e2z * e1x, nz = e1x * e2y - e2x * e1y;
                    const double nl = sqrt((nx * nx + ny * ny) + nz * nz);
                    const double cosl = fabs(((nx / nl) * odx + (ny / nl) * ody) + (nz / nl) * odz);
                    const float ox_ = (float)odx, oy_ = (float)ody, oz_ = (float)odz;
                    const float dw = dot3(wx, wy, wz, ox_, oy_, oz_);
                    const double pdf = ((we / W) * d2) / (area * cosl);
                    const float w_ = (float)(((double)dw / 3.141592653589793) / pdf);
                    bool keep = !(we == 0.0) && !(d2 == 0.0) && !(cosl == 0.0) && !(dw <= 0.f) && isfinite(w_) && step_em != (int)lo;
                    // a direction inside the cone of an emitter sphere belongs to that sphere's sample
                    for (uint32_t j = 0; j < nsph; ++j) {
                        if (!((emask >> j) & 1u)) continue;
                        float bx, by, bz;
                        double qj;
                        nee_cone(s_geom[j], P.ox, P.oy, P.oz, bx, by, bz, qj);
                        const float ex = ox_ - bx, ey = oy_ - by, ez = oz_ - bz;
                        if (0.5 * (double)dot3(ex, ey, ez, ex, ey, ez) <= qj) keep = false;
                    }
                    if (keep) {
                        sx = ox_, sy = oy_, sz = oz_;
                        wt = w_;
                        shadow = true;
                        sh_em = (int)lo;
                        ++n_sec;
                    }
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

#undef VMX_NEE_KERNEL
#undef VMX_NEE_TABLE_ARG
