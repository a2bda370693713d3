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

// the kernel, twice: k_nee<SRC, TEX> for a scene without emissive triangles, k_nee_mesh<SRC, TEX> for one with a table
#define VMX_NEE_MESH 0
#include "vmx_nee_kernel.inc"
#undef VMX_NEE_MESH
#define VMX_NEE_MESH 1
#include "vmx_nee_kernel.inc"
#undef VMX_NEE_MESH

// wk: heads (one counter, zeroed), reserve, the stack fields; camera paths (rays == NULL): active, n_active, samples,
// div_samples, `items` = padded slots * samples; explicit rays: o / d, `items` rays; a budgeted step (rays == NULL,
// wk.flat_ids the item bases): active, n_active, `items` = base[n_active]
int launch_nee(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PixelStateDev px, const float *o, const float *d,
               uint32_t items, void *rad, DevCounters *counters, LaunchCfg cfg, void *stream, const EmitDev &ed) {
    hipStream_t s = (hipStream_t)stream;
    dim3 g(cfg.grid), b(cfg.block);
#define VMX_GO(S, T)                                                                                                              \
    do {                                                                                                                          \
        if (ed.n) /* the scene has a table of emissive triangles */                                                               \
            hipLaunchKernelGGL((k_nee_mesh<S, T>), g, b, cfg.lds_bytes, s, sc, fr, wk, px, o, d, items, (float4 *)rad, counters, ed); \
        else                                                                                                                      \
            hipLaunchKernelGGL((k_nee<S, T>), g, b, cfg.lds_bytes, s, sc, fr, wk, px, o, d, items, (float4 *)rad, counters);      \
    } while (0)
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

template <int SRC, bool MESH>
static hipError_t nee_blocks(uint32_t block, uint32_t lds_bytes, int &a, int &b) {
    hipError_t e = MESH ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_nee_mesh<SRC, true>, (int)block, lds_bytes)
                        : hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_nee<SRC, true>, (int)block, lds_bytes);
    if (e != hipSuccess) return e;
    return MESH ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_nee_mesh<SRC, false>, (int)block, lds_bytes)
                : hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_nee<SRC, false>, (int)block, lds_bytes);
}

int query_nee_blocks_per_cu(uint32_t block, uint32_t lds_bytes, bool rays, int *blocks, bool budgeted, bool mesh) {
    int a = 0, b = 0;
    hipError_t e;
    if (budgeted) e = mesh ? nee_blocks<2, true>(block, lds_bytes, a, b) : nee_blocks<2, false>(block, lds_bytes, a, b);
    else if (rays) e = mesh ? nee_blocks<1, true>(block, lds_bytes, a, b) : nee_blocks<1, false>(block, lds_bytes, a, b);
    else e = mesh ? nee_blocks<0, true>(block, lds_bytes, a, b) : nee_blocks<0, false>(block, lds_bytes, a, b);
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
