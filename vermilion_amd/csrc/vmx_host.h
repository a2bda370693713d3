// vmx_host.h — first part of vmx_api.cpp (not a header of its own: it relies on that file's includes)
namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(VMX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));           \
    } while (0)

#define LAUNCH_TRY(expr)                                                                           \
    do {                                                                                           \
        int e_ = (expr);                                                                           \
        if (e_ != 0)                                                                               \
            return fail(VMX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString((hipError_t)e_)); \
    } while (0)

// The reference's eight spheres, core/engines/meshEngine.cpp:377-500.
// sizeOfSpheres = 1e7*5 is a double narrowed to float by glm::vec3 / the float
// `rad` parameter (meshEngine.cpp:182, 425).
const vmx_sphere kReferenceSpheres[8] = {
    {{15.f, 140.f, 25.f}, 3.5f, {0.f * 15.f, .5f * 15.f, 1.0f * 15.f}, VMX_SPHERE_EMIT, {-55.f, 350.f, -150.f}, -1.f},
    {{0.f, 3300.f, 1300.f}, 250.f, {1.0f * 15.2f, 1.0f * 15.2f, 1.0f * 15.2f}, VMX_SPHERE_EMIT, {500.f, 800.f, 1300.f}, 1.f},
    {{0.f, (float)(-5e7), 0.f}, (float)5e7, {0, 0, 0}, 0u, {0.f, (float)(-5e7), 0.f}, 1.f},
    {{0.f, (float)(5e7 + 1000), 0.f}, (float)5e7, {0, 0, 0}, 0u, {0.f, (float)(5e7 + 1000), 0.f}, 1.f},
    {{(float)(-5e7 + 2000), 0.f, 0.f}, (float)5e7, {0, 0, 0}, 0u, {(float)(-5e7 + 2000), 0.f, 0.f}, -1.f},
    {{(float)(5e7 - 2000), 0.f, 0.f}, (float)5e7, {0, 0, 0}, 0u, {(float)(5e7 - 2000), 0.f, 0.f}, -1.f},
    {{0.f, 0.f, (float)(-5e7 + 2000)}, (float)5e7, {0, 0, 0}, 0u, {0.f, 0.f, (float)(-5e7 + 2000)}, -1.f},
    {{0.f, 0.f, (float)(5e7 - 2000)}, (float)5e7, {0, 0, 0}, 0u, {0.f, 0.f, (float)(5e7 - 2000)}, 1.f},
};

// device memory, freed when its owner dies (move-only).  ensure: grow only, contents not preserved.  Work in flight
// that still uses the memory is the owner's to wait for before that
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p, n = o.n;
            o.p = nullptr, o.n = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    int ensure(size_t count) {
        if (count <= n && p) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        hipError_t e = hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e != hipSuccess) return (int)e;
        n = count;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};
static_assert(!std::is_copy_constructible<DevBuf<float>>::value, "DevBuf owns its memory: it moves, it is never copied");

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

struct DevStream : NoCopy {
    hipStream_t s = nullptr;
    ~DevStream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

struct EventPool : NoCopy {
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    ~EventPool() { for (auto e : ev) (void)hipEventDestroy(e); }
    hipEvent_t get() {
        if (used == ev.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            ev.push_back(e);
        }
        return ev[used++];
    }
    void reset() { used = 0; }
};

// An event recorded after each call and waited on by the next, whatever its stream: how calls that share a workspace,
// or a scene's records, are ordered.  The event is created by the first record; until then wait and sync do nothing.
struct Fence : NoCopy {
    hipEvent_t ev = nullptr;
    bool recorded = false;
    ~Fence() { if (ev) (void)hipEventDestroy(ev); }
    int wait(hipStream_t s) const {
        if (recorded) HIP_TRY(hipStreamWaitEvent(s, ev, 0));
        return VMX_OK;
    }
    int record(hipStream_t s) {
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ev, s));
        recorded = true;
        return VMX_OK;
    }
    int sync() const {
        if (recorded) HIP_TRY(hipEventSynchronize(ev));
        return VMX_OK;
    }
};

// per-pixel state of a frame in progress: what a pass reads and k_resolve advances
struct PixelBufs {
    DevBuf<unsigned char> accum;               // float4 per local pixel
    DevBuf<unsigned int> count, cursor, active[2];  // samples taken, next sample index, the pixels that still take samples (ping-pong)
    int ensure(size_t npix) {
        return accum.ensure(npix * 16) || count.ensure(npix) || cursor.ensure(npix) || active[0].ensure(npix) || active[1].ensure(npix);
    }
};

// per-scene reusable device workspace for the render pipeline
struct Workspace {
    DevBuf<unsigned char> queue_planes[2];  // first-generation kernels (A/B library) only
    DevBuf<unsigned int> queue_counts;      // 2 * kSubQueues * 32
    DevBuf<unsigned int> heads;         // kSubQueues * 32 reservation heads of k_paths
    DevBuf<unsigned char> overflow_stack;  // k_paths: stack levels beyond the LDS part
    DevBuf<unsigned char> rayA, state, hit, thr;  // split wavefront: per-path state
    DevBuf<unsigned int> ids[3], id_counts;             // split wavefront: live path ids ([2]: two-phase shading)
    DevBuf<unsigned int> sort_keys[2], ids_sorted;      // bounce reordering (path_sort.hip)
    DevBuf<unsigned char> sort_tmp;
    DevBuf<unsigned char> cam_inner;                    // per-frame camera-relative scene tables: 8 node copies, then the triangles
    DevBuf<unsigned int> claims;                        // per-pixel claims of the run's frame (pixel_claim.h) + the number of claimed pixels
    DevBuf<unsigned int> claim_lists;                   // ... and the list records of its pixels without a claim (kListWords words each)
    // the pixels whose list k_pixel_lists makes (build_claims): their bits per tile; [popcounts | their exclusive scan |
    // the list's length, the kernel's work head]; the tile-ordered list; scan scratch
    DevBuf<unsigned long long> claim_pend_mask;
    DevBuf<unsigned int> claim_pend_u32, claim_pend_ids;
    DevBuf<unsigned char> claim_pend_tmp;
    // passes that fuse their claimed pixels: the ordered lists of the pass's unclaimed and claimed slots, rebuilt per pass;
    // "unclaimed" bits per 64 slots; [popcounts | their exclusive scan | the two lists' lengths]; scan scratch
    DevBuf<unsigned int> unclaimed, claimed_slots, unclaimed_u32;
    DevBuf<unsigned long long> unclaimed_mask;
    DevBuf<unsigned char> unclaimed_tmp;
    size_t unclaimed_words = 0, unclaimed_tmp_bytes = 0;
    // ... and, in a run with list claims, the ordered list of the walk slots (unclaimed, no list): the same three, with
    // the scan scratch above.  (The straggler list of such a pass lies in ids[2], which only two-phase shading uses.)
    DevBuf<unsigned int> walk_slots, walk_u32;
    DevBuf<unsigned long long> walk_mask;
    DevBuf<unsigned char> rad;          // float4 per path of a pass
    DevBuf<unsigned long long> rad_mask;  // split pipeline: one bit per path, "its radiance was stored" (PathArrays::rad_mask)
    // VMX_SAMPLING_ELIDE_DEAD: live bits per 64 paths; [popcounts | their exclusive scan | list length]; the list; scan scratch
    DevBuf<unsigned long long> live_mask;
    DevBuf<unsigned int> live_u32, live_ids;
    DevBuf<unsigned char> live_tmp;
    // two-phase shading (k_shade_ends -> k_shade): the same three for the positions left to k_shade; their list is ids[2]
    DevBuf<unsigned long long> full_mask;
    DevBuf<unsigned int> full_u32;
    DevBuf<unsigned char> full_tmp;
    size_t full_words = 0, full_tmp_bytes = 0;
    DevBuf<unsigned char> out_rec;   // k_trace_w<.., SORT>: 32-byte records of the camera rays that still need shading
    DevBuf<unsigned int> out_count;
    size_t out_capacity = 0;         // entries out_rec was sized for
    // k_trace_w<1, .., GUIDE>: the fallback list of a bounce generation (path ids; [0] of guide_fb_count is its length,
    // which the second launch reads on the device) and the frame's (settled, fallback) ray counts
    DevBuf<unsigned int> guide_fb, guide_fb_count, guide_heads;
    DevBuf<unsigned long long> guide_ctr;
    DevBuf<unsigned long long> guide_fused_ctr;  // k_paths<.., GuidePathsDev>: the frame's (settled, reference-tree) ray counts
    uint64_t guide_entries = 0;  // entries of the bounce lists handed to the GUIDE launches of the call in progress (host count)
    PixelBufs pixels;                   // vmx_render's frames (a vmx_progressive handle owns its own); active[0]: BruteForceTracer's pixel order
    DevBuf<unsigned int> next_count;
    DevBuf<DevCounters> counters;
    DevBuf<float> out;  // frame buffer for host-output renders
    std::vector<unsigned int> order;
    uint32_t order_w = 0, order_rows = 0;
    EventPool events;
};

}  // namespace

// (the handles are opaque to callers; what an owning member adds to them — an implicit destructor, a template over the
// type — is kept out of the exported symbols)
#define VMX_OPAQUE __attribute__((visibility("hidden")))

struct vmx_scene {
    int device = 0;
    int num_cus = 0;
    DevStream stream;   // (declared before the buffers: destroyed after them)
    HostBvh bvh;        // host-built trees: flat layout + device records; device-built (LBVH): filled on demand
    LbvhDevice lbvh;    // VMX_BVH_LBVH: the tree was built and flattened on the device (lbvh_build.hip)
    bool device_built = false;
    uint32_t builder = VMX_BVH_REFERENCE;  // what vmx_scene_update's VMX_UPDATE_REBUILD runs again
    std::atomic<bool> flat_ready{true};
    bool flat_topology = true;  // bvh.start / nprims / right_offset / prim_order hold the current tree (device-built: on demand)
    uint32_t n_inner = 0;  // inner record slots on the device
    uint32_t ntris = 0, leaf_size = 4;
    std::vector<vmx_sphere> spheres;
    // inner records, then (64-byte aligned) the triangle records, in ONE allocation: a lane of the bounce
    // traversal kernel addresses either kind of record with a 32-bit byte offset from `dev.inner`
    // (SceneDev::tri_off), so inner-node lanes and leaf lanes of a wave fetch in one set of loads
    DevBuf<unsigned char> d_geom;
    DevBuf<AttrRecord> d_attrs;
    DevBuf<SphereDev> d_spheres;
    DevBuf<float> d_tex, d_tex1;
    uint32_t n_textures = 0;
    SceneDev dev{};
    std::mutex mu;
    Workspace ws;
    uint32_t block = 256;
    float bounds_lo[3] = {0, 0, 0}, bounds_hi[3] = {1, 1, 1};  // vertex bounds (origin cells of the bounce reordering)
    vmx_timings timings{};  // per-kernel durations of the last render on this scene
    uint64_t fused_paths = 0;  // ... and its camera paths that took the fused route (vmx_fused_camera_paths)
    uint64_t list_settled = 0;  // ... and its camera rays that a list claim settled (vmx_list_settled_rays)
    uint64_t guide_settled = 0, guide_fallback = 0;  // ... and its bounce rays that walked the guide (vmx_guide_rays)
    uint64_t guide_entries = 0;  // ... and the entries of the lists its GUIDE launches were handed (vmx_guide_list_entries)
    uint64_t guide_fused_settled = 0, guide_fused_fallback = 0;  // ... and the rays of its fused launches' GUIDE forms (vmx_guide_fused_rays)
    // the guide of a VMX_BVH_REFERENCE scene (guide_walk.h): the binned-SAH tree of the same triangles, its records in
    // d_geom behind the reference's (geom_layout: `off` bytes from d_geom.p, in the upload_records shape: inner records,
    // then the triangle records), so that a lane of the fused kernel addresses either tree with a 32-bit offset from
    // dev.inner; no attribute table.  `host` is the one host build the replicas of a vmx_multi share.  Stale after any
    // update that moves vertices or rebuilds: then it is not used (refitting it is a follow-up).
    struct VMX_OPAQUE Guide {
        std::shared_ptr<const HostBvh> host;
        const unsigned char *base = nullptr;  // d_geom.p + off, or NULL: d_geom has no room for a guide
        uint32_t off = 0;
        size_t bytes = 0;
        uint32_t tri_off = 0, root_ref = 0, stack_entries = 0;
        float scene_max = 0.f;
        bool valid = false;
    } guide;
    // device ray queries (vmx_query_device): allocated on the first query, then reused.  `done` is recorded after each
    // query's last kernel and waited on by the next one: one query at a time uses the workspace
    struct QueryWs {
        DevBuf<unsigned int> head;             // work counter of k_query
        DevBuf<unsigned char> overflow_stack;  // stack levels beyond the LDS part, per wave of the largest grid
        Fence done;
        uint32_t lds_entries = 0, overflow_entries = 0;
        uint32_t grid[2][kQueryModes] = {};    // persistent blocks per [per-lane fetch][mode]: VMX_QUERY_* and the
                                               // raycast entries' kQueryCastRays / kQueryCastCamera
        uint32_t stack_entries = 0;            // the tree depth the slab was sized for (a REBUILD can change it)
        DevBuf<unsigned char> albedo_rec;      // vmx_albedo_camera_device: 64 bytes per pixel for k_query's (tri_t, slot), on first use
    } qws;
    // in-place geometry updates (vmx_scene_update*): `done` is recorded after each update and waited on by every later
    // render, query and export of the scene, whatever its stream.  The refit plan is built on the first update that
    // moves vertices (scene creation is unchanged) and dropped by a REBUILD.
    struct VMX_OPAQUE UpdateState {
        Fence done;
        bool plan_ready = false;
        bool refitted = false;      // boxes differ from the builder's: the flat export's bbox comes from the records
        bool bounds_stale = false;  // bounds_lo / bounds_hi are root_box (a device REFIT does not wait for it)
        DevBuf<unsigned char> plan;                // RefitItem[], deepest tree level first
        std::vector<std::pair<uint32_t, uint32_t>> levels;  // (first entry, entries) per launch
        DevBuf<float> root_box;                    // [6] the root's box (no record holds it)
        DevBuf<float> scratch;                     // host-variant uploads and REBUILD inputs: pos | nrm | uv
    } upd;
    // progressive renders (vmx_progressive_*): every successful update moves `generation` on, and a handle begun before
    // it refuses further steps (its tuning and stack sizing came from the tree it saw); the scene outlives its handles
    uint64_t generation = 0;
    uint32_t progressive_open = 0;
    // emissive triangles (vmx_scene_set_emitters): the caller's table on the host and on the device, and the table derived
    // from it and the scene's records (vmx_emitters.inc) — made at the next light-sampled launch after the generation
    // moved (nee_emitters), so every update and every builder is covered without a hook of its own
    struct VMX_OPAQUE Emitters {
        std::vector<vmx_emitter> table;  // empty: the scene has no table
        DevBuf<uint32_t> ids;
        DevBuf<float> radiance;
        DevBuf<EmitRecord> rec;
        DevBuf<double> area, weight, cdf;
        DevBuf<int32_t> slot_em, id_em;
        Fence done;              // recorded after each derivation
        uint64_t built = ~0ull;  // the generation the derived table belongs to
        uint64_t builds = 0;     // derivations so far
        EmitDev dev{};           // what launch_nee takes (n == 0: no table)
    } em;
    ~vmx_scene() { lbvh_release(lbvh); }
};

namespace {

uint32_t local_rows_of(uint32_t height, uint32_t stripe_rows, uint32_t rank, uint32_t world) {
    if (world <= 1) return height;
    uint32_t rows = 0;
    const uint32_t n_stripes = (height + stripe_rows - 1) / stripe_rows;
    for (uint32_t s = rank; s < n_stripes; s += world)
        rows += std::min(stripe_rows, height - s * stripe_rows);
    return rows;
}

// Camera ctor conversion (camera.cpp:43-47) + camera matrix (pathtracer.cpp:216-221).
// glm::rotate (gtc/matrix_transform) on the upper-left 3x3; column-major.
struct M3 {
    float c[3][3];
};
M3 rotate_axis(const M3 &m, float angle, float ax, float ay, float az) {
    const float c = std::cos(angle), s = std::sin(angle);
    const float inv = 1.0f / std::sqrt((ax * ax + ay * ay) + az * az);  // glm::normalize
    const float a[3] = {ax * inv, ay * inv, az * inv};
    const float t[3] = {a[0] * (1.0f - c), a[1] * (1.0f - c), a[2] * (1.0f - c)};
    float r[3][3];
    r[0][0] = c + t[0] * a[0];
    r[0][1] = t[0] * a[1] + s * a[2];
    r[0][2] = t[0] * a[2] - s * a[1];
    r[1][0] = t[1] * a[0] - s * a[2];
    r[1][1] = c + t[1] * a[1];
    r[1][2] = t[1] * a[2] + s * a[0];
    r[2][0] = t[2] * a[0] + s * a[1];
    r[2][1] = t[2] * a[1] - s * a[0];
    r[2][2] = c + t[2] * a[2];
    M3 out;
    for (int col = 0; col < 3; ++col)
        for (int row = 0; row < 3; ++row)
            out.c[col][row] = (m.c[0][row] * r[col][0] + m.c[1][row] * r[col][1]) + m.c[2][row] * r[col][2];
    return out;
}

int make_frame(const vmx_camera &cam, const vmx_opts &o, FrameDev &fr) {
    std::memset(&fr, 0, sizeof(fr));  // (fields a caller sets later — lead, bounce_bits — start defined: a fixed-count frame reads lead)
    const uint32_t W = cam.image_res[0], H = cam.image_res[1], spp = cam.rays_per_pixel;
    if (W == 0 || H == 0) return fail(VMX_ERR_INVALID, "image resolution must be non-zero");
    if ((uint64_t)W * H > 0x7fffffffull / 8) return fail(VMX_ERR_INVALID, "image too large");
    if (spp < 4)
        return fail(VMX_ERR_INVALID,
                    "rays_per_pixel < 4 renders no sample (uSamplesPerPixel/4 == 0, pathtracer.cpp:247)");
    if ((o.sampling & VMX_SAMPLING_MODE_MASK) > VMX_SAMPLING_CORRECTED || (o.sampling & ~(VMX_SAMPLING_MODE_MASK | VMX_SAMPLING_LIBM_DOUBLE | VMX_SAMPLING_ELIDE_DEAD)))
        return fail(VMX_ERR_INVALID, "unknown sampling mode");
    if (cam.rotation_units > VMX_ROTATION_RADIANS) return fail(VMX_ERR_INVALID, "unknown rotation_units");
    // Camera ctor (camera.cpp:43-47): mRotation = (-rx, -ry, +rz) * 3.1415926535 / 180, double arithmetic narrowed to
    // float; with VMX_ROTATION_RADIANS the caller hands over mRotation itself
    const bool rad = cam.rotation_units == VMX_ROTATION_RADIANS;
    const float rx = rad ? cam.rotation_rad[0] : (float)(-cam.rotation_deg[0] * 3.1415926535 / 180);
    const float ry = rad ? cam.rotation_rad[1] : (float)(-cam.rotation_deg[1] * 3.1415926535 / 180);
    const float rz = rad ? cam.rotation_rad[2] : (float)(cam.rotation_deg[2] * 3.1415926535 / 180);
    M3 m = {{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}};
    m = rotate_axis(m, ry, 0, 1, 0);
    m = rotate_axis(m, rx, 1, 0, 0);
    m = rotate_axis(m, rz, 0, 0, 1);
    for (int col = 0; col < 3; ++col)
        for (int row = 0; row < 3; ++row) fr.m[col * 3 + row] = m.c[col][row];
    fr.px = cam.position[0], fr.py = cam.position[1], fr.pz = cam.position[2];
    fr.film_dist = cam.back_distance;
    fr.sensor_x = cam.back_size[0], fr.sensor_y = cam.back_size[1];
    fr.width = W, fr.height = H;
    fr.inv_width = 1.0 / (double)W, fr.inv_height = 1.0 / (double)H;
    fr.div_width = make_fastdiv(W);
    fr.spp = spp, fr.quarter = spp / 4, fr.kmax = 4 * (spp / 4);
    fr.nmin = (uint32_t)std::floor(std::sqrt((double)spp));
    fr.early_stop = o.early_stop ? 1u : 0u;
    fr.r2scale = (o.sampling & VMX_SAMPLING_MODE_MASK) == VMX_SAMPLING_CORRECTED ? 1.0f : 10.0f;
    fr.libm_double = (o.sampling & VMX_SAMPLING_LIBM_DOUBLE) ? 1u : 0u;
    fr.elide_dead = (o.sampling & VMX_SAMPLING_ELIDE_DEAD) ? 1u : 0u;  // split passes of vmx_render only (k_raygen)
    fr.bounce_bits = 0;  // render_impl
    fr.world = o.world <= 1 ? 1u : o.world;
    fr.rank = o.world <= 1 ? 0u : o.rank;
    fr.stripe_rows = o.stripe_rows ? o.stripe_rows : 16u;
    fr.div_stripe = make_fastdiv(fr.stripe_rows);
    if (fr.rank >= fr.world) return fail(VMX_ERR_INVALID, "rank must be < world");
    fr.local_rows = local_rows_of(H, fr.stripe_rows, fr.rank, fr.world);
    fr.seed = o.seed;
    return VMX_OK;
}

int bind_device(const vmx_scene *sc) {
    HIP_TRY(hipSetDevice(sc->device));
    return VMX_OK;
}

// (work on a scene waits on its last geometry update — sc->upd.done.wait(s) — whatever stream that ran on; nothing is
// enqueued before a scene's first update)
LaunchCfg trace_cfg(const vmx_scene *sc, uint32_t work_items, int blocks_per_cu) {
    LaunchCfg c;
    c.block = sc->block;
    c.lds_bytes = (sc->block / 64) * sc->dev.stack_entries * 512;
    if (blocks_per_cu < 1) blocks_per_cu = 1;
    uint32_t grid = (uint32_t)sc->num_cus * (uint32_t)blocks_per_cu;
    grid = std::max(8u, grid & ~7u);
    if (work_items < grid) grid = std::max(1u, work_items);
    c.grid = grid;
    return c;
}

// 8x8-pixel tiles, tile-major: consecutive slots are neighbouring pixels, so a
// wave's 64 primary rays are coherent.
void tile_order(uint32_t W, uint32_t rows, std::vector<unsigned int> &order) {
    order.clear();
    order.reserve((size_t)W * rows);
    for (uint32_t ty = 0; ty < rows; ty += 8)
        for (uint32_t tx = 0; tx < W; tx += 8)
            for (uint32_t y = ty; y < std::min(ty + 8, rows); ++y)
                for (uint32_t x = tx; x < std::min(tx + 8, W); ++x) order.push_back(y * W + x);
}

void stage_out(vmx_stage_stats &dst, const StageCounters &c) {
    dst.rays = c.rays, dst.inner_visits = c.inner_visits, dst.tri_tests = c.tri_tests;
    dst.tri_hits = c.tri_hits, dst.continued = c.continued;
}

struct TimedLaunch {
    hipEvent_t a, b;
    int stage;   // vmx_stats bucket: 0 primary, 1 bounce, 2 shade
    int kernel;  // VMX_K_* of vmx_timings (per-kernel durations of the last call)
};

// The timed bracket: what is enqueued on `s` between timed_begin and timed_end lies between two events of the workspace's
// pool and is filed under (stage, kernel) of the call's statistics; stage -1: no vmx_stats bucket.  Brackets do not nest.
int timed_begin(Workspace &ws, std::vector<TimedLaunch> &timed, hipStream_t s, int stage, int kernel) {
    const TimedLaunch tl{ws.events.get(), ws.events.get(), stage, kernel};
    if (!tl.a || !tl.b) return fail(VMX_ERR_HIP, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(tl.a, s));
    timed.push_back(tl);
    return VMX_OK;
}

int timed_end(std::vector<TimedLaunch> &timed, hipStream_t s) {
    HIP_TRY(hipEventRecord(timed.back().b, s));
    return VMX_OK;
}

int finish_stats(vmx_scene *sc, hipStream_t s, std::vector<TimedLaunch> &timed, hipEvent_t ev0, hipEvent_t ev1, vmx_stats *stats,
                 uint64_t launches, uint64_t passes, std::chrono::steady_clock::time_point t0);  // api_render.inc

// One timed call on a scene's workspace.  open: the event pool starts over and the call's two events are taken; start /
// stop: ev0 / ev1 go on the stream — stats->ms_device is what lies between them, and each entry decides where that is
// relative to its own copies; clear_counters: the three device counters a call's statistics are read from; finish: stop,
// unless the entry already has, then finish_stats waits for the stream and reads them.
struct CallScope {
    vmx_scene *sc;
    hipStream_t s;
    std::chrono::steady_clock::time_point t0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool stopped = false;
    int open() {
        sc->ws.events.reset();
        ev0 = sc->ws.events.get(), ev1 = sc->ws.events.get();
        return ev0 && ev1 ? VMX_OK : fail(VMX_ERR_HIP, "hipEventCreate failed");
    }
    int start() {
        HIP_TRY(hipEventRecord(ev0, s));
        return VMX_OK;
    }
    int clear_counters() {
        Workspace &ws = sc->ws;
        HIP_TRY(hipMemsetAsync(ws.counters.p, 0, sizeof(DevCounters), s));
        if (ws.guide_ctr.p) HIP_TRY(hipMemsetAsync(ws.guide_ctr.p, 0, 16, s));
        if (ws.guide_fused_ctr.p) HIP_TRY(hipMemsetAsync(ws.guide_fused_ctr.p, 0, 16, s));
        return VMX_OK;
    }
    int stop() {
        HIP_TRY(hipEventRecord(ev1, s));
        stopped = true;
        return VMX_OK;
    }
    int finish(std::vector<TimedLaunch> &timed, vmx_stats *stats, uint64_t launches, uint64_t passes) {
        if (!stopped)
            if (int rc = stop()) return rc;
        return finish_stats(sc, s, timed, ev0, ev1, stats, launches, passes, t0);
    }
};

// reads the 16 sub-queue tails; returns total and the largest
int read_counts(vmx_scene *sc, unsigned int *d_counts, hipStream_t s, uint64_t &total, uint32_t &largest,
                uint32_t sub_capacity = 0xffffffffu, uint32_t *per_queue = nullptr) {
    unsigned int h[kSubQueues * 32];
    HIP_TRY(hipMemcpyAsync(h, d_counts, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    total = 0, largest = 0;
    for (uint32_t q = 0; q < kSubQueues; ++q) {
        // an append that would have written past its sub-list wrote nothing and left the tail high (id_append)
        if (h[q * 32] > sub_capacity) return fail(VMX_ERR_NOMEM, "live-path list overflow (sub-list " + std::to_string(q) + ")");
        const uint32_t c = h[q * 32];
        total += c;
        largest = std::max(largest, c);
        if (per_queue) per_queue[q] = c;
    }
    (void)sc;
    return VMX_OK;
}

struct Tuning {
    uint32_t refill_min, refill_primary, shade_min, leaf_min, tail_threshold;
    uint32_t lds_entries, lds_primary, lds_bounce;  // LDS stack levels: fused kernels, camera-ray trace, bounce trace
    uint32_t sort_mode;  // bounce reordering: obits | dbits << 4 | dir_major << 8 | chunk_log2 << 12 | shade_sorted << 20
};

// the WorkDev every launch site starts from: zeroed, the work heads, and with a tuning its refill and shade thresholds
WorkDev make_work(unsigned int *heads, const Tuning *tn) {
    WorkDev wk;
    std::memset(&wk, 0, sizeof(wk));
    wk.heads = heads;
    if (tn) wk.refill_min = tn->refill_min, wk.shade_min = tn->shade_min;
    return wk;
}

// ---- vmx_opts.reserved[0]: the pipeline form in the low byte, above it the switches the host reads --------------------
constexpr uint32_t kFormPipeline = 0xFFu;      // the pipeline form, 0..4 (render_forms)
constexpr uint32_t kFormOnePhase = 1u << 8;    // one-phase shading of the split passes: no k_shade_ends (Forms::two_phase)
constexpr uint32_t kFormKeepEnds = 1u << 9;    // the camera rays keep k_shade_ends: the trace kernel does not sort them (Forms::sorted)
constexpr uint32_t kFormPool = 1u << 10;       // A/B library: bounce generations through k_trace_pool (Forms::pool)
constexpr uint32_t kFormNoClaims = 1u << 11;   // no per-pixel claims (Forms::claims_on)
constexpr uint32_t kFormNoFuse = 1u << 12;     // claimed pixels are not fused into k_shade<0> (Forms::fuse_on)
constexpr uint32_t kFormNoLists = 1u << 13;    // no list claims (Forms::lists_on)
constexpr uint32_t kFormNoGuide = 1u << 14;    // bounce rays keep the reference tree (Forms::guide)
// The bits vmx_render accepts: all of them.
constexpr uint32_t kFormsRender = kFormPipeline | kFormOnePhase | kFormKeepEnds | kFormPool | kFormNoClaims | kFormNoFuse | kFormNoLists | kFormNoGuide;
// The bits vmx_radiance accepts: it has no camera pass and never walks the guide, so the switches of the claims and of the
// guide (bits 11-14) name nothing it runs and are refused as unknown; bits 8-9 are older than that rule — accepted and
// ignored, so that one vmx_opts serves a frame and the rays that check it — and bit 10 selects its traversal (Forms::pool).
constexpr uint32_t kFormsRadiance = kFormPipeline | kFormOnePhase | kFormKeepEnds | kFormPool;

// what a call derives from those bits and its frame (render_forms: one statement per member, with the reasons)
struct Forms {
    uint32_t pipeline = 0;
    bool count = false;           // the counting build (vmx_opts.collect_counters)
    bool split_any = false, legacy = false;
    bool two_phase = false;       // split passes: k_shade_ends + k_shade on what it queues
    bool sorted = false;          // ... and the camera rays sorted by the trace kernel itself (k_trace_w<0, .., SORT>): no k_shade_ends
    bool pool = false;            // A/B library: the bounce generations of a pass through k_trace_pool — unsorted passes only
    bool guide = false;           // bounce generations walk the scene's guide tree (k_trace_w<1, .., GUIDE>, guide_walk.h), a second
                                  // launch traces the fallback list; the fused launches are k_paths' GUIDE forms
    bool bounce_records = false;  // one-phase shading: the traversal kernel hands every bounce ray on as a dense (t, leaf slot, path id)
                                  // record (k_trace_w<1, .., SORT> with WorkDev::keep_all) instead of a scattered hit[pid] store
    bool elide = false;           // camera paths of the split passes: compacted live list (VMX_SAMPLING_ELIDE_DEAD)
    bool claims_on = false;       // split passes may use per-pixel claims (pixel_claim.h)
    bool fuse_on = false;         // ... and a dense plain camera pass fuses its claimed pixels into k_shade<0>
    bool lists_on = false;        // ... and the pixels without a claim get list claims
};

constexpr uint32_t kPathsBlock = 256;

// ---- PathTracer::Render in three pieces: set-up, one pass, a run of passes ------------------------------------------
// vmx_render[_device] is set-up + one run to completion; a vmx_progressive handle keeps the RenderJob (and its own
// PixelBufs and frame buffer) between runs of a few samples each.  The per-pass scratch — path arrays, id lists, ray
// records, camera tables — is the scene's shared workspace: a run binds it again (render_bind), because any other call
// on the scene may have used or regrown it since the last one.
struct RenderJob {
    // fixed by render_setup
    FrameDev fr;
    vmx_opts opts;
    Tuning tn;
    Forms f;
    uint32_t npix = 0;
    // the light-sampling integrator (api_nee.inc; set by the caller right after render_setup): a pass's paths run in k_nee,
    // whatever the pipeline form, and a run binds only what that kernel and k_resolve use
    bool nee = false;
    uint32_t smax = 0, smax_alloc = 0;  // samples per pixel and pass: the most a pass takes / what the buffers are sized for
    uint32_t n_pad_max = 0, sub_cap = 0;
    uint64_t mem_budget = 0;
    int pb = 1, bb = 1, rb = 1, tb = 1, tbb = 1;  // blocks per CU: first-generation kernels, fused kernel, camera / bounce trace
    size_t live_words_max = 0, live_tmp_bytes = 0;
    PixelBufs *pixels = nullptr;  // per-pixel state: the workspace's (vmx_render) or the handle's
    float *d_out = nullptr;       // where k_resolve writes a finished pixel
    hipStream_t s = nullptr;
    // bound to the workspace by render_bind, every run
    PixelStateDev px{nullptr, nullptr, nullptr};
    PathArrays pa{};
    IdQueue qi[3];
    QueueDev q[2];  // first-generation kernels (A/B library) only
    const unsigned int *claims = nullptr;  // this run's claim table, or NULL: none was built (render_bind)
    const unsigned int *claim_lists = nullptr;  // ... and its list records, or NULL
    // the schedule's state between passes
    bool initialised = false;  // the tile-ordered pixel list is uploaded and the per-pixel state zeroed
    uint32_t n_active = 0;
    int cur_list = 0;
    PassSchedule sched;      // pass_schedule.h: what plan_pass advances, and `ragged`
    bool moments = false;    // k_resolve<true>: accum.w carries the sum of squared luminances (VMX_PROGRESSIVE_MOMENTS)
    uint64_t frame_passes = 0;  // passes since set-up
    // the current run
    std::vector<TimedLaunch> timed;
    uint64_t launches = 0, passes = 0;
};

}  // namespace
