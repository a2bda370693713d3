// vmx_kernels.h — host-callable launchers of the gfx950 kernels (vmx_kernels.hip).
// All launchers enqueue on `stream` and return the hipError_t of the launch as int.
#pragma once
#include <stdint.h>
#include "vmx_device.h"

namespace vmx {

constexpr uint32_t kSubQueues = 16;  // path sub-queues (one tail counter each, own cache line)

struct QueueDev {  // first-generation kernels only (vmx_kernels_ab.inc): queue of 96-byte path records
    void *planes;             // float4[kPathPlanes][capacity]
    unsigned int *counts;     // [kSubQueues * 32] — counter q at counts[q*32] (128-byte spacing)
    uint32_t capacity;        // total slots = kSubQueues * sub_capacity
    uint32_t sub_capacity;
};

struct PixelStateDev {
    void *accum;              // float4[npix_local]  (rgb sum; w: the sum of squared luminances on a moments handle, else 0)
    unsigned int *count;      // samples taken
    unsigned int *cursor;     // next linear sample index k
};

// Per-pass path state, one slot per path id `pid` = sample_plane * n_pad + slot (fixed for the
// pass: compaction between bounces moves 4-byte ids, never the state).
struct PathArrays {
    void *rayA;   // camera rays: float4 (d.x, d.y, d.z, bits(depth flag)), read densely by path id
    // paths past their first hit: one 64-byte record per path id — (o.xyz, d.x) (d.yz, bits(depth), 0)
    // (xoshiro s0, s1) (s2, s3).  Few paths live on (16 % after the first hit with the reference's
    // sampling), so their readers touch scattered ids: one line per path instead of four.
    void *state;
    void *hit;    // float2 (t of the BVH query, bits(leaf slot or -1))
    void *rad;    // float4 accumColour, updated in place; final when the path ends
    void *thr;    // float4 accumRadiance (rgb); only with a bound texture (else it stays 1,1,1)
    // one bit per path id: rad[pid] holds something k_resolve has to read — the path went on past its first hit, or
    // its first hit already gave it a non-zero colour.  ~85 % of the bench frame's paths end black at their first hit:
    // k_shade<0> does not store their radiance and k_resolve adds an exact +0 instead of loading it.  NULL: every
    // path's radiance is in `rad` (fused kernel, vmx_radiance)
    unsigned long long *rad_mask;
};

// compacted list of live path ids: kSubQueues sub-lists, each `sub_capacity` ids long
struct IdQueue {
    unsigned int *ids;
    unsigned int *counts;   // counter q at counts[q*32]
    uint32_t sub_capacity;
    uint32_t pad;
};

// work source of k_paths
struct WorkDev {
    unsigned int *heads;        // [nsrc * 32] reservation heads, zeroed before the launch
    uint32_t nsrc;              // 8 image bands (primary) or kSubQueues (queue)
    uint32_t refill_min;        // refill when this many lanes of a wave are idle
    uint32_t reserve;           // items a wave reserves per atomic on a head (multiple of 64)
    uint32_t shade_min;         // shade when this many lanes have finished traversal
    uint32_t leaf_min;          // k_paths: run the triangle step when this many lanes sit at a leaf
    uint32_t lds_entries;       // stack levels kept in LDS
    uint32_t overflow_entries;  // deeper levels, in the global slab below (64 lanes x 8 B each)
    void *overflow_stack;       // uint2[waves][overflow_entries][64]
    // primary source
    const unsigned int *active;
    uint32_t n_active, n_pad, samples;
    FastDiv div_samples;        // path id / samples (pixel-major ids); make_fastdiv(samples), set with samples
    uint32_t band_slots;        // slots per band (multiple of 64)
    uint32_t band_items;        // band_slots * samples
    uint32_t pixel_major;       // 1: pid = slot * samples + j (samples of a pixel contiguous); 0: j * n_pad + slot
    // queue source
    IdQueue qids;     // k_trace_w / k_trace_q / k_shade / tail (path ids)
    // VMX_SAMPLING_ELIDE_DEAD: camera paths whose radiance is provably zero are not traced.  k_raygen<1> leaves one word
    // of live bits + its popcount per 64 path ids; launch_live_compact turns them into the ordered list of live path ids;
    // k_raygen_live writes their rays to rayA[list position], k_trace_w<0> the hit records to hit[list position], and
    // k_shade<0> walks the list (NULL: every path of the pass, rayA / hit indexed by path id)
    unsigned long long *live_mask;
    unsigned int *live_cnt;
    const unsigned int *live_ids;
    const unsigned int *live_count;  // device scalar: entries of live_ids
    // classified output of k_trace_w<.., SORT> (DESIGN_HISTORY.md 5.1): 32-byte records of the rays that still need shading,
    // the number of list entries reserved so far (device scalar, multiple of 256), the frame's counters
    void *out_rec;
    unsigned int *out_count;
    DevCounters *out_ctr;
    uint32_t keep_all;      // k_trace_w<.., SORT>: hand EVERY finished ray on as a record, settle none (the one-phase form
                            // of a bounce generation: k_shade reads dense (t, leaf slot, path id) records instead of hit[pid])
    uint32_t pool_slots;    // A/B library: ray slots per block of k_trace_pool (vmx_trace_pool.inc)
    uint32_t out_capacity;  // entries the list holds (paths of the pass + 256 per wave of the launch): an append never
                            // writes at or past it, and a count beyond it is reported (DevCounters::overflow)
    // two-phase shading: the ordered list of positions k_shade_ends left for k_shade (NULL: one phase)
    const unsigned int *flat_ids;
    const unsigned int *flat_count;
    // camera rays: per-frame origin-relative node / triangle tables (k_camera_tables)
    const void *cam_inner;  // float4[8 * n_inner * 4]: one copy per direction octant, octant 0 = plain (lo, hi)
    uint32_t cam_n_inner;   // records per copy
    const void *cam_tris;   // float4[ntris * 4]
    // camera rays: one claim word per local pixel (pixel_claim.h; k_pixel_claims) or NULL: a claimed pixel's rays take
    // one triangle test in k_trace_w<0> instead of the BVH walk
    const unsigned int *claims;
    // ... and one list record (kListWords words) per local pixel or NULL: the rays of a pixel without a claim that
    // pc_list_settle settles skip the walk too; list_ctr: the frame's counters (DevCounters::listed).  Who runs the rule: in
    // a pass that fuses its claimed pixels k_raygen<0, true>, on the ray it forms (it is handed the lists and, in qids —
    // ids, counts[0], sub_capacity —, the straggler list for the path ids of the rays the rule leaves to the walk; the
    // traversal kernel is then handed no lists, the walk slots as `unclaimed`, and the stragglers in qids as its last
    // source, nsrc = bands + 1); in every other form k_trace_w<0> at refill time
    const unsigned int *claim_lists;
    DevCounters *list_ctr;
    // fused claimed pixels (render_pass; plain dense camera pass with claims): k_raygen<0> and k_trace_w<0> work on the
    // ordered list of the pass's slots whose pixel has no claim (launch_slot_lists); k_shade<0, .., DENSE> is launched
    // twice, over that list and — `fused`: its CLAIMED form, which forms, tests and shades the rays itself — over the
    // ordered list of the claimed slots.  NULL / 0: every slot of the pass
    const unsigned int *unclaimed;
    const unsigned int *unclaimed_count;  // device scalar: entries of `unclaimed`
    const unsigned int *shade_slots;      // the list a dense k_shade<0> walks (unclaimed slots; CLAIMED: the claimed slots)
    const unsigned int *shade_count;      // device scalar: its entries
    uint32_t fused;
};

// the guide of a reference-tree scene as k_trace_w<1, .., GUIDE> reads it (guide_walk.h); base = NULL: no guide, the
// launch is today's
struct GuideDev {
    const void *base;         // the guide's InnerRecord[], then (tri_off bytes on) its TriRecord[]; pad[0] = reference leaf slot
    uint32_t tri_off, root_ref;
    float scene_max;          // the pad's and the rule's M: no ray that starts beyond it on an axis walks the guide
    uint32_t fb_capacity;     // entries fb_ids holds
    unsigned int *fb_ids;     // fallback list: path ids of the rays the rule did not settle
    unsigned int *fb_count;   // device scalar: its length
    unsigned long long *ctr;  // [0] rays settled by the guide, [1] fallback rays
    DevCounters *overflow;    // the frame's counters: a fallback entry that does not fit is reported (DevCounters::overflow)
};

// ... and as the GUIDE forms of the fused kernel read it (k_paths<.., GuidePathsDev>): the guide's records lie in the scene's own
// record allocation, behind the reference's, so a lane addresses either tree with a 32-bit offset from SceneDev::inner
struct GuidePathsDev {
    uint32_t off;             // the guide's InnerRecord[]: bytes from SceneDev::inner (a multiple of 64, never 0)
    uint32_t tri_off;         // its TriRecord[]: bytes from SceneDev::inner; pad[0] = reference leaf slot
    uint32_t root_ref;
    float scene_max;
    unsigned long long *ctr;  // [0] rays settled by the guide, [1] rays traced over the reference tree: the rule's
                              // fallbacks and the rays that never walked the guide
};

// explicit ray batch of k_query (vmx_query.inc): device pointers, any output may be NULL
struct QueryDev {
    const float *o, *d;     // [n*3] origins / directions
    const float *tmax;      // [n] or NULL (no bound: 999999999.f, bvh.cpp:48)
    uint32_t n;
    uint32_t reserve;       // ray indices a wave reserves per atomic on `head` (multiple of 64)
    uint32_t refill_min;    // refill when this many lanes of a wave are idle
    uint32_t lds_entries;   // stack levels kept in LDS
    uint32_t overflow_entries;  // deeper levels, in the global slab below (64 lanes x 8 B each)
    uint32_t sample;        // camera source of k_query<kQueryCastCamera>: the sample index k of every pixel's ray
    void *overflow_stack;   // uint2[waves][overflow_entries][64]
    unsigned int *head;     // work counter, zeroed before the launch
    int32_t *tri_id;
    float *t;
    uint8_t *hit;
};

struct LaunchCfg {
    uint32_t grid;            // persistent blocks
    uint32_t block;           // threads per block (multiple of 64)
    uint32_t lds_bytes;       // dynamic LDS = waves_per_block * stack_entries * 512
};

// The grid of a launch whose blocks stride over `blocks` blocks' worth of work: at most per_cu blocks for each of the
// scene's compute units (cus = vmx_scene::num_cus, which VMX_CU_LIMIT lowers), at least one.  The launches below that
// take `cus` were measured on 256 compute units, where these bounds are the literals they had: 256 * per_cu.
inline uint32_t strided_grid(uint64_t blocks, uint32_t cus, uint32_t per_cu) {
    const uint64_t cap = (uint64_t)(cus ? cus : 1u) * per_cu;
    return (uint32_t)(blocks < cap ? (blocks ? blocks : 1u) : cap);
}

// ---- parity hooks -----------------------------------------------------------
int launch_trace(const SceneDev &sc, const float *o, const float *d, uint32_t n, int32_t *tri_id,
                 float *t, DevCounters *counters, bool count, LaunchCfg cfg, void *stream);
int launch_raycast(const SceneDev &sc, const float *o, const float *d, uint32_t n, void *out_rayhit,
                   LaunchCfg cfg, void *stream);
int launch_primary_ids(const SceneDev &sc, const FrameDev &fr, uint32_t k, int32_t *tri_id, float *t,
                       LaunchCfg cfg, void *stream);

// device ray queries (vmx_query.inc): mode = VMX_QUERY_NEAREST / _ANY / _COLLISION; quad: quad-cooperative record fetch
// Internal modes of the raycast entries (no ABI name, k_query<3 / 4, true | false, QueryCast>): unbounded NEAREST over explicit rays / camera rays
constexpr uint32_t kQueryCastRays = 3, kQueryCastCamera = 4, kQueryModes = 5;
int launch_query(const SceneDev &sc, const QueryDev &q, uint32_t mode, bool quad, LaunchCfg cfg, void *stream);
int query_query_blocks_per_cu(uint32_t block, uint32_t lds_bytes, uint32_t mode, bool quad, int *blocks);
// MeshEngine::RayCast of a device batch (vmx_raycast_device, camera = false: rays q.o / q.d) or of sample q.sample's
// camera ray of every pixel of fr (vmx_raycast_camera_device, camera = true; q.n = W * H): k_query<3 | 4> with cfg, then
// k_raycast_finish on finish_grid blocks of 256; out = vmx_rayhit[q.n], 16-byte aligned.  Occupancy: the modes
// kQueryCastRays = 3 / kQueryCastCamera = 4 of query_query_blocks_per_cu
int launch_raycast_query(const SceneDev &sc, const QueryDev &q, const FrameDev &fr, bool camera, bool quad, void *out,
                         LaunchCfg cfg, uint32_t finish_grid, void *stream);

// in-place geometry updates (vmx_update.inc).  Refit plan entry: a child reference (vmx_device.h) and where its box goes —
// parent record * 2 + side (0: lmin/lmax, 1: rmin/rmax), or kRefitRoot for the root's box
struct RefitItem {
    uint32_t ref, dst;
};
constexpr uint32_t kRefitRoot = 0xFFFFFFFFu;
// records of every leaf slot from new positions (pos) and / or attributes (nrm, uv); NULL keeps that part
int launch_update_records(uint32_t ntris, const float *pos, const float *nrm, const float *uv, void *tris, void *attrs,
                          void *stream);
// one tree level of the refit: n plan entries
int launch_refit_level(const RefitItem *items, uint32_t n, const float *pos, const void *tris, void *inner,
                       float *root_box, void *stream);
// attribute records back in triangle-ID order: nrm [ntris*9], uv [ntris*6] (either may be NULL)
int launch_attrs_by_id(uint32_t ntris, const void *tris, const void *attrs, float *nrm, float *uv, void *stream);

int launch_trig(const float *x, uint32_t n, float *cs, float *sn, void *stream);

// ---- render pipeline -----------------------------------------------------------
int launch_init_pixels(PixelStateDev px, uint32_t npix, void *stream);
int launch_zero_u32(unsigned int *p, uint32_t n, void *stream);
#ifdef VMX_AB_KERNELS  // first-generation kernels (vmx_kernels_ab.inc), A/B library only
// raygen + trace + shade for `samples` samples of each of n_active pixels.
// loop_to_end: every lane follows its path to termination (megakernel form).
int launch_primary(const SceneDev &sc, const FrameDev &fr, const unsigned int *active,
                   uint32_t n_active, uint32_t samples, PixelStateDev px, QueueDev qout, void *rad,
                   DevCounters *counters, bool count, bool loop_to_end, LaunchCfg cfg, void *stream);
// explicit-ray path starts for vmx_radiance: writes initial path states
int launch_radiance_init(const float *o, const float *d, uint32_t n, uint64_t seed, QueueDev qout,
                         void *stream);
// one bounce (or, loop_to_end, all remaining bounces) of every queued path
int launch_bounce(const SceneDev &sc, float r2scale, uint32_t libm_double, QueueDev qin, uint32_t max_chunks, QueueDev qout,
                  void *rad, DevCounters *counters, bool count, bool loop_to_end, bool first_step,
                  LaunchCfg cfg, void *stream);
int query_blocks_per_cu(uint32_t block, uint32_t lds_bytes, bool count, int *primary_blocks, int *bounce_blocks);
// phase-pure bounce traversal with the ray state in LDS (vmx_trace_pool.inc; profiles/r04_state_pool.txt)
int launch_trace_pool(const SceneDev &sc, const WorkDev &wk, PathArrays pa, LaunchCfg cfg, void *stream);
int query_trace_pool(uint32_t block, uint32_t pool_slots, uint32_t lds_levels, uint32_t *lds_bytes, int *blocks);
#endif
// per-pixel accumulation in sample order, early-stop rule, pixel write, next active list
// persistent fused kernel with per-lane refill (ray generation source): every lane keeps its path to the end
// (guide: the GUIDE form, k_paths<false, .., GuidePathsDev>, which launch_paths / launch_tail launch when they are handed a guide and do not
// count; query_paths_blocks_per_cu then reports that form's occupancy)
int launch_paths(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PixelStateDev px, void *rad,
                 DevCounters *counters, bool count, LaunchCfg cfg, void *stream, const GuidePathsDev *guide = nullptr);
int query_paths_blocks_per_cu(uint32_t block, uint32_t lds_bytes, bool count, int *blocks, bool guide = false);
// split wavefront: persistent trace kernel (per-lane refill) ...
int launch_camera_tables(const SceneDev &sc, uint32_t n_inner, float ox, float oy, float oz, void *cam_inner,
                         void *cam_tris, uint32_t cus, void *stream);
// the per-pixel claims of a frame (pixel_claim.h) from the camera tables in wk: claims[local pixel], *n_claimed += the
// pixels with a slot or a miss claim (n_claimed[1]: the kernel's work head, zeroed by the caller like the count; the grid
// is persistent, query_pixel_claims_blocks_per_cu blocks per CU); lists (or NULL: none): the list records of the pixels without one; wk: cam_inner, cam_tris, lds_entries, overflow_entries, overflow_stack
// With lists the launch settles the empty records and leaves, per 8 x 8 tile, one word with the bits of the pixels whose
// list is still to be made and its popcount (pend_mask, pend_cnt: one per tile), their (cand, other) parked in their
// records; launch_live_compact lists them in tile order (entry = tile * 64 + lane) and launch_pixel_lists walks for them,
// one lane per entry: *count entries, *head zeroed by the caller, a persistent grid of query_pixel_lists_blocks_per_cu
// blocks per CU (wk as above, its overflow slab sized for that grid)
int launch_pixel_claims(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, unsigned int *claims, unsigned int *lists, unsigned int *n_claimed,
                        unsigned long long *pend_mask, unsigned int *pend_cnt, LaunchCfg cfg, void *stream);
int launch_pixel_lists(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, const unsigned int *entries, const unsigned int *count,
                       unsigned int *head, unsigned int *lists, LaunchCfg cfg, void *stream);
int query_pixel_claims_blocks_per_cu(uint32_t block, uint32_t lds_bytes, int *blocks);
int query_pixel_lists_blocks_per_cu(uint32_t block, uint32_t lds_bytes, int *blocks);
int launch_raygen(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PixelStateDev px, PathArrays pa, uint32_t cus, void *stream);
int launch_raygen_live(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PixelStateDev px, PathArrays pa, uint32_t cus, void *stream);
size_t live_compact_tmp_bytes(uint32_t nwords);
int launch_live_compact(const unsigned long long *live_mask, const unsigned int *live_cnt, uint32_t nwords,
                        unsigned int *offs, unsigned int *ids, unsigned int *count, void *tmp, size_t tmp_bytes, uint32_t cus, void *stream);
// the ordered lists of the slots [0, n_active) whose pixel has no claim / a claim, for a pass that fuses its claimed
// pixels: one word of "unclaimed" bits and its popcount per 64 slots (mask, cnt: n_pad / 64 words), then launch_slot_lists:
// set bits -> unclaimed, the other slots below n_active -> claimed; counts[0], counts[1] = the lists' lengths
int launch_slot_lists(const unsigned long long *mask, const unsigned int *cnt, uint32_t nwords, uint32_t n_active, unsigned int *offs,
                      unsigned int *unclaimed, unsigned int *claimed, unsigned int *counts, void *tmp, size_t tmp_bytes, uint32_t cus, void *stream);
int launch_unclaimed_words(const unsigned int *active, uint32_t n_active, uint32_t n_pad, const unsigned int *claims,
                           unsigned long long *mask, unsigned int *cnt, uint32_t cus, void *stream);
// ... and, in a run with list claims, of the walk slots: the unclaimed slots whose pixel has no list either (lists: the
// list records, kListWords words per local pixel).  One word of their bits and its popcount per 64 slots, then
// launch_live_compact: the ordered list and its length.  k_trace_w<0> works on that list and on the straggler list that
// k_raygen<0, true> leaves in wk.qids (ids, counts[0], sub_capacity) — launch_raygen launches that form when it is handed
// unclaimed, claim_lists and qids.ids; launch_trace_q's kernel takes the stragglers as its last source when qids.ids is
// set (nsrc = the bands + 1)
int launch_walk_words(const unsigned int *active, uint32_t n_active, uint32_t n_pad, const unsigned int *claims,
                      const unsigned int *lists, unsigned long long *mask, unsigned int *cnt, uint32_t cus, void *stream);
int launch_trace_q(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PixelStateDev px, PathArrays pa,
                   DevCounters *counters, bool count, bool from_queue, LaunchCfg cfg, void *stream, const GuideDev *guide = nullptr,
                   unsigned int *visits = nullptr);
// (guide: the GUIDE form of the bounce kernel, which launch_trace_q launches when it is handed a guide; visits, with a
// guide and hit records only: its counting form k_trace_w_visits, which leaves two words per path id there — the inner
// records and the triangle tests of the ray's guide walk)
int query_trace_q_blocks_per_cu(uint32_t block, uint32_t lds_bytes, bool count, bool from_queue, bool sorted, bool live, int *blocks,
                                bool guide = false);
// ... and the wide shading kernel: RayCast tail + Radiance step + id compaction
int launch_shade(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PixelStateDev px, PathArrays pa,
                 IdQueue qout, uint32_t max_chunks, DevCounters *counters, bool from_queue, uint32_t cus, void *stream);
int launch_shade_ends(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PathArrays pa, unsigned long long *full_mask,
                      unsigned int *full_cnt, uint32_t max_chunks, DevCounters *counters, bool from_queue, uint32_t cus, void *stream);
// follows every queued path (ids) to its end in one launch
int launch_tail(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PathArrays pa, DevCounters *counters,
                bool count, LaunchCfg cfg, void *stream, const GuidePathsDev *guide = nullptr);
int launch_radiance_init_ids(const float *o, const float *d, uint32_t n, uint64_t seed, PathArrays pa,
                             IdQueue qout, uint32_t cus, void *stream);
int launch_resolve(const FrameDev &fr, const unsigned int *active, uint32_t n_active, uint32_t samples,
                   bool pixel_major, const void *rad, const unsigned long long *rad_mask, PixelStateDev px, unsigned int *next_active,
                   unsigned int *next_count, float *out_rgbaz, DevCounters *counters, void *stream, bool moments = false);
// adaptive sampling of a progressive handle (vmx_sampling.inc; the arithmetic is stated in include/vermilion_hip.h)
// one word of bits and its popcount per 64 slots of `list` (nwords = ceil(n / 64)): slot i < n is set if its pixel lp =
// list[i] has cursor[lp] < kmax and (select == NULL or select[lp] != 0); launch_list_compact then writes the set slots'
// pixels to `dst` in order and their number to *count
int launch_list_words(const unsigned int *list, uint32_t n, const unsigned char *select, const unsigned int *cursor, uint32_t kmax,
                      unsigned long long *mask, unsigned int *cnt, void *stream);
int launch_list_compact(const unsigned long long *mask, const unsigned int *cnt, uint32_t nwords, unsigned int *offs,
                        const unsigned int *src, unsigned int *dst, unsigned int *count, void *tmp, size_t tmp_bytes, uint32_t cus, void *stream);
struct SamplingPass {
    uint32_t width, height;  // the handle's local image
    uint32_t kmax, min_samples, radius;
    float threshold, floor;
    PixelStateDev px;
};
int launch_sampling_error(const SamplingPass &a, float *error, float *variance, void *stream);
int launch_sampling_select(const SamplingPass &a, unsigned char *select, unsigned int *count, void *stream);
// BruteForceTracer::Render (integrators.cpp:9-186): one lane per pixel of `order` (tile-ordered local pixels)
int launch_bruteforce(const SceneDev &sc, const FrameDev &fr, const unsigned int *order, uint32_t npix, uint32_t flags,
                      float *out, DevCounters *counters, void *longs /* 64 bytes per pixel */, unsigned int *long_count,
                      const WorkDev &stack /* lds_entries, overflow_entries, overflow_stack */, LaunchCfg cfg, void *stream);
int launch_bruteforce_long(const SceneDev &sc, const FrameDev &fr, uint32_t flags, float *out, DevCounters *counters,
                           const void *longs, const unsigned int *long_count, uint32_t count, const WorkDev &stack,
                           LaunchCfg cfg, void *stream);
// progressive rendering (vmx_progressive_preview*): the frame of per-pixel state that may be unfinished; `finished` is the
// buffer k_resolve wrote the finished pixels to; out_rgbaz / rgba8: either may be NULL
int launch_preview(PixelStateDev px, uint32_t npix, uint32_t kmax, const float *finished, float *out_rgbaz, void *rgba8,
                   void *stream);
// G-buffer-guided a-trous filter (vmx_filter.inc; the arithmetic is stated in include/vermilion_hip.h)
// where the filter's first iteration reads its colours and its last one the alpha / depth it passes through: a W*H*5
// RGBAZ frame, or (frame == nullptr) the per-pixel state of a progressive render as k_preview shows it
struct FilterSrc {
    const float *frame;
    PixelStateDev px;
    const float *finished;  // the buffer k_resolve wrote the finished pixels to
    uint32_t kmax;
};
struct FilterPass {  // one iteration
    uint32_t width, height;
    uint32_t step;       // 1 << iteration
    uint32_t squarings;  // normal_squarings
    float isc2, kz;      // 1 / sigma_colour_it^2, sigma_depth * step
    const void *guide;   // float4 (n.xyz, z) per pixel
    FilterSrc src;
    const void *in_plane;  // float4 (r, g, b, -) per pixel: the input of every iteration but the first
    void *out_plane;       // ... and the output of every iteration but the last
    float *out_rgbaz;      // the last iteration's outputs, either may be NULL
    void *rgba8;
    bool first, last;
    float sl2;           // the variance-guided call: sigma_luminance * sigma_luminance (in the padding before the next pointer,
                         // so that every other member is where it was); its planes are (r, g, b, v)
    const void *albedo;  // float4 (a.rgb, -) per pixel or NULL: the demodulated call (last, so that every other member is where it was)
};
static_assert(sizeof(FilterPass) == 128, "FilterPass: a member moved (the kernels' argument offsets would)");
int launch_filter_guide(const void *rayhit, uint32_t npix, void *guide, void *stream);
int launch_atrous(const FilterPass &pass, void *stream);
// the demodulated call's pre-pass: pass.src / pass.albedo into pass.out_plane, which the first iteration then reads as a plane
int launch_demod_divide(const FilterPass &pass, void *stream);
// the variance-guided call (vmx_variance.inc): its pre-pass, (pass.src [/ pass.albedo], variance) into pass.out_plane, and
// one iteration from pass.in_plane
int launch_variance_pack(const FilterPass &pass, const float *variance, void *stream);
int launch_atrous_var(const FilterPass &pass, void *stream);
// G-buffer-guided upsampling (vmx_upsample.inc; the arithmetic is stated in include/vermilion_hip.h): one call
struct UpsamplePass {
    uint32_t width, height, low_width, low_height;
    uint32_t squarings;  // normal_squarings
    float sigma_depth;
    const void *guide_low, *guide_full;  // float4 (n.xyz, z) per pixel, as launch_filter_guide packs them
    const float *low;                    // the low RGBAZ frame
    float *out_rgbaz;                    // outputs, either may be NULL
    void *rgba8;
};
int launch_upsample(const UpsamplePass &pass, void *stream);
// the albedo plane of a camera (vmx_albedo.inc; the arithmetic is stated in include/vermilion_hip.h): sample q.sample
// of a run of n — k_query<kQueryCastCamera> (per-lane fetch) with cfg into `rec` (64 bytes per pixel, q.n = W * H), then k_albedo_finish
// into `plane` (float4 per pixel); first / last: of the run
int launch_albedo_sample(const SceneDev &sc, const QueryDev &q, const FrameDev &fr, void *rec, bool first, bool last,
                         uint32_t n, void *plane, LaunchCfg cfg, void *stream);
// temporal accumulation (vmx_temporal.inc; the arithmetic is stated in include/vermilion_hip.h)
struct TemporalCam {  // what proj reads of a FrameDev
    float m[9];       // m[col * 3 + row]
    float px, py, pz;
    float film_dist, sensor_x, sensor_y;
};
struct TemporalPass {  // one call
    uint32_t width, height;
    TemporalCam cam, hist_cam;  // this call's camera, the previous call's (not read by a first call)
    float normal_min, tol2, max_history;  // tol2 = plane_tol * plane_tol
    const void *rayhit;    // vmx_rayhit per pixel
    const float *in_rgbaz;
    const void *old_state;  // three float4 planes of W*H: (c_h.rgb, n_h) (n.xyz, z) (X.xyz, -); not read by a first call
    void *new_state;
    float *out_rgbaz;      // outputs, any may be NULL
    void *rgba8;
    float *history_len;
    bool first;
    const void *motion;    // vmx_motion per pixel or NULL (last, so that every other member is where it was); not read by a first call
    bool moments;          // a fourth plane of float2 (m1, m2) follows the three in both states (after `motion`, for the same reason)
};
int launch_temporal(const TemporalPass &pass, void *stream);
// adaptive temporal accumulation (vmx_adaptive.inc; the arithmetic is stated in include/vermilion_hip.h): a call that is
// no first call, as two passes — k_temporal_gather, the reprojection alone, into `plane`, and k_rectify, the window test,
// the cut and the blend
struct AdaptivePass {
    TemporalPass t;        // as launch_temporal takes it (first == false); out_rgbaz NULL for a call in place
    void *plane;           // float4 (hh.rgb, any ? nh : 0) per pixel, then with moments float2 (g1, g2) per pixel
    float *change;         // W*H floats or NULL
    float gamma2;          // gamma * gamma
    float min_support, sigma_depth;
    uint32_t squarings;    // normal_squarings
};
// store_in_place: the frame of a call in place (k_rectify leaves it alone, its r, g, b are copied from the new state
// afterwards) or NULL
int launch_adaptive(const AdaptivePass &pass, float *store_in_place, void *stream);
// the variance of a moments state (vmx_variance.inc; the arithmetic is stated in include/vermilion_hip.h)
struct VariancePass {
    uint32_t width, height;
    uint32_t squarings;     // normal_squarings
    float min_history, sigma_depth;
    const void *state;      // the state k_temporal<.., MOMENTS> just wrote: (c.rgb, n') (n.xyz, z) (X.xyz, -) and float2 (m1, m2)
    float *variance;        // W*H floats
};
int launch_variance(const VariancePass &pass, void *stream);
// motion records for refitted geometry (vmx_motion.inc; the arithmetic is stated in include/vermilion_hip.h)
constexpr uint32_t kMotionMoved = 1u;  // VMX_MOTION_MOVED
int launch_motion(const void *rayhit, uint32_t n, const float *pos_now, const float *pos_prev, const float *nrm_prev,
                  uint32_t ntris, void *out, void *stream);
// motion records for pixels on a moved analytic sphere (vmx_motion_spheres.inc; stated in include/vermilion_hip.h): the
// two tables of one call, passed to the kernel by value
struct SphereMotionDev {
    float now[kMaxSpheres][4];    // centre, radius of the table now
    float prev[kMaxSpheres][4];   // centre, radius before
    float nprev[kMaxSpheres][4];  // normal_centre before, normal_sign before as scene creation normalises it (-1.f / 1.f)
    uint32_t nspheres;
    uint32_t moved;               // bit i: sphere i differs between the two tables
    float ox, oy, oz;             // the G-buffer's common ray origin
};
int launch_motion_spheres(const void *rayhit, uint32_t n, const SphereMotionDev &tb, const void *motion_in, void *out,
                          void *stream);
// light sampling (vmx_nee.inc; the estimator is stated in include/vermilion_hip.h): the persistent kernel k_nee.  wk: heads
// (its first counter, zeroed before the launch), reserve and the stack fields; camera paths (o == NULL): active, n_active,
// samples, div_samples, and `items` = padded slots * samples path ids, numbered pixel-major as k_resolve reads `rad`;
// explicit rays (o, d): ray i on stream (fr.seed, i, 0), `items` of them, rad[i] its accumColour
// ed: the scene's emissive triangles (n == 0: none — the MESH = false instantiations, which never read it)
struct EmitRecord {  // what one area sample reads of its emitter: 64 bytes, one per emitter in the caller's order
    float v0[3], e1[3], e2[3];  // the triangle record's
    float rad[3];
    uint32_t slot;  // its leaf slot in the current tree
    uint32_t pad[3];
};
static_assert(sizeof(EmitRecord) == 64, "emitter record must be 64 bytes");
struct EmitDev {
    const EmitRecord *rec;
    const double *area, *weight, *cdf;  // [n]; cdf[n - 1] = W
    const int32_t *slot_em;             // [ntris] leaf slot -> emitter index, -1: not an emitter
    uint32_t n;
};
int launch_nee(const SceneDev &sc, const FrameDev &fr, const WorkDev &wk, PixelStateDev px, const float *o, const float *d,
               uint32_t items, void *rad, DevCounters *counters, LaunchCfg cfg, void *stream, const EmitDev &ed);
// the derived table (vmx_emitters.inc): k_emitter_slots, k_emitter_table, k_emitter_cdf from the scene's current records
int launch_emitter_table(const void *tris, uint32_t ntris, const uint32_t *ids, const float *radiance, int32_t *id_em,
                         const EmitDev &ed, void *stream);
// a budgeted step of a light-sampled progressive handle (o == NULL, wk.flat_ids != NULL): k_nee's third work source.
// wk.active / n_active: the step's pixel list; wk.flat_ids: the exclusive scan of the pixels' sample counts, n_active + 1
// entries, every count >= 1; `items` = its last entry; item i is sample i - base[s] of slot s, rad[i] its accumColour
int query_nee_blocks_per_cu(uint32_t block, uint32_t lds_bytes, bool rays, int *blocks, bool budgeted = false, bool mesh = false);
// ... and its fold: k_resolve's statements over rad[base[s] + j], j < base[s + 1] - base[s], per slot s in order
int launch_resolve_budget(const FrameDev &fr, const unsigned int *active, uint32_t n_active, const unsigned int *base, const void *rad,
                          PixelStateDev px, unsigned int *next_active, unsigned int *next_count, float *out_rgbaz, DevCounters *counters,
                          void *stream, bool moments);
// per-pixel sample budgets of a moments handle (vmx_sampling.inc; the rule is stated in include/vermilion_hip.h): budget[p]
// for every local pixel, *total (or NULL; zeroed by the caller) += their sum
struct BudgetPass {
    SamplingPass a;
    uint32_t cap;  // min(max_step, B) or B
};
int launch_sampling_budget(const BudgetPass &b, unsigned int *budget, unsigned long long *total, void *stream);
// launch_list_words over a word map: slot i < n is set if its pixel lp = list[i] has cursor[lp] < kmax and budget[lp] != 0
int launch_list_words_budget(const unsigned int *list, uint32_t n, const unsigned int *budget, const unsigned int *cursor, uint32_t kmax,
                             unsigned long long *mask, unsigned int *cnt, void *stream);
// the step's sample counts and their exclusive scan: cnt[s] = min(budget[list[s]], B, kmax - cursor) for s < *len, 0 for
// *len <= s <= n_max; base[0 .. n_max] their exclusive sums, so base[*len] = base[n_max] = the step's items
size_t item_base_tmp_bytes(uint32_t n_max);
int launch_item_base(const unsigned int *list, const unsigned int *len, uint32_t n_max, const unsigned int *budget,
                     const unsigned int *cursor, uint32_t kmax, uint32_t B, unsigned int *cnt, unsigned int *base, void *tmp,
                     size_t tmp_bytes, void *stream);
int launch_quantize(const float *frame, uint64_t npix, void *rgba8, float *depth, void *stream);
int launch_assemble(const float *gathered, uint64_t rank_stride_floats, uint32_t width, uint32_t height,
                    uint32_t stripe_rows, uint32_t world, float *frame, void *stream);

// ---- live-path reordering between bounce generations (path_sort.hip) -----------------------------
struct SortKeyCfg {
    float lo[3], inv[3];  // scene bounds: cell = (o - lo) * inv in [0,1)
    uint32_t obits;       // bits per axis of the origin cell (Morton-interleaved), 0 = no origin part
    uint32_t dbits;       // bits per axis of the octahedral direction cell, 0 = no direction part
    uint32_t dir_major;   // 1: direction cell in the high bits
    uint32_t chunk_log2;  // > 0: key = (queue position >> chunk_log2, direction cell): direction order inside chunks
};
size_t path_sort_tmp_bytes(uint32_t max_n);
// sorts every sub-queue of `q` (h_counts[kSubQueues] entries each) by the key of its paths' next rays into ids_out
// (same sub-queue layout); keys_a / keys_b: scratch of the queue's size
int path_sort_ids(const IdQueue &q, const uint32_t *h_counts, const void *state, const SortKeyCfg &cfg,
                  unsigned int *keys_a, unsigned int *keys_b, unsigned int *ids_out, void *tmp, size_t tmp_bytes,
                  void *stream);

}  // namespace vmx
