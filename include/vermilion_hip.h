/*
 * vermilion_hip.h — C ABI of the MI355X (gfx950) path-tracing hot path.
 *
 * This is the drop-in boundary for Vermilion's `Integrator::Render` seam
 * (reference: core/integrators/integrators.h:11-16, installed through
 * RenderEngine::assignIntegrator, core/engines/renderEngine.cpp:70-78, and
 * called from RenderEngine::draw, core/engines/renderEngine.cpp:163-164).
 * A `HipPathTracer : Vermilion::Integrator` adapter flattens
 * MeshEngine::sceneMeshes in createBVH order (core/engines/meshEngine.cpp:660-718)
 * into plain float arrays and calls the functions below; everything else
 * (Assimp import, OIIO texture read / image write, logging) stays on the host.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ / torch types cross this boundary
 *   - every function returns an int status (VMX_OK == 0); the message for the
 *     last failure on the calling thread is vmx_last_error()
 *   - nothing throws across the ABI; the library never falls back to a CPU
 *     path: without a usable HIP device every compute entry point fails with
 *     VMX_ERR_NO_DEVICE
 *   - synchronous and blocking unless a stream is passed explicitly
 *     (reference Render is one synchronous call, renderEngine.cpp:163-164)
 */
#ifndef VERMILION_HIP_H
#define VERMILION_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VMX_ABI_VERSION 2 /* 2: vmx_camera.rotation_units / rotation_rad, vmx_multi_timings */

/* status codes */
#define VMX_OK 0
#define VMX_ERR_INVALID 1     /* bad argument (NULL, zero size, NaN geometry ...)  */
#define VMX_ERR_NO_DEVICE 2   /* no HIP device / device ordinal out of range        */
#define VMX_ERR_HIP 3         /* a hip* call failed; text in vmx_last_error()       */
#define VMX_ERR_DEPTH 4       /* BVH deeper than the reference's 64-entry traversal
                                 stack (core/accelerators/bvh.cpp:54)               */
#define VMX_ERR_NOMEM 5

/* sphere flags */
#define VMX_SPHERE_EMIT 1u /* hit writes `colour` into hitColour (meshEngine.cpp:382-383,415-416) */

/* sampling modes (vmx_opts.sampling) */
#define VMX_SAMPLING_PARITY 0u    /* r2 = 10*U, reference-faithful (pathtracer.cpp:156,170) */
#define VMX_SAMPLING_CORRECTED 1u /* r2 = U, an actual cosine-weighted lobe; not a parity mode */
#define VMX_SAMPLING_MODE_MASK 0xFFu
/* Flag, OR-ed into vmx_opts.sampling.  pathtracer.cpp:155,162 call the unqualified cos(r1) / sin(r1) with a
 * `float r1`.  Default reading: <cmath>'s float overloads are visible in the global namespace (the premise
 * under which integrators.cpp:170's abs(float) is std::abs(float), see VMX_BF_ABS_INT), so these are
 * cosf / sinf — evaluated on the device by glibc's algorithm (sysdeps/ieee754/flt-32/s_sinf.c, s_cosf.c),
 * the libm the reference links on Linux.  With this flag they are C's `double cos(double)` / `sin` of the
 * widened argument, narrowed to float.  The two readings differ in the last bit for ~1.3 % of the arguments
 * (uniform in [0, 2 pi)); of 10^6 paths' radiance none differed (tests/test_oracle.py). */
#define VMX_SAMPLING_LIBM_DOUBLE 0x100u
/* Flag, OR-ed into vmx_opts.sampling; OFF by default.  Under the reference's sampling (r2 = 10 U, pathtracer.cpp:156,170)
 * nine in ten diffuse bounces produce a NaN direction and end the path.  A Radiance step adds
 * accumRadiance * hitColour (pathtracer.cpp:43), and hitColour is non-zero only where the hit — or a nearer-so-far test on
 * the way (meshEngine.cpp:377-420) — is a light sphere.  Whether a step is the path's last one whatever it hits is
 * decided by the path's own random draws alone (Russian roulette :56, the specular test :98 and r2 :156 / :170, for both
 * values of the material flag), and whether a light sphere can colour it by the ray alone.  With this flag a ray whose
 * step is provably the last one and cannot meet a light sphere is not traced — camera rays and bounce rays alike, 78 % of
 * all rays of a parity frame: the frame is bit-identical (Camera::mImage holds r,g,b and the sample count,
 * camera.cpp:106-113 — the primary hit distance Radiance also returns, :44-47, is not part of it), but
 * vmx_stats.rays_primary / rays_secondary count only the rays that were traced, so throughput figures are not comparable
 * with the default.  Applies to vmx_render* (split-wavefront and fused passes; not to vmx_radiance, whose output includes
 * that distance, nor to a call with collect_counters, whose totals are the reference's).  With VMX_SAMPLING_CORRECTED
 * (r2 = U) only Russian roulette past depth 5 ever ends a path by its draws alone and the flag changes little. */
#define VMX_SAMPLING_ELIDE_DEAD 0x200u

/*
 * One analytic sphere of MeshEngine::RayCast's hard-coded table
 * (core/engines/meshEngine.cpp:377-500).  Spheres are tested after the BVH,
 * in table order, each with `testHit > 0 && testHit < nearestHit`
 * (meshEngine.cpp:378); a nearer sphere overwrites the hit normal with
 *   normal_sign * normalize(hit - normal_centre)
 * and, if VMX_SPHERE_EMIT is set, overwrites hitColour with `colour`.
 * hitColour is never cleared by a later, nearer sphere (quirk kept on purpose).
 */
typedef struct vmx_sphere {
    float centre[3];
    float radius;
    float colour[3];
    uint32_t flags;
    float normal_centre[3];
    float normal_sign; /* +1 or -1 */
} vmx_sphere;

/*
 * Camera parameters = Vermilion::cameraSettings (core/camera/camera.h:32-47)
 * restricted to the fields PathTracer::Render reads.  The library applies the
 * Camera constructor's conversion (core/camera/camera.cpp:43-47):
 *   mRotation = (-rx, -ry, +rz) * 3.1415926535 / 180.
 */
#define VMX_ROTATION_DEGREES 0u /* rotation_deg = cameraSettings.rotation; the library applies camera.cpp:43-47 */
#define VMX_ROTATION_RADIANS 1u /* rotation_rad = Camera::mRotation as it stands (already negated in x, y and in
                                   radians): what an Integrator holds — PathTracer::Render reads mRotation, not the
                                   settings (pathtracer.cpp:219-221) — passed through without a degree round trip */
typedef struct vmx_camera {
    float position[3];     /* cameraSettings.position                        */
    float rotation_deg[3]; /* cameraSettings.rotation (degrees); read when rotation_units == VMX_ROTATION_DEGREES */
    float back_distance;   /* cameraSettings.fBackDistance -> mDistToFilm    */
    float back_size[2];    /* cameraSettings.fBackSizeX/Y  -> sensorSizeX/Y  */
    uint32_t image_res[2]; /* imageResX, imageResY                           */
    uint32_t rays_per_pixel; /* raysPerPixel -> uSamplesPerPixel             */
    uint32_t rotation_units; /* VMX_ROTATION_DEGREES (0, the default of a zeroed struct) or VMX_ROTATION_RADIANS */
    float rotation_rad[3]; /* Camera::mRotation (camera.h, set at camera.cpp:43-47); read when rotation_units ==
                              VMX_ROTATION_RADIANS: the three angles glm::rotate gets at pathtracer.cpp:219-221 */
} vmx_camera;

typedef struct vmx_opts {
    uint64_t seed;         /* the reference seeds from std::random_device (pathtracer.cpp:231);
                              here the stream of sample k of pixel p is keyed by (seed, p, k) */
    uint32_t early_stop;   /* 1: reference early-stop rule (pathtracer.cpp:290-311); 0: fixed spp */
    uint32_t sampling;     /* VMX_SAMPLING_PARITY / _CORRECTED, | VMX_SAMPLING_LIBM_DOUBLE | VMX_SAMPLING_ELIDE_DEAD */
    uint32_t rank;         /* image-stripe sharding: this call renders the stripes s   */
    uint32_t world;        /*   with s % world == rank; world 0 or 1 = whole image     */
    uint32_t stripe_rows;  /* rows per stripe; 0 -> 16                         */
    uint32_t samples_per_batch; /* fixed-spp mode: samples per pixel in flight per pass; 0 -> auto */
    uint32_t collect_counters;  /* 1: also count inner-node visits / triangle tests
                                   (instrumented kernels, slower; for roofline accounting) */
    uint32_t reserved[7];  /* 0 unless tuning: [0] pipeline form (bits 0-7: 0 default routing, 1 fused kernel for every
                              pass, 4 split wavefront for every pass; bit 8: plain one-phase shading; bit 9: two-phase
                              shading through k_shade_ends instead of rays sorted by the traversal kernel; bit 11: no
                              per-pixel claims for the camera rays; bit 12: the rays of a claimed pixel go through ray
                              generation, traversal and shading kernels as the others do, instead of being formed, tested
                              and shaded in the shading kernel alone; bit 13: no list claims for the pixels without a
                              claim; bit 14: bounce rays walk the reference tree alone, not the scene's guide tree),
                              [1] max paths per pass, [2] tail threshold, [3] refill_min, [4] shade_min,
                              [5] bounce reordering key (A/B library only), [6] LDS stack levels — all forms and
                              settings produce the same frame (see vmx_host.h: kForm*, api_render.inc: render_forms, make_tuning) */
} vmx_opts;

/* per-stage figures: `primary` = Radiance steps taken at depth 0 (the fused
 * raygen + trace + shade kernel), `bounce` = every later step */
typedef struct vmx_stage_stats {
    uint64_t rays;          /* RayCast-equivalents with a finite direction            */
    uint64_t inner_visits;  /* inner-node visits (both child boxes tested); 0 unless collect_counters */
    uint64_t tri_tests;     /* Moller-Trumbore tests; 0 unless collect_counters       */
    uint64_t tri_hits;      /* rays whose BVH query hit a triangle                    */
    uint64_t continued;     /* path states written across a bounce boundary           */
    uint64_t launches;      /* kernel launches of this stage                          */
    double ms;              /* sum of hipEvent durations of those launches            */
} vmx_stage_stats;

typedef struct vmx_stats {
    uint64_t rays_primary;      /* = primary.rays                                      */
    uint64_t rays_secondary;    /* = bounce.rays (NaN directions are not rays)         */
    uint64_t samples;           /* pixel samples accumulated into the image            */
    uint64_t samples_discarded; /* speculative samples traced but dropped by early stop */
    uint64_t passes;            /* sample batches processed                            */
    uint64_t kernel_launches;   /* approximate, and the one count that depends on the pipeline form: a claim table adds
                                   one, the lists of a pass with fused claimed pixels (reserved[0] bit 12 clear) four */
    double ms_total;            /* wall time of the call, host clock                   */
    double ms_device;           /* hipEvent time of the device work on the render stream */
    vmx_stage_stats primary; /* ms/launches: the depth-0 traversal kernel                  */
    vmx_stage_stats bounce;  /* ms/launches: bounce traversal kernels + the tail kernel    */
    vmx_stage_stats shade;   /* ms/launches only: the shading kernels of the split wavefront */
} vmx_stats;

/* per-kernel device time (hipEvent pairs on the render stream) of the LAST render / radiance call on
 * a scene: what bench.py's roofline object is computed from (the dominant kernel of a step) */
#define VMX_K_RAYGEN 0        /* k_raygen (+ live-path list under VMX_SAMPLING_ELIDE_DEAD, + the slot lists of a pass with fused claimed pixels) */
#define VMX_K_TRACE_CAMERA 1  /* k_trace_w<0>: BVH traversal of the camera rays            */
#define VMX_K_SHADE_CAMERA 2  /* k_shade<0> (with k_shade_ends<0> + list compaction where used) */
#define VMX_K_TRACE_BOUNCE 3  /* k_trace_w<1>: BVH traversal of the bounce generations     */
#define VMX_K_SHADE_BOUNCE 4  /* k_shade<1> (with k_shade_ends<1> + list compaction where used) */
#define VMX_K_TAIL 5          /* k_paths<2>: fused kernel that finishes the last generations */
#define VMX_K_FUSED 6         /* k_paths<0>: whole small passes in one fused kernel        */
#define VMX_K_RESOLVE 7       /* k_resolve                                                 */
#define VMX_K_BRUTEFORCE 8    /* k_bruteforce                                              */
#define VMX_K_OTHER 9         /* k_pixel_claims; k_nee (vmx_render_nee*, vmx_radiance_nee); first-generation kernels (pipeline forms 2, 3) */
#define VMX_K_COUNT 10
typedef struct vmx_timings {
    double ms[VMX_K_COUNT];          /* summed over the launches of the call */
    double longest_ms[VMX_K_COUNT];  /* the longest single launch            */
    uint64_t launches[VMX_K_COUNT];
} vmx_timings;

typedef struct vmx_scene_desc {
    uint32_t ntris;
    uint32_t nspheres;
    uint32_t leaf_size;
    uint32_t n_nodes;      /* reference flat-tree node count (bvh.cpp:203)   */
    uint32_t n_leaves;     /* bvh.cpp:221                                    */
    uint32_t n_inner;      /* 2-wide records on the device                   */
    uint32_t max_depth;    /* root = 0                                       */
    uint32_t stack_entries;/* per-lane LDS stack entries the kernels use     */
    uint64_t device_bytes; /* HBM held by the scene                          */
    int32_t device;
    uint32_t pad;
} vmx_scene_desc;

/* full output tuple of MeshEngine::RayCast (meshEngine.cpp:239-509) for one ray */
typedef struct vmx_rayhit {
    float location[3]; /* pHitLocation                                         */
    float distance;    /* pHitDistance (INFINITY on a miss)                    */
    float normal[3];   /* pHitNormal                                           */
    int32_t tri_id;    /* createBVH push-order index of the BVH hit, -1 if none */
    float uv[2];       /* pHitTexCoord                                         */
    float tri_t;       /* BVH t (999999999.f if none), bvh.cpp:48              */
    uint32_t flags;    /* bit0: return value (nearest < INF); bit1: material non-null */
    float colour[3];   /* pHitColour                                           */
    uint32_t pad;
} vmx_rayhit;

typedef struct vmx_scene vmx_scene;

/* ---- library ---------------------------------------------------------- */
int vmx_abi_version(void);
const char *vmx_last_error(void);
/* number of HIP devices visible to the library (0 if none / runtime missing) */
int vmx_device_count(void);

/* The reference's eight spheres (meshEngine.cpp:377-500): 2 lights + 6 walls. */
const vmx_sphere *vmx_default_spheres(uint32_t *count);

/* ---- scene ------------------------------------------------------------ */
/*
 * Replaces MeshEngine::createBVH + BVH::BVH/build (meshEngine.cpp:649-724,
 * bvh.cpp:155-279) for the device: `pos`/`nrm` are [ntris*9] floats
 * (v0,v1,v2 / n0,n1,n2 per triangle), `uv` is [ntris*6] or NULL (zeros),
 * in createBVH push order — that order defines triangle IDs.
 * spheres == NULL && nspheres == 0 selects vmx_default_spheres(); a non-NULL
 * pointer with nspheres == 0 means no spheres at all.
 * leaf_size 0 -> 4 (bvh.h:29).  The BVH is built on the host with the
 * reference's topology, flattened to 2-wide records and uploaded to `device`.
 */
int vmx_scene_create(const float *pos, const float *nrm, const float *uv, uint32_t ntris,
                     const vmx_sphere *spheres, uint32_t nspheres, uint32_t leaf_size,
                     int device, vmx_scene **out);
/* BVH builders for vmx_scene_create_ex */
#define VMX_BVH_REFERENCE 0u /* BVH::build's topology (bvh.cpp:179-279): triangle-ID / tie parity        */
#define VMX_BVH_SAH 1u       /* binned-SAH quality tree: same triangle tests and nearest
                                distance, but exact-distance ties and `near > t` pruning follow ITS order */
#define VMX_BVH_LBVH 2u      /* linear BVH built on the GPU (Morton sort, Karras hierarchy, bottom-up fit):
                                for scenes that change per frame; same caveat as SAH.  Many coincident
                                centroids can make the tree deeper than the 64-entry traversal stack the
                                reference allows (bvh.cpp:54): VMX_ERR_DEPTH, use another builder */
#define VMX_BVH_PLOC 3u      /* quality tree built on the GPU by parallel locally-ordered clustering (Morton
                                sort, rounds of nearest-neighbour merging within 16 positions): close to the SAH
                                tree's visit counts at a few ms per build; same caveat as SAH */
int vmx_scene_create_ex(const float *pos, const float *nrm, const float *uv, uint32_t ntris,
                        const vmx_sphere *spheres, uint32_t nspheres, uint32_t leaf_size, uint32_t builder,
                        int device, vmx_scene **out);
int vmx_scene_destroy(vmx_scene *scene);
/*
 * Replaces MeshEngine::bindTexture (meshEngine.cpp:74-93) minus the OpenImageIO read: `data` is the
 * float image bindTexture would hand to VermiTexture (height rows of width texels of `channels`
 * floats, 1..4 channels, width/height <= 65535 as VermiTexture stores uint16_t).  Only the FIRST
 * bound texture is ever sampled by the path tracer (pathtracer.cpp:63-66: boundTextures[0], wrap
 * + nearest, meshEngine.cpp:21-46); the SECOND one is kept for BruteForceTracer, which reads
 * boundTextures[1] as its albedo (integrators.cpp:141-147); later calls are counted and otherwise
 * ignored, as there.
 */
int vmx_scene_bind_texture(vmx_scene *scene, const float *data, uint32_t width, uint32_t height,
                           uint32_t channels);
int vmx_scene_describe(const vmx_scene *scene, vmx_scene_desc *out);
int vmx_scene_timings(const vmx_scene *scene, vmx_timings *out);
/*
 * The number of compute units the scene sizes its launches for: the device's own count, or less under
 * VMX_CU_LIMIT (0 for a NULL scene).  Two environment variables are read by the library, both diagnostic:
 *   VMX_MEM_BUDGET_MB  lowers the memory a render's passes are sized for (read per render);
 *   VMX_CU_LIMIT       read once when a scene is created: the scene counts min(device's units, limit) compute
 *                      units, so its persistent grids, block-stride grids and the buffers sized from them are
 *                      those of a smaller device.  It can only lower the count — unset, empty, 0, unparsable or
 *                      at least the device's count leave the device's — and it changes no result: every kernel
 *                      hands out its work on the device and none synchronises across blocks.
 */
uint32_t vmx_scene_compute_units(const vmx_scene *scene);
/*
 * Host-side BVH topology in the reference's flat layout (bvh.h:11-14): per
 * node start, nPrims, rightOffset ([n_nodes] each, any may be NULL), bbox
 * [n_nodes*6] (min,max) and the final build_prims permutation [ntris].
 */
int vmx_scene_bvh(const vmx_scene *scene, uint32_t *start, uint32_t *nprims,
                  uint32_t *right_offset, float *bbox, uint32_t *prim_order);

/* ---- moving geometry: in-place updates ----------------------------------
 * New positions, normals and / or uvs for the SAME triangles: pos / nrm [ntris*9], uv [ntris*6], in the createBVH
 * order of the scene's creation (triangle IDs keep their meaning); ntris must be the scene's count (another count or
 * order is a new scene).  Each of pos / nrm / uv may be NULL, which KEEPS that attribute — unlike creation, where a
 * NULL uv means zeros; all three NULL is VMX_ERR_INVALID.  Updating only nrm / uv does no box work.
 *
 * VMX_UPDATE_REFIT: the tree's nodes, leaves and prim_order stay; every box becomes the tight union of its triangles'
 *   new vertices, and the triangle / attribute records are rewritten with the float operations of a fresh build (a
 *   rewritten record is bit-identical to the one a build writes for that triangle).  The scene then behaves exactly
 *   like the OLD topology with tight boxes over the new positions.  A refitted VMX_BVH_REFERENCE tree is therefore no
 *   longer the reference's topology for the new positions: its parity bar becomes that of SAH / LBVH / PLOC — the
 *   reference's traversal over the exported tree.  Boxes loosen as vertices move: see VMX_UPDATE_REBUILD.
 * VMX_UPDATE_REBUILD: runs the scene's own builder again on the new positions, in place: export and frames are
 *   bit-identical to a fresh vmx_scene_create_ex on the same arrays.  Built into new buffers that replace the old ones
 *   only when the build succeeds; everything sized from the tree's depth (stack entries, block size, the render and
 *   query workspaces' overflow stacks) follows.
 *
 * A failed update leaves the scene exactly as it was: non-finite positions (host variant), a wrong ntris, unknown
 * flags, a REBUILD whose tree exceeds the 64-entry stack (VMX_ERR_DEPTH).
 *
 * Ordering: an update waits for the scene's last query before it writes a record.  Every later render (path tracer and
 * BruteForceTracer), query, parity hook and flat export of the scene waits for the update, whatever stream either runs
 * on.  vmx_scene_bvh / vmx_scene_describe report the refitted boxes (topology arrays and prim_order unchanged).
 */
#define VMX_UPDATE_REFIT 0u   /* keep the tree's topology, recompute every box from the new positions */
#define VMX_UPDATE_REBUILD 1u /* run the scene's own builder again on the new positions, in place      */
/* HOST arrays; returns once the scene is updated.  Positions are checked as vmx_scene_create checks them.  The first
 * update that moves vertices derives the refit plan from the tree (creation time and memory are unchanged); the host
 * variant keeps a device staging buffer of ntris * 96 bytes after its first call. */
int vmx_scene_update(vmx_scene *scene, const float *pos, const float *nrm, const float *uv, uint32_t ntris,
                     uint32_t flags);
/* DEVICE arrays of the scene's device (checked as vmx_query_device checks its pointers), enqueued on `stream` (a
 * hipStream_t; NULL = the scene's stream).  Positions are not validated: finite positions are the caller's
 * precondition.  A REFIT returns without synchronising (except the scene's first, which derives the refit plan); the
 * arrays must stay valid until it completes on `stream`.  VMX_UPDATE_REBUILD is accepted for VMX_BVH_LBVH / _PLOC
 * only (the device builders read the arrays where they are) and blocks: the depth check needs the root's height on
 * the host.  For VMX_BVH_REFERENCE / _SAH it is VMX_ERR_INVALID: use vmx_scene_update. */
int vmx_scene_update_device(vmx_scene *scene, const void *d_pos, const void *d_nrm, const void *d_uv, uint32_t ntris,
                            uint32_t flags, void *stream);

/* ---- changing lights: the sphere table of a live scene ---------------------
 * All light comes from the analytic sphere table.  vmx_scene_set_spheres replaces it in place: dim, recolour or move a
 * light, move a wall, or change the count, without building or uploading the scene again.  (spheres, nspheres) mean
 * exactly what they mean to vmx_scene_create_ex: NULL, 0 selects vmx_default_spheres(); a non-NULL pointer with
 * nspheres == 0 means no spheres at all; NULL with nspheres > 0, or more than 16 spheres, is VMX_ERR_INVALID; normal_sign
 * is read as -1 if negative and +1 otherwise, and rad*rad is the float product.  The count may change between calls.
 * After the call the scene renders, casts and answers exactly as a scene created with that table does, bit for bit:
 * nothing derived from the old table outlives it (the emitter prefix, the per-run claim tables and pixel-sphere bounds,
 * the rays' "light in reach" notes).
 *
 * Checks that need no device come first, in this order: the (spheres, nspheres) pair, then the NULL handle.
 * HOST array; returns once the table is written.  Ordering is vmx_scene_update's: the write waits for the scene's last
 * query and last update, whatever stream they ran on (a render or parity hook has returned before, and a progressive step
 * likewise); every later render (path tracer and BruteForceTracer), vmx_raycast*, vmx_query*, vmx_albedo_camera_device,
 * vmx_radiance and parity hook waits for it.  Like a geometry update it ends the progressive handles begun before it:
 * their next step is VMX_ERR_INVALID ("scene updated since vmx_progressive_begin"); handles begun afterwards see the new
 * table.  A failed call leaves the scene exactly as it was.  vmx_scene_describe reports the new count.
 * Temporal accumulation: a dimmed or recoloured light is what vmx_temporal_accumulate_adaptive_device is for; a sphere
 * that MOVED is followed by vmx_motion_spheres_device (below, "motion records").
 */
int vmx_scene_set_spheres(vmx_scene *scene, const vmx_sphere *spheres, uint32_t nspheres);

/* ---- parity hooks (explicit ray batches, host buffers) ----------------- */
/* BVH::getIntersection (bvh.cpp:47-145): tri_id[n] (-1 = miss), t[n] */
int vmx_trace(const vmx_scene *scene, const float *origin, const float *dir, uint32_t n,
              int32_t *tri_id, float *t);
/* MeshEngine::RayCast (meshEngine.cpp:239-509) */
int vmx_raycast(const vmx_scene *scene, const float *origin, const float *dir, uint32_t n,
                vmx_rayhit *out);
/* ---- device ray queries (explicit ray batches) --------------------------
 * The query side of the reference's MeshEngine / BVH, served by a persistent traversal kernel (k_query).
 * Rays: origin[n*3], dir[n*3] f32 packed like vmx_trace; tmax[n] f32 or NULL (no bound).
 * Outputs (any may be NULL, at least one non-NULL when n > 0): tri_id[n] int32 (createBVH order, -1 = miss),
 * t[n] f32, hit[n] uint8 (0 / 1).  Spheres are not part of any mode (neither BVH::getIntersection nor
 * RayCastCollision sees them, meshEngine.cpp:201).
 *
 * With L = min(tmax, 999999999.f) (the reference's initial intersection->t, bvh.cpp:48; L = 999999999.f when
 * tmax is NULL, +inf or larger):
 *   - a ray with !(tmax > 0) (<= 0 or NaN) is a miss and is not traversed: tri_id -1, t = tmax, hit 0
 *   - VMX_QUERY_NEAREST: BVH::getIntersection(occlusion == false) with the running nearest distance starting at L
 *     instead of 999999999.f; same box tests, near-first order, strict `<` tie rule and NaN behaviour.  tri_id,
 *     t (L on a miss), hit = tri_id >= 0.  So with (id, t) = vmx_trace's result: (t < L ? (id, t) : (-1, L)) —
 *     except for L a few ulps above t, where a box's slab `near` can exceed the triangle's t and the box is pruned:
 *     then a miss (-1, L) is possible (never another triangle).
 *   - VMX_QUERY_ANY: occlusion == true (bvh.cpp:83-86): the first triangle Triangle::getIntersection accepts with
 *     dist < L ends the ray; nodes with near > L are pruned.  hit only (tri_id or t non-NULL: VMX_ERR_INVALID);
 *     hit == (vmx_trace's id >= 0 && its t < L).  Known difference: the reference's occlusion mode also accepts
 *     a triangle beyond 999999999 found in a node it did not prune; that matters only for geometry ~1e9 away.
 *   - VMX_QUERY_COLLISION: MeshEngine::RayCastCollision (meshEngine.cpp:196-206; public, meshEngine.h:114): NEAREST,
 *     then hit = tri_id >= 0 && t > 1e-3, the float t compared with the DOUBLE 1e-3 — in float that is
 *     t >= 1e-3f.  tri_id / t, if asked for, are the nearest hit that was judged.
 */
#define VMX_QUERY_NEAREST 0u   /* BVH::getIntersection(occlusion == false), bvh.cpp:47-145              */
#define VMX_QUERY_ANY 1u       /* occlusion == true (bvh.cpp:83-86): stop at the first accepted triangle   */
#define VMX_QUERY_COLLISION 2u /* MeshEngine::RayCastCollision (meshEngine.cpp:196-206)                   */
/* Flag, OR-ed into the mode; tuning only, same results: each lane reads its own 64-byte node / triangle record
 * instead of the quad-cooperative fetch the kernel uses by default (profiles/query_bench.txt has both). */
#define VMX_QUERY_FETCH_PER_LANE 0x100u
/* All pointers are DEVICE memory of the scene's device (checked with hipPointerGetAttributes: anything else is
 * VMX_ERR_INVALID before any launch).  Enqueued on `stream` (a hipStream_t; NULL = the scene's stream); returns
 * without synchronising.  The query workspace (work counter, stack overflow slab) is allocated on a scene's first
 * query and reused: no allocation after that.  Queries of one scene on different streams are ordered by enqueue
 * (each waits on an event the previous one recorded), so they never share the workspace while in flight. */
int vmx_query_device(const vmx_scene *scene, uint32_t mode, const void *d_origin, const void *d_dir,
                     const void *d_tmax, uint32_t n, void *d_tri_id, void *d_t, void *d_hit, void *stream);
/* Same with HOST buffers: copies in, runs the device path on the scene's stream, copies out, synchronises. */
int vmx_query(const vmx_scene *scene, uint32_t mode, const float *origin, const float *dir, const float *tmax,
              uint32_t n, int32_t *tri_id, float *t, uint8_t *hit);
/* ---- MeshEngine::RayCast of device batches -------------------------------
 * The whole hit record (meshEngine.cpp:239-509: BVH nearest hit, shading normal, uv, the sphere table) for device
 * rays, without copies through the host.  out[n] vmx_rayhit is byte for byte what vmx_raycast returns for the same
 * rays (pad = 0); no bound: the reference's RayCast has none.  Served by the query kernel (unbounded NEAREST, which
 * leaves (tri_t, leaf slot) in each record) and a dense finish kernel (normal, uv, spheres, the rest of the record).
 * flags: 0 or VMX_QUERY_FETCH_PER_LANE (same meaning as in vmx_query_device, same results); anything else is
 * VMX_ERR_INVALID.  Pointers follow vmx_query_device's rules (DEVICE memory of the scene's device, checked before any
 * launch); in addition d_out must be 16-byte aligned and must not overlap the rays.  n > 2^31 - 1 is VMX_ERR_INVALID,
 * n == 0 is VMX_OK with no launch.  Enqueued on `stream` (NULL = the scene's stream), no synchronisation: ordered
 * with the scene's queries and updates exactly as vmx_query_device (same workspace and event); no allocation after
 * the scene's first query. */
int vmx_raycast_device(const vmx_scene *scene, const void *d_origin, const void *d_dir, uint32_t n, void *d_out,
                       uint32_t flags, void *stream);
/* The same for sample k's camera ray of every pixel — the ray vmx_render traces for that sample and vmx_primary_ids
 * reports (origin = cam->position): a device G-buffer, out[W*H] vmx_rayhit in pixel order p = y*W + x.  cam / opts
 * are checked as vmx_render checks them (rays_per_pixel >= 4, rotation_units); only opts->seed is used, and
 * opts->world > 1 is VMX_ERR_INVALID (whole images only).  k < 4 * (rays_per_pixel / 4), as in vmx_primary_ids. */
int vmx_raycast_camera_device(const vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts, uint32_t k,
                              void *d_out, uint32_t flags, void *stream);

/*
 * Primary-hit AOV: generates sample k's camera ray of every pixel on the
 * device (pathtracer.cpp:251-280) and returns BVH::getIntersection's result,
 * tri_id[W*H] / t[W*H] in pixel order (the "primary-hit triangle ID" map).
 */
int vmx_primary_ids(const vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts, uint32_t k,
                    int32_t *tri_id, float *t);

/* Debug entry: the per-pixel claims a render of this camera would use for its camera rays (one 32-bit word per pixel of
 * this rank's rows, packed as vmx_render packs them): 0xFFFFFFFF none, 0xFFFFFFFE "no camera ray of the pixel hits a
 * triangle", else the leaf-order slot (vmx_scene_bvh's prim_order index) of the one triangle every camera ray of the
 * pixel hits.  Built whatever the sample count; *n_claimed = pixels with a claim.  Either output may be NULL. */
int vmx_pixel_claims(const vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts, uint32_t *claims_out,
                     uint32_t *n_claimed);
/* Debug entry: how many camera paths of the last render call on this scene (vmx_render*, a vmx_progressive step) took the
 * fused route — the paths of claimed pixels in a one-phase split pass (reserved[0] bit 8) of a multiple of 64 samples per
 * pixel, whose rays the shading kernel forms and tests itself.  0 where no pass did, and with reserved[0] bit 12. */
int vmx_fused_camera_paths(const vmx_scene *scene, uint64_t *paths);
/* Debug entry: vmx_pixel_claims and, for the pixels without a claim, the list claims a render would use: four 32-bit words
 * per pixel of this rank's rows, up to four leaf-order slots padded with 0xFFFFFFFF (all four: no list).  A camera ray of
 * such a pixel is tested against the listed triangles alone and skips the BVH walk where that test is decisive.
 * lists_out is required; claims_out and n_claimed may be NULL. */
int vmx_pixel_claim_lists(const vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts, uint32_t *claims_out,
                          uint32_t *lists_out, uint32_t *n_claimed);
/* Debug entry: how many camera rays of the last render call on this scene were settled by a list claim.  0 where no
 * claims were built, with reserved[0] bit 11 or bit 13, and in the counting build. */
int vmx_list_settled_rays(const vmx_scene *scene, uint64_t *rays);
/* Debug entry: the bounce rays of the last render call on this scene that the bounce traversal kernel took over the
 * scene's guide tree.  A VMX_BVH_REFERENCE scene also holds a quality tree of the same triangles (the guide; about
 * 64 bytes per triangle of device memory, counted by vmx_scene_describe).  A bounce ray walks the guide, and a per-ray
 * rule decides whether the reference tree returns exactly the pair (t, triangle) that walk found: `settled` counts
 * those rays, `fallback` the others, which the same kernel then traces over the reference tree; the frame is the same
 * bit for bit either way.  Both are 0 with reserved[0] bit 14, in the counting build, for a scene built with another
 * builder, and after a vmx_scene_update that moved vertices without VMX_UPDATE_REBUILD (a refit leaves the guide stale
 * from then on; a VMX_UPDATE_REBUILD of a host-built reference tree builds the guide of the new positions beside it). */
int vmx_guide_rays(const vmx_scene *scene, uint64_t *settled, uint64_t *fallback);
/* Debug entry: the entries of the bounce-generation lists that the last render call on this scene handed to the
 * guide form of the traversal kernel, counted on the host: settled + fallback of vmx_guide_rays equals it. */
int vmx_guide_list_entries(const vmx_scene *scene, uint64_t *entries);
/* Debug entry: the same two counts for the FUSED launches of the last render call on this scene (the kernel that keeps
 * paths to their end: the tail of a split pass, the passes of pipeline form 1 and the small passes of form 0), where
 * rays of any depth, camera rays included, walk the guide.  `settled` counts the traversals the rule settled;
 * `fallback` those that ran over the reference tree: the rule's fallbacks, which start again there in the same lane,
 * and the rays that may not walk the guide at all (a non-finite origin, direction or reciprocal, an origin beyond the
 * rule's reach).  Every traversal of those launches is counted once, one with a non-finite direction too, which is no
 * ray of vmx_stats.  Both are 0 wherever vmx_guide_rays' are; vmx_guide_rays and vmx_guide_list_entries do not
 * count these launches. */
int vmx_guide_fused_rays(const vmx_scene *scene, uint64_t *settled, uint64_t *fallback);
/* Debug entry: the guide form of the bounce traversal kernel on n explicit rays (host buffers), so that a test can hold
 * the device's guide walk against the host program of guide_walk.h ray by ray.  The rays become path state and one id
 * list as vmx_radiance forms them; one launch walks the guide as a render's guided bounce generation does (same stack
 * binding, same lists; opts' tuning words act as in a render).  flags bit 0: the form that hands every ray on as a dense
 * record (what the default frame's bounce generations run) instead of the form that writes a hit record per path; bit 1:
 * the render's second launch follows, the unchanged kernel over the fallback list, so every ray has an answer.
 * grid_blocks caps the blocks of the guided launch (0: what a render launches), so that few rays still pass many refills.
 * settled[i]: 1 if the guided launch settled ray i, 0 if it went to the fallback list; slot[i]: the leaf slot in the
 * scene's tree (vmx_scene_bvh's prim_order index), 0xFFFFFFFF for no hit; t[i]: the kernel's t.  Without bit 1 a fallback
 * ray has slot 0xFFFFFFFF and t 0.  The entry itself checks that every ray was settled or listed, never both, and listed
 * and answered at most once: a violation is VMX_ERR_HIP with the counts in the message.  VMX_ERR_INVALID: a NULL
 * argument, an unknown flag, opts->collect_counters, a scene without a valid guide (see vmx_guide_rays).  n = 0 does
 * nothing.  Afterwards vmx_guide_rays reports this call's counts and vmx_guide_list_entries n. */
int vmx_guide_trace(const vmx_scene *scene, const float *origin, const float *dir, uint32_t n, const vmx_opts *opts,
                    uint32_t flags, uint32_t grid_blocks, uint8_t *settled, uint32_t *slot, float *t);
/* vmx_guide_trace through the kernel's counting form: additionally inner_visits[i] and tri_tests[i], the inner records
 * and the triangle tests of ray i's walk over the guide (0 and 0 for a ray that never walked it), so that a test can hold
 * the device's walk against the host program's visit by visit: a device that never skips a box behind the ray's origin
 * passes every comparison of answers.  flags bit 0 is VMX_ERR_INVALID here (hit records only); the rest as above. */
int vmx_guide_trace_visits(const vmx_scene *scene, const float *origin, const float *dir, uint32_t n, const vmx_opts *opts,
                           uint32_t flags, uint32_t grid_blocks, uint8_t *settled, uint32_t *slot, float *t,
                           uint32_t *inner_visits, uint32_t *tri_tests);
/*
 * Radiance (pathtracer.cpp:21-198) for n explicit camera rays; ray i draws
 * from the stream keyed (opts->seed, i, 0) with the two pixel-jitter draws
 * skipped.  out[n*4] = accumColour (rgb, w = primary hit distance or -100).
 */
int vmx_radiance(const vmx_scene *scene, const float *origin, const float *dir, uint32_t n,
                 const vmx_opts *opts, float *out, vmx_stats *stats);

/* cosf(x[i]), sinf(x[i]) for x in [0, 2 pi] exactly as the shading kernels evaluate the cos(r1) / sin(r1) of
 * pathtracer.cpp:162 under the default reading (see VMX_SAMPLING_LIBM_DOUBLE); host buffers */
int vmx_trig(const float *x, uint32_t n, float *cos_out, float *sin_out, int device);

/* ---- render (replaces PathTracer::Render, pathtracer.cpp:200-328) ------ */
/* number of image rows / pixels this (rank, world) owns */
int vmx_local_rows(uint32_t height, uint32_t stripe_rows, uint32_t rank, uint32_t world,
                   uint32_t *rows);
/*
 * Render into a caller-owned HOST buffer.  world <= 1: out is W*H*5 floats in
 * Camera::mImage RGBAZ layout (camera.cpp:106-113): r,g,b in [0,1], alpha 1,
 * depth = samples taken (pathtracer.cpp:318-323).  world > 1: out holds only
 * this rank's rows, packed in ascending row order (local_rows*W*5 floats).
 */
int vmx_render(const vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts,
               float *out_rgbaz, vmx_stats *stats);
/* Same, but `d_out` is DEVICE memory on the scene's device and the work is
 * enqueued on `stream` (a hipStream_t; NULL = the library's own stream).
 * Blocks until the frame is complete (the early-stop loop needs the host). */
int vmx_render_device(const vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts,
                      void *d_out_rgbaz, void *stream, vmx_stats *stats);
/* ---- progressive rendering: the same frame in resumable steps, with previews -------------------
 * vmx_render is one blocking call that shows nothing before the last sample.  A vmx_progressive handle renders the same
 * frame — bit for bit, whatever the steps — a few samples at a time, and can show its unfinished state in between.
 *
 * begin: cam / opts as vmx_render takes them (same checks and messages; everything vmx_render accepts, including
 *   rank / world / stripes and the tuning words).  The handle owns its per-pixel state, a buffer for the finished pixels
 *   and the pass schedule; the per-pass scratch stays the scene's shared workspace.  `stream`: a hipStream_t, NULL = the
 *   scene's stream.  The target spp of a handle cannot change (the 2x2 stratification maps a sample index to its
 *   stratum through spp / 4): a longer frame is a new handle.
 * step: issues more samples and blocks until they are resolved (the pass loop needs the host, as in vmx_render).
 *   `samples` is the most samples any pixel takes in this step; every pixel that was active before the step takes at
 *   least one; 0 = run to completion.  How a step is cut into passes is the library's choice.  A step of a complete
 *   frame is VMX_OK and does nothing.  `stats` (may be NULL) and vmx_scene_timings report this step alone.
 * preview: for each local pixel, in the layout vmx_render writes (W*H*5 floats, or this rank's packed rows):
 *     a finished pixel     exactly what vmx_render writes for it
 *     n >= 1 samples so far  vmx_render's pixel write applied to the sums so far: clamped mean, alpha 1.f, depth (float)n
 *     no sample yet        (0, 0, 0, 1, 0)
 *   and / or rgba8[p*4 + c] = (unsigned char)floor(that * 255), c = 0..3 (vmx_quantize_device's arithmetic), in the same
 *   launch.  At least one of the two outputs must be non-NULL.  The device variant takes DEVICE pointers of the scene's
 *   device (checked as vmx_query_device checks its pointers; 4-byte aligned), is enqueued on the handle's stream and
 *   returns without synchronising; the host variant synchronises.  A preview never changes the state.
 * Between steps the scene may serve any other call — queries, raycasts, vmx_render, other handles — and the handle's
 * frames do not change.  A geometry update (vmx_scene_update[_device], refit or rebuild) after begin makes every later
 * step fail with VMX_ERR_INVALID ("scene updated since vmx_progressive_begin"): the handle's tuning and stack sizing
 * came from the tree it saw.  preview, info and end still work on such a handle.  vmx_scene_destroy with open handles
 * fails with VMX_ERR_INVALID and leaves the scene intact.
 */
typedef struct vmx_progressive vmx_progressive;
typedef struct vmx_progressive_info {
    uint32_t width, rows;   /* rows = this (rank, world)'s local rows, as vmx_local_rows            */
    uint32_t kmax;          /* 4 * (rays_per_pixel / 4): the most samples a pixel can take         */
    uint32_t pixels_active; /* pixels that still take samples; 0 = the frame is complete           */
    uint64_t samples;       /* samples accumulated into the image so far                           */
    uint64_t passes, steps; /* sample batches processed; steps that issued any                     */
} vmx_progressive_info;
int vmx_progressive_begin(vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts, void *stream,
                          vmx_progressive **out);
int vmx_progressive_step(vmx_progressive *p, uint32_t samples, vmx_stats *stats);
int vmx_progressive_info_get(const vmx_progressive *p, vmx_progressive_info *out);
int vmx_progressive_preview_device(vmx_progressive *p, void *d_rgbaz, void *d_rgba8);
int vmx_progressive_preview(vmx_progressive *p, float *rgbaz, unsigned char *rgba8);
int vmx_progressive_end(vmx_progressive *p);

/* ---- G-buffer-guided denoising of frames and previews ---------------------------------------------
 * A few-sample frame of the reference's sampling is salt-and-pepper (nine in ten diffuse
 * bounces end the path, the lights are far brighter than 1 and the pixel write clamps).  This is the edge-avoiding
 * a-trous filter of Dammertz et al. 2010, guided by a vmx_rayhit G-buffer (what vmx_raycast_camera_device writes): per
 * pixel the guide is (normal, distance) where flags bit 0 is set and ((0, 0, 0), -1) elsewhere; "a hit" is z >= 0.
 * Colour c = r, g, b of an RGBAZ pixel; alpha and depth pass through, bitwise.
 *
 * For iteration it = 0 .. iterations-1, all in float, one rounding per written operation, left to right:
 *   s = 1 << it;  sc_0 = sigma_colour, sc_{it+1} = sc_it * 0.5f;  isc2 = 1.f / (sc_it * sc_it);  kz = sigma_depth * (float)s
 *   per pixel p: isz = 1.f / (kz * z_p) (used where p is a hit); sum_c = (0, 0, 0), sum_w = 0
 *   taps dy = -2..2 (outer), dx = -2..2 (inner), q = p + s * (dx, dy); a tap outside the image or with
 *   (z_q >= 0) != (z_p >= 0) is skipped;  hh = h[dy+2] * h[dx+2], h = {1/16, 1/4, 3/8, 1/4, 1/16}
 *     p a hit:  d = n_p.x*n_q.x + n_p.y*n_q.y + n_p.z*n_q.z;  d = d > 0 ? d : 0;  normal_squarings times d = d*d;
 *               t = (z_p - z_q) * isz;  num = hh * d;  g = 1.f + t*t          p a miss:  num = hh;  g = 1.f
 *     e = dr*dr + dg*dg + db*db, d. = c_p. - c_q. of this iteration's input;  w = num / (g * (1.f + e * isc2))
 *     if w > 0 and finite:  sum_c. = sum_c. + w * c_q.;  sum_w = sum_w + w     (the centre tap is a tap like any other)
 *   out. = sum_w > 0 ? sum_c. / sum_w : c_p.   (the fallback: a zero or NaN normal, a NaN colour, a z_p so small that
 *   isz overflows).  Denormals are kept.  Iterations ping-pong between the filter's planes; the last one writes the
 *   caller's RGBAZ buffer and / or rgba8 (vmx_quantize_device's arithmetic on that output pixel).
 * The kernels hold to this restatement bit for bit (tests/filter_spec.py).
 */
typedef struct vmx_filter_params {
    uint32_t iterations, normal_squarings; /* 1..10 (default 5); 0..8 (default 5)                 */
    float sigma_colour, sigma_depth;       /* finite, > 0 (defaults 2.f, 0.1f)                    */
    uint32_t reserved[4];                  /* must be 0                                           */
} vmx_filter_params;

typedef struct vmx_filter vmx_filter;

int vmx_filter_default_params(vmx_filter_params *out);
/* A filter for width x height frames on `device`.  It owns the guide (16 B per pixel) and two colour planes (16 B per
 * pixel each); nothing is allocated after creation.  width or height 0, or a frame vmx_render would call too large, is
 * VMX_ERR_INVALID; without a usable device VMX_ERR_NO_DEVICE. */
int vmx_filter_create(int device, uint32_t width, uint32_t height, vmx_filter **out);
int vmx_filter_destroy(vmx_filter *f);
/* d_rayhit: width*height vmx_rayhit records in pixel order (what vmx_raycast_camera_device writes), packed into the
 * filter's guide on `stream` (a hipStream_t; NULL = the legacy default stream).  The guide stays until the next call. */
int vmx_filter_set_guide_device(vmx_filter *f, const void *d_rayhit, void *stream);
/* Filters the W*H*5-float frame d_in_rgbaz into d_out_rgbaz (same layout) and / or d_rgba8 (W*H*4 bytes); at least one
 * of the two must be non-NULL.  params == NULL selects the defaults; a field out of range or a non-zero reserved word
 * is VMX_ERR_INVALID before any launch, as is a call before any guide was set.  d_out_rgbaz == d_in_rgbaz (in place)
 * is allowed; any other overlap of the three buffers is VMX_ERR_INVALID.  Pointers are checked as vmx_query_device
 * checks its own (DEVICE memory of the filter's device) and must be 4-byte aligned.  Enqueued on `stream`, no
 * synchronisation.  Calls on one handle from different streams are ordered by enqueue (each waits on an event the
 * previous one recorded), so they never share the guide and the planes while in flight. */
int vmx_filter_apply_device(vmx_filter *f, const void *d_in_rgbaz, void *d_out_rgbaz, void *d_rgba8,
                            const vmx_filter_params *params, void *stream);
/* vmx_progressive_preview[_device]'s frame pushed through the filter, bit for bit, at any point of the frame (no sample
 * yet, a complete frame); the outputs follow the plain previews' rules.  The first iteration reads the per-pixel state
 * itself.  On its first filtered preview a handle builds its guide — sample 0's camera ray of every pixel from its own
 * camera and seed, through vmx_raycast_camera_device's code path — and creates its filter; that call blocks until the
 * guide is built.  Both are freed by vmx_progressive_end.  A filtered preview never changes the handle's state.
 * VMX_ERR_INVALID: a handle begun with opts->world > 1 ("whole images only", vmx_raycast_camera_device's rule), and
 * a first filtered preview after a geometry update ("scene updated since vmx_progressive_begin": the guide cannot be
 * built from the tree the handle saw); a guide built before the update keeps working.  The device variant runs on
 * the handle's stream and does not synchronise (after the first call); the host variant synchronises. */
int vmx_progressive_preview_filtered_device(vmx_progressive *p, void *d_rgbaz, void *d_rgba8,
                                            const vmx_filter_params *params);
int vmx_progressive_preview_filtered(vmx_progressive *p, float *rgbaz, unsigned char *rgba8,
                                     const vmx_filter_params *params);

/* ---- albedo-demodulated denoising: textured surfaces keep their texture ------------------------------
 * With a bound texture (vmx_scene_bind_texture) the integrator multiplies a path's throughput by the texel at every
 * diffuse triangle hit (pathtracer.cpp:63-66).  A texture on a flat wall has no edge in the filter's guide, so the
 * filter above averages it away with the noise.  The remedy is to filter colour / albedo and multiply the albedo back:
 * a per-pixel albedo plane, and a filter call that divides by it on the way in and multiplies by it on the way out.
 * It pays on resolved textures on surfaces wider than the filter's footprint; on thin geometry with a minified texture
 * it is no better than the plain call.
 *
 * The albedo plane.  d_albedo holds W*H float4 in pixel order, 16-byte aligned, DEVICE memory of the scene's device.
 * cam / opts are checked exactly as vmx_raycast_camera_device checks them (only opts->seed is used; opts->world > 1 is
 * VMX_ERR_INVALID); nsamples >= 1 and first_sample + nsamples <= 4 * (rays_per_pixel / 4).  Per pixel p, in float, one
 * rounding per written operation:
 *   sum = (0, 0, 0), cnt = 0
 *   for k = first_sample .. first_sample + nsamples - 1, ascending:
 *     r = the MeshEngine::RayCast record of sample k's camera ray — what vmx_raycast_camera_device(.., k, ..) writes for p
 *     mat = (r.flags & 2) != 0
 *     t = mat ? VermiTexture::Sample(r.uv).xyz : (1, 1, 1)   texture 0 as the integrator samples it (meshEngine.cpp:21-46:
 *         wrap x - floor(x), nearest round(x * (W - 1)), 1-4 channels — one channel is (v, v, v), two are (a, b, 0) —
 *         the texel index clamped), with the reference's stale uv and a material hit hidden behind a nearer sphere,
 *         because that is what the integrator multiplies by; a scene with no bound texture gives t = (1, 1, 1)
 *         (pathtracer.cpp:75-79)
 *     sum. = sum. + t.;  cnt += mat
 *   out = (sum.x / (float)n, sum.y / (float)n, sum.z / (float)n, (float)cnt / (float)n),  n = nsamples
 * Enqueued on `stream` (NULL = the scene's stream), no synchronisation; ordered with the scene's queries and updates as
 * vmx_raycast_camera_device is (same workspace, same event).  Its scratch (64 bytes per pixel) is allocated on first
 * use and then reused.  Served by the camera-ray query of the G-buffer path and a dense finish kernel that computes
 * only uv and the material bit, samples the texture and accumulates: no 64-byte record per sample leaves the library. */
#define VMX_ALBEDO_FLOOR 0.0009765625f /* 2^-10 */
int vmx_albedo_camera_device(const vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts,
                             uint32_t first_sample, uint32_t nsamples, void *d_albedo, void *stream);
/* vmx_filter_apply_device with demodulation: the same rules for arguments, order of checks, overlaps, in place, guide
 * and stream ordering.  In addition d_albedo (W*H float4, what vmx_albedo_camera_device writes; .w is not read) is read
 * only, non-NULL, 16-byte aligned, DEVICE memory of the filter's device, and may overlap no written buffer.  Per pixel
 * q and channel:
 *   am_q. = (a_q. > VMX_ALBEDO_FLOOR && a_q. <= 3.402823466e+38f) ? a_q. : VMX_ALBEDO_FLOOR
 *           (NaN, zero, negative and infinite albedo all take the floor)
 *   the first iteration's input colour of every pixel q, centre and taps:  c_q. = frame_q. / am_q.
 *   the last iteration's result:  out. = o. * am_p.,  o what the restatement above would have written, fallback included
 * and everything between is that restatement unchanged.  Alpha and depth pass through bitwise; rgba8 is computed from
 * the multiplied result.  A dense pre-pass writes frame / albedo into the filter's plane, which the first iteration then
 * reads (so an in-place single iteration needs no copy of the frame).  tests/demod_spec.py restates it. */
int vmx_filter_apply_demodulated_device(vmx_filter *f, const void *d_in_rgbaz, const void *d_albedo,
                                        void *d_out_rgbaz, void *d_rgba8, const vmx_filter_params *params,
                                        void *stream);
/* The filtered previews with the demodulated call's arithmetic.  The handle builds its albedo plane once, on its first
 * demodulated preview, from its own camera and seed — samples 0 .. albedo_samples - 1, albedo_samples in
 * 1 .. 4 * (rays_per_pixel / 4) — under the guide's refusals (opts->world > 1, scene updated since begin); a later call
 * with a different albedo_samples builds it again.  The plane is freed by vmx_progressive_end.  A demodulated preview
 * never changes the handle's render state. */
int vmx_progressive_preview_demodulated_device(vmx_progressive *p, void *d_rgbaz, void *d_rgba8,
                                               const vmx_filter_params *params, uint32_t albedo_samples);
int vmx_progressive_preview_demodulated(vmx_progressive *p, float *rgbaz, unsigned char *rgba8,
                                        const vmx_filter_params *params, uint32_t albedo_samples);

/* ---- temporal accumulation: frames over time, across camera moves -------------------------------------
 * A few-sample frame per camera position flickers, although nearly every surface it shows was sampled a frame
 * earlier.  A vmx_temporal handle keeps an accumulated frame and reprojects it into each new camera through that
 * frame's G-buffer (vmx_rayhit records, what vmx_raycast_camera_device(scene, cam, opts, 0, ...) writes), rejects stale
 * history by normal and plane distance, and blends the new frame in.  Per pixel the handle owns the accumulated colour
 * c_h and history length n_h, the previous guide (n, z: the filter's rule, z = -1 and n = 0 where the ray missed), the
 * previous hit location X and the previous call's camera; double-buffered, 2 x 48 B per pixel.
 *
 * Everything is float, one rounding per written operation, left to right; `/` is correctly rounded, denormals are kept.
 * proj(X, cam), with m = the camera's 3x3 matrix (m[col*3 + row]), pos, d = back_distance, (sx, sy) = back_size:
 *   v = X - pos;  c_k = (m[3k]*v.x + m[3k+1]*v.y) + m[3k+2]*v.z, k = 0, 1, 2;  t = d / (-c_2)
 *   u = ((c_0*t)/sx + 0.5f) * (float)W;  w = ((-(c_1*t))/sy + 0.5f) * (float)H;  front = c_2 < 0
 * (the transpose of the matrix a camera ray is made with: its inverse up to rounding).
 * Per pixel p = (x, y) with its record's hit = flags bit 0, n_p = normal, z_p = distance, X = location, and c = the
 * input frame's r, g, b:
 *   the first call after create or reset, or !hit:  out = c, n' = 1.f.  Otherwise
 *   (u_c, w_c, -) = proj(X, this call's cam);  (u_h, w_h, front) = proj(X, the previous call's cam)
 *   gx = (float)x + (u_h - u_c);  gy = (float)y + (w_h - w_c)      (a camera that did not move: exactly x, y)
 *   inrange = front && gx >= -1.f && gx < (float)W && gy >= -1.f && gy < (float)H      (false for NaN)
 *   x0 = floorf(gx), fx = gx - x0;  y0 = floorf(gy), fy = gy - y0
 *   four taps, dy = 0, 1 (outer), dx = 0, 1 (inner):  q = (x0 + dx, y0 + dy);  wx = dx ? fx : 1.f - fx, wy likewise,
 *   wt = wx*wy.  A tap counts iff inrange, q is inside the image, z_q >= 0,
 *     (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z >= normal_min,
 *     pd*pd <= (plane_tol*plane_tol) * (z_p*z_p) with e = X - X_q, pd = (n_p.x*e.x + n_p.y*e.y) + n_p.z*e.z,
 *     and wt > 0; then  sum_c. = sum_c. + wt*c_h(q).;  sum_n = sum_n + wt*n_h(q);  sum_w = sum_w + wt   (from 0)
 *   sum_w > 0:  h. = sum_c./sum_w;  nh = sum_n/sum_w;  t = nh + 1.f;  n' = t < max_history ? t : max_history;
 *               a = 1.f/n';  out. = h. + (c. - h.)*a            else:  out = c, n' = 1.f
 * New state: c_h = out, n_h = n', guide, X (the record's location as it stands) and camera of this call.
 * Outputs: d_out_rgbaz = out in r, g, b, alpha and depth the input's bits; d_rgba8 = vmx_quantize_device's arithmetic
 * on that pixel; d_history_len[p] = n'.
 * Limits: without motion records (below) the world is taken as static between the two frames — after
 * vmx_scene_update a moved surface fails the plane test and restarts at n' = 1, and a face that slid within its own
 * plane keeps history of other surface points; vmx_motion_device and vmx_temporal_accumulate_motion_device follow
 * refitted triangles, vmx_motion_spheres_device an analytic sphere that vmx_scene_set_spheres moved.  A NaN colour passes into the history and stays
 * until that pixel is invalidated or the handle is reset.
 * The kernel holds to this restatement bit for bit (tests/temporal_spec.py).
 */
typedef struct vmx_temporal_params {
    float normal_min;     /* finite, -1..1; default 0.9f                     */
    float plane_tol;      /* finite, > 0;   default 0.01f                    */
    float max_history;    /* finite, >= 1;  default 32.f                     */
    uint32_t reserved[5]; /* must be 0                                       */
} vmx_temporal_params;

typedef struct vmx_temporal vmx_temporal;

int vmx_temporal_default_params(vmx_temporal_params *out);
/* An accumulator for width x height frames on `device`, checked and refused as vmx_filter_create does.  It owns its
 * two state buffers (48 B per pixel each); nothing is allocated after creation, except that the first
 * vmx_temporal_accumulate_adaptive_device on a handle allocates that call's reprojection plane (below), which
 * vmx_temporal_destroy frees. */
int vmx_temporal_create(int device, uint32_t width, uint32_t height, vmx_temporal **out);
int vmx_temporal_destroy(vmx_temporal *t);
/* Forgets the history: the next call is a first call.  A first call reads none of the state, so nothing is enqueued
 * (`stream` is not used); like the calls themselves, resets take effect in the order they are made. */
int vmx_temporal_reset(vmx_temporal *t, void *stream);
int vmx_temporal_frames(const vmx_temporal *t, uint64_t *frames_since_reset);
/* One frame: d_rayhit = W*H vmx_rayhit records in pixel order, 16-byte aligned (that frame's G-buffer); d_in_rgbaz the
 * W*H*5-float frame; d_out_rgbaz (same layout) and / or d_rgba8 (W*H*4 bytes), at least one non-NULL; d_history_len
 * W*H floats or NULL.  cam is checked as vmx_raycast_camera_device checks its camera and its image_res must be the
 * handle's size; the call reads its matrix, position, back_distance and back_size only.  params == NULL selects the
 * defaults; a field out of range or a non-zero reserved word is VMX_ERR_INVALID before any launch.  d_out_rgbaz ==
 * d_in_rgbaz (in place) is allowed; any other overlap with a buffer the call writes is VMX_ERR_INVALID.  Pointers follow
 * vmx_filter_apply_device's rules (DEVICE memory of the handle's device, 4-byte aligned).  Enqueued on `stream`, no
 * synchronisation; calls on one handle from different streams are ordered by enqueue. */
int vmx_temporal_accumulate_device(vmx_temporal *t, const vmx_camera *cam, const void *d_rayhit,
                                   const void *d_in_rgbaz, void *d_out_rgbaz, void *d_rgba8, void *d_history_len,
                                   const vmx_temporal_params *params, void *stream);

/* ---- motion records: temporal accumulation that follows refitted geometry -------------------------------
 * After vmx_scene_update[_device] a pixel's surface point was somewhere else a frame earlier.  vmx_motion_device is a
 * pure function of a G-buffer and the two position arrays the caller of vmx_scene_update_device already holds (no scene
 * handle): per record, the point its surface point occupied before the update and the normal the previous frame's
 * G-buffer had there.  Everything is float, one rounding per written operation, left to right; `/` and sqrtf are
 * correctly rounded, denormals are kept.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 * For record r:  P = r.location, id = r.tri_id, a0 a1 a2 = the vertices at pos_now[id*9 ..], q0 q1 q2 = those at
 * pos_prev[id*9 ..].
 *   on = (r.flags & 1) && id >= 0 && id < ntris && r.distance == r.tri_t      (tri_id stays set when a sphere is nearer
 *        than the triangle: the location then lies on the sphere and the distances differ); when !on no array is read
 *   moved = any of the nine position words differs bitwise between pos_now and pos_prev
 *   e1 = a1 - a0;  e2 = a2 - a0;  ep = P - a0
 *   d11 = dot(e1,e1);  d12 = dot(e1,e2);  d22 = dot(e2,e2);  dp1 = dot(ep,e1);  dp2 = dot(ep,e2)
 *   den = d11*d22 - d12*d12;  b1 = (d22*dp1 - d12*dp2)/den;  b2 = (d11*dp2 - d12*dp1)/den;  b0 = (1.f - b1) - b2
 *   Xh. = (b0*q0. + b1*q1.) + b2*q2.  per component;  good = den > 0 && every component of Xh finite
 *   with d_nrm_prev (n0 n1 n2 = the normals at nrm_prev[id*9 ..]):  m. = (b0*n0. + b1*n1.) + b2*n2.;
 *     s = 1.f / sqrtf(dot(m, m));  nh. = -(m.*s)  (negated, as Triangle::getNormal negates);  nh = r.normal if any
 *     component is not finite.  Without d_nrm_prev:  nh = r.normal  (right for translations).
 *   on && moved && good:  the output is (Xh, VMX_MOTION_MOVED, nh, 0);  otherwise (r.location, 0, r.normal, 0), the
 *   record's own bits — a triangle that did not move takes exactly the path without motion records.
 * The kernel holds to this restatement bit for bit (tests/motion_spec.py).
 */
#define VMX_MOTION_MOVED 1u
typedef struct vmx_motion {       /* 32 bytes, two float4 */
    float prev_location[3];       /* where this pixel's surface point was before the update   */
    uint32_t flags;               /* VMX_MOTION_MOVED or 0                                    */
    float prev_normal[3];         /* the normal the previous frame's G-buffer had there       */
    uint32_t pad;                 /* 0                                                        */
} vmx_motion;
/* d_rayhit: n vmx_rayhit records, 16-byte aligned; d_pos_now, d_pos_prev: ntris*9 floats each, the positions after and
 * before the update (what vmx_scene_update_device takes); d_nrm_prev: the normals before it, or NULL; d_out: n vmx_motion
 * records, 16-byte aligned, overlapping no input.  All DEVICE memory of `device`, checked as vmx_query_device checks its
 * pointers; the arrays are 4-byte aligned.  ntris == 0, n > 2^31 - 1 or a NULL pointer other than d_nrm_prev is
 * VMX_ERR_INVALID; n == 0 is VMX_OK and launches nothing.  Enqueued on `stream`, no synchronisation. */
int vmx_motion_device(const void *d_rayhit, uint32_t n, const void *d_pos_now, const void *d_pos_prev,
                      const void *d_nrm_prev /* or NULL */, uint32_t ntris, void *d_out, int device, void *stream);
/* Motion records for pixels that lie on an analytic sphere which vmx_scene_set_spheres moved or resized.  A pure function
 * of a G-buffer whose rays share one origin (vmx_raycast_camera_device's: origin = the camera's position) and of the
 * sphere table now and before, as HOST arrays of the same count (no scene handle; a sphere that appears or disappears
 * between the two tables is outside the rule).  Same arithmetic rules as above; sphereIntersect's discriminant and roots
 * are double, as in the reference (meshEngine.cpp:182-194).  O = origin; per table entry i: c, r, nc = centre, radius,
 * normal_centre; sg = normal_sign < 0 ? -1.f : 1.f (as scene creation reads it); _now / _prev name the table.
 *   moved_i = centre, radius or normal_centre differ bitwise between now and prev, or sg differs
 * For record r, P = r.location:
 *   sphere = (r.flags & 1) && !(r.tri_id >= 0 && r.distance == r.tri_t)     (the complement of `on` above without its
 *            ntris bound: a hit that does not lie on its triangle lies on a sphere)
 *   Which sphere — the record does not say — is decided as MeshEngine::RayCast decides it, on the table now:
 *     d = P - O;  s = 1.f / sqrtf(dot(d, d));  d = d * s;  if any component of d is not finite, no sphere is accepted
 *     nearest = +inf;  for i in table order:  op = c_i - O;  B = dot(op, d);  C = dot(op, op);  R2 = r_i * r_i;
 *       det = ((double)B*(double)B - (double)C) + (double)R2;  th = 0 if det < 0, else with q = sqrt(det):
 *       t = (double)B - q;  th = (float)t if t > 1e-4, else t = (double)B + q;  th = (float)t if t > 1e-4, else 0
 *       th > 0 && th < nearest:  nearest = th, sphere i is accepted        (the last one accepted is the one)
 *     (never by a residual | |P - c| - r |: any point of the reference's room lies within 3e-6 relative of a radius-5e7
 *     wall, and the floor would be taken for the small light)
 *   With the accepted sphere's entries:
 *     k = r_prev / r_now;  Xh. = c_prev. + (P. - c_now.) * k   per component
 *     m = Xh - nc_prev;  s = 1.f / sqrtf(dot(m, m));  nh. = (m. * s) * sg_prev;  nh = r.normal if any component is not
 *     finite (nc_prev == Xh)
 *   sphere && a sphere was accepted && moved && every component of Xh finite (r_now == 0 is not):  the output is
 *   (Xh, VMX_MOTION_MOVED, nh, 0);  otherwise the record leaves as d_motion_in's record for that pixel, bit for bit, or
 *   without d_motion_in as (r.location, 0, r.normal, 0) — what vmx_motion_device writes for an unmoved pixel.  The call
 *   therefore composes after vmx_motion_device (its d_out as d_motion_in here, in place if wanted) or stands alone.
 * A record on a sphere that did not move is never rewritten.  That matters on the reference's radius-5e7 walls, where
 * P - c has an ulp of 4: the rule applies to a wall that moves, but to that precision only.
 * The kernel holds to this restatement bit for bit (tests/sphere_motion_spec.py).
 * d_rayhit: n records, d_out: n vmx_motion records, d_motion_in: n vmx_motion records or NULL; all 16-byte aligned DEVICE
 * memory of one device (the one d_rayhit lies on), checked as vmx_motion_device checks its pointers.  d_out may be
 * d_motion_in exactly (in place); any other overlap of d_out with an input is VMX_ERR_INVALID.  nspheres > 16, a NULL
 * pointer other than d_motion_in (the tables may be NULL when nspheres == 0) or n > 2^31 - 1 is VMX_ERR_INVALID, checked
 * in this order: d_rayhit, origin, spheres_now, spheres_prev, d_out, nspheres, alignment, n, overlap.  n == 0 is VMX_OK
 * and launches nothing.  The tables are passed to the kernel by value: they may change as soon as the call returns.
 * Enqueued on `stream`, no synchronisation. */
int vmx_motion_spheres_device(const void *d_rayhit, uint32_t n, const float origin[3], const vmx_sphere *spheres_now,
                              const vmx_sphere *spheres_prev, uint32_t nspheres, const void *d_motion_in /* or NULL */,
                              void *d_out, void *stream);
/* vmx_temporal_accumulate_device with motion records: d_motion = W*H vmx_motion records in pixel order, 16-byte aligned,
 * read only (it may overlap no buffer the call writes), or NULL — then the call IS vmx_temporal_accumulate_device.
 * Per pixel Xh, nh = prev_location, prev_normal of its record (X, n_p wherever the flag is clear), and the
 * restatement above changes in exactly three places:
 *   (u_h, w_h, front) = proj(Xh, the previous call's cam)      ((u_c, w_c) stays proj(X, this call's cam))
 *   the normal test is  (nh.x*n_q.x + nh.y*n_q.y) + nh.z*n_q.z >= normal_min
 *   e = Xh - X_q,  pd = (nh.x*e.x + nh.y*e.y) + nh.z*e.z
 * zz stays (plane_tol*plane_tol) * (z_p*z_p); the new state stays this call's guide, X and camera.  A first call
 * ignores the records. */
int vmx_temporal_accumulate_motion_device(vmx_temporal *t, const vmx_camera *cam, const void *d_rayhit,
                                          const void *d_motion, const void *d_in_rgbaz, void *d_out_rgbaz,
                                          void *d_rgba8, void *d_history_len, const vmx_temporal_params *params,
                                          void *stream);

/* ---- variance-guided denoising: temporal luminance moments steer the filter -----------------------------
 * The filter's colour stop above is one sigma_colour for every pixel: a pixel that has converged over 32 reprojected
 * frames is blurred as hard as one disoccluded this frame, and a shading detail with no G-buffer edge behind it (a
 * contact shadow, a light's falloff on a wall) goes at the rate of noise of its amplitude.  This is the variance
 * estimate and the variance-driven edge stop of Schied et al. 2017 (SVGF): the accumulator carries the first and second
 * moment of the luminance through its reprojection taps, a second kernel turns them into a per-pixel variance, and a
 * filter call replaces the colour stop by the luminance difference measured in standard deviations.  The stop is
 * rational, as the existing weights are; there are no transcendentals.  Everything is float, one rounding per written
 * operation, left to right; `/` is correctly rounded, denormals are kept.
 *   lum(c) = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b
 *
 * Moments.  A handle made with VMX_TEMPORAL_MOMENTS keeps a fourth state plane of float2 (m1, m2): 2 x 56 B per pixel.
 * vmx_temporal_accumulate_variance_device is vmx_temporal_accumulate_motion_device (colour, n', guide, X and camera are
 * exactly what that call computes, d_motion may be NULL) and in addition, per pixel, l = lum(c) of the input frame:
 *   in each of the four taps, right after sum_n, with the colour's ok and wt:
 *     sum_m1 = sum_m1 + wt*m1_h(q);  sum_m2 = sum_m2 + wt*m2_h(q)                                          (from 0)
 *   sum_w > 0:  h1 = sum_m1/sum_w;  h2 = sum_m2/sum_w;  m1' = h1 + (l - h1)*a;  m2' = h2 + (l*l - h2)*a   (the colour's a)
 *   else, and on a first call and on a miss:  m1' = l;  m2' = l*l
 * Variance, from the new state (n', guide n / z, m1', m2'), per pixel p:
 *   vt = m2' - m1'*m1';  vt = vt > 0 ? vt : 0
 *   n' >= min_history:  var = vt.  Otherwise a 7 x 7 window, dy = -3..3 (outer), dx = -3..3 (inner), q = p + (dx, dy); a
 *   tap outside the image or with (z_q >= 0) != (z_p >= 0) is skipped;
 *     p a hit:  d = n_p.x*n_q.x + n_p.y*n_q.y + n_p.z*n_q.z;  d = d > 0 ? d : 0;  normal_squarings times d = d*d;
 *               t = (z_p - z_q) * (1.f/(sigma_depth*z_p));  w = d / (1.f + t*t)          p a miss:  w = 1.f
 *     if w > 0 and finite:  s1 = s1 + w*m1'(q);  s2 = s2 + w*m2'(q);  sw = sw + w                           (from 0)
 *   sw > 0:  a1 = s1/sw;  a2 = s2/sw;  vs = a2 - a1*a1;  vs = vs > 0 ? vs : 0;  var = vs * (min_history / n')
 *   else:    var = vt
 * A first frame has vt == 0 exactly, so its variance is all spatial, boosted by min_history.
 * d_variance: W*H floats, non-NULL — it counts as an output, so d_out_rgbaz and d_rgba8 may both be NULL — DEVICE memory
 * of the handle's device, 4-byte aligned, overlapping no other buffer of the call.  Every other rule is the motion
 * call's, in its order of checks (vparams right after tparams, d_variance after d_in_rgbaz).  A handle without moments
 * is refused (VMX_ERR_INVALID, "... VMX_TEMPORAL_MOMENTS ..."); on a moments handle the two calls above are
 * VMX_ERR_INVALID, because they would leave the moments stale.  Reset and frames work on both kinds of handle.
 * tests/variance_spec.py restates it; the kernels hold to it bit for bit.
 * A progressive preview gets its variance plane from the handle itself: vmx_progressive_error_device on a
 * VMX_PROGRESSIVE_MOMENTS handle (the adaptive sampling section below) writes d_variance in this layout.
 * Out of scope: a variance output of the filter.  (d_motion may carry vmx_motion_spheres_device's records.) */
#define VMX_TEMPORAL_MOMENTS 1u
typedef struct vmx_variance_params {
    float min_history;         /* finite, >= 1; default 4.f                       */
    uint32_t normal_squarings; /* 0..8;         default 5                         */
    float sigma_depth;         /* finite, > 0;  default 0.1f                      */
    uint32_t reserved[5];      /* must be 0                                       */
} vmx_variance_params;
int vmx_variance_default_params(vmx_variance_params *out);
/* vmx_temporal_create with flags: 0 (that call) or VMX_TEMPORAL_MOMENTS; any other bit is VMX_ERR_INVALID. */
int vmx_temporal_create_ex(int device, uint32_t width, uint32_t height, uint32_t flags, vmx_temporal **out);
int vmx_temporal_accumulate_variance_device(vmx_temporal *t, const vmx_camera *cam, const void *d_rayhit,
                                            const void *d_motion /* or NULL */, const void *d_in_rgbaz,
                                            void *d_out_rgbaz, void *d_rgba8, void *d_history_len, void *d_variance,
                                            const vmx_temporal_params *tparams, const vmx_variance_params *vparams,
                                            void *stream);
/* The variance-guided filter call.  Arguments, order of checks, overlaps, in place, guide and stream ordering follow
 * vmx_filter_apply_demodulated_device, with d_albedo NULL for the call without demodulation.  d_variance: W*H floats
 * (what the call above writes), read only, non-NULL, 4-byte aligned, overlapping no written buffer.  sigma_luminance:
 * finite, > 0 (VMX_SIGMA_LUMINANCE_DEFAULT); params->sigma_colour is checked as ever and not used.
 * A dense pre-pass writes the filter's plane as (c.r, c.g, c.b, v):
 *   without albedo:  c = the frame's r, g, b;  v = d_variance[p]
 *   with albedo:     c. = frame. / am.  (am: the demodulated call's clamped albedo);  la = lum(am);
 *                    v = d_variance[p] / (la*la)        (exact only for a grey albedo: the variance is the luminance's)
 * Every iteration is the restatement of "G-buffer-guided denoising" reading that plane, with these changes only:
 *   per pixel p:  vbar = sum of (k[dy+1]*k[dx+1]) * v(p + (dx, dy)),  dy = -1..1 (outer), dx = -1..1 (inner), from 0 in
 *                 tap order, k = {0.25f, 0.5f, 0.25f}, at one pixel's distance whatever the step; a neighbour outside
 *                 the image takes v_p;  den = (sigma_luminance*sigma_luminance)*vbar + VMX_VARIANCE_EPS
 *   per tap:      dl = lum(c_p) - lum(c_q);  w = num / (g * (1.f + (dl*dl)/den))      (num, g, skip rules unchanged)
 *                 if w > 0 and finite:  sum_c. = sum_c. + w*c_q.;  sum_v = sum_v + (w*w)*v_q;  sum_w = sum_w + w
 *   sum_w > 0:    out. = sum_c./sum_w;  v_out = sum_v/(sum_w*sum_w)           else:  out = c_p, v_out = v_p
 * sigma_luminance does not shrink over the iterations: the variance does, by propagation.  kz = sigma_depth*(float)s as
 * before.  The last iteration writes the caller's buffers as the plain call's does — with albedo the result is
 * multiplied by am_p first — and drops the propagated variance. */
#define VMX_VARIANCE_EPS 1e-10f
#define VMX_SIGMA_LUMINANCE_DEFAULT 4.f
int vmx_filter_apply_variance_device(vmx_filter *f, const void *d_in_rgbaz, const void *d_variance,
                                     const void *d_albedo /* or NULL */, void *d_out_rgbaz, void *d_rgba8,
                                     const vmx_filter_params *params, float sigma_luminance, void *stream);

/* ---- adaptive temporal accumulation: cut history where lighting changed ---------------------------------
 * The calls above blend with a = 1/min(n_h + 1, max_history) wherever the geometry test passes: the world's lighting is
 * taken as static.  A static pixel whose illumination changed — a light dimmed or recoloured, the shadow and bounce
 * light of a block moved by vmx_scene_update, a texture rebound — keeps its old colour and sheds it at 1/9, 1/10, ... per
 * frame.  vmx_temporal_accumulate_adaptive_device carries a change detector: over a 7 x 7 window of like surface it
 * compares the mean of the new frame with the mean of the reprojected history, per colour channel, in standard errors of
 * the new frame's window mean, and where they differ by more than gamma it shortens the history length before the blend.
 * The state layout does not change, so this call and the existing ones may alternate frame by frame on one handle.
 *
 * Everything is float, one rounding per written operation, left to right; `/` is correctly rounded, denormals are kept.
 * Per pixel p the motion call computes any_p = sum_w > 0, h_p, nh_p, and on a moments handle the variance call g1_p = h1,
 * g2_p = h2; all exactly as above.  hh_p = h_p where any_p, else 0.
 * On a first call, on a miss, or where !any_p, the result is the existing call's, and d_change[p] = 0.  Otherwise a
 * 7 x 7 window, dy = -3..3 (outer), dx = -3..3 (inner), q = p + (dx, dy); a tap outside the image, a tap with z_q < 0
 * (this frame's guide) and a tap with !any_q are skipped;
 *     d = n_p.x*n_q.x + n_p.y*n_q.y + n_p.z*n_q.z;  d = d > 0 ? d : 0;  normal_squarings times d = d*d;
 *     t = (z_p - z_q) * (1.f/(sigma_depth*z_p));  w = d / (1.f + t*t)        (the variance window's weight for a hit)
 *     if w > 0 and finite:  sw = sw + w;  sww = sww + w*w;  per channel k, c the input frame's colour:
 *       sc.k = sc.k + w*c_q.k;  scc.k = scc.k + w*(c_q.k*c_q.k);  sh.k = sh.k + w*hh_q.k                    (all from 0)
 *   support = sw > 0 && sw*sw >= min_support*sww                  (sw*sw/sww: the window's effective number of taps)
 *   per channel:  mc = sc/sw;  mh = sh/sw;  v = scc/sw - mc*mc;  v = v > 0 ? v : 0;
 *                 s2 = (2.f*v)*(sww/(sw*sw)) + VMX_ADAPTIVE_EPS;  dm = mc - mh;  k = (dm*dm)/s2
 *                 (the factor 2 bounds the noise of the history's window mean by that of the input's)
 *   K = k.r;  if (k.g > K) K = k.g;  if (k.b > K) K = k.b;  r = K/(gamma*gamma)
 *   cut = support && r > 1.f      (false for NaN: a NaN colour in the window never cuts; an infinite one follows the
 *                                  arithmetic)
 *   nh_e = cut ? nh/r : nh;  t = nh_e + 1.f;  n' = t < max_history ? t : max_history;  a = 1.f/n';  out. = h. + (c. - h.)*a
 *   the moments blend with the same a:  m1' = g1 + (l - g1)*a;  m2' = g2 + (l*l - g2)*a
 *   d_change[p] = support ? r : 0
 * and the variance is then computed from the new state, as in the variance call.  With gamma*gamma = +inf (gamma = 3e38f)
 * r is 0 or NaN and the call is the existing one bit for bit.
 * Arguments: on a handle without moments the call is vmx_temporal_accumulate_motion_device with the changes above;
 * d_variance and vparams must be NULL.  On a VMX_TEMPORAL_MOMENTS handle it is vmx_temporal_accumulate_variance_device
 * with them; d_variance is required.  The existing calls stay allowed or refused on each kind of handle as before.
 * aparams (NULL: the defaults) is checked right after vparams; d_change — W*H floats or NULL, DEVICE memory of the
 * handle's device, 4-byte aligned, overlapping no other buffer of the call — after d_variance; what depends on the kind of
 * handle (a missing or a surplus d_variance) is checked with the handle.  Every other rule, message and order of checks
 * is the motion or variance call's.
 * The first adaptive call on a handle allocates one reprojection plane, 16 B per pixel (24 B with moments): the only
 * allocation after creation; if it fails the call is VMX_ERR_NOMEM and the handle is untouched.  A call in place
 * (d_out_rgbaz == d_in_rgbaz) costs one more dense pass, because the window reads neighbouring blocks' input.
 * tests/adaptive_spec.py restates it; the kernels hold to it bit for bit. */
#define VMX_ADAPTIVE_EPS 1e-10f
typedef struct vmx_adaptive_params {
    float gamma;               /* finite, > 0;  default 3.f   (standard errors)   */
    float min_support;         /* finite, >= 1; default 4.f   (effective taps)    */
    uint32_t normal_squarings; /* 0..8;         default 5                         */
    float sigma_depth;         /* finite, > 0;  default 0.1f                      */
    uint32_t reserved[4];      /* must be 0                                       */
} vmx_adaptive_params;
int vmx_adaptive_default_params(vmx_adaptive_params *out);
int vmx_temporal_accumulate_adaptive_device(vmx_temporal *t, const vmx_camera *cam, const void *d_rayhit,
                                            const void *d_motion /* or NULL */, const void *d_in_rgbaz,
                                            void *d_out_rgbaz, void *d_rgba8, void *d_history_len, void *d_variance,
                                            void *d_change /* W*H floats or NULL */, const vmx_temporal_params *tparams,
                                            const vmx_variance_params *vparams, const vmx_adaptive_params *aparams,
                                            void *stream);

/* ---- guided upsampling: render small, reconstruct at full size ----------------------------------------------
 * A render costs rays = pixels x samples, a G-buffer one camera ray per pixel at any size.  So paths are traced at a
 * reduced resolution (and denoised there) and the full-size frame is reconstructed under a full-size G-buffer: joint
 * bilateral upsampling (Kopf et al. 2007) with the guide the filter already uses, a 2 x 2 tent footprint.
 *
 * Pixel x of a W-wide image is centred on sensor coordinate x / W (pathtracer.cpp:251-252, no half-pixel offset), and a
 * low camera that differs from the full one only in image_res sees the same field: full pixel x lies at low coordinate
 * x*lw/W.  Inputs: a low frame `lo` of lw x lh RGBAZ pixels; a low and a full guide, each (n, z) per pixel exactly as
 * the filter packs them from vmx_rayhit records ((normal, distance) where flags bit 0 is set, ((0, 0, 0), -1) elsewhere;
 * "a hit" is z >= 0).  1 <= lw <= W <= 4*lw and 1 <= lh <= H <= 4*lh; the ratios need not be integers.
 *
 * Per full pixel p = (x, y), all in float, one rounding per written operation, left to right, denormals kept:
 *   rx = (float)lw / (float)W;  ry = (float)lh / (float)H                                                 (once per call)
 *   u = (float)x * rx;  X0 = min((int)floorf(u), lw-1);  fx = u - (float)X0;       v, Y0, fy alike from y, ry, lh
 *     (the min acts only where rounding lifts u to lw, beyond 2^21 pixels across: it keeps tap (0, 0) inside)
 *   isz = 1.f / (sigma_depth * z_p)                                                       (used where p is a hit)
 *   sum_c = (0, 0, 0);  sum_w = 0;  best_b = -1
 *   taps j = 0..1 (outer), i = 0..1 (inner):  q = (X0 + i, Y0 + j); a tap with X0+i >= lw or Y0+j >= lh is outside
 *   and skipped;
 *     b = (j ? fy : 1.f - fy) * (i ? fx : 1.f - fx)
 *     if b > best_b:  best_b = b, anchor = q         (strictly greater: ties keep the earlier tap; tap (0, 0) is inside)
 *     a tap with (z_q >= 0) != (z_p >= 0) contributes nothing further
 *     p a hit:  d = n_p.x*n_q.x + n_p.y*n_q.y + n_p.z*n_q.z;  d = d > 0 ? d : 0;  normal_squarings times d = d*d;
 *               t = (z_p - z_q) * isz;  num = b * d;  g = 1.f + t*t               p a miss:  num = b;  g = 1.f
 *     w = num / g;   if w > 0 and finite:  sum_c. = sum_c. + w * lo_q.;  sum_w = sum_w + w
 *   out.rgb = sum_w > 0 ? sum_c. / sum_w : lo_anchor.rgb   (the fallback: no tap of p's kind, a zero or NaN normal, a
 *   z_p so small that isz overflows);  out.alpha, out.depth = lo_anchor's, bitwise, always
 *   rgba8 = vmx_quantize_device's arithmetic on that output pixel
 * The kernel holds to this restatement bit for bit (tests/upsample_spec.py).
 * Out of scope: upsampled progressive previews, multi-device frames, fusing the filter's last iteration into this call,
 * and a temporal pass at full size after it. */
typedef struct vmx_upsample_params {
    uint32_t normal_squarings; /* 0..8;        default 5                          */
    float sigma_depth;         /* finite, > 0; default 0.1f                       */
    uint32_t reserved[6];      /* must be 0                                       */
} vmx_upsample_params;

typedef struct vmx_upsample vmx_upsample;

int vmx_upsample_default_params(vmx_upsample_params *out);
/* An upsampler from low_width x low_height frames to width x height frames on `device`.  It owns the two packed guides
 * (16 B per pixel each); nothing is allocated after creation.  A zero size, a size outside the limits above, or a frame
 * vmx_render would call too large, is VMX_ERR_INVALID; without a usable device VMX_ERR_NO_DEVICE. */
int vmx_upsample_create(int device, uint32_t low_width, uint32_t low_height, uint32_t width, uint32_t height,
                        vmx_upsample **out);
int vmx_upsample_destroy(vmx_upsample *u);
/* d_rayhit_low, d_rayhit_full: low_width*low_height and width*height vmx_rayhit records in pixel order (what
 * vmx_raycast_camera_device writes for the low and the full camera), 16-byte aligned DEVICE memory of the handle's
 * device, packed into the handle's guides on `stream`.  The guides stay until the next call. */
int vmx_upsample_set_guides_device(vmx_upsample *u, const void *d_rayhit_low, const void *d_rayhit_full, void *stream);
/* Reconstructs the lw*lh*5-float frame d_low_rgbaz into d_out_rgbaz (W*H*5 floats) and / or d_rgba8 (W*H*4 bytes); at
 * least one of the two must be non-NULL.  params == NULL selects the defaults; a field out of range or a non-zero
 * reserved word is VMX_ERR_INVALID before any launch, as is a call before any guides were set.  The sizes differ, so
 * there is no in-place form: any overlap of the input with an output, or of the two outputs, is VMX_ERR_INVALID.
 * Pointers are checked as vmx_query_device checks its own (DEVICE memory of the handle's device) and must be 4-byte
 * aligned.  Enqueued on `stream`, no synchronisation.  Calls on one handle from different streams are ordered by
 * enqueue (each waits on an event the previous one recorded), as vmx_filter_apply_device's are. */
int vmx_upsample_apply_device(vmx_upsample *u, const void *d_low_rgbaz, void *d_out_rgbaz, void *d_rgba8,
                              const vmx_upsample_params *params, void *stream);

/*
 * Multi-GPU assembly on the root: `d_gathered` = world packed per-rank buffers
 * back to back, each padded to `rank_stride_floats`; writes the W*H*5 frame.
 */
int vmx_assemble_device(const void *d_gathered, uint64_t rank_stride_floats, uint32_t width,
                        uint32_t height, uint32_t stripe_rows, uint32_t world, void *d_frame,
                        int device, void *stream);

/* ---- multi-device render in one process ---------------------------------------------------
 * Vermilion's main.cpp (main.cpp:58-104) is ONE process; these entry points let its Integrator use
 * every GPU of the node: the scene is replicated on each device of the list (one host-side BVH build,
 * one upload per device), every replica renders its interleaved stripes of `stripe_rows` rows
 * (vmx_opts.rank/world are set by the library; the RNG is keyed by the global pixel, so the frame does
 * not depend on the device count), the packed stripes are pushed device-to-device into a gather buffer
 * on devices[0] (peer copies over xGMI — each peer has its own link to the root, no ring) and
 * de-interleaved there.  A device may appear more than once in the list (rehearsal of the N-rank path
 * on fewer GPUs).  The result is bit-identical to vmx_render on one device.
 */
typedef struct vmx_multi vmx_multi;
int vmx_multi_create(const float *pos, const float *nrm, const float *uv, uint32_t ntris, const vmx_sphere *spheres,
                     uint32_t nspheres, uint32_t leaf_size, uint32_t builder, const int *devices, uint32_t ndevices,
                     vmx_multi **out);
int vmx_multi_destroy(vmx_multi *m);
uint32_t vmx_multi_world(const vmx_multi *m);
/* per entry of the device list: its device, and how its stripes reach devices[0] — 2 same device, 1 direct peer
 * copy (xGMI), 0 staged through the host (peer access unavailable; a warning went to stderr at creation).
 * Either array may be NULL; each holds vmx_multi_world() ints. */
int vmx_multi_routes(const vmx_multi *m, int *devices, int *routes);
/* The exchange step of the LAST vmx_multi_render* call, timed apart from the rendering ("gather time
 * separately"): hipEvent pairs on each replica's stream around its stripes' copy into the root's gather buffer and on the
 * root's stream around the de-interleave kernel.  render_ms / copy_ms: per entry of the device list
 * (vmx_multi_world() doubles each), either may be NULL. */
typedef struct vmx_multi_times {
    double slowest_render_ms; /* max over the replicas of vmx_stats.ms_device of its stripes' render  */
    double gather_ms;         /* max over the replicas of its device-to-device (or staged) copy        */
    double gather_sum_ms;     /* sum of those copies                                                    */
    double assemble_ms;       /* k_assemble on devices[0]                                               */
    double wall_ms;           /* host clock from handing the jobs out to the assembled frame            */
    uint32_t world, pad;
} vmx_multi_times;
int vmx_multi_timings(const vmx_multi *m, vmx_multi_times *out, double *render_ms, double *copy_ms);
int vmx_multi_bind_texture(vmx_multi *m, const float *data, uint32_t width, uint32_t height, uint32_t channels);
/* vmx_scene_update on every replica (HOST arrays).  Host builders with VMX_UPDATE_REBUILD: one host build, uploaded to
 * each device; device builders build on each device.  The frame is bit-identical to one scene updated the same way. */
int vmx_multi_update(vmx_multi *m, const float *pos, const float *nrm, const float *uv, uint32_t ntris, uint32_t flags);
/* vmx_scene_set_spheres on every replica, and on the host copy of the table that later vmx_multi_* calls read.  A table
 * that is refused is refused before any replica changed.  If a device fails part-way (VMX_ERR_HIP), the replicas already
 * changed are given the old table back, so every replica renders the old table again; their generation has moved on,
 * so progressive handles of those replicas end as after any update. */
int vmx_multi_set_spheres(vmx_multi *m, const vmx_sphere *spheres, uint32_t nspheres);
/* whole frame (W*H*5 floats) into a caller-owned HOST buffer / into DEVICE memory on devices[0];
 * stats: rays and samples summed over the devices, times = the slowest device's */
int vmx_multi_render(vmx_multi *m, const vmx_camera *cam, const vmx_opts *opts, float *out_rgbaz, vmx_stats *stats);
int vmx_multi_render_device(vmx_multi *m, const vmx_camera *cam, const vmx_opts *opts, void *d_out_rgbaz,
                            vmx_stats *stats);
int vmx_multi_render_bruteforce(vmx_multi *m, const vmx_camera *cam, const vmx_opts *opts, uint32_t flags,
                                float *out_rgbaz, vmx_stats *stats);

/* ---- adaptive sampling: progressive steps that trace only the unconverged pixels ---------------------------------
 * vmx_progressive_step gives every active pixel the same samples.  The entries below let a step take samples for a
 * subset of the pixels, keep the second moment from which to choose that subset, and choose it.  Sample k of local pixel
 * p is what it always was, keyed (seed, p, k), and a pixel's samples are folded in its own order: whatever the steps and
 * maps, a handle that is run to completion holds vmx_render's frame, bit for bit.
 *
 * begin_ex: flags 0 is vmx_progressive_begin exactly; VMX_PROGRESSIVE_MOMENTS makes the handle keep, per pixel, the sum m2
 *   of the squared luminance of its samples: right after the three colour adds of a taken sample s,
 *     l = lum(s.r, s.g, s.b);  m2 = m2 + l*l         (lum as in the variance section; a black path adds an exact +0)
 *   Sums, counts, frames and previews of a moments handle are a plain handle's, bit for bit.  Any other bit of `flags` is
 *   VMX_ERR_INVALID.
 * state_device: the handle's raw state per local pixel, copied on the handle's stream without synchronising: d_sums
 *   float4 (r, g, b sums; w = m2 on a moments handle, else 0) and / or d_counts uint32; at least one must be non-NULL;
 *   DEVICE pointers of the scene's device, 4-byte aligned, not overlapping.
 * step_selected_device: a step in which only the pixels with d_select[p] != 0 (one byte per local pixel, a DEVICE
 *   pointer, read during the call) take samples.  A pixel takes samples only if it is active (fewer than kmax samples so
 *   far) and selected; it takes min(samples, kmax - its count) of them, the next ones in its own order; samples == 0 runs
 *   the selected pixels to kmax.  Unselected pixels keep their state bit for bit and stay active.  A step with no selected
 *   active pixel is VMX_OK, issues nothing and does not count as a step.  *selected (may be NULL) is the number of pixels
 *   that took samples; stats and vmx_scene_timings report this step alone, stats.samples the samples folded.
 *   Afterwards the handle is ragged — its pixels hold different counts.  vmx_progressive_step still works on it: every
 *   active pixel takes at least one sample and at most `samples`, 0 runs everyone to kmax; pixels_active is the number of
 *   pixels below kmax; the previews show an unfinished pixel as the clamped mean of its own n samples with depth n.
 *   Works under rank / world / stripe_rows (maps are indexed by LOCAL pixel), VMX_SAMPLING_ELIDE_DEAD,
 *   VMX_SAMPLING_CORRECTED and every pipeline form of the product.  A handle that never takes a selected step
 *   schedules, renders and previews exactly as before.
 * Error, variance and selection, per local pixel p, n = count, (sr, sg, sb, m2) = sums, fn = (float)n.  All float, one
 * rounding per written operation, `/` and sqrtf correctly rounded, denormals kept:
 *   n < 2:  e = 3.402823466e+38f;  var = 0.f
 *   else:   m1 = lum(sr, sg, sb) / fn
 *           v = m2/fn - m1*m1;  v = v > 0 ? v : 0                        (a NaN gives 0)
 *           var = v / (fn - 1.f)                                         (the variance of the pixel's mean luminance)
 *           e = sqrtf(var) / (fabsf(m1) + floor)
 *   error_device: d_error[p] = e and / or d_variance[p] = var (W * rows floats each, the layout
 *     vmx_filter_apply_variance_device reads; at least one non-NULL; 4-byte aligned, not overlapping).
 *   select_device: d_select[p] = cursor_p < kmax && (n_p < min_samples || max over q of e_q > threshold) ? 1 : 0, q over the
 *     (2*radius+1)^2 window around p, taps clipped to the handle's local rows and width — under world > 1 the window is
 *     taken in the rank's packed rows and never sees another rank's pixels, so it does not cross stripe borders as the
 *     full image would.  Comparisons with a NaN are false.  d_count (one uint32, or NULL) receives the number of selected
 *     pixels.  d_select is one byte per local pixel and may not overlap d_count.
 *   step_adaptive: select_device into a map the handle owns, then step_selected_device with it: the same state as the
 *     two calls by hand.
 * Order of checks: params, then the pointers (NULL, alignment, buffers that meet in their first element), then the handle
 * and how it was begun, then what needs the device (pointer kinds, overlaps at the image's size), then the handle's state.  The selection entries (step_selected_device,
 * select_device, step_adaptive) are VMX_ERR_INVALID on a handle begun with opts.early_stop == 1: the early-stop schedule
 * assumes that all pixels advance together, and the reference's rule is a different stopping rule.  error_device,
 * select_device and step_adaptive are VMX_ERR_INVALID on a handle begun without VMX_PROGRESSIVE_MOMENTS.
 * Defaults (vmx_sampling_default_params): threshold 0.5f, floor 0.05f, min_samples 8, radius 1 — threshold and floor as
 * chosen from the grid of profiles/sampling_quality.txt.  tests/sampling_spec.py restates the arithmetic.
 * Out of scope: selection on early-stop handles, per-pixel sample budgets on handles that are not light-sampled (the
 * budgeted steps of the light sampling section), windows across ranks, adaptive sampling inside vmx_render and
 * vmx_multi_*. */
#define VMX_PROGRESSIVE_MOMENTS 1u
int vmx_progressive_begin_ex(vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts, uint32_t flags, void *stream,
                             vmx_progressive **out);
int vmx_progressive_state_device(vmx_progressive *p, void *d_sums /* or NULL */, void *d_counts /* or NULL */);
int vmx_progressive_step_selected_device(vmx_progressive *p, uint32_t samples, const void *d_select, vmx_stats *stats,
                                         uint32_t *selected /* or NULL */);
typedef struct vmx_sampling_params {
    float threshold;      /* finite, >= 0; default 0.5f  */
    float floor;          /* finite, > 0;  default 0.05f */
    uint32_t min_samples; /* >= 2;         default 8     */
    uint32_t radius;      /* 0..3;         default 1     */
    uint32_t reserved[4]; /* must be 0                   */
} vmx_sampling_params;
int vmx_sampling_default_params(vmx_sampling_params *out);
int vmx_progressive_error_device(vmx_progressive *p, const vmx_sampling_params *params, void *d_error /* or NULL */,
                                 void *d_variance /* or NULL */);
int vmx_progressive_select_device(vmx_progressive *p, const vmx_sampling_params *params, void *d_select,
                                  void *d_count /* one uint32, or NULL */);
int vmx_progressive_step_adaptive(vmx_progressive *p, uint32_t samples, const vmx_sampling_params *params,
                                  vmx_stats *stats, uint32_t *selected /* or NULL */);

/* ---- BruteForceTracer: the engine's DEFAULT integrator --------------------
 * Replaces Vermilion::BruteForceTracer::Render (core/integrators/integrators.cpp:9-186; installed by
 * RenderEngine::Initialise when no integrator is assigned, core/engines/renderEngine.cpp:49-53):
 * per pixel up to raysPerPixel jittered camera rays (:59-81), N.L against a point light at
 * (500,1100,2000) (:16,83-88), the normal perturbed by boundTextures[0] (:98-106), one mirror
 * probe whose MISS lifts the term to 0.9 N.L + 0.1 (:119-137), albedo from boundTextures[1] or the
 * constant (0.890196078, 0.258823529, 0.203921569) (:141-156), and a convergence break once more
 * than two samples are in (:166-172).  Output layout as vmx_render (RGBAZ, camera.cpp:106-113) with
 * alpha = accum.w / samples (the hit fraction, :180) and depth = the LAST sample's hitDistance
 * (:181; INFINITY after a miss, meshEngine.cpp:507).  vmx_opts: seed, rank/world/stripe_rows are
 * used (the jitter of sample s of pixel p comes from the stream keyed (seed, p, s): the reference
 * shares one time(0)-seeded std::mt19937 between its OpenMP threads, :30, and is not reproducible);
 * early_stop / sampling / samples_per_batch do not apply.  rays_per_pixel must be 1..65535 (the
 * reference's loop counter is a uint16_t, :59).
 */
#define VMX_BF_ABS_INT 1u /* read the unqualified `abs(float)` of integrators.cpp:170 as C's abs(int) (the sum is
                             truncated to int first) instead of std::abs(float), the default */
int vmx_render_bruteforce(const vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts, uint32_t flags,
                          float *out_rgbaz, vmx_stats *stats);
int vmx_render_bruteforce_device(const vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts, uint32_t flags,
                                 void *d_out_rgbaz, void *stream, vmx_stats *stats);

/* ---- light sampling: a path integrator with next-event estimation ---------------------------
 * A third integrator entry beside vmx_render* and vmx_render_bruteforce*; this build's own (the reference has none).
 * Under VMX_SAMPLING_CORRECTED a path of vmx_render collects light only by hitting a VMX_SPHERE_EMIT sphere by chance.
 * Here every diffuse step samples the emitters directly.  The estimator is Radiance (pathtracer.cpp:21-198) with r2 = U
 * and one more bit of state per path, `lit`, false at the start:
 *   1. RayCast; a miss returns.
 *   2. !lit: accumColour += accumRadiance * hitColour.  At depth 0, accumColour.w = distance.
 *   3. length(hitColour) > 1 returns, lit or not (the path distribution stays that of `corrected`).
 *   4. Russian roulette, the texture sample, the branch draw and the arms follow the reference draw for draw, the three
 *      unused draws of an arm included.  The specular arm sets lit = false.
 *   5. A diffuse arm (triangle or sphere) has w, the flipped normal, has multiplied accumRadiance by the sample colour
 *      (triangle arm), moves the origin to x = hit - dir * 0.001 and draws the bounce direction.
 *   6. It then runs the emitter loop over the VMX_SPHERE_EMIT spheres in table order, float32 unless stated:
 *        op_i = c_i - x, C_i = dot(op_i, op_i), R2_i = r_i * r_i, as sphereIntersect forms them.
 *        If C_i <= R2_i for any emitter (x inside or on it): no draw is consumed and lit = false.
 *        Else for every emitter i two draws xi1, xi2 (always consumed), then in DOUBLE
 *          s2 = R2_i / C_i,  q_i = s2 / (1 + sqrt(1 - s2)),  Omega = 2 pi q_i,
 *          z = xi1 q_i,  cos t = 1 - z,  sin t = sqrt(z (2 - z));
 *        phi = float(2 pi xi2), its cosine and sine by cosf / sinf (VMX_SAMPLING_LIBM_DOUBLE: C's double functions);
 *        a_i = normalize(op_i), u = normalize(cross(|a.x| > .1 ? (0,1,0) : (1,0,0), a)), v = cross(a, u);
 *        omega = normalize((u cos(phi) float(sin t) + v sin(phi) float(sin t)) + a float(cos t)).
 *        The sample is dropped if 0.5 * double(|omega - a_j|^2) <= q_j for an emitter j < i (overlapping cones count
 *        once: the earlier emitter's sample owns the direction), or if dot(w, omega) <= 0.  Otherwise RayCast(x, omega)
 *        and accumColour.rgb += (accumRadiance.rgb * hitColour) * float(double(dot(w, omega)) / pi * Omega).
 *        Then lit = true.
 * RayCast's own hitColour is used, so the reference's quirks stay: an emitter shines through a nearer non-emitting
 * sphere that the table lists after it, and a later nearer triangle-less wall never clears the colour.
 *
 * vmx_opts: (sampling & VMX_SAMPLING_MODE_MASK) must be VMX_SAMPLING_CORRECTED (parity's r2 = 10 U has no estimator to
 * improve); VMX_SAMPLING_LIBM_DOUBLE is honoured; seed and samples_per_batch apply as in vmx_render.  VMX_ERR_INVALID,
 * with a message naming it, for VMX_SAMPLING_ELIDE_DEAD, early_stop != 0, world > 1, collect_counters and a non-zero
 * reserved[0].  Frame layout as vmx_render: W * H * 5 floats, rgb = clamp(sum / n, 0, 1) with the samples added in
 * ascending k, alpha 1, the fifth float n; sample k of pixel p uses the stream keyed (seed, p, k): two jitter draws,
 * then the path.  vmx_stats: rays_primary as vmx_render, rays_secondary = bounce rays + the shadow rays traced, samples.
 * vmx_render_nee_device follows vmx_render_device's stream and output conventions.  vmx_radiance_nee treats ray i as
 * vmx_radiance does: stream (seed, i, 0) past its two jitter draws, unclamped accumColour, w = primary hit distance.
 * Valid after vmx_scene_update*, vmx_scene_set_spheres and vmx_scene_bind_texture, on scenes of any builder.
 */
int vmx_render_nee(const vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts, float *out_rgbaz, vmx_stats *stats);
int vmx_render_nee_device(const vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts, void *d_out_rgbaz,
                          vmx_stats *stats, void *stream);
int vmx_radiance_nee(const vmx_scene *scene, const float *origin, const float *dir, uint32_t n, const vmx_opts *opts,
                     float *out4, vmx_stats *stats);

/* ---- light sampling in progressive handles, with per-pixel sample budgets ---------------------------------------------
 * begin_nee: a vmx_progressive whose passes run the light-sampling integrator.  flags is 0 or VMX_PROGRESSIVE_MOMENTS; it
 *   accepts exactly the vmx_opts vmx_render_nee accepts, with the same messages.  The refusals that need no device come
 *   in the order cam / opts, out, flags, opts contents, frame, scene.  Every entry that takes a handle works on it with
 *   its documented meaning: step, info_get, end, the plain, filtered and demodulated previews, state_device,
 *   step_selected_device, error_device, select_device, step_adaptive; "scene updated since vmx_progressive_begin" and the
 *   `failed` latch apply as on plain handles.  Sample k of local pixel p runs on stream (seed, p, k) and a pixel's samples
 *   are folded in ascending k: whatever the schedule of steps, maps and budgets, a handle run to completion holds
 *   vmx_render_nee's frame, bit for bit.  A moments handle folds l*l right after the three colour adds and is otherwise a
 *   plain light-sampled handle bit for bit.
 *
 * Budgeted steps (handles begun with begin_nee only).  A selected step gives every selected pixel the same samples; the
 * error statistic says how many each needs: the standard error of a mean falls as 1 / sqrt(n), so a pixel at error e with
 * n samples needs about n (e / threshold)^2.  One budgeted step gives every pixel its own count, in ONE pass.
 * B = the handle's effective samples_per_batch; cap = max_step ? min(max_step, B) : B.
 * budget_device: d_budget[p], one uint32 per local pixel; d_total (one uint64, or NULL) receives their sum.  Enqueued on
 *   the handle's stream without synchronising.  Per local pixel p, n = count, fn = (float)n, e_q exactly error_device's
 *   error under select.floor; all float, one rounding per written operation, `/` correctly rounded, denormals kept:
 *     cursor_p >= kmax                  : b = 0
 *     n < select.min_samples            : want = select.min_samples - n
 *     else  E = max over select_device's window of e_q   (x > E ? x : E from E = 0: a NaN never wins)
 *           !(E > select.threshold)     : b = 0
 *           else r = E / select.threshold;  t = (fn * r) * r;  d = ceilf(t) - fn
 *                want = d >= (float)cap ? cap : (d >= 1.f ? (uint32_t)d : 1)     (a NaN d gives 1; inf gives cap)
 *     b = min(want, cap, kmax - n)
 *   b_p != 0 exactly where select_device writes 1 under the same `select` params.
 * step_budget_device: every active pixel p takes min(d_budget[p], B, kmax - n_p) samples, the next ones in its own order,
 *   in one pass (the clamp by B keeps the pass within the radiance workspace the handle already sizes).  Pixels with
 *   budget 0 keep their state bit for bit and stay active.  A step whose budgets are all 0 is VMX_OK, issues nothing and
 *   does not count as a step.  *selected (may be NULL) is the number of pixels that took samples, stats.samples the samples
 *   folded, stats.passes 1.  Afterwards the handle is ragged, exactly as after a selected step.  d_budget is a DEVICE
 *   pointer, read during the call.
 * step_budgeted: budget_device into a plane the handle owns, then step_budget_device: the same state as the two calls by
 *   hand.
 * Order of checks: params, then the pointers (NULL, 4-byte alignment, 8-byte for d_total, buffers that meet in their
 * first element), then the handle and how it was begun, then what needs the device (pointer kinds, overlaps at the image's
 * size), then the handle's state.  All three are VMX_ERR_INVALID on a handle not begun with begin_nee (budgeted steps are
 * built for light-sampled handles only); budget_device and step_budgeted on a handle without VMX_PROGRESSIVE_MOMENTS.
 * Defaults (vmx_sampling_budget_default_params): select as vmx_sampling_default_params, max_step 0.
 * tests/budget_spec.py restates the rule and a budgeted step's fold.
 * Out of scope: budgeted steps on plain handles (k_raygen / k_paths would need the same per-item work source, and this
 * section leaves them untouched); splitting a budget above B over several passes; multi-device light-sampled handles. */
int vmx_progressive_begin_nee(vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts, uint32_t flags, void *stream,
                              vmx_progressive **out);
typedef struct vmx_sampling_budget_params {
    vmx_sampling_params select; /* as vmx_sampling_default_params */
    uint32_t max_step;          /* 0: the handle's samples per batch; default 0 */
    uint32_t reserved[3];       /* must be 0 */
} vmx_sampling_budget_params;
int vmx_sampling_budget_default_params(vmx_sampling_budget_params *out);
int vmx_progressive_budget_device(vmx_progressive *p, const vmx_sampling_budget_params *params, void *d_budget,
                                  void *d_total /* one uint64, or NULL */);
int vmx_progressive_step_budget_device(vmx_progressive *p, const void *d_budget, vmx_stats *stats,
                                       uint32_t *selected /* or NULL */);
int vmx_progressive_step_budgeted(vmx_progressive *p, const vmx_sampling_budget_params *params, vmx_stats *stats,
                                  uint32_t *selected /* or NULL */);

/* ---- light sampling across ranks and devices, and on device batches ---------------------------------------------------
 * The entries above keep their contract exactly, "world > 1 is not supported" included.  The entries below reach the
 * library's scale-out seams through the same routine and the same kernels (k_nee keys every stream by the GLOBAL pixel,
 * so no frame depends on how it is cut).
 *
 * vmx_render_nee_rank / _rank_device: vmx_render_nee / vmx_render_nee_device with opts.rank, opts.world and
 *   opts.stripe_rows honoured as vmx_render / vmx_render_device honour them: the output is the rank's rows of
 *   vmx_render_nee's frame, bit for bit, packed in ascending order — vmx_local_rows() rows of W * 5 floats; world 0 or 1
 *   gives the whole frame; vmx_stats covers the rank's pixels only.  Refusals that need no device, in this order: a NULL
 *   cam / opts / output, the opts contents (vmx_render_nee's checks and messages in their order, without the world one),
 *   the frame (vmx_render's checks, "rank must be < world" among them), the NULL scene.  A rank that owns no row (more
 *   ranks than stripes) behaves as in vmx_render_device: VMX_OK, nothing is launched, the output is not written (it must
 *   still be non-NULL) and *stats is zeroed.
 * vmx_progressive_begin_nee_rank: vmx_progressive_begin_nee with world > 1 accepted.  Every entry that takes a handle
 *   works on it with LOCAL pixel indices, as on a plain handle begun with world > 1: step, the previews (the filtered and
 *   demodulated ones stay "whole images only"), state_device, the selected and adaptive steps, budget_device,
 *   step_budget_device, step_budgeted.  The windows of select_device and budget_device are taken in the rank's packed rows
 *   and stop at the rank's own rows: they never see another rank's pixels, so a rank's maps and budgets near a stripe
 *   border differ from what the whole image would give.  Whatever the schedule, a handle run to completion holds the
 *   rank's rows of vmx_render_nee's frame, bit for bit.
 * vmx_multi_render_nee / _device: vmx_multi_render / _device whose replicas render their stripes through the routine of
 *   vmx_render_nee_rank_device; gather, assembly and vmx_multi_timings are those of vmx_multi_render.  The frame is
 *   vmx_render_nee's, bit for bit, for any device list; rays and samples are summed over the replicas, times are the
 *   slowest replica's.  The library sets rank and world: the caller's opts are checked as vmx_render_nee checks them, so a
 *   caller's world > 1 is refused.  Order: NULL cam / opts / output, the opts contents, the NULL vmx_multi.  Valid after
 *   vmx_multi_update, vmx_multi_set_spheres and vmx_multi_bind_texture.
 * vmx_radiance_nee_device: vmx_radiance_nee on DEVICE arrays of the scene's device — d_origin and d_dir n x 3 floats,
 *   d_out4 n x 4 floats — enqueued on `stream` (NULL: the scene's stream).  Like vmx_render_nee_device it returns when the
 *   batch is done (vmx_stats is the counters' read-back).  Order of checks: NULL d_origin / d_dir / opts / d_out4, the opts
 *   contents, n == 0 (VMX_OK, whatever follows), the rays' 4-byte alignment, d_out4's 16-byte alignment, n > 2^31 - 1,
 *   d_out4 overlapping either ray array (results are written while other rays are still read), the NULL scene; then, on
 *   the device, the pointer kinds as vmx_raycast_device checks them (origin, dir, d_out4).  vmx_radiance_nee is an upload,
 *   this routine and a download.
 * Measured on one device only (profiles/nee_multi.txt): no node with several GPUs has run this project, so peer copies
 * between distinct devices stay unexecuted and no scaling curve is claimed.
 * Out of scope: early stop under light sampling, windows across ranks, multi-device progressive handles. */
int vmx_render_nee_rank(const vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts, float *out_local, vmx_stats *stats);
int vmx_render_nee_rank_device(const vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts, void *d_out_local,
                               vmx_stats *stats, void *stream);
int vmx_progressive_begin_nee_rank(vmx_scene *scene, const vmx_camera *cam, const vmx_opts *opts, uint32_t flags, void *stream,
                                   vmx_progressive **out);
int vmx_multi_render_nee(vmx_multi *m, const vmx_camera *cam, const vmx_opts *opts, float *out_rgbaz, vmx_stats *stats);
int vmx_multi_render_nee_device(vmx_multi *m, const vmx_camera *cam, const vmx_opts *opts, void *d_out_rgbaz, vmx_stats *stats);
int vmx_radiance_nee_device(const vmx_scene *scene, const void *d_origin, const void *d_dir, uint32_t n, const vmx_opts *opts,
                            void *d_out4, vmx_stats *stats, void *stream);

/* ---- light sampling: emissive triangles as area lights -----------------------------------------------------------------
 * A per-scene table names triangles (by their createBVH-order id) that emit, each with a radiance; both faces emit.  The
 * table means something to the LIGHT-SAMPLED integrator only (vmx_render_nee*, vmx_radiance_nee*, light-sampled
 * progressive handles, the rank entries and vmx_multi_render_nee*).  vmx_render*, BruteForceTracer, the queries,
 * vmx_raycast*, the albedo plane and the image-space chain see ordinary unlit triangles, exactly as before.  A scene
 * without a table is, bit for bit and instruction for instruction, the scene it was before this section existed.
 *
 * vmx_scene_set_emitters replaces the table (NULL, 0 clears it).  VMX_ERR_INVALID, in this order and before any device
 * work: a NULL scene; NULL with n > 0; n > VMX_MAX_EMITTERS or n > the scene's triangle count; an id >= that count; a
 * repeated id; a radiance component that is negative or not finite.  vmx_emitters_check runs the checks after the
 * scene's against a triangle count alone (what a host can validate before it has a scene).  The call takes the scene's
 * lock and moves its generation on as vmx_scene_set_spheres does: progressive handles begun before it refuse further
 * steps.  vmx_multi_set_emitters does the same on every replica.
 * vmx_scene_emitters reads the DERIVED table back: *n = the table's length, out[0 .. min(cap, *n)) filled.
 *
 * Definition, in addition to the numbered definition of light sampling above; tests/nee_mesh_spec.py restates it and the
 * kernel matches it bit for bit.
 *   E1. Override.  For every RayCast the integrator makes (path rays, cone shadow rays, area shadow rays): if the returned
 *       hit is the BVH's triangle (tri_id >= 0 and distance == tri_t: no sphere came nearer; the material bit stays set
 *       behind a sphere and cannot be used) and that triangle is emitter e, hitColour = radiance_e.  hitColour is
 *       necessarily black there, so no sphere colour is lost.  Steps 2 and 3 then apply unchanged.
 *   E2. Derived table, in the caller's order, all in DOUBLE from the triangle record's float32 v0, e1 = v1 - v0,
 *       e2 = v2 - v0 widened:  Nraw = cross(E1, E2) (each component a*b - c*d, two roundings and one subtraction),
 *       nn = (Nx^2 + Ny^2) + Nz^2,  area = 0.5 sqrt(nn),  N = Nraw / sqrt(nn) per component,
 *       weight = area * double(luminance(radiance)) with the float32 luminance (0.2126 r + 0.7152 g) + 0.0722 b,
 *       cdf_e = cdf_{e-1} + weight_e sequentially from 0,  W = cdf_{n-1}.
 *   E3. The table is derived from the scene's CURRENT records: after any sequence of vmx_scene_update* (refit: the areas
 *       change; rebuild: the leaf slots permute) and builders, the table and every frame equal those of a fresh scene on
 *       the same arrays.  (It is rebuilt at the next light-sampled launch or vmx_scene_emitters, keyed by the generation.)
 *   E4. Sampling: in the emitter loop of a diffuse arm, after the last sphere emitter; skipped (no draw) when the point is
 *       inside an emitter sphere, by rule 6, or when W == 0.  Three draws xi0, xi1, xi2, always consumed.
 *         u = xi0 W;  e = the smallest index with cdf_e > u, clamped to n - 1;  p_e = weight_e / W.
 *         In DOUBLE:  s = sqrt(xi1), b1 = s (1 - xi2), b2 = s xi2,  y = (V0 + b1 E1) + b2 E2,  d = y - X (X = x widened),
 *         d2 = (dx^2 + dy^2) + dz^2,  omega_d = d * (1 / sqrt(d2)),  omega = float(omega_d) per component (not renormalised),
 *         cosl = |(Nx ox + Ny oy) + Nz oz| with o = omega_d,  dw = dot(w, omega) in float32,
 *         pdf = (p_e d2) / (area_e cosl),  wt = float((double(dw) / pi) / pdf).
 *       Dropped, with no ray: weight_e == 0, d2 == 0, cosl == 0, dw <= 0, wt not finite, the step's own hit was emitter
 *       e's triangle (E1's condition), or omega lies in the cone of ANY emitter sphere j: 0.5 double(|omega - a_j|^2)
 *       <= q_j (the spheres own their cones).  Otherwise RayCast(x, omega), and accumColour.rgb += (accumRadiance.rgb *
 *       hitColour) * wt only if the returned hit is emitter e's triangle.  lit is set as the sphere loop sets it.
 *       vmx_stats.rays_secondary counts the area shadow rays traced with the others.
 * Out of scope: one-sided emitters, textured emission, a mode that leaves triangles unsampled, more than one area sample
 * per step, emission in vmx_render / BruteForceTracer, MIS. */
#define VMX_MAX_EMITTERS 65536u
typedef struct vmx_emitter {
    uint32_t tri_id; /* createBVH-order id */
    float radiance[3];
} vmx_emitter;
typedef struct vmx_emitter_info {
    uint32_t tri_id;
    float radiance[3];
    double area;
    double weight;
    double cdf;
} vmx_emitter_info;
int vmx_scene_set_emitters(vmx_scene *scene, const vmx_emitter *emitters, uint32_t n);
int vmx_scene_emitters(const vmx_scene *scene, vmx_emitter_info *out, uint32_t cap, uint32_t *n);
int vmx_multi_set_emitters(vmx_multi *m, const vmx_emitter *emitters, uint32_t n);
int vmx_emitters_check(const vmx_emitter *emitters, uint32_t n, uint32_t ntris);

/* ---- frame output (the step after the path; replaces the conversion loop of
 * Camera::saveFrame, core/camera/camera.cpp:140-175, for the default RGBAZ mode) ------------ */
/*
 * rgba8[p*4 + c] = (unsigned char)floor(frame[p*5 + c] * 255)   c = 0..3   (camera.cpp:159-162)
 * depth[p]       = frame[p*5 + 4]                                          (camera.cpp:163)
 * All three pointers are DEVICE memory on `device`; depth may be NULL.  The PNG/EXR encoding
 * (OpenImageIO, camera.cpp:178-188) stays with the host application.
 */
int vmx_quantize_device(const void *d_frame_rgbaz, uint64_t npixels, void *d_rgba8, void *d_depth, int device,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VERMILION_HIP_H */
