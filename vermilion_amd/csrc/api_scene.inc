// api_scene.inc — part of vmx_api.cpp
extern "C" {

int vmx_abi_version(void) { return VMX_ABI_VERSION; }

const char *vmx_last_error(void) { return g_err.c_str(); }

int vmx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const vmx_sphere *vmx_default_spheres(uint32_t *count) {
    if (count) *count = 8;
    return kReferenceSpheres;
}

int vmx_scene_create(const float *pos, const float *nrm, const float *uv, uint32_t ntris,
                     const vmx_sphere *spheres, uint32_t nspheres, uint32_t leaf_size, int device,
                     vmx_scene **out) {
    return vmx_scene_create_ex(pos, nrm, uv, ntris, spheres, nspheres, leaf_size, VMX_BVH_REFERENCE, device, out);
}

// Where the records of a host-built scene lie in its ONE allocation (d_geom): the tree's inner records, its triangle
// records and 64 bytes of slack (the quad-cooperative fetch reads 64 bytes from a 48-byte triangle record's start); then,
// for a reference-tree scene with a guide (guide_walk.h), 64-byte aligned, the guide's records in the same shape with the
// same slack.  Offsets of the tree's own records do not depend on the guide.  guide_off = 0: no room is laid out for a
// guide — there is none, or the two trees together pass what a 32-bit record offset reaches (the scene then renders
// without one).  fits = false: the tree alone does.
struct GeomLayout {
    size_t inner_bytes, tri_bytes;              // the tree's records: [0, inner_bytes), then tri_bytes from there
    size_t guide_off, guide_inner_bytes, guide_tri_bytes;
    size_t total;                               // bytes of the allocation
    bool fits;
};
static GeomLayout geom_layout(size_t n_inner, size_t n_tris, bool guide, size_t guide_n_inner, size_t guide_n_tris) {
    GeomLayout l{};
    l.inner_bytes = std::max<size_t>(n_inner, 1) * sizeof(InnerRecord);
    l.tri_bytes = n_tris * sizeof(TriRecord);
    l.total = l.inner_bytes + l.tri_bytes + 64;
    l.fits = l.total <= 0xFFFFFFFFull;
    if (guide && l.fits) {
        const size_t off = (l.total + 63) & ~(size_t)63;
        const size_t gi = std::max<size_t>(guide_n_inner, 1) * sizeof(InnerRecord), gt = guide_n_tris * sizeof(TriRecord);
        if (off + gi + gt + 64 <= 0xFFFFFFFFull)
            l.guide_off = off, l.guide_inner_bytes = gi, l.guide_tri_bytes = gt, l.total = off + gi + gt + 64;
    }
    return l;
}

// the device records of a host-built tree, into `geom` (geom_layout; with room for `guide`'s records, which upload_guide
// writes) and `attrs`
static int upload_records(const HostBvh &b, const HostBvh *guide, DevBuf<unsigned char> &geom, DevBuf<AttrRecord> &attrs) {
    const GeomLayout l = geom_layout(b.inner.size(), b.tris.size(), guide != nullptr, guide ? guide->inner.size() : 0,
                                     guide ? guide->tris.size() : 0);
    if (!l.fits) return fail(VMX_ERR_INVALID, "scene too large for 32-bit record offsets");
    if (geom.ensure(l.total) || attrs.ensure(b.attrs.size()))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed for the scene");
    HIP_TRY(hipMemset(geom.p, 0, l.total));
    if (b.inner.size()) HIP_TRY(hipMemcpy(geom.p, b.inner.data(), b.inner.size() * sizeof(InnerRecord), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(geom.p + l.inner_bytes, b.tris.data(), l.tri_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(attrs.p, b.attrs.data(), b.attrs.size() * sizeof(AttrRecord), hipMemcpyHostToDevice));
    return VMX_OK;
}

// the guide's records (guide_walk.h) into the room upload_records left for them behind the records of sc->bvh in
// sc->d_geom (the same geom_layout of the same two trees; an allocation without that room: no guide)
static int upload_guide(vmx_scene *sc) {
    vmx_scene::Guide &g = sc->guide;
    g.valid = false, g.base = nullptr, g.off = 0, g.bytes = 0;
    if (!g.host || sc->device_built) return VMX_OK;
    const HostBvh &b = *g.host;
    const GeomLayout l = geom_layout(sc->bvh.inner.size(), sc->bvh.tris.size(), true, b.inner.size(), b.tris.size());
    if (!l.guide_off || sc->d_geom.n < l.total) return VMX_OK;  // (no guide: the scene renders as before)
    unsigned char *at = sc->d_geom.p + l.guide_off;
    if (b.inner.size()) HIP_TRY(hipMemcpy(at, b.inner.data(), b.inner.size() * sizeof(InnerRecord), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(at + l.guide_inner_bytes, b.tris.data(), l.guide_tri_bytes, hipMemcpyHostToDevice));
    g.base = at, g.off = (uint32_t)l.guide_off;
    g.bytes = b.inner.size() * sizeof(InnerRecord) + l.guide_tri_bytes;
    g.tri_off = (uint32_t)l.guide_inner_bytes, g.root_ref = b.root_ref, g.stack_entries = b.max_depth + 2;
    g.valid = true;
    return VMX_OK;
}

// one host build, at creation and at a REBUILD: the scene's tree and, for a reference-tree scene, its guide
// (guide_walk.h) — the quality tree of the same inputs, built beside it on a second thread.  A quality tree that cannot
// be built (too deep, no memory, no thread) leaves the scene without a guide; only the scene's own tree can fail.
struct HostTrees {
    HostBvh tree;
    std::shared_ptr<const HostBvh> guide;
    float scene_max = 0.f;
};
static bool host_build_trees(uint32_t builder, const float *pos, const float *nrm, const float *uv, uint32_t ntris,
                             uint32_t leaf_size, HostTrees &out, std::string &err) {
    std::shared_ptr<HostBvh> guide;
    std::thread guide_build;
    bool guide_ok = false;
    struct Joiner {  // (an exception of the build below must not meet a joinable thread)
        std::thread &t;
        ~Joiner() { if (t.joinable()) t.join(); }
    } joiner{guide_build};
    if (builder == VMX_BVH_REFERENCE) {
        try {
            guide = std::make_shared<HostBvh>();
            guide_build = std::thread([&guide_ok, guide, pos, nrm, uv, ntris, leaf_size] {
                try {
                    std::string gerr;
                    guide_ok = build_bvh_sah(pos, nrm, uv, ntris, leaf_size, *guide, gerr);
                } catch (...) {
                    guide_ok = false;
                }
            });
        } catch (...) {
            guide.reset();
        }
    }
    const bool built = builder == VMX_BVH_SAH ? build_bvh_sah(pos, nrm, uv, ntris, leaf_size, out.tree, err)
                                              : build_bvh(pos, nrm, uv, ntris, leaf_size, out.tree, err);
    if (guide_build.joinable()) guide_build.join();
    out.guide.reset();
    if (built && guide && guide_ok) {
        try {
            out.scene_max = make_guide_records(*guide, out.tree, pos, ntris);
            out.guide = guide;
        } catch (...) {
        }
    }
    return built;
}

// after a host REBUILD (sc->bvh is the new tree and sc->d_geom its allocation, laid out with room for t.guide; nothing in
// flight reads the old records): the guide that was built beside it, as a fresh scene would have it, or none.  A REFIT
// only marks the guide stale.
static int apply_guide(vmx_scene *sc, const HostTrees &t) {
    vmx_scene::Guide &g = sc->guide;
    g.host = t.guide, g.scene_max = t.scene_max;
    return upload_guide(sc);
}

// points the kernels' view of the scene (SceneDev) at its records; sizes what follows the tree's depth
static void bind_records(vmx_scene *sc) {
    if (sc->device_built) {
        // records were written on the device (k_lbvh_emit_*): the scene takes the builder's buffers over
        const LbvhDevice &l = sc->lbvh;
        sc->dev.inner = l.geom;
        sc->dev.tris = (const unsigned char *)l.geom + l.tri_off;
        sc->dev.tri_off = l.tri_off;
        sc->dev.attrs = l.attrs;
        sc->dev.root_ref = l.root_ref;
        sc->dev.stack_entries = l.height + 2;
        sc->n_inner = l.n_inner;
    } else {
        const HostBvh &b = sc->bvh;
        const size_t inner_bytes = std::max<size_t>(b.inner.size(), 1) * sizeof(InnerRecord);
        sc->dev.inner = sc->d_geom.p;
        sc->dev.tris = sc->d_geom.p + inner_bytes;
        sc->dev.tri_off = (uint32_t)inner_bytes;
        sc->dev.attrs = sc->d_attrs.p;
        sc->dev.root_ref = b.root_ref;
        sc->dev.stack_entries = b.max_depth + 2;
        sc->n_inner = (uint32_t)b.inner.size();
    }
    // LDS budget: shrink the block until one block's stacks fit in 64 KiB
    sc->block = 256;
    while (sc->block > 64 && (sc->block / 64) * sc->dev.stack_entries * 512 > 65536) sc->block /= 2;
}

// the (spheres, nspheres) pair of vmx_scene_create_ex, vmx_multi_create and vmx_*_set_spheres: checked the same way
static int sphere_table_args(const vmx_sphere *spheres, uint32_t nspheres) {
    if (spheres == nullptr && nspheres != 0)
        return fail(VMX_ERR_INVALID, "spheres is NULL but nspheres > 0 (NULL,0 selects the reference table)");
    if (nspheres > kMaxSpheres) return fail(VMX_ERR_INVALID, "more than 16 spheres");
    return VMX_OK;
}

// ... and what it selects: the caller's table, or the reference's for NULL
static std::vector<vmx_sphere> sphere_table(const vmx_sphere *spheres, uint32_t nspheres) {
    if (spheres) return std::vector<vmx_sphere>(spheres, spheres + nspheres);
    return std::vector<vmx_sphere>(kReferenceSpheres, kReferenceSpheres + 8);
}

// the normal_sign the kernels multiply by
static float sphere_sign(const vmx_sphere &s) { return s.normal_sign < 0.f ? -1.f : 1.f; }

// The device's form of a table — sd[kMaxSpheres], entries past the table zeroed — and what is derived from it
// (SceneDev::emit_prefix): the one place, for scene creation and for vmx_scene_set_spheres
static void derive_spheres(const std::vector<vmx_sphere> &table, SphereDev *sd, uint32_t &emit_prefix) {
    std::memset(sd, 0, kMaxSpheres * sizeof(SphereDev));
    emit_prefix = 0;
    for (size_t i = 0; i < table.size(); ++i) {
        const vmx_sphere &s = table[i];
        SphereDev &d = sd[i];
        d.cx = s.centre[0], d.cy = s.centre[1], d.cz = s.centre[2];
        d.rad = s.radius;
        d.rad2 = s.radius * s.radius;  // float product (meshEngine.cpp:188)
        d.colr = s.colour[0], d.colg = s.colour[1], d.colb = s.colour[2];
        d.ncx = s.normal_centre[0], d.ncy = s.normal_centre[1], d.ncz = s.normal_centre[2];
        d.nsign = sphere_sign(s);
        d.flags = s.flags;
        if (d.flags & 1u) emit_prefix = (uint32_t)i + 1;
    }
}

// VMX_CU_LIMIT (diagnostic; include/vermilion_hip.h): the compute units a scene counts, min(the device's, the limit).
// Lower-only: no kernel here synchronises across blocks, so a grid below the resident one is always safe (DESIGN.md §9),
// while a count above the device's would size "resident" grids that are not.  Unset, empty, 0 or unparsable: the device's.
static int limited_cus(int device_cus) {
    const char *e = std::getenv("VMX_CU_LIMIT");
    if (!e || !*e) return device_cus;
    char *end = nullptr;
    const unsigned long v = std::strtoul(e, &end, 10);
    if (end == e || *end != '\0' || v == 0 || v >= (unsigned long)device_cus) return device_cus;
    return (int)v;
}

// device half of scene creation: uploads sc->bvh / sc->spheres to sc->device (used for the first scene
// and for the replicas of a multi-device scene, which share one host-side build)
static int scene_upload(vmx_scene *sc) {
    const int device = sc->device;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    sc->num_cus = limited_cus(prop.multiProcessorCount);
    HIP_TRY(hipStreamCreateWithFlags(&sc->stream.s, hipStreamNonBlocking));

    // room for the largest table from the start: vmx_scene_set_spheres rewrites it in place, whatever its count
    SphereDev sd[kMaxSpheres];
    derive_spheres(sc->spheres, sd, sc->dev.emit_prefix);
    if (sc->d_spheres.ensure(kMaxSpheres)) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the scene");
    HIP_TRY(hipMemcpy(sc->d_spheres.p, sd, sizeof(sd), hipMemcpyHostToDevice));
    sc->dev.spheres = sc->d_spheres.p;
    sc->dev.nspheres = (uint32_t)sc->spheres.size();
    sc->dev.ntris = sc->ntris;
    if (!sc->device_built)
        if (int rc = upload_records(sc->bvh, sc->guide.host.get(), sc->d_geom, sc->d_attrs)) return rc;
    if (int rc = upload_guide(sc)) return rc;
    bind_records(sc);
    return VMX_OK;
}

// vertex bounds (origin cells of the bounce reordering), at creation and after every update that moves vertices
static void vertex_bounds(vmx_scene *sc, const float *pos) {
    for (int a = 0; a < 3; ++a) sc->bounds_lo[a] = sc->bounds_hi[a] = pos[a];
    for (size_t v = 0; v < (size_t)sc->ntris * 3; ++v)
        for (int a = 0; a < 3; ++a) {
            sc->bounds_lo[a] = std::min(sc->bounds_lo[a], pos[v * 3 + a]);
            sc->bounds_hi[a] = std::max(sc->bounds_hi[a], pos[v * 3 + a]);
        }
    sc->upd.bounds_stale = false;
}

// a builder's error: the device builders report HIP failures as "LBVH builder: <call>: <hipGetErrorString>"
static int build_error(const std::string &err) {
    int code = VMX_ERR_INVALID;
    if (err.find("deeper") != std::string::npos) code = VMX_ERR_DEPTH;
    else if (err.rfind("LBVH builder: hip", 0) == 0)
        code = (err.find("hipMalloc") != std::string::npos || err.find("out of memory") != std::string::npos) ? VMX_ERR_NOMEM : VMX_ERR_HIP;
    return fail(code, err);
}

int vmx_scene_create_ex(const float *pos, const float *nrm, const float *uv, uint32_t ntris,
                        const vmx_sphere *spheres, uint32_t nspheres, uint32_t leaf_size, uint32_t builder,
                        int device, vmx_scene **out) {
    if (!out) return fail(VMX_ERR_INVALID, "out is NULL");
    if (builder > VMX_BVH_PLOC) return fail(VMX_ERR_INVALID, "unknown BVH builder");
    *out = nullptr;
    if (!pos || !nrm || ntris == 0) return fail(VMX_ERR_INVALID, "scene needs positions, normals, ntris > 0");
    if (int rc = sphere_table_args(spheres, nspheres)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(VMX_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(VMX_ERR_NO_DEVICE, "device ordinal out of range");

    vmx_scene *sc = new vmx_scene();
    sc->device = device;
    sc->ntris = ntris;
    sc->leaf_size = leaf_size ? leaf_size : 4;
    sc->builder = builder;
    std::string err;
    bool built;
    if (builder == VMX_BVH_LBVH || builder == VMX_BVH_PLOC) {
        sc->device_built = true, sc->flat_ready.store(false), sc->flat_topology = false;
        built = builder == VMX_BVH_PLOC ? build_bvh_ploc_device(pos, nrm, uv, ntris, sc->leaf_size, device, sc->lbvh, err)
                                        : build_bvh_lbvh_device(pos, nrm, uv, ntris, sc->leaf_size, device, sc->lbvh, err);
    } else {
        HostTrees t;
        built = host_build_trees(builder, pos, nrm, uv, ntris, sc->leaf_size, t, err);
        if (built) {
            sc->bvh = std::move(t.tree);
            sc->guide.host = t.guide, sc->guide.scene_max = t.scene_max;
        }
    }
    if (!built) {
        delete sc;
        return build_error(err);
    }
    sc->spheres = sphere_table(spheres, nspheres);
    vertex_bounds(sc, pos);
    const int rc = scene_upload(sc);
    if (rc) {
        const std::string keep = g_err;
        vmx_scene_destroy(sc);
        return fail(rc, keep);
    }
    *out = sc;
    return VMX_OK;
}

int vmx_scene_destroy(vmx_scene *sc) {
    if (!sc) return VMX_OK;
    {
        std::lock_guard<std::mutex> lock(sc->mu);
        if (sc->progressive_open)
            return fail(VMX_ERR_INVALID, "scene has " + std::to_string(sc->progressive_open) +
                                             " open vmx_progressive handle(s): vmx_progressive_end them first");
    }
    (void)hipSetDevice(sc->device);
    delete sc;
    return VMX_OK;
}

int vmx_scene_bind_texture(vmx_scene *sc, const float *data, uint32_t width, uint32_t height, uint32_t channels) {
    if (!sc || !data) return fail(VMX_ERR_INVALID, "NULL argument");
    if (width == 0 || height == 0 || channels == 0 || channels > 4 || width > 65535 || height > 65535)
        return fail(VMX_ERR_INVALID, "texture must be 1..65535 texels wide/high with 1..4 channels");
    std::lock_guard<std::mutex> lock(sc->mu);
    int rc = bind_device(sc);
    if (rc) return rc;
    // only boundTextures[0] is sampled by PathTracer (pathtracer.cpp:65); boundTextures[1] is BruteForceTracer's albedo
    // (integrators.cpp:141-147); further ones are counted and not kept
    if (sc->n_textures < 2) {
        const bool first = sc->n_textures == 0;
        DevBuf<float> &tex = first ? sc->d_tex : sc->d_tex1;
        const size_t n = (size_t)width * height * channels;
        if (tex.ensure(n)) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the texture");
        HIP_TRY(hipMemcpy(tex.p, data, n * 4, hipMemcpyHostToDevice));
        if (first) sc->dev.tex = tex.p, sc->dev.tex_w = width, sc->dev.tex_h = height, sc->dev.tex_c = channels;
        else sc->dev.tex1 = tex.p, sc->dev.tex1_w = width, sc->dev.tex1_h = height, sc->dev.tex1_c = channels;
    }
    sc->n_textures++;
    return VMX_OK;
}

// A refitted tree's boxes in the flat layout: one depth-first walk from root_ref over the downloaded records, left child
// first — the export order of both kinds of builder (pre-order, left child = i + 1).  A node's box is its half of the
// parent's record; the root's is the refit's root_box.  Topology and prim_order are the builder's and stay.
static int export_refit_boxes(vmx_scene *sc) {
    HostBvh &b = sc->bvh;
    const size_t n_nodes = b.start.size();
    std::vector<InnerRecord> rec(sc->n_inner);
    if (sc->n_inner) HIP_TRY(hipMemcpy(rec.data(), sc->dev.inner, rec.size() * sizeof(InnerRecord), hipMemcpyDeviceToHost));
    float root[6];
    HIP_TRY(hipMemcpy(root, sc->upd.root_box.p, sizeof(root), hipMemcpyDeviceToHost));
    struct Item {
        uint32_t ref;
        const float *box;  // six floats: min, max
    };
    std::vector<Item> work{{sc->dev.root_ref, root}};
    size_t i = 0;
    while (!work.empty()) {
        const Item it = work.back();
        work.pop_back();
        const bool leaf = (it.ref & kLeafBit) != 0;
        if (i >= n_nodes || leaf != (b.right_offset[i] == 0) || (!leaf && it.ref >= rec.size()))
            return fail(VMX_ERR_HIP, "flat export: the device records do not match the tree's topology");
        std::memcpy(&b.bbox[i * 6], it.box, 24);
        ++i;
        if (leaf) continue;
        const InnerRecord &r = rec[it.ref];
        work.push_back({r.right, r.rmin});  // rmin, rmax: six consecutive floats
        work.push_back({r.left, r.lmin});
    }
    if (i != n_nodes) return fail(VMX_ERR_HIP, "flat export: the device records do not match the tree's topology");
    return VMX_OK;
}

// device-built trees: the reference's flat layout is produced on the first request for it; after a REFIT the boxes are
// read back from the records
static int ensure_flat(const vmx_scene *csc) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (sc->flat_ready.load(std::memory_order_acquire)) return VMX_OK;
    std::lock_guard<std::mutex> lock(sc->mu);
    if (sc->flat_ready.load(std::memory_order_relaxed)) return VMX_OK;
    if (int rc = bind_device(sc)) return rc;
    if (int rc = sc->upd.done.sync()) return rc;
    std::string err;
    if (!sc->flat_topology) {
        if (!lbvh_export_flat(sc->lbvh, sc->device, sc->bvh, err)) return fail(VMX_ERR_HIP, err);
        sc->flat_topology = true;
    }
    if (sc->upd.refitted)
        if (int rc = export_refit_boxes(sc)) return rc;
    sc->flat_ready.store(true, std::memory_order_release);
    return VMX_OK;
}

int vmx_scene_describe(const vmx_scene *sc, vmx_scene_desc *out) {
    if (!sc || !out) return fail(VMX_ERR_INVALID, "NULL argument");
    if (int rc = ensure_flat(sc)) return rc;
    std::memset(out, 0, sizeof(*out));
    out->ntris = sc->ntris;
    out->nspheres = (uint32_t)sc->spheres.size();
    out->leaf_size = sc->leaf_size;
    out->n_nodes = (uint32_t)sc->bvh.start.size();
    out->n_leaves = sc->bvh.n_leaves;
    out->n_inner = sc->n_inner;
    out->max_depth = sc->bvh.max_depth;
    out->stack_entries = sc->dev.stack_entries;
    out->device_bytes = (size_t)sc->n_inner * sizeof(InnerRecord) + (size_t)sc->ntris * sizeof(TriRecord) +
                        (size_t)sc->ntris * sizeof(AttrRecord) + sc->spheres.size() * sizeof(SphereDev) +
                        (sc->device_built ? sc->lbvh.arena_bytes : 0) +  // device-built trees keep their hierarchy arrays
                        (sc->guide.base ? sc->guide.bytes : 0);             // a reference-tree scene's guide (guide_walk.h)
    out->device = sc->device;
    return VMX_OK;
}

int vmx_scene_timings(const vmx_scene *sc, vmx_timings *out) {
    if (!sc || !out) return fail(VMX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(const_cast<vmx_scene *>(sc)->mu);  // a render on another thread rewrites them
    *out = sc->timings;
    return VMX_OK;
}

uint32_t vmx_scene_compute_units(const vmx_scene *sc) { return sc ? (uint32_t)sc->num_cus : 0u; }

int vmx_scene_bvh(const vmx_scene *sc, uint32_t *start, uint32_t *nprims, uint32_t *right_offset, float *bbox,
                  uint32_t *prim_order) {
    if (!sc) return fail(VMX_ERR_INVALID, "NULL scene");
    if (int rc = ensure_flat(sc)) return rc;
    const HostBvh &b = sc->bvh;
    const size_t n = b.start.size();
    if (start) std::memcpy(start, b.start.data(), n * 4);
    if (nprims) std::memcpy(nprims, b.nprims.data(), n * 4);
    if (right_offset) std::memcpy(right_offset, b.right_offset.data(), n * 4);
    if (bbox) std::memcpy(bbox, b.bbox.data(), n * 24);
    if (prim_order) std::memcpy(prim_order, b.prim_order.data(), b.prim_order.size() * 4);
    return VMX_OK;
}

} /* extern "C" */
