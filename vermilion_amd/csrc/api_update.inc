// api_update.inc — part of vmx_api.cpp
namespace {

// argument checks that need no device, in this order so that each can be seen alone (the scene is checked last)
int update_args(const void *scene, const void *pos, const void *nrm, const void *uv, uint32_t ntris, uint32_t flags) {
    if (flags & ~VMX_UPDATE_REBUILD) return fail(VMX_ERR_INVALID, "unknown update flags");
    if (!pos && !nrm && !uv) return fail(VMX_ERR_INVALID, "nothing to update: pos, nrm and uv are all NULL");
    if (ntris == 0) return fail(VMX_ERR_INVALID, "ntris is 0: it must be the scene's triangle count");
    if (!scene) return fail(VMX_ERR_INVALID, "NULL scene");
    return VMX_OK;
}

int update_scene_args(const vmx_scene *sc, const float *pos, uint32_t ntris) {
    if (ntris != sc->ntris)
        return fail(VMX_ERR_INVALID, "ntris " + std::to_string(ntris) + " is not the scene's triangle count " +
                                         std::to_string(sc->ntris) + " (another count or order is a new scene)");
    if (pos)  // as vmx_scene_create checks them (bvh_build.cpp: check_input)
        for (size_t i = 0; i < (size_t)ntris * 9; ++i)
            if (!std::isfinite(pos[i])) return fail(VMX_ERR_INVALID, "non-finite vertex position");
    return VMX_OK;
}

// the next update's writes wait for the last query (it reads the records) and the last update
int update_wait(vmx_scene *sc, hipStream_t s) {
    if (int rc = sc->qws.done.wait(s)) return rc;
    return sc->upd.done.wait(s);
}

// The refit plan: every referenced child of every inner record with the half of its parent it goes to, plus the root,
// bucketed by tree level (deepest first: one launch each).  Derived by a walk from root_ref — the device builders leave
// unused records zeroed, and their left = right = 0 would read as references to record 0.
int ensure_refit_plan(vmx_scene *sc, hipStream_t s) {
    auto &u = sc->upd;
    if (u.plan_ready) return VMX_OK;
    std::vector<InnerRecord> rec(sc->n_inner);
    if (!(sc->dev.root_ref & kLeafBit)) {
        HIP_TRY(hipMemcpyAsync(rec.data(), sc->dev.inner, rec.size() * sizeof(InnerRecord), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    struct Item {
        uint32_t ref, dst, depth;
    };
    std::vector<std::vector<RefitItem>> level;
    std::vector<Item> work{{sc->dev.root_ref, kRefitRoot, 0u}};
    while (!work.empty()) {
        const Item it = work.back();
        work.pop_back();
        if (it.depth >= kMaxStack || (!(it.ref & kLeafBit) && it.ref >= rec.size()))
            return fail(VMX_ERR_HIP, "refit plan: the device records do not form a tree");
        if (level.size() <= it.depth) level.resize(it.depth + 1);
        level[it.depth].push_back({it.ref, it.dst});
        if (it.ref & kLeafBit) continue;
        const InnerRecord &r = rec[it.ref];
        work.push_back({r.right, it.ref * 2u + 1u, it.depth + 1});
        work.push_back({r.left, it.ref * 2u, it.depth + 1});
    }
    std::vector<RefitItem> flat;
    u.levels.clear();
    for (size_t d = level.size(); d-- > 0;) {
        u.levels.emplace_back((uint32_t)flat.size(), (uint32_t)level[d].size());
        flat.insert(flat.end(), level[d].begin(), level[d].end());
    }
    if (u.plan.ensure(flat.size() * sizeof(RefitItem)) || u.root_box.ensure(6))
        return fail(VMX_ERR_NOMEM, "hipMalloc failed for the refit plan");
    HIP_TRY(hipMemcpyAsync(u.plan.p, flat.data(), flat.size() * sizeof(RefitItem), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // (`flat` is a host temporary)
    u.plan_ready = true;
    return VMX_OK;
}

// record rewrite and, with positions, the refit: enqueued on `s`, not synchronised (the first update that moves
// vertices builds the refit plan and does)
int update_enqueue(vmx_scene *sc, const float *d_pos, const float *d_nrm, const float *d_uv, hipStream_t s) {
    auto &u = sc->upd;
    if (d_pos)
        if (int rc = ensure_refit_plan(sc, s)) return rc;
    if (int rc = update_wait(sc, s)) return rc;
    unsigned char *inner = (unsigned char *)const_cast<void *>(sc->dev.inner);
    unsigned char *tris = inner + sc->dev.tri_off;
    LAUNCH_TRY(launch_update_records(sc->ntris, d_pos, d_nrm, d_uv, tris, const_cast<void *>(sc->dev.attrs), s));
    if (d_pos) {
        const RefitItem *plan = (const RefitItem *)u.plan.p;
        for (const auto &lv : u.levels)
            LAUNCH_TRY(launch_refit_level(plan + lv.first, lv.second, d_pos, tris, inner, u.root_box.p, s));
        u.refitted = true, u.bounds_stale = true;
        sc->guide.valid = false;  // the guide's boxes are the old positions': not used from here on (guide_walk.h)
        sc->flat_ready.store(false, std::memory_order_release);
    }
    return sc->upd.done.record(s);
}

// after a REBUILD: the new tree's records are bound; what was derived from the old tree goes
void rebuilt(vmx_scene *sc) {
    bind_records(sc);  // stack_entries, block; the render workspace's overflow stacks follow in bind_stack, the query
                       // workspace in ensure_query_ws
    sc->upd.plan_ready = false, sc->upd.refitted = false;
    sc->guide.valid = false, sc->guide.base = nullptr, sc->guide.off = 0, sc->guide.bytes = 0;  // (its records went with the old allocation)
    sc->flat_topology = !sc->device_built;
    sc->flat_ready.store(!sc->device_built, std::memory_order_release);
}

// normals / uvs of a host-built scene in triangle-ID order (what a REBUILD that keeps them hands the builder); the
// caller has synchronised with the scene's last update
int host_attrs_by_id(vmx_scene *sc, std::vector<float> &nrm, std::vector<float> &uv) {
    std::vector<AttrRecord> a(sc->ntris);
    HIP_TRY(hipMemcpy(a.data(), sc->dev.attrs, a.size() * sizeof(AttrRecord), hipMemcpyDeviceToHost));
    const std::vector<uint32_t> &order = sc->bvh.prim_order;  // leaf slot -> triangle ID
    nrm.resize((size_t)sc->ntris * 9), uv.resize((size_t)sc->ntris * 6);
    for (uint32_t slot = 0; slot < sc->ntris; ++slot) {
        const size_t t = order[slot];
        std::memcpy(&nrm[t * 9], a[slot].n0, 36);
        std::memcpy(&uv[t * 6], a[slot].uv0, 24);
    }
    return VMX_OK;
}

// host builders: build on the host (into new trees — a reference-tree scene's guide beside its tree, as at creation; the
// scene is untouched on failure)
int host_rebuild_tree(vmx_scene *sc, const float *pos, const float *nrm, const float *uv, HostTrees &out) {
    std::vector<float> kn, ku;
    if (!nrm || !uv) {
        if (int rc = host_attrs_by_id(sc, kn, ku)) return rc;
        if (!nrm) nrm = kn.data();
        if (!uv) uv = ku.data();
    }
    std::string err;
    return host_build_trees(sc->builder, pos, nrm, uv, sc->ntris, sc->leaf_size, out, err) ? VMX_OK : build_error(err);
}

// swaps a host-built tree in: new buffers, uploaded, then the old ones freed.  The caller has synchronised `s` after
// update_wait, so nothing in flight reads the old records.
// (guide: the guide built beside it or NULL — the allocation gets room for its records, which apply_guide then writes)
int host_apply_tree(vmx_scene *sc, const HostBvh &b, const HostBvh *guide, hipStream_t s) {
    DevBuf<unsigned char> geom;
    DevBuf<AttrRecord> attrs;
    if (int rc = upload_records(b, guide, geom, attrs)) return rc;
    sc->d_geom = std::move(geom), sc->d_attrs = std::move(attrs);
    sc->bvh = b;
    rebuilt(sc);
    return sc->upd.done.record(s);
}

// device builders: the build runs on `s` from device inputs; a kept attribute comes back from the records in
// triangle-ID order first.  Blocks (the depth check needs the root's height on the host).
int device_rebuild(vmx_scene *sc, const float *d_pos, const float *d_nrm, const float *d_uv, hipStream_t s) {
    auto &u = sc->upd;
    if (int rc = update_wait(sc, s)) return rc;
    const size_t n = sc->ntris;
    if (!d_nrm || !d_uv) {
        if (u.scratch.ensure(n * 24)) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the update inputs");
        float *kn = d_nrm ? nullptr : u.scratch.p + n * 9, *ku = d_uv ? nullptr : u.scratch.p + n * 18;
        LAUNCH_TRY(launch_attrs_by_id(sc->ntris, sc->dev.tris, sc->dev.attrs, kn, ku, s));
        if (kn) d_nrm = kn;
        if (ku) d_uv = ku;
    }
    LbvhDevice l;
    std::string err;
    const bool ok = build_bvh_device_inputs(d_pos, d_nrm, d_uv, sc->ntris, sc->leaf_size, sc->device,
                                            sc->builder == VMX_BVH_PLOC, s, l, err);
    if (!ok) {
        (void)hipStreamSynchronize(s);
        lbvh_release(l);
        return build_error(err);
    }
    lbvh_release(sc->lbvh);  // (the build synchronised `s` after the waits: nothing in flight reads it)
    sc->lbvh = l;
    rebuilt(sc);
    float rb[6];  // the root's box: vertex bounds of the new positions
    HIP_TRY(hipMemcpy(rb, n > 1 ? l.node_box : l.leaf_box, sizeof(rb), hipMemcpyDeviceToHost));
    for (int a = 0; a < 3; ++a) sc->bounds_lo[a] = rb[a], sc->bounds_hi[a] = rb[3 + a];
    u.bounds_stale = false;
    return sc->upd.done.record(s);
}

// vmx_scene_update after the argument checks, under the scene's lock; `tree`: a host build shared by the replicas of
// a vmx_multi (host builders with REBUILD), else NULL
int host_update(vmx_scene *sc, const float *pos, const float *nrm, const float *uv, uint32_t flags, const HostTrees *tree) {
    if (int rc = bind_device(sc)) return rc;
    hipStream_t s = sc->stream;
    const size_t n = sc->ntris;
    const bool rebuild = (flags & VMX_UPDATE_REBUILD) && pos;
    if (rebuild && !sc->device_built) {
        if (int rc = update_wait(sc, s)) return rc;
        HIP_TRY(hipStreamSynchronize(s));
        HostTrees own;
        if (!tree) {
            if (int rc = host_rebuild_tree(sc, pos, nrm, uv, own)) return rc;
            tree = &own;
        }
        if (int rc = host_apply_tree(sc, tree->tree, tree->guide.get(), s)) return rc;
        if (int rc = apply_guide(sc, *tree)) return rc;  // (the guide of the new positions, built beside the tree)
        vertex_bounds(sc, pos);
        HIP_TRY(hipStreamSynchronize(s));
        sc->generation++;
        return VMX_OK;
    }
    if (sc->upd.scratch.ensure(n * 24)) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the update inputs");
    float *d_pos = pos ? sc->upd.scratch.p : nullptr, *d_nrm = nrm ? sc->upd.scratch.p + n * 9 : nullptr;
    float *d_uv = uv ? sc->upd.scratch.p + n * 18 : nullptr;
    // (the scratch may still feed the previous update if that one ran on another stream)
    if (int rc = sc->upd.done.wait(s)) return rc;
    if (pos) HIP_TRY(hipMemcpyAsync(d_pos, pos, n * 36, hipMemcpyHostToDevice, s));
    if (nrm) HIP_TRY(hipMemcpyAsync(d_nrm, nrm, n * 36, hipMemcpyHostToDevice, s));
    if (uv) HIP_TRY(hipMemcpyAsync(d_uv, uv, n * 24, hipMemcpyHostToDevice, s));
    int rc = rebuild ? device_rebuild(sc, d_pos, d_nrm, d_uv, s) : update_enqueue(sc, d_pos, d_nrm, d_uv, s);
    const hipError_t es = hipStreamSynchronize(s);  // (also before the inputs are overwritten when the update failed)
    if (rc) return rc;
    if (es != hipSuccess) return fail(VMX_ERR_HIP, std::string("vmx_scene_update: ") + hipGetErrorString(es));
    if (pos) vertex_bounds(sc, pos);
    sc->generation++;
    return VMX_OK;
}

// ---- the sphere table of a live scene (vmx_scene_set_spheres, vmx_multi_set_spheres) ------------------------------------
// argument checks that need no device, in this order so that each can be seen alone (the handle is checked last)
int set_spheres_args(const void *handle, const vmx_sphere *spheres, uint32_t nspheres, const char *null_handle) {
    if (int rc = sphere_table_args(spheres, nspheres)) return rc;
    if (!handle) return fail(VMX_ERR_INVALID, null_handle);
    return VMX_OK;
}

// Rewrites the table in place, under the scene's lock, and returns once it is written.  d_spheres holds kMaxSpheres
// entries from creation on, so no count needs another allocation.  The write waits for the scene's last query and last
// update (update_wait); renders, parity hooks and progressive steps block until their kernels are done and hold the lock
// meanwhile, so none of them is still reading.  Every later call waits on upd.done, as after a geometry update.  What
// the kernels get by value with each launch — nspheres, emit_prefix — and the host copy change only once the device
// has the table: a failed call leaves the scene as it was.  Everything else derived from the table (claim tables, pixel
// bounds, the rays' "light in reach" notes) is made per run from the table a launch sees.
int set_spheres(vmx_scene *sc, const std::vector<vmx_sphere> &table) {
    if (int rc = bind_device(sc)) return rc;
    hipStream_t s = sc->stream;
    SphereDev sd[kMaxSpheres];
    uint32_t emit_prefix = 0;
    derive_spheres(table, sd, emit_prefix);
    if (int rc = update_wait(sc, s)) return rc;
    HIP_TRY(hipMemcpyAsync(sc->d_spheres.p, sd, sizeof(sd), hipMemcpyHostToDevice, s));
    const int rc = sc->upd.done.record(s);
    const hipError_t es = hipStreamSynchronize(s);  // (`sd` is a host temporary)
    if (rc) return rc;
    if (es != hipSuccess) return fail(VMX_ERR_HIP, std::string("vmx_scene_set_spheres: ") + hipGetErrorString(es));
    sc->spheres = table;
    sc->dev.nspheres = (uint32_t)table.size();
    sc->dev.emit_prefix = emit_prefix;
    sc->generation++;
    return VMX_OK;
}

// ---- the emissive triangles of a live scene (vmx_scene_set_emitters, vmx_multi_set_emitters) ----------------------------
// argument checks that need no device, in the documented order (ntris: the handle's triangle count)
int set_emitters_args(const vmx_emitter *e, uint32_t n, uint32_t ntris) {
    if (!e && n > 0) return fail(VMX_ERR_INVALID, "NULL emitters with n > 0");
    if (n > VMX_MAX_EMITTERS) return fail(VMX_ERR_INVALID, "more than VMX_MAX_EMITTERS emitters");
    if (n > ntris) return fail(VMX_ERR_INVALID, "more emitters than the scene has triangles");
    for (uint32_t i = 0; i < n; ++i)
        if (e[i].tri_id >= ntris)
            return fail(VMX_ERR_INVALID, "emitter " + std::to_string(i) + ": triangle id " + std::to_string(e[i].tri_id) +
                                             " is not below the scene's triangle count " + std::to_string(ntris));
    {
        std::vector<uint32_t> ids(n);
        for (uint32_t i = 0; i < n; ++i) ids[i] = e[i].tri_id;
        std::sort(ids.begin(), ids.end());
        const auto dup = std::adjacent_find(ids.begin(), ids.end());
        if (dup != ids.end()) return fail(VMX_ERR_INVALID, "triangle id " + std::to_string(*dup) + " is listed more than once");
    }
    for (uint32_t i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(e[i].radiance[c]) || e[i].radiance[c] < 0.f)
                return fail(VMX_ERR_INVALID, "emitter " + std::to_string(i) + ": a radiance component is negative or not finite");
    return VMX_OK;
}

// The caller's table goes to the device and the generation moves on, under the scene's lock; the derived table follows at
// the next light-sampled launch (nee_emitters).  Nothing is still reading: see set_spheres.  A failed call leaves the
// scene as it was.
int set_emitters(vmx_scene *sc, const std::vector<vmx_emitter> &table) {
    auto &em = sc->em;
    const size_t n = table.size();
    if (n) {
        if (int rc = bind_device(sc)) return rc;
        hipStream_t s = sc->stream;
        std::vector<uint32_t> ids(n);
        std::vector<float> rad(n * 3);
        for (size_t i = 0; i < n; ++i) {
            ids[i] = table[i].tri_id;
            for (int c = 0; c < 3; ++c) rad[i * 3 + c] = table[i].radiance[c];
        }
        if (int rc = update_wait(sc, s)) return rc;
        HIP_TRY(hipStreamSynchronize(s));  // (ensure may free what the last launch read)
        if (em.ids.ensure(n) || em.radiance.ensure(n * 3)) {
            em.table.clear(), em.dev = EmitDev{};
            sc->generation++;
            return fail(VMX_ERR_NOMEM, "hipMalloc failed for the emitter table (the scene now has none)");
        }
        HIP_TRY(hipMemcpy(em.ids.p, ids.data(), n * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(em.radiance.p, rad.data(), n * 12, hipMemcpyHostToDevice));
    }
    em.table = table;
    em.built = ~0ull;
    if (n == 0) em.dev = EmitDev{};
    sc->generation++;
    return VMX_OK;
}

}  // namespace

extern "C" {

int vmx_scene_set_emitters(vmx_scene *sc, const vmx_emitter *emitters, uint32_t n) {
    if (!sc) return fail(VMX_ERR_INVALID, "NULL scene");
    if (int rc = set_emitters_args(emitters, n, sc->ntris)) return rc;
    const std::vector<vmx_emitter> table(emitters, emitters + n);
    std::lock_guard<std::mutex> lock(sc->mu);
    return set_emitters(sc, table);
}

int vmx_emitters_check(const vmx_emitter *emitters, uint32_t n, uint32_t ntris) { return set_emitters_args(emitters, n, ntris); }

int vmx_scene_emitters(const vmx_scene *csc, vmx_emitter_info *out, uint32_t cap, uint32_t *n_out) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!sc) return fail(VMX_ERR_INVALID, "NULL scene");
    if (!n_out) return fail(VMX_ERR_INVALID, "NULL n");
    if (!out && cap > 0) return fail(VMX_ERR_INVALID, "NULL out with cap > 0");
    std::lock_guard<std::mutex> lock(sc->mu);
    const uint32_t n = (uint32_t)sc->em.table.size();
    *n_out = n;
    const uint32_t m = std::min(n, cap);
    if (m == 0) return VMX_OK;
    if (int rc = bind_device(sc)) return rc;
    hipStream_t s = sc->stream;
    if (int rc = nee_emitters(sc, s)) return rc;
    std::vector<double> area(m), weight(m), cdf(m);
    HIP_TRY(hipMemcpyAsync(area.data(), sc->em.area.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(weight.data(), sc->em.weight.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cdf.data(), sc->em.cdf.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < m; ++i) {
        out[i].tri_id = sc->em.table[i].tri_id;
        for (int c = 0; c < 3; ++c) out[i].radiance[c] = sc->em.table[i].radiance[c];
        out[i].area = area[i], out[i].weight = weight[i], out[i].cdf = cdf[i];
    }
    return VMX_OK;
}

int vmx_multi_set_emitters(vmx_multi *m, const vmx_emitter *emitters, uint32_t n) {
    if (!m) return fail(VMX_ERR_INVALID, "NULL vmx_multi");
    if (int rc = set_emitters_args(emitters, n, m->replica[0]->ntris)) return rc;
    const std::vector<vmx_emitter> table(emitters, emitters + n);
    std::lock_guard<std::mutex> mlock(m->mu);
    // replica by replica, as vmx_multi_set_spheres: the replicas already changed get the old table back on a failure
    const std::vector<vmx_emitter> old = m->replica[0]->em.table;
    for (size_t r = 0; r < m->replica.size(); ++r) {
        vmx_scene *sc = m->replica[r];
        int rc;
        {
            std::lock_guard<std::mutex> lock(sc->mu);
            rc = set_emitters(sc, table);
        }
        if (rc == VMX_OK) continue;
        const std::string keep = r ? "device " + std::to_string(sc->device) + ": " + g_err : g_err;
        for (size_t q = 0; q < r; ++q) {
            std::lock_guard<std::mutex> lock(m->replica[q]->mu);
            (void)set_emitters(m->replica[q], old);
        }
        return fail(rc, keep);
    }
    return VMX_OK;
}

int vmx_scene_set_spheres(vmx_scene *sc, const vmx_sphere *spheres, uint32_t nspheres) {
    if (int rc = set_spheres_args(sc, spheres, nspheres, "NULL scene")) return rc;
    const std::vector<vmx_sphere> table = sphere_table(spheres, nspheres);
    std::lock_guard<std::mutex> lock(sc->mu);
    return set_spheres(sc, table);
}

int vmx_multi_set_spheres(vmx_multi *m, const vmx_sphere *spheres, uint32_t nspheres) {
    if (int rc = set_spheres_args(m, spheres, nspheres, "NULL vmx_multi")) return rc;
    const std::vector<vmx_sphere> table = sphere_table(spheres, nspheres);
    std::lock_guard<std::mutex> mlock(m->mu);
    // replica by replica, each with its own host copy (replica[0]'s is the one later vmx_multi_* calls read).  Nothing
    // about a table can fail on one device and not on another, but a device can: the replicas already changed then get
    // the old table back, so that all of them still hold one table
    const std::vector<vmx_sphere> old = m->replica[0]->spheres;
    for (size_t r = 0; r < m->replica.size(); ++r) {
        vmx_scene *sc = m->replica[r];
        int rc;
        {
            std::lock_guard<std::mutex> lock(sc->mu);
            rc = set_spheres(sc, table);
        }
        if (rc == VMX_OK) continue;
        const std::string keep = r ? "device " + std::to_string(sc->device) + ": " + g_err : g_err;
        for (size_t q = 0; q < r; ++q) {
            std::lock_guard<std::mutex> lock(m->replica[q]->mu);
            (void)set_spheres(m->replica[q], old);
        }
        return fail(rc, keep);
    }
    return VMX_OK;
}

int vmx_scene_update(vmx_scene *sc, const float *pos, const float *nrm, const float *uv, uint32_t ntris, uint32_t flags) {
    if (int rc = update_args(sc, pos, nrm, uv, ntris, flags)) return rc;
    if (int rc = update_scene_args(sc, pos, ntris)) return rc;
    std::lock_guard<std::mutex> lock(sc->mu);
    return host_update(sc, pos, nrm, uv, flags, nullptr);
}

int vmx_scene_update_device(vmx_scene *sc, const void *d_pos, const void *d_nrm, const void *d_uv, uint32_t ntris,
                            uint32_t flags, void *stream) {
    if (int rc = update_args(sc, d_pos, d_nrm, d_uv, ntris, flags)) return rc;
    if (int rc = update_scene_args(sc, nullptr, ntris)) return rc;
    const bool rebuild = (flags & VMX_UPDATE_REBUILD) && d_pos;
    if (rebuild && !sc->device_built)
        return fail(VMX_ERR_INVALID, "VMX_UPDATE_REBUILD of a tree built on the host (VMX_BVH_REFERENCE / VMX_BVH_SAH) "
                                     "needs host positions: use vmx_scene_update");
    std::lock_guard<std::mutex> lock(sc->mu);
    if (int rc = bind_device(sc)) return rc;
    if (int rc = check_device_ptrs(sc->device, {{d_pos, "pos"}, {d_nrm, "nrm"}, {d_uv, "uv"}})) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : sc->stream;
    const int rc = rebuild ? device_rebuild(sc, (const float *)d_pos, (const float *)d_nrm, (const float *)d_uv, s)
                           : update_enqueue(sc, (const float *)d_pos, (const float *)d_nrm, (const float *)d_uv, s);
    if (rc == VMX_OK) sc->generation++;
    return rc;
}

int vmx_multi_update(vmx_multi *m, const float *pos, const float *nrm, const float *uv, uint32_t ntris, uint32_t flags) {
    if (int rc = update_args(m, pos, nrm, uv, ntris, flags)) return rc;
    std::lock_guard<std::mutex> mlock(m->mu);
    vmx_scene *first = m->replica[0];
    if (int rc = update_scene_args(first, pos, ntris)) return rc;
    HostTrees tree;
    const HostTrees *shared = nullptr;
    if ((flags & VMX_UPDATE_REBUILD) && pos && !first->device_built) {
        // host builders: one host build, uploaded to every replica
        std::lock_guard<std::mutex> lock(first->mu);
        if (int rc = bind_device(first)) return rc;
        if (int rc = update_wait(first, first->stream)) return rc;
        HIP_TRY(hipStreamSynchronize(first->stream));
        if (int rc = host_rebuild_tree(first, pos, nrm, uv, tree)) return rc;
        shared = &tree;
    }
    // replica by replica; device builders build on each device (a failure — too deep a tree — shows on the first one,
    // before any replica changed)
    for (size_t r = 0; r < m->replica.size(); ++r) {
        vmx_scene *sc = m->replica[r];
        std::lock_guard<std::mutex> lock(sc->mu);
        const int rc = host_update(sc, pos, nrm, uv, flags, shared);
        if (rc) return r ? fail(rc, "device " + std::to_string(sc->device) + ": " + g_err) : rc;
    }
    return VMX_OK;
}

} /* extern "C" */
