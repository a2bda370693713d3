// vmx_update.inc — in-place geometry updates of a scene (vmx_scene_update / vmx_scene_update_device).
// Included by vmx_kernels.hip (inside its namespace).
//
//   k_update_records  one lane per leaf slot: rewrites the slot's TriRecord (v0, e1 = v1 - v0, e2 = v2 - v0, id) and/or
//                     its AttrRecord with the float operations of bvh_build.cpp's flatten and k_lbvh_emit_tris, so a
//                     rewritten record is bit-identical to the one a fresh build writes for that triangle
//   k_refit_level     one lane per node of one tree level (vmx_api.cpp: the refit plan, deepest level first): a leaf's
//                     box is the min / max over its triangles' vertices, an inner node's box the union of the two halves
//                     of its own record (written by the previous launch); either goes into its half of the parent's
//                     record, the root's into a 6-float slot of the scene (the flat export's node 0).  One launch per
//                     level: the kernel boundary makes the children's boxes visible to every CU of every XCD
//   k_attrs_by_id     the inverse permutation of the attribute records (slot -> triangle ID order): what a REBUILD
//                     that keeps the normals or uvs hands the builder
__global__ void __launch_bounds__(256) k_update_records(uint32_t ntris, const float *__restrict__ pos,
                                                        const float *__restrict__ nrm, const float *__restrict__ uv,
                                                        TriRecord *__restrict__ tris, AttrRecord *__restrict__ attrs) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= ntris) return;
    const uint32_t t = tris[slot].id;
    if (pos) {
        const float *p = pos + (size_t)t * 9;
        TriRecord tr;
        for (int a = 0; a < 3; ++a) {
            tr.v0[a] = p[a];
            tr.e1[a] = p[3 + a] - p[a];  // triangle.cpp:12
            tr.e2[a] = p[6 + a] - p[a];  // triangle.cpp:13
        }
        tr.id = t, tr.pad[0] = tr.pad[1] = 0;
        tris[slot] = tr;
    }
    if (nrm || uv) {
        AttrRecord ar = attrs[slot];
        if (nrm) {
            const float *q = nrm + (size_t)t * 9;
            for (int a = 0; a < 3; ++a) ar.n0[a] = q[a], ar.n1[a] = q[3 + a], ar.n2[a] = q[6 + a];
        }
        if (uv) {
            const float *q = uv + (size_t)t * 6;
            for (int a = 0; a < 2; ++a) ar.uv0[a] = q[a], ar.uv1[a] = q[2 + a], ar.uv2[a] = q[4 + a];
        }
        ar.pad = 0.f;
        attrs[slot] = ar;
    }
}

// `inner` is read (this level's own records) and written (the parents' halves, one level up) by the same launch: the
// two sets are disjoint, and no two lanes write the same half
__global__ void __launch_bounds__(256) k_refit_level(const RefitItem *__restrict__ items, uint32_t n,
                                                     const float *__restrict__ pos, const TriRecord *__restrict__ tris,
                                                     InnerRecord *inner, float *__restrict__ root_box) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RefitItem it = items[i];
    float lo[3], hi[3];
    if (it.ref & kLeafBit) {
        const uint32_t start = it.ref & kLeafStartMask, cnt = (it.ref >> kLeafCountShift) & kMaxLeafSize;
        for (int a = 0; a < 3; ++a) lo[a] = INFINITY, hi[a] = -INFINITY;
        for (uint32_t k = 0; k < cnt; ++k) {
            const float *p = pos + (size_t)tris[start + k].id * 9;
            for (int a = 0; a < 3; ++a) {  // Triangle::getBBox (triangle.cpp:107-114)
                lo[a] = fminf(lo[a], fminf(fminf(p[a], p[3 + a]), p[6 + a]));
                hi[a] = fmaxf(hi[a], fmaxf(fmaxf(p[a], p[3 + a]), p[6 + a]));
            }
        }
    } else {
        const InnerRecord r = inner[it.ref];
        for (int a = 0; a < 3; ++a) lo[a] = fminf(r.lmin[a], r.rmin[a]), hi[a] = fmaxf(r.lmax[a], r.rmax[a]);
    }
    // lmin, lmax (and rmin, rmax) are six consecutive floats of the record
    float *b = it.dst == kRefitRoot ? root_box : ((it.dst & 1u) ? inner[it.dst >> 1].rmin : inner[it.dst >> 1].lmin);
    for (int a = 0; a < 3; ++a) b[a] = lo[a], b[3 + a] = hi[a];
}

__global__ void __launch_bounds__(256) k_attrs_by_id(uint32_t ntris, const TriRecord *__restrict__ tris,
                                                     const AttrRecord *__restrict__ attrs, float *__restrict__ nrm,
                                                     float *__restrict__ uv) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= ntris) return;
    const uint32_t t = tris[slot].id;
    const AttrRecord ar = attrs[slot];
    if (nrm)
        for (int a = 0; a < 3; ++a)
            nrm[(size_t)t * 9 + a] = ar.n0[a], nrm[(size_t)t * 9 + 3 + a] = ar.n1[a], nrm[(size_t)t * 9 + 6 + a] = ar.n2[a];
    if (uv)
        for (int a = 0; a < 2; ++a)
            uv[(size_t)t * 6 + a] = ar.uv0[a], uv[(size_t)t * 6 + 2 + a] = ar.uv1[a], uv[(size_t)t * 6 + 4 + a] = ar.uv2[a];
}

int launch_update_records(uint32_t ntris, const float *pos, const float *nrm, const float *uv, void *tris, void *attrs,
                          void *stream) {
    hipLaunchKernelGGL(k_update_records, dim3((ntris + 255) / 256), dim3(256), 0, (hipStream_t)stream, ntris, pos, nrm,
                       uv, (TriRecord *)tris, (AttrRecord *)attrs);
    return launch_status();
}

int launch_refit_level(const RefitItem *items, uint32_t n, const float *pos, const void *tris, void *inner,
                       float *root_box, void *stream) {
    hipLaunchKernelGGL(k_refit_level, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, items, n, pos,
                       (const TriRecord *)tris, (InnerRecord *)inner, root_box);
    return launch_status();
}

int launch_attrs_by_id(uint32_t ntris, const void *tris, const void *attrs, float *nrm, float *uv, void *stream) {
    hipLaunchKernelGGL(k_attrs_by_id, dim3((ntris + 255) / 256), dim3(256), 0, (hipStream_t)stream, ntris,
                       (const TriRecord *)tris, (const AttrRecord *)attrs, nrm, uv);
    return launch_status();
}
