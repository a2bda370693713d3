// vmx_emitters.inc — part of vmx_kernels.hip: the derived table of a scene's emissive triangles (vmx_scene_set_emitters),
// what k_nee<.., MESH = true> samples.  The table is stated in include/vermilion_hip.h ("emissive triangles") and restated
// in tests/nee_mesh_spec.py; it is rebuilt from the scene's CURRENT triangle records, so a refit changes its areas and a
// rebuild its leaf slots.
//
//   k_emitter_slots  one lane per leaf slot: the emitter index of the slot's triangle id (id_em, -1: none) goes into
//                    slot_em[slot], and the slot into the emitter's record — the inverse of a permutation only the
//                    records hold on a device-built scene
//   k_emitter_table  one lane per emitter: the 64-byte sampling record (v0, e1, e2 of the triangle record, the radiance,
//                    the slot) and, in double, area = 0.5 sqrt(nn) and weight = area * double(luminance(radiance))
//   k_emitter_cdf    cdf_e = cdf_{e-1} + weight_e in TABLE ORDER by one lane, the weights staged through LDS by the block:
//                    the order of the additions is the definition, so this is not a tree reduction

__global__ void __launch_bounds__(256) k_emitter_ids(const uint32_t *__restrict__ ids, uint32_t n, int32_t *__restrict__ id_em) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) id_em[ids[e]] = (int32_t)e;
}

__global__ void __launch_bounds__(256) k_emitter_slots(const TriRecord *__restrict__ tris, uint32_t ntris,
                                                       const int32_t *__restrict__ id_em, int32_t *__restrict__ slot_em,
                                                       EmitRecord *__restrict__ rec) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= ntris) return;
    const uint32_t id = tris[slot].id;
    const int32_t e = id < ntris ? id_em[id] : -1;
    slot_em[slot] = e;
    if (e >= 0) rec[e].slot = slot;
}

__global__ void __launch_bounds__(256) k_emitter_table(const TriRecord *__restrict__ tris, uint32_t ntris,
                                                       const float *__restrict__ radiance, uint32_t n, EmitRecord *__restrict__ rec,
                                                       double *__restrict__ area, double *__restrict__ weight) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const uint32_t slot = rec[e].slot;
    if (slot >= ntris) return;  // (every id is below ntris and every id has a slot: not taken)
    const TriRecord t = tris[slot];
    EmitRecord r;
    for (int a = 0; a < 3; ++a) r.v0[a] = t.v0[a], r.e1[a] = t.e1[a], r.e2[a] = t.e2[a], r.rad[a] = radiance[(size_t)e * 3 + a];
    r.slot = slot, r.pad[0] = r.pad[1] = r.pad[2] = 0;
    rec[e] = r;
    const double ax = (double)t.e1[0], ay = (double)t.e1[1], az = (double)t.e1[2];
    const double bx = (double)t.e2[0], by = (double)t.e2[1], bz = (double)t.e2[2];
    const double nx = ay * bz - by * az, ny = az * bx - bz * ax, nz = ax * by - bx * ay;
    const double nn = (nx * nx + ny * ny) + nz * nz;
    const double ar = 0.5 * sqrt(nn);
    area[e] = ar;
    weight[e] = ar * (double)luminance(r.rad[0], r.rad[1], r.rad[2]);
}

constexpr uint32_t kEmitScanChunk = 2048;
__global__ void __launch_bounds__(256) k_emitter_cdf(const double *__restrict__ weight, double *__restrict__ cdf, uint32_t n) {
    __shared__ double s_w[kEmitScanChunk];
    double run = 0.0;  // (lane 0's)
    for (uint32_t base = 0; base < n; base += kEmitScanChunk) {
        const uint32_t m = min(kEmitScanChunk, n - base);
        for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) s_w[i] = weight[base + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (uint32_t i = 0; i < m; ++i) {
                run = run + s_w[i];
                s_w[i] = run;
            }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) cdf[base + i] = s_w[i];
        __syncthreads();
    }
}

// ids / radiance: the caller's table on the device (n ids, 3 n floats); id_em: ntris int32 of scratch.  Writes ed's arrays
// (rec, area, weight, cdf: n entries; slot_em: ntris).  Enqueued on `stream`, nothing synchronised.
int launch_emitter_table(const void *tris, uint32_t ntris, const uint32_t *ids, const float *radiance, int32_t *id_em,
                         const EmitDev &ed, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = ed.n;
    if (n == 0 || ntris == 0) return 0;
    hipError_t e = hipMemsetAsync(id_em, 0xFF, (size_t)ntris * 4, s);
    if (e != hipSuccess) return (int)e;
    EmitRecord *rec = const_cast<EmitRecord *>(ed.rec);
    e = hipMemsetAsync(rec, 0xFF, (size_t)n * sizeof(EmitRecord), s);  // (slot = ~0: k_emitter_table passes over it)
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_emitter_ids, dim3((n + 255) / 256), dim3(256), 0, s, ids, n, id_em);
    hipLaunchKernelGGL(k_emitter_slots, dim3((ntris + 255) / 256), dim3(256), 0, s, (const TriRecord *)tris, ntris, id_em,
                       const_cast<int32_t *>(ed.slot_em), rec);
    hipLaunchKernelGGL(k_emitter_table, dim3((n + 255) / 256), dim3(256), 0, s, (const TriRecord *)tris, ntris, radiance, n, rec,
                       const_cast<double *>(ed.area), const_cast<double *>(ed.weight));
    hipLaunchKernelGGL(k_emitter_cdf, dim3(1), dim3(256), 0, s, ed.weight, const_cast<double *>(ed.cdf), n);
    return launch_status();
}
