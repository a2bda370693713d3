// vmx_albedo.inc — the per-pixel albedo plane of a camera (vmx_albedo_camera_device): what the integrator multiplies a
// camera path's throughput by at its first hit (pathtracer.cpp:63-66, 75-79), averaged over a run of samples.  Included
// by vmx_kernels.hip (inside its namespace, after vmx_query.inc).  The arithmetic is stated in include/vermilion_hip.h
// and restated in tests/demod_spec.py: one rounding per written operation, bit for bit the restatement.
//
// Per sample k the camera-ray query of the G-buffer path runs as it is — k_query<kQueryCastCamera> with per-lane record
// fetch, the faster of its two forms on coherent camera rays (profiles/raycast_bench.txt; same results) — which leaves
// (tri_t, leaf slot) in words 10 and 15 of a 64-byte record per pixel (here: the scene's scratch, never a caller's
// buffer) — and then
//   k_albedo_finish  one lane per pixel, dense.  Of MeshEngine::RayCast's record only the material bit and uv matter:
//                    the bit is "the BVH query hit a triangle" (hitMeshIndex is set there and never reset by a nearer
//                    sphere, meshEngine.cpp:370) and uv is that triangle's (stale behind a nearer sphere, as the
//                    integrator reads it), so no sphere is tested and no normal formed.  TEX: the scene has a bound
//                    texture — the ray is formed again (primary_ray), the hit point and its barycentrics as
//                    tri_shading_normal forms them, then tex_sample; without one every sample is (1, 1, 1) and only
//                    the slot is read.  The plane carries (sum.xyz, bits(cnt)) between the samples' launches and
//                    leaves as (sum / n, cnt / n) from the last: one float4 per lane to consecutive addresses.

// uv of Triangle::getNormal (triangle.cpp:67-86): tri_shading_normal's barycentrics and uv, operation for operation
__device__ __forceinline__ void tri_uv(const SceneDev &sc, int slot, float hx, float hy, float hz, float &uvx, float &uvy) {
    const float4 *__restrict__ tris = (const float4 *)sc.tris;
    const float4 *__restrict__ attrs = (const float4 *)sc.attrs;
    const float4 a = tris[slot * 3], b = tris[slot * 3 + 1], c = tris[slot * 3 + 2];
    const float f0x = a.w, f0y = b.x, f0z = b.y, f1x = b.z, f1y = b.w, f1z = c.x;
    const float f2x = hx - a.x, f2y = hy - a.y, f2z = hz - a.z;
    const float d00 = dot3(f0x, f0y, f0z, f0x, f0y, f0z);
    const float d01 = dot3(f0x, f0y, f0z, f1x, f1y, f1z);
    const float d11 = dot3(f1x, f1y, f1z, f1x, f1y, f1z);
    const float d20 = dot3(f2x, f2y, f2z, f0x, f0y, f0z);
    const float d21 = dot3(f2x, f2y, f2z, f1x, f1y, f1z);
    const float denom = d00 * d11 - d01 * d01;
    const float w1 = (d11 * d20 - d01 * d21) / denom;
    const float w2 = (d00 * d21 - d01 * d20) / denom;
    const float w0 = 1.0f - w1 - w2;
    const float4 g2 = attrs[slot * 4 + 2], g3 = attrs[slot * 4 + 3];
    // uv0 = (g2.y, g2.z), uv1 = (g2.w, g3.x), uv2 = (g3.y, g3.z)
    uvx = (g2.y * w0 + g2.w * w1) + g3.y * w2;
    uvy = (g2.z * w0 + g3.x * w1) + g3.z * w2;
}

template <bool TEX>
__global__ void __launch_bounds__(256)
k_albedo_finish(SceneDev sc, FrameDev fr, const float *__restrict__ rec, uint32_t npix, uint32_t k, uint32_t first,
                uint32_t last, uint32_t n, float4 *__restrict__ plane) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int slot = __float_as_int(rec[(size_t)p * 16 + 15]);
    const bool mat = slot >= 0;
    float t0 = 1.f, t1 = 1.f, t2 = 1.f;
    if (TEX && mat) {
        const float best = rec[(size_t)p * 16 + 10];
        Rng rng;
        float dx, dy, dz;
        primary_ray(fr, p, k, rng, dx, dy, dz);
        const float hx = fr.px + dx * best, hy = fr.py + dy * best, hz = fr.pz + dz * best;  // bvh.cpp:140
        float u, v;
        tri_uv(sc, slot, hx, hy, hz, u, v);
        const float4 t = tex_sample(sc, u, v);
        t0 = t.x, t1 = t.y, t2 = t.z;
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);  // (sum.xyz, bits(cnt))
    if (!first) acc = plane[p];
    acc.x = acc.x + t0, acc.y = acc.y + t1, acc.z = acc.z + t2;
    const uint32_t cnt = __float_as_uint(acc.w) + (mat ? 1u : 0u);
    if (last) {
        const float fn = (float)n;
        plane[p] = make_float4(acc.x / fn, acc.y / fn, acc.z / fn, (float)cnt / fn);
    } else {
        plane[p] = make_float4(acc.x, acc.y, acc.z, __uint_as_float(cnt));
    }
}

// sample q.sample of a plane's run: the camera-ray query into `rec` (64 bytes per pixel, words 10 and 15 written), then
// the finish into `plane`; first / last: of the run's samples, n of them
int launch_albedo_sample(const SceneDev &sc, const QueryDev &q, const FrameDev &fr, void *rec, bool first, bool last,
                         uint32_t n, void *plane, LaunchCfg cfg, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const QueryCast c = {fr, (float *)rec};
    hipLaunchKernelGGL(query_cast_kernel(true, false), dim3(cfg.grid), dim3(cfg.block), cfg.lds_bytes, s, sc, q, c);
    if (int e = launch_status()) return e;
    const dim3 grid((q.n + 255) / 256);
    if (sc.tex)
        hipLaunchKernelGGL(k_albedo_finish<true>, grid, dim3(256), 0, s, sc, fr, (const float *)rec, q.n, q.sample,
                           first ? 1u : 0u, last ? 1u : 0u, n, (float4 *)plane);
    else
        hipLaunchKernelGGL(k_albedo_finish<false>, grid, dim3(256), 0, s, sc, fr, (const float *)rec, q.n, q.sample,
                           first ? 1u : 0u, last ? 1u : 0u, n, (float4 *)plane);
    return launch_status();
}
