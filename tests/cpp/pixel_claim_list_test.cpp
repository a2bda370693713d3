// pixel_claim_list_test.cpp — the list claims of vermilion_amd/csrc/pixel_claim.h (pc_pixel_list, pc_list_settle) on the
// host (tests/test_claim_lists.py builds and runs it; tests/test_gpu_claim_lists.py compares its plane with the device's).
//
//   pixel_claim_list_test IN OUT
// IN (little endian, 32-bit words): ntris, n_nodes, ncams; pos float[ntris * 9]; start, nprims, right_offset
// uint32[n_nodes]; bbox float[n_nodes * 6]; prim_order uint32[ntris] (Scene.bvh() / OracleScene.bvh()); then per camera
// m float[9] (m[col * 3 + row]), position float[3], sensor_x, sensor_y, film_dist (float), width, height (uint32), then
// nrays (uint32) and per ray: pixel (uint32), direction float[3].
// OUT per camera: width * height uint32 single claims (pc_pixel_claim), rows top to bottom; width * height * kListWords
// uint32 list records (the pixels with a single claim: empty); per ray the verdict of pc_list_settle on the ray's pixel:
// slot (uint32, kClaimNone: the ray walks) and t (float).
// The tables are formed as k_camera_tables forms them: the same float operation on the same inputs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#ifdef VMX_PC_DIAG  // why pixels get no list: 1 member's distance out of range, 3 overflow, 4 member not live, 5 budget, 6 unsure, 7 empty
static unsigned long long g_why[8];
#define VMX_PC_WHY(code) (++g_why[code])
#endif
#include "bvh_build.h"
#include "pixel_claim.h"

using namespace vmx;

namespace {

struct HostStack {
    uint32_t ref[kMaxStack + 2];
    float near[kMaxStack + 2];
    void put(int i, uint32_t r, float n) { ref[i] = r, near[i] = n; }
    void get(int i, uint32_t &r, float &n) const { r = ref[i], n = near[i]; }
};

template <class T>
bool read_n(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head[3];
    if (fread(head, 4, 3, f) != 3) return 2;
    const uint32_t ntris = head[0], n_nodes = head[1], ncams = head[2];
    std::vector<float> pos;
    HostBvh bvh;
    if (!read_n(f, pos, (size_t)ntris * 9) || !read_n(f, bvh.start, n_nodes) || !read_n(f, bvh.nprims, n_nodes) ||
        !read_n(f, bvh.right_offset, n_nodes) || !read_n(f, bvh.bbox, (size_t)n_nodes * 6) || !read_n(f, bvh.prim_order, ntris))
        return 2;
    std::string err;
    if (!flatten_bvh(pos.data(), pos.data(), nullptr, ntris, bvh, err)) {
        fprintf(stderr, "flatten_bvh: %s\n", err.c_str());
        return 2;
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    const size_t n_inner = bvh.inner.size();
    std::vector<float> cam_inner(std::max<size_t>(n_inner, 1) * 16), cam_tris((size_t)ntris * 16);
    for (uint32_t ci = 0; ci < ncams; ++ci) {
        PcFilm fm;
        float o[3], sensor[3];
        uint32_t wh[2];
        if (fread(fm.m, 4, 9, f) != 9 || fread(o, 4, 3, f) != 3 || fread(sensor, 4, 3, f) != 3 || fread(wh, 4, 2, f) != 2) return 2;
        fm.sensor_x = sensor[0], fm.sensor_y = sensor[1], fm.film_dist = sensor[2];
        fm.width = wh[0], fm.height = wh[1];
        for (size_t i = 0; i < n_inner; ++i) {  // (lo - o), (hi - o) of both children; the references
            const InnerRecord &r = bvh.inner[i];
            float *q = &cam_inner[i * 16];
            for (int k = 0; k < 3; ++k) {
                q[k] = r.lmin[k] - o[k], q[3 + k] = r.lmax[k] - o[k];
                q[6 + k] = r.rmin[k] - o[k], q[9 + k] = r.rmax[k] - o[k];
            }
            memcpy(q + 12, &r.left, 4), memcpy(q + 13, &r.right, 4);
            q[14] = q[15] = 0.f;
        }
        for (uint32_t t = 0; t < ntris; ++t) {  // e1, e2, tvec = o - v0, qvec = cross(tvec, e1), cd = dot(e2, qvec)
            const TriRecord &r = bvh.tris[t];
            float *q = &cam_tris[(size_t)t * 16];
            const float tx = o[0] - r.v0[0], ty = o[1] - r.v0[1], tz = o[2] - r.v0[2];
            const float qx = ty * r.e1[2] - r.e1[1] * tz, qy = tz * r.e1[0] - r.e1[2] * tx, qz = tx * r.e1[1] - r.e1[0] * ty;
            const float cd = (r.e2[0] * qx + r.e2[1] * qy) + r.e2[2] * qz;
            q[0] = r.e1[0], q[1] = r.e1[1], q[2] = r.e1[2], q[3] = r.e2[0], q[4] = r.e2[1], q[5] = r.e2[2];
            q[6] = tx, q[7] = ty, q[8] = tz, q[9] = qx, q[10] = qy, q[11] = qz, q[12] = cd, q[13] = q[14] = q[15] = 0.f;
        }
        const size_t npix = (size_t)fm.width * fm.height;
        std::vector<uint32_t> claims(npix), lists(npix * kListWords, kClaimNone);
        HostStack stk;
        for (uint32_t p = 0; p < npix; ++p)
            claims[p] = pc_pixel_claim_and_list(fm, p, cam_inner.data(), cam_tris.data(), bvh.root_ref, stk, (int)kMaxStack, &lists[(size_t)p * kListWords]);
        if (fwrite(claims.data(), 4, claims.size(), out) != claims.size()) return 2;
        if (fwrite(lists.data(), 4, lists.size(), out) != lists.size()) return 2;
        uint32_t nrays;
        if (fread(&nrays, 4, 1, f) != 1) return 2;
        std::vector<uint32_t> res((size_t)nrays * 2);
        for (uint32_t i = 0; i < nrays; ++i) {
            uint32_t p;
            float d[3];
            if (fread(&p, 4, 1, f) != 1 || fread(d, 4, 3, f) != 3 || p >= npix) return 2;
            const uint32_t *l = &lists[(size_t)p * kListWords];
            float t = 0.f;
            uint32_t slot = kClaimNone;
            if (l[0] == kClaimNone || !pc_list_settle(cam_tris.data(), l[0], l[1], l[2], l[3], d[0], d[1], d[2], t, slot)) slot = kClaimNone, t = 0.f;
            res[(size_t)i * 2] = slot;
            memcpy(&res[(size_t)i * 2 + 1], &t, 4);
        }
        if (nrays && fwrite(res.data(), 4, res.size(), out) != res.size()) return 2;
    }
#ifdef VMX_PC_DIAG
    for (int i = 1; i < 8; ++i) fprintf(stderr, "why %d: %llu\n", i, g_why[i]);
#endif
    fclose(out);
    fclose(f);
    return 0;
}
