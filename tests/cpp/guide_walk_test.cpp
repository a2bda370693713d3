// guide_walk_test.cpp — the walk and the per-ray rule of vermilion_amd/csrc/guide_walk.h on the host, over the guide
// that a scene builds (build_bvh_sah + make_guide_records of bvh_build.cpp) beside a given reference tree.
//   guide_walk_test IN OUT
// IN : uint32 ntris, n_nodes, nrays; float pos[ntris*9]; the reference tree's flat layout (uint32 start, nprims,
//      right_offset [n_nodes]; float bbox[n_nodes*6]; uint32 prim_order[ntris]); nrays x (float o[3], float d[3])
// OUT: uint64 guide visits (inner, triangle) at kappa = 2^-10, 2^-8, 2^-6 over the rays that walk [6]; uint64 depth of
//      the guide's and of the reference tree's deepest node (the root is 0) [2]; then per ray
//      uint32 verdict (GwVerdict), uint32 reference leaf slot of the winner (0xFFFFFFFF: none), float best,
//      uint32 guide inner visits, guide triangle tests, reference inner visits, reference triangle tests
// tests/guide_spec.py builds and runs it; the oracle judges what it settles.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bvh_build.h"
#include "guide_walk.h"

using namespace vmx;

namespace {

template <class T>
bool read_n(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

// depth of the flat tree's deepest node (the root is 0), as the builders count it
uint32_t flat_depth(const HostBvh &b) {
    struct Item {
        uint32_t node, depth;
    };
    std::vector<Item> work{{0u, 0u}};
    uint32_t deepest = 0;
    while (!work.empty()) {
        const Item it = work.back();
        work.pop_back();
        if (it.depth > deepest) deepest = it.depth;
        if (b.right_offset[it.node] == 0) continue;
        work.push_back({it.node + 1, it.depth + 1});
        work.push_back({it.node + b.right_offset[it.node], it.depth + 1});
    }
    return deepest;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: guide_walk_test IN OUT\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head[3];
    if (std::fread(head, 4, 3, f) != 3) return 2;
    const uint32_t ntris = head[0], n_nodes = head[1], nrays = head[2];
    std::vector<float> pos, rays;
    HostBvh ref;
    if (!read_n(f, pos, (size_t)ntris * 9) || !read_n(f, ref.start, n_nodes) || !read_n(f, ref.nprims, n_nodes) ||
        !read_n(f, ref.right_offset, n_nodes) || !read_n(f, ref.bbox, (size_t)n_nodes * 6) || !read_n(f, ref.prim_order, ntris) ||
        !read_n(f, rays, (size_t)nrays * 6)) {
        std::fprintf(stderr, "guide_walk_test: short input\n");
        return 2;
    }
    std::fclose(f);
    for (uint32_t i = 0; i < n_nodes; ++i)
        if (ref.right_offset[i] == 0) ref.n_leaves++;
    ref.max_depth = flat_depth(ref);
    std::string err;
    if (!flatten_bvh(pos.data(), pos.data(), nullptr, ntris, ref, err)) {
        std::fprintf(stderr, "guide_walk_test: %s\n", err.c_str());
        return 2;
    }
    HostBvh guide;
    if (!build_bvh_sah(pos.data(), pos.data(), nullptr, ntris, 4, guide, err)) {
        std::fprintf(stderr, "guide_walk_test: %s\n", err.c_str());
        return 2;
    }
    const float scene_max = make_guide_records(guide, ref, pos.data(), ntris);

    const float kappas[3] = {9.765625e-04f, 3.90625e-03f, 1.5625e-02f};
    uint64_t visits[6] = {0, 0, 0, 0, 0, 0};
    std::vector<uint32_t> out((size_t)nrays * 7);
    for (uint32_t i = 0; i < nrays; ++i) {
        const float *o = &rays[(size_t)i * 6], *d = o + 3;
        const float inv[3] = {1.0f / d[0], 1.0f / d[1], 1.0f / d[2]};
        uint32_t *w = &out[(size_t)i * 7];
        w[1] = 0xFFFFFFFFu;
        for (int k = 2; k < 7; ++k) w[k] = 0;
        if (!gw_ray_ok(o[0], o[1], o[2], d[0], d[1], d[2], inv[0], inv[1], inv[2], scene_max)) {
            w[0] = (uint32_t)kGwInput;
            continue;
        }
        GwResult g, r;
        if (!gw_walk(guide.inner.data(), guide.tris.data(), guide.root_ref, o, d, inv, kGwCut, g) ||
            !gw_walk(ref.inner.data(), ref.tris.data(), ref.root_ref, o, d, inv, 1.0f, r))
            return 3;
        const bool have = g.slot >= 0;
        const float *rec = have ? guide.tris[g.slot].v0 : nullptr;
        w[0] = (uint32_t)gw_verdict(have, rec, g.best, g.second, o, d, inv, scene_max);
        if (have) w[1] = guide.tris[g.slot].pad[0];
        std::memcpy(&w[2], &g.best, 4);
        w[3] = g.inner_visits, w[4] = g.tri_tests, w[5] = r.inner_visits, w[6] = r.tri_tests;
        for (int k = 0; k < 3; ++k) {
            GwResult v;
            if (!gw_walk(guide.inner.data(), guide.tris.data(), guide.root_ref, o, d, inv, 1.0f + kappas[k], v)) return 3;
            visits[2 * k] += v.inner_visits, visits[2 * k + 1] += v.tri_tests;
        }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    const uint64_t depths[2] = {guide.max_depth, ref.max_depth};
    std::fwrite(visits, 8, 6, f);
    std::fwrite(depths, 8, 2, f);
    std::fwrite(out.data(), 4, out.size(), f);
    std::fclose(f);
    return 0;
}
