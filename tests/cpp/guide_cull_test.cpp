// guide_cull_test.cpp — the guide walk of vermilion_amd/csrc/guide_walk.h with and without the skip of boxes that end
// behind the ray's origin ((B) there), on the host, over the guide that a scene builds beside a given reference tree.
//   guide_cull_test IN OUT [LIMIT ...]
// IN : as guide_walk_test reads it: uint32 ntris, n_nodes, nrays; float pos[ntris*9]; the reference tree's flat layout
//      (uint32 start, nprims, right_offset [n_nodes]; float bbox[n_nodes*6]; uint32 prim_order[ntris]); nrays x (float
//      o[3], float d[3])
// LIMIT: the shape limits to mark the guide's child boxes with (mark_guide_children); "inf" marks every child, the plain
//      cull.  None given: the library's own kGwShapeMax, the marks make_guide_records left.
// OUT: uint32 nsets = 1 + number of limits; double kGwShapeMax, the library's limit; per set uint32 flagged triangles,
//      unmarked child boxes, child boxes in all
//      (set 0 is the walk that never skips: the marks of a copy of the records cleared); then per ray and set
//      uint32 verdict (GwVerdict), uint32 reference leaf slot of the winner (0xFFFFFFFF: none), float best,
//      uint32 guide inner visits, guide triangle tests
// tests/guide_cull_spec.py builds and runs it; the oracle judges what it settles.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
    if (argc < 3) {
        std::fprintf(stderr, "usage: guide_cull_test IN OUT [LIMIT ...]\n");
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
        std::fprintf(stderr, "guide_cull_test: short input\n");
        return 2;
    }
    std::fclose(f);
    for (uint32_t i = 0; i < n_nodes; ++i)
        if (ref.right_offset[i] == 0) ref.n_leaves++;
    ref.max_depth = flat_depth(ref);
    std::string err;
    if (!flatten_bvh(pos.data(), pos.data(), nullptr, ntris, ref, err)) {
        std::fprintf(stderr, "guide_cull_test: %s\n", err.c_str());
        return 2;
    }
    HostBvh guide;
    if (!build_bvh_sah(pos.data(), pos.data(), nullptr, ntris, 4, guide, err)) {
        std::fprintf(stderr, "guide_cull_test: %s\n", err.c_str());
        return 2;
    }
    const float scene_max = make_guide_records(guide, ref, pos.data(), ntris);

    // set 0: no child is marked; then one set of inner records per limit
    const uint32_t nsets = argc > 3 ? (uint32_t)(argc - 2) : 2u;
    std::vector<std::vector<InnerRecord>> sets(nsets, guide.inner);
    std::vector<uint32_t> counts((size_t)nsets * 3, 0u);
    for (uint32_t s = 0; s < nsets; ++s) {
        HostBvh g = guide;  // (the marks of make_guide_records stay in `guide`)
        double limit = kGwShapeMax;
        if (s == 0) limit = -1.0;
        else if (argc > 3) limit = std::strcmp(argv[2 + s], "inf") == 0 ? (double)INFINITY : std::atof(argv[2 + s]);
        uint32_t unmarked = 0;
        counts[(size_t)s * 3] = mark_guide_children(g, limit, &unmarked);
        counts[(size_t)s * 3 + 1] = unmarked, counts[(size_t)s * 3 + 2] = 2u * (uint32_t)g.inner.size();
        if (s == 1 && argc == 3 && std::memcmp(g.inner.data(), guide.inner.data(), g.inner.size() * sizeof(InnerRecord)) != 0) {
            std::fprintf(stderr, "guide_cull_test: make_guide_records did not mark with kGwShapeMax\n");
            return 3;
        }
        sets[s].swap(g.inner);
    }

    std::vector<uint32_t> out((size_t)nrays * nsets * 5);
    for (uint32_t i = 0; i < nrays; ++i) {
        const float *o = &rays[(size_t)i * 6], *d = o + 3;
        const float inv[3] = {1.0f / d[0], 1.0f / d[1], 1.0f / d[2]};
        const bool walks = gw_ray_ok(o[0], o[1], o[2], d[0], d[1], d[2], inv[0], inv[1], inv[2], scene_max);
        for (uint32_t s = 0; s < nsets; ++s) {
            uint32_t *w = &out[((size_t)i * nsets + s) * 5];
            w[0] = (uint32_t)kGwInput, w[1] = 0xFFFFFFFFu, w[2] = w[3] = w[4] = 0;
            if (!walks) continue;
            GwResult g;
            if (!gw_walk(sets[s].data(), guide.tris.data(), guide.root_ref, o, d, inv, kGwCut, g)) return 3;
            const bool have = g.slot >= 0;
            const float *rec = have ? guide.tris[g.slot].v0 : nullptr;
            w[0] = (uint32_t)gw_verdict(have, rec, g.best, g.second, o, d, inv, scene_max);
            if (have) w[1] = guide.tris[g.slot].pad[0];
            std::memcpy(&w[2], &g.best, 4);
            w[3] = g.inner_visits, w[4] = g.tri_tests;
        }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(&nsets, 4, 1, f);
    const double shape_max = kGwShapeMax;
    std::fwrite(&shape_max, 8, 1, f);
    std::fwrite(counts.data(), 4, counts.size(), f);
    std::fwrite(out.data(), 4, out.size(), f);
    std::fclose(f);
    return 0;
}
