/*
 * ref_driver.cpp — C ABI over the REFERENCE'S OWN compiled classes (TEST INFRASTRUCTURE ONLY).
 *
 * `make -C oracle ref` compiles the reference's translation units in place and unmodified, against the
 * stand-in headers of oracle/ref_standin/, and links them with this file into oracle/_ref/libvmx_ref*.so
 * (never committed).  The entry points are shaped like vmx_oracle.h so that the same numpy inputs feed the
 * reference, the oracle and the kernels; tests/ref_lib.py binds them, tests/test_ref_pin.py compares.
 *
 * Every result below is computed by reference code: BVH::BVH / BVH::getIntersection, MeshEngine::load ->
 * processScene -> createBVH, MeshEngine::RayCast / RayCastCollision / bindTexture, VermiTexture::Sample,
 * the free function Radiance of pathtracer.cpp, Camera::saveFrame.  This file only carries arrays in and out.
 */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <mutex>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include <fcntl.h>
#include <unistd.h>

#include "glm/glm.hpp"

/* BVH and Triangle keep their data in default-private sections (no access keyword to redefine), and the flat
 * tree has no accessor.  Open them for THIS translation unit's view of the two headers only — every standard
 * and stand-in header they include is already in above; the reference's own units are compiled untouched. */
#define class struct
#include "accelerators/bvh.h"
#include "accelerators/triangle.h"
#undef class

#include "OpenImageIO/imagebuf.h"
#include "camera/camera.h"
#include "engines/loggingEngine.h"
#include "engines/meshEngine.h"

#include "../include/vermilion_hip.h"

/* pathtracer.cpp:21 — a free function without a declaration in any header */
glm::vec4 Radiance(Vermilion::MeshEngine *mEng, glm::vec3 rStart, glm::vec3 rDir, std::mt19937_64 &mtRanEngine);

namespace {

/* The reference prints build statistics with printf (bvh.cpp, meshEngine.cpp) and saveFrame writes to
 * std::cout: keep a test run's output clean by pointing fd 1 at the null device for the duration. */
struct QuietStdout {
    int saved;
    QuietStdout() {
        fflush(stdout);
        std::cout.flush();
        saved = dup(1);
        int nul = open("/dev/null", O_WRONLY);
        if (nul >= 0) {
            dup2(nul, 1);
            close(nul);
        }
    }
    ~QuietStdout() {
        fflush(stdout);
        std::cout.flush();
        if (saved >= 0) {
            dup2(saved, 1);
            close(saved);
        }
    }
};

std::mutex g_build_mutex; /* the stand-in importer's "next scene" and the image registry are process-wide */
uint64_t g_texture_serial = 0;

inline glm::vec3 v3(const float *p) { return glm::vec3(p[0], p[1], p[2]); }

} // namespace

struct ref_scene {
    uint32_t ntris = 0;
    /* direct path: our Triangle objects -> BVH(objects, leaf) */
    std::vector<Triangle *> tris;
    std::unordered_map<const Object *, int32_t> index_of;
    BVH *bvh = nullptr;
    /* engine path: aiScene carriers -> MeshEngine::load -> createBVH (always leaf 4) */
    std::vector<aiVector3D> vertices, normals, texcoords;
    std::vector<unsigned int> indices;
    std::vector<aiFace> faces;
    std::vector<aiMesh> meshes;
    std::vector<aiMesh *> mesh_ptrs;
    std::vector<aiMaterial> materials;
    std::vector<aiMaterial *> material_ptrs;
    aiScene scene;
    Vermilion::LogEngine *logger = nullptr;
    Vermilion::MeshEngine *engine = nullptr;

    ~ref_scene() {
        delete engine;
        delete logger;
        delete bvh;
        for (Triangle *t : tris) delete t;
    }
};

extern "C" {

const char *ref_build_flags(void) {
#ifdef REF_BUILD_FLAGS
    return REF_BUILD_FLAGS;
#else
    return "unknown";
#endif
}

/* pos/nrm [ntris*9], uv [ntris*6] or NULL.  mesh_sizes[nmeshes]: consecutive triangle ranges, one aiMesh each
 * (NULL: one mesh); mesh_has_uv[nmeshes]: 0 leaves that mesh's mTextureCoords[0] null (NULL: all follow `uv`).
 * leaf_size is for the direct BVH only. */
ref_scene *ref_scene_create(const float *pos, const float *nrm, const float *uv, uint32_t ntris, uint32_t leaf_size,
                            const uint32_t *mesh_sizes, const uint8_t *mesh_has_uv, uint32_t nmeshes) {
    if (!pos || !nrm || ntris == 0) return nullptr;
    const uint32_t one = ntris;
    if (!mesh_sizes) mesh_sizes = &one, nmeshes = 1, mesh_has_uv = nullptr;
    uint64_t total = 0;
    for (uint32_t m = 0; m < nmeshes; ++m) total += mesh_sizes[m];
    if (total != ntris) return nullptr;

    std::lock_guard<std::mutex> lock(g_build_mutex);
    QuietStdout quiet;
    ref_scene *sc = new ref_scene();
    sc->ntris = ntris;
    const size_t nv = (size_t)ntris * 3;
    sc->vertices.resize(nv), sc->normals.resize(nv), sc->texcoords.resize(nv), sc->indices.resize(nv);
    sc->faces.resize(ntris), sc->meshes.resize(nmeshes), sc->mesh_ptrs.resize(nmeshes);
    sc->materials.resize(nmeshes), sc->material_ptrs.resize(nmeshes);
    for (size_t v = 0; v < nv; ++v) {
        sc->vertices[v] = aiVector3D{pos[v * 3], pos[v * 3 + 1], pos[v * 3 + 2]};
        sc->normals[v] = aiVector3D{nrm[v * 3], nrm[v * 3 + 1], nrm[v * 3 + 2]};
        sc->texcoords[v] = uv ? aiVector3D{uv[v * 2], uv[v * 2 + 1], 0.f} : aiVector3D{0.f, 0.f, 0.f};
    }
    uint32_t first = 0;
    std::vector<uint8_t> tri_has_uv(ntris);
    for (uint32_t m = 0; m < nmeshes; ++m) {
        const bool has_uv = uv && (!mesh_has_uv || mesh_has_uv[m]);
        aiMesh &mesh = sc->meshes[m];
        mesh.mNumFaces = mesh_sizes[m];
        mesh.mNumVertices = mesh_sizes[m] * 3;
        mesh.mVertices = sc->vertices.data() + (size_t)first * 3;
        mesh.mNormals = sc->normals.data() + (size_t)first * 3;
        mesh.mTextureCoords[0] = has_uv ? sc->texcoords.data() + (size_t)first * 3 : nullptr;
        mesh.mFaces = sc->faces.data() + first;
        mesh.mMaterialIndex = m;
        for (uint32_t f = 0; f < mesh_sizes[m]; ++f) {
            unsigned int *idx = sc->indices.data() + (size_t)(first + f) * 3;
            idx[0] = f * 3, idx[1] = f * 3 + 1, idx[2] = f * 3 + 2; /* per-mesh vertex indices */
            sc->faces[first + f] = aiFace{3, idx};
            tri_has_uv[first + f] = has_uv;
        }
        sc->mesh_ptrs[m] = &mesh;
        sc->material_ptrs[m] = &sc->materials[m];
        first += mesh_sizes[m];
    }
    sc->scene.mNumMeshes = nmeshes, sc->scene.mMeshes = sc->mesh_ptrs.data();
    sc->scene.mNumMaterials = nmeshes, sc->scene.mMaterials = sc->material_ptrs.data();

    /* engine path */
    sc->logger = new Vermilion::LogEngine(std::string("/dev/null"), Vermilion::VermiLogFile, Vermilion::VermiLogLevelNone);
    sc->engine = new Vermilion::MeshEngine(sc->logger);
    Assimp::standin_set_next_scene(&sc->scene);
    std::string any_existing_path("/dev/null"); /* load() only checks that the file opens */
    const bool ok = sc->engine->load(any_existing_path);
    Assimp::standin_set_next_scene(nullptr);
    if (!ok || !sc->engine->sceneAccelerator) {
        delete sc;
        return nullptr;
    }

    /* direct path: Triangle's own constructor, then BVH(objects, leaf) */
    sc->tris.resize(ntris);
    std::vector<Object *> objects(ntris);
    for (uint32_t i = 0; i < ntris; ++i) {
        const float *p = pos + (size_t)i * 9, *n = nrm + (size_t)i * 9;
        glm::vec2 t0, t1, t2; /* a mesh without UVs leaves createBVH's default-constructed vec2 in place */
        if (tri_has_uv[i]) {
            const float *q = uv + (size_t)i * 6;
            t0 = glm::vec2(q[0], q[1]), t1 = glm::vec2(q[2], q[3]), t2 = glm::vec2(q[4], q[5]);
        }
        sc->tris[i] = new Triangle(v3(p), v3(p + 3), v3(p + 6), v3(n), v3(n + 3), v3(n + 6), t0, t1, t2);
        objects[i] = sc->tris[i];
        sc->index_of[sc->tris[i]] = (int32_t)i;
    }
    sc->bvh = new BVH(objects, leaf_size ? leaf_size : 4);
    return sc;
}

void ref_scene_destroy(ref_scene *sc) { delete sc; }

/* MeshEngine::bindTexture as written, fed by the stand-in ImageInput */
int ref_scene_bind_texture(ref_scene *sc, const float *data, uint32_t w, uint32_t h, uint32_t c) {
    if (!sc || !data || w == 0 || h == 0 || c == 0 || c > 4 || w > 65535 || h > 65535) return 1;
    std::lock_guard<std::mutex> lock(g_build_mutex);
    std::string name = "vmx-ref-texture-" + std::to_string(g_texture_serial++);
    OpenImageIO::standin_register_image(name, (int)w, (int)h, (int)c, data);
    const bool ok = sc->engine->bindTexture(name);
    OpenImageIO::standin_images().erase(name);
    return ok ? 0 : 1;
}

/* which: 0 = BVH(objects, leaf_size) built here, 1 = the tree MeshEngine::createBVH built */
static const BVH *tree_of(const ref_scene *sc, int which) { return which ? sc->engine->sceneAccelerator : sc->bvh; }

void ref_scene_describe(const ref_scene *sc, int which, uint32_t *n_nodes, uint32_t *n_leaves) {
    if (n_nodes) *n_nodes = tree_of(sc, which)->nNodes;
    if (n_leaves) *n_leaves = tree_of(sc, which)->nLeafs;
}

/* prim_order is available for the direct tree only (the engine's Triangle objects are its own) */
void ref_scene_bvh(const ref_scene *sc, int which, uint32_t *start, uint32_t *nprims, uint32_t *right_offset, float *bbox,
                   uint32_t *prim_order) {
    const BVH *t = tree_of(sc, which);
    for (uint32_t i = 0; i < t->nNodes; ++i) {
        const BVHFlatNode &n = t->flatTree[i];
        if (start) start[i] = n.start;
        if (nprims) nprims[i] = n.nPrims;
        if (right_offset) right_offset[i] = n.rightOffset;
        if (bbox) {
            float *b = bbox + (size_t)i * 6;
            b[0] = n.bbox.min.x, b[1] = n.bbox.min.y, b[2] = n.bbox.min.z;
            b[3] = n.bbox.max.x, b[4] = n.bbox.max.y, b[5] = n.bbox.max.z;
        }
    }
    if (prim_order && which == 0)
        for (size_t i = 0; i < t->build_prims.size(); ++i) prim_order[i] = (uint32_t)sc->index_of.at(t->build_prims[i]);
}

/* BVH::getIntersection(ray, &ii, false) on the direct tree: tri_id = input index of ii.object (-1: none), t = ii.t */
void ref_trace(const ref_scene *sc, const float *o, const float *d, uint32_t n, int32_t *tri_id, float *t) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; ++i) {
        Ray r(v3(o + i * 3), v3(d + i * 3));
        IntersectionInfo ii{};
        const bool hit = sc->bvh->getIntersection(r, &ii, false);
        tri_id[i] = hit ? sc->index_of.at(ii.object) : -1;
        t[i] = ii.t;
    }
}

/* MeshEngine::RayCast with every out-pointer given.  Filled: location, distance, normal, uv, colour, flags
 * (bit0 return value, bit1 *ppImpactMaterial != nullptr).  tri_id / tri_t are this project's additions to the
 * record — RayCast does not return them — and are left at -1 / 0; `pad` carries the index of the returned material
 * in aiScene::mMaterials plus one (0: null), which the reference always takes from slot 0. */
void ref_raycast(const ref_scene *sc, const float *o, const float *d, uint32_t n, vmx_rayhit *out) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; ++i) {
        aiMaterial *mat = nullptr;
        glm::vec3 loc, nor, col;
        glm::vec2 tex;
        float dist = 0.f;
        const bool hit = sc->engine->RayCast(v3(o + i * 3), v3(d + i * 3), &mat, &loc, &nor, &dist, &tex, &col);
        vmx_rayhit &h = out[i];
        std::memset(&h, 0, sizeof(h));
        h.location[0] = loc.x, h.location[1] = loc.y, h.location[2] = loc.z;
        h.distance = dist;
        h.normal[0] = nor.x, h.normal[1] = nor.y, h.normal[2] = nor.z;
        h.tri_id = -1;
        h.uv[0] = tex.x, h.uv[1] = tex.y;
        h.flags = (hit ? 1u : 0u) | (mat ? 2u : 0u);
        h.colour[0] = col.x, h.colour[1] = col.y, h.colour[2] = col.z;
        h.pad = mat ? (uint32_t)(mat - sc->materials.data()) + 1u : 0u;
    }
}

void ref_collision(const ref_scene *sc, const float *o, const float *d, uint32_t n, uint8_t *out) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; ++i) out[i] = sc->engine->RayCastCollision(v3(o + i * 3), v3(d + i * 3)) ? 1 : 0;
}

/* VermiTexture::Sample on a texture of our making; out4 is preset to -1 so an untouched sample shows */
void ref_texture_sample(const float *data, uint32_t w, uint32_t h, uint32_t c, const float *uv, uint32_t n, float *out4) {
    Vermilion::VermiTexture tex((uint16_t)w, (uint16_t)h, (uint16_t)c, const_cast<float *>(data));
    for (uint32_t i = 0; i < n; ++i) {
        glm::vec4 s(-1.f, -1.f, -1.f, -1.f);
        tex.Sample(glm::vec2(uv[i * 2], uv[i * 2 + 1]), &s);
        out4[i * 4] = s.x, out4[i * 4 + 1] = s.y, out4[i * 4 + 2] = s.z, out4[i * 4 + 3] = s.w;
    }
}

/* Radiance(mEng, o, d, engine) with std::mt19937_64 seeded seeds[i] per ray, as orc_radiance_mt seeds it */
void ref_radiance_mt(const ref_scene *sc, const float *o, const float *d, uint32_t n, const uint64_t *seeds, float *out4) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; ++i) {
        std::mt19937_64 eng;
        eng.seed(seeds[i]);
        glm::vec4 r = Radiance(sc->engine, v3(o + i * 3), v3(d + i * 3), eng);
        out4[i * 4] = r.x, out4[i * 4 + 1] = r.y, out4[i * 4 + 2] = r.z, out4[i * 4 + 3] = r.w;
    }
}

/* Camera::saveFrame's conversion of an RGBAZ frame [W*H*5]: the stand-in ImageBuf hands the two buffers to the hook
 * below instead of encoding files.  Not thread-safe (one hook target). */
static unsigned char *g_q_rgba = nullptr;
static float *g_q_depth = nullptr;
static void quantize_hook(const std::string &, const OpenImageIO::ImageSpec &spec, const void *pixels) {
    const size_t npix = (size_t)spec.width * spec.height;
    if (spec.nchannels == 4 && g_q_rgba) std::memcpy(g_q_rgba, pixels, npix * 4);
    if (spec.nchannels == 1 && g_q_depth) std::memcpy(g_q_depth, pixels, npix * sizeof(float));
}
void ref_quantize(const float *frame, uint32_t W, uint32_t H, unsigned char *rgba8, float *depth) {
    std::lock_guard<std::mutex> lock(g_build_mutex);
    QuietStdout quiet;
    Vermilion::cameraSettings s{};
    s.imageResX = W, s.imageResY = H;
    s.renderMode = Vermilion::vermRenderMode::RGBAZ;
    Vermilion::Camera cam(s);
    std::memcpy(cam.mImage, frame, (size_t)W * H * 5 * sizeof(float));
    g_q_rgba = rgba8, g_q_depth = depth;
    OpenImageIO::standin_on_write() = quantize_hook;
    cam.saveFrame("vmx-ref-frame");
    OpenImageIO::standin_on_write() = nullptr;
    g_q_rgba = nullptr, g_q_depth = nullptr;
}

} /* extern "C" */
