// render_cornell.cpp — a C++ host that drives the MI355X path tracer through the C ABI only
// (include/vermilion_hip.h), in the call order of the reference's main.cpp:58-95:
// build the scene -> install the integrator -> draw -> save the frame.
//
//   g++ -std=c++17 -I include examples/render_cornell.cpp vermilion_amd/libvermilion_hip.so
//       -Wl,-rpath,$PWD/vermilion_amd -o examples/render_cornell     (done by __graft_entry__.build())
//   ./examples/render_cornell out.ppm 256 256 64 [seed] [--nee [--panel]]
// --nee: the light-sampling integrator (vmx_render_nee: VMX_SAMPLING_CORRECTED, every diffuse step samples the emitters)
// instead of PathTracer::Render.
// --panel (with --nee): a ceiling quad is added and its two triangles are named as emitters (vmx_scene_set_emitters): the
// reference's meshes carry no emission, so the host says which triangles light the scene.
//
// Writes a binary PPM the way Camera::saveFrame quantises (floor(x*255), core/camera/camera.cpp:150-170)
// and prints the statistics the reference cannot report (camera.h:101-102 are never incremented).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vermilion_hip.h"

namespace {

// the 8-triangle Cornell-like set of vermilion_amd/scenes.py: floor, back wall, block front + top
void quad(std::vector<float> &pos, std::vector<float> &nrm, std::vector<float> &uv, const float a[3], const float b[3],
          const float c[3], const float d[3], const float n[3]) {
    const float *tri[2][3] = {{a, b, c}, {a, c, d}};
    const float tuv[2][6] = {{0, 0, 1, 0, 1, 1}, {0, 0, 1, 1, 0, 1}};
    for (int t = 0; t < 2; ++t) {
        for (int v = 0; v < 3; ++v) {
            pos.insert(pos.end(), tri[t][v], tri[t][v] + 3);
            nrm.insert(nrm.end(), n, n + 3);
        }
        uv.insert(uv.end(), tuv[t], tuv[t] + 6);
    }
}

}  // namespace

int main(int argc, char **argv) {
    bool nee = false, panel = false;
    int kept = 1;
    for (int i = 1; i < argc; ++i) {  // the flags may stand anywhere: the positional arguments close up
        if (std::strcmp(argv[i], "--nee") == 0) nee = true;
        else if (std::strcmp(argv[i], "--panel") == 0) panel = true;
        else argv[kept++] = argv[i];
    }
    argc = kept;
    if (panel && !nee) {
        std::fprintf(stderr, "--panel needs --nee: only the light-sampling integrator sees emissive triangles\n");
        return 1;
    }
    const char *out = argc > 1 ? argv[1] : "cornell.ppm";
    const uint32_t W = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 256, H = argc > 3 ? (uint32_t)std::atoi(argv[3]) : 256;
    const uint32_t spp = argc > 4 ? (uint32_t)std::atoi(argv[4]) : 64;
    const uint64_t seed = argc > 5 ? std::strtoull(argv[5], nullptr, 10) : 1;

    std::vector<float> pos, nrm, uv;
    const float up[3] = {0, 1, 0}, front[3] = {0, 0, 1};
    const float f0[3] = {-600, 1, 600}, f1[3] = {600, 1, 600}, f2[3] = {600, 1, -800}, f3[3] = {-600, 1, -800};
    quad(pos, nrm, uv, f0, f1, f2, f3, up);
    const float b0[3] = {-600, 1, -800}, b1[3] = {600, 1, -800}, b2[3] = {600, 900, -800}, b3[3] = {-600, 900, -800};
    quad(pos, nrm, uv, b0, b1, b2, b3, front);
    const float k0[3] = {-250, 1, 0}, k1[3] = {150, 1, 0}, k2[3] = {150, 400, 0}, k3[3] = {-250, 400, 0};
    quad(pos, nrm, uv, k0, k1, k2, k3, front);
    const float t0[3] = {-250, 400, 0}, t1[3] = {150, 400, 0}, t2[3] = {150, 400, -400}, t3[3] = {-250, 400, -400};
    quad(pos, nrm, uv, t0, t1, t2, t3, up);
    const uint32_t panel_first = (uint32_t)(pos.size() / 9);  // createBVH-order ids of the panel's two triangles
    if (panel) {
        const float down[3] = {0, -1, 0};
        const float p0[3] = {-300, 880, 300}, p1[3] = {300, 880, 300}, p2[3] = {300, 880, -300}, p3[3] = {-300, 880, -300};
        quad(pos, nrm, uv, p0, p1, p2, p3, down);
    }

    vmx_scene *scene = nullptr;
    if (vmx_scene_create(pos.data(), nrm.data(), uv.data(), (uint32_t)(pos.size() / 9), nullptr, 0, 4, 0, &scene) != VMX_OK) {
        std::fprintf(stderr, "scene: %s\n", vmx_last_error());
        return 1;
    }
    if (panel) {
        const vmx_emitter lights[2] = {{panel_first, {6.f, 5.f, 4.f}}, {panel_first + 1, {6.f, 5.f, 4.f}}};
        vmx_emitter_info info[2];
        uint32_t n = 0;
        if (vmx_scene_set_emitters(scene, lights, 2) != VMX_OK || vmx_scene_emitters(scene, info, 2, &n) != VMX_OK) {
            std::fprintf(stderr, "emitters: %s\n", vmx_last_error());
            return 1;
        }
        std::printf("panel: %u emissive triangles, area %.0f + %.0f\n", n, info[0].area, info[1].area);
    }
    vmx_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.position[0] = 0, cam.position[1] = 420, cam.position[2] = 1900;
    cam.back_distance = 6.0f;  // renderEngine.cpp:135
    cam.back_size[0] = 3.6f, cam.back_size[1] = 3.6f * (float)H / (float)W;
    cam.image_res[0] = W, cam.image_res[1] = H;
    cam.rays_per_pixel = spp;
    vmx_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    opts.seed = seed;
    opts.early_stop = 1;
    opts.sampling = VMX_SAMPLING_PARITY;
    std::vector<float> frame((size_t)W * H * 5);
    vmx_stats st;
    if (nee) opts.early_stop = 0, opts.sampling = VMX_SAMPLING_CORRECTED;
    if ((nee ? vmx_render_nee(scene, &cam, &opts, frame.data(), &st) : vmx_render(scene, &cam, &opts, frame.data(), &st)) != VMX_OK) {
        std::fprintf(stderr, "render: %s\n", vmx_last_error());
        vmx_scene_destroy(scene);
        return 1;
    }
    FILE *f = std::fopen(out, "wb");
    if (!f) return 2;
    std::fprintf(f, "P6\n%u %u\n255\n", W, H);
    double sum = 0;
    for (size_t p = 0; p < (size_t)W * H; ++p) {
        unsigned char rgb[3];
        for (int c = 0; c < 3; ++c) {
            rgb[c] = (unsigned char)std::floor(frame[p * 5 + c] * 255.0f);
            sum += frame[p * 5 + c];
        }
        std::fwrite(rgb, 1, 3, f);
    }
    std::fclose(f);
    std::printf("frame %ux%u spp %u seed %llu: rays %llu (+%llu secondary), samples %llu, %.2f ms device, checksum %.9g\n", W, H,
                spp, (unsigned long long)seed, (unsigned long long)st.rays_primary, (unsigned long long)st.rays_secondary,
                (unsigned long long)st.samples, st.ms_device, sum);
    vmx_scene_destroy(scene);
    return 0;
}
