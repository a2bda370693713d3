// render_progressive.cpp — the frame of render_cornell.cpp in steps of a few samples, through the C ABI only
// (include/vermilion_hip.h): vmx_progressive_begin -> { vmx_progressive_step, vmx_progressive_preview } -> end.
// A host application shows every preview (this one prints how many pixels still take samples) and may stop at any
// step; the frame of the last step is vmx_render's, bit for bit.
//
//   g++ -std=c++17 -I include examples/render_progressive.cpp vermilion_amd/libvermilion_hip.so
//       -Wl,-rpath,$PWD/vermilion_amd -o examples/render_progressive     (done by __graft_entry__.build())
//   ./examples/render_progressive out.ppm 256 256 64 [seed [samples_per_step [frame.f32]]]
//
//   ./examples/render_progressive --adaptive out.ppm 256 256 16 [seed [samples_per_step [frame.f32]]]
//     adaptive sampling: a handle with four times the given spp as its ceiling (fixed spp, VMX_PROGRESSIVE_MOMENTS) takes 8
//     uniform samples, then vmx_progressive_step_adaptive of samples_per_step (default 4) — only the pixels whose mean is
//     still uncertain, by the library's default parameters — until the mean count per pixel reaches the given spp or
//     nothing is selected any more, and the final PREVIEW is written: unfinished pixels show the mean of their own samples.
//
//   ./examples/render_progressive --nee [--budget] out.ppm 256 256 16 [seed [samples_per_step [frame.f32]]]
//     light sampling: the handle is begun with vmx_progressive_begin_nee (VMX_SAMPLING_CORRECTED, fixed spp) and ends at
//     vmx_render_nee's frame.  With --budget it works as --adaptive does, but after the 8 uniform samples every step is one
//     vmx_progressive_step_budgeted: each pixel takes the number of samples its own error asks for, at most
//     samples_per_step (max_step), in one pass.  --nee --adaptive: vmx_progressive_step_adaptive on the light-sampled handle.
//
// Writes the last preview's rgba8 form as a binary PPM (Camera::saveFrame's quantisation, done on the device) and,
// if a third file name is given, the RGBAZ floats of the frame as they are.
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
    bool adaptive = false, nee = false, budget = false;
    for (int i = 1; i < argc; ++i) {
        const bool a = !std::strcmp(argv[i], "--adaptive"), n = !std::strcmp(argv[i], "--nee"), b = !std::strcmp(argv[i], "--budget");
        if (a || n || b) {
            adaptive = adaptive || a || b, nee = nee || n || b, budget = budget || b;  // (budgeted steps are light-sampled and adaptive)
            for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
            --argc, --i;
        }
    }
    const char *out = argc > 1 ? argv[1] : "cornell.ppm";
    const uint32_t W = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 256, H = argc > 3 ? (uint32_t)std::atoi(argv[3]) : 256;
    const uint32_t spp = argc > 4 ? (uint32_t)std::atoi(argv[4]) : 64;
    const uint64_t seed = argc > 5 ? std::strtoull(argv[5], nullptr, 10) : 1;
    const uint32_t per_step = argc > 6 ? (uint32_t)std::atoi(argv[6]) : 4;
    const char *raw = argc > 7 ? argv[7] : nullptr;

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

    vmx_scene *scene = nullptr;
    if (vmx_scene_create(pos.data(), nrm.data(), uv.data(), (uint32_t)(pos.size() / 9), nullptr, 0, 4, 0, &scene) != VMX_OK) {
        std::fprintf(stderr, "scene: %s\n", vmx_last_error());
        return 1;
    }
    vmx_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.position[0] = 0, cam.position[1] = 420, cam.position[2] = 1900;
    cam.back_distance = 6.0f;  // renderEngine.cpp:135
    cam.back_size[0] = 3.6f, cam.back_size[1] = 3.6f * (float)H / (float)W;
    cam.image_res[0] = W, cam.image_res[1] = H;
    cam.rays_per_pixel = adaptive ? 4 * spp : spp;  // (adaptive: the ceiling of a pixel's count; the mean ends at spp)
    vmx_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    opts.seed = seed;
    opts.early_stop = adaptive || nee ? 0 : 1;  // (selected steps need the fixed-spp schedule; light sampling has no other)
    opts.sampling = nee ? VMX_SAMPLING_CORRECTED : VMX_SAMPLING_PARITY;
    vmx_sampling_budget_params bprm;
    vmx_sampling_budget_default_params(&bprm);
    bprm.max_step = per_step;
    vmx_progressive *job = nullptr;
    const uint32_t flags = adaptive ? VMX_PROGRESSIVE_MOMENTS : 0u;
    if ((nee ? vmx_progressive_begin_nee(scene, &cam, &opts, flags, nullptr, &job)
             : vmx_progressive_begin_ex(scene, &cam, &opts, flags, nullptr, &job)) != VMX_OK) {
        std::fprintf(stderr, "begin: %s\n", vmx_last_error());
        vmx_scene_destroy(scene);
        return 1;
    }
    std::vector<float> frame((size_t)W * H * 5);
    std::vector<unsigned char> rgba((size_t)W * H * 4);
    vmx_progressive_info info;
    double ms = 0;
    int rc = vmx_progressive_info_get(job, &info);
    const uint64_t target = (uint64_t)spp * W * H;  // (adaptive: the samples of a uniform frame at the given spp)
    while (rc == VMX_OK && info.pixels_active > 0 && !(adaptive && info.samples >= target)) {
        vmx_stats st;
        if (adaptive && info.steps > 0) {
            uint32_t selected = 0;
            if ((rc = budget ? vmx_progressive_step_budgeted(job, &bprm, &st, &selected)
                             : vmx_progressive_step_adaptive(job, per_step, nullptr, &st, &selected)) != VMX_OK) break;
            if (selected == 0) {  // every pixel is below the threshold: more steps would select nothing either
                std::printf("converged: no pixel selected\n");
                break;
            }
            std::printf("selected %u pixels; ", selected);
        } else if ((rc = vmx_progressive_step(job, adaptive ? 8u : per_step, &st)) != VMX_OK) break;
        if ((rc = vmx_progressive_preview(job, frame.data(), rgba.data())) != VMX_OK) break;  // what a viewer would show
        if ((rc = vmx_progressive_info_get(job, &info)) != VMX_OK) break;
        ms += st.ms_device;
        std::printf("step %llu: pixels_active %u, samples %llu, %.2f ms device\n", (unsigned long long)info.steps,
                    info.pixels_active, (unsigned long long)info.samples, st.ms_device);
    }
    if (rc != VMX_OK) {
        std::fprintf(stderr, "progressive: %s\n", vmx_last_error());
        vmx_progressive_end(job);
        vmx_scene_destroy(scene);
        return 1;
    }
    vmx_progressive_end(job);
    vmx_scene_destroy(scene);
    FILE *f = std::fopen(out, "wb");
    if (!f) return 2;
    std::fprintf(f, "P6\n%u %u\n255\n", W, H);
    for (size_t p = 0; p < (size_t)W * H; ++p) std::fwrite(&rgba[p * 4], 1, 3, f);
    std::fclose(f);
    if (raw) {
        if (!(f = std::fopen(raw, "wb"))) return 2;
        std::fwrite(frame.data(), sizeof(float), frame.size(), f);
        std::fclose(f);
    }
    std::printf("frame %ux%u spp %u seed %llu: %llu steps of %u, %llu passes, samples %llu, %.2f ms device\n", W, H, spp,
                (unsigned long long)seed, (unsigned long long)info.steps, per_step, (unsigned long long)info.passes,
                (unsigned long long)info.samples, ms);
    return 0;
}
