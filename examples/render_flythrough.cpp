// render_flythrough.cpp — N frames of a few samples along a camera path, each pushed through the preview chain on the
// device, through the C ABI only (include/vermilion_hip.h):
//   vmx_raycast_camera_device    the frame's G-buffer: sample 0's camera ray of every pixel
//   vmx_render_device            the frame at 4 spp (by default), a new seed per frame
//   vmx_temporal_accumulate_motion_device  the frames so far, reprojected into this camera, blended with the new one;
//                                with no motion records (NULL) it is vmx_temporal_accumulate_device
//   vmx_filter_set_guide_device + vmx_filter_apply_device  the a-trous filter on the accumulated frame -> rgba8
// (the G-buffer comes first in both modes, because --moving needs it before the motion records; the two calls write
// different buffers on one stream, so the order changes no result)
// Everything stays on one stream and in device memory; only the rgba8 form of the frames that are written comes back.
// The library has no allocator of its own: a host application brings its device buffers.  This one takes the few HIP
// runtime calls it needs from the runtime the library has loaded, so that it builds like the other examples; that
// leans on the library's own link to the runtime.  A real application includes <hip/hip_runtime_api.h> and links
// the HIP runtime itself.
//
//   g++ -std=c++17 -I include examples/render_flythrough.cpp vermilion_amd/libvermilion_hip.so
//       -Wl,-rpath,$PWD/vermilion_amd -o examples/render_flythrough     (done by __graft_entry__.build())
//   ./examples/render_flythrough [--moving] [--light] [--textured] [--variance] [--adaptive] [--upsample N/D] fly 256 256 [frames [spp [seed]]]
//
// Writes fly_raw.ppm (the last frame as rendered), fly_acc.ppm (accumulated) and fly_out.ppm (accumulated and filtered),
// and prints the mean history length of each frame.
//
// --moving: the block moves by (30, 0, 40) every frame as well, and each frame becomes
//   vmx_scene_update_device (refit)   the new positions, from a device buffer
//   vmx_raycast_camera_device         the G-buffer of the moved scene
//   vmx_motion_device                 where each pixel's surface point was before the update
//   vmx_render_device
//   vmx_temporal_accumulate_motion_device   the history looked up where the surface was: the block keeps its own
//   vmx_filter_set_guide_device + vmx_filter_apply_device
// A second accumulator takes the same frames without the motion records; the mean history length of both is printed.
//
// --light: from frame 8 on (so: with more than the default 8 frames) the lights change every frame — the small emitter
// moves by (3, 0, 2) a frame and the big one is dimmed to a quarter — and each such frame adds
//   vmx_scene_set_spheres             the new sphere table, in place: no rebuild, no upload of the scene
//   vmx_motion_spheres_device         after the G-buffer: where the pixels on the moved emitter were a frame before; it
//                                     writes over vmx_motion_device's records in place under --moving, else stands alone
// The records go wherever --moving's go, so it composes with --moving, --variance and --adaptive (whose history cut is
// what answers the dimmed light).
//
// --textured: a procedural checker is bound (vmx_scene_bind_texture), and the filter step becomes
//   vmx_albedo_camera_device             the frame's albedo plane: 4 samples of what the integrator multiplies by
//   vmx_filter_apply_demodulated_device  the filter on colour / albedo, the albedo multiplied back
// The accumulator is untouched: reprojection follows surface points, so textured history is valid.  fly_plain.ppm is
// the same accumulated frame through vmx_filter_apply_device, where the checker on the flat walls is averaged away.
//
// --variance: the accumulator is made with VMX_TEMPORAL_MOMENTS and the accumulate and filter steps become
//   vmx_temporal_accumulate_variance_device  the same accumulation, and the variance of every pixel's luminance
//   vmx_filter_apply_variance_device         the filter's colour stop measured in standard deviations of that pixel
// It composes with --moving (the motion records go to the variance call) and with --textured (the albedo plane goes to
// the variance-guided call, which then works on colour / albedo as the demodulated call does).  The mean variance of each
// frame is printed beside its history length.
//
// --adaptive: the accumulate step becomes
//   vmx_temporal_accumulate_adaptive_device  the same accumulation with the history cut where the lighting changed: the
//                                            moved block's shadow and bounce light under --moving
// on either kind of handle, so it composes with --moving (the motion records go to it) and --variance (it writes the
// variance too).  Beside each frame's mean history length the share of pixels whose change ratio r exceeds 1 is printed.
//
// --upsample N/D (1 <= N <= D <= 4 N): every frame is rendered at N/D of the size with (D/N)^2 times the samples, rounded
// down to a multiple of 4 — the same ray count — and accumulated and filtered at that low size; then
//   vmx_raycast_camera_device            a second G-buffer, of the full-size camera: one ray per pixel
//   vmx_upsample_set_guides_device + vmx_upsample_apply_device  the filtered low frame reconstructed at full size -> rgba8
// It composes with --moving, --textured and --variance, which then all work at the low size; fly_out.ppm is full size,
// fly_raw.ppm, fly_acc.ppm and fly_plain.ppm are the low size.
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
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

// the HIP runtime's entries, as hip_runtime_api.h declares them (hipError_t is an int-sized enum, 0 = hipSuccess;
// hipMemcpyDeviceToHost = 2)
struct Hip {
    int (*malloc_)(void **, size_t) = nullptr;
    int (*free_)(void *) = nullptr;
    int (*memcpy_)(void *, const void *, size_t, int) = nullptr;
    int (*stream_create)(void **) = nullptr;
    int (*stream_sync)(void *) = nullptr;
    int (*stream_destroy)(void *) = nullptr;
    int (*memcpy_async)(void *, const void *, size_t, int, void *) = nullptr;
    bool load() {
        malloc_ = (int (*)(void **, size_t))dlsym(RTLD_DEFAULT, "hipMalloc");
        free_ = (int (*)(void *))dlsym(RTLD_DEFAULT, "hipFree");
        memcpy_ = (int (*)(void *, const void *, size_t, int))dlsym(RTLD_DEFAULT, "hipMemcpy");
        stream_create = (int (*)(void **))dlsym(RTLD_DEFAULT, "hipStreamCreate");
        stream_sync = (int (*)(void *))dlsym(RTLD_DEFAULT, "hipStreamSynchronize");
        stream_destroy = (int (*)(void *))dlsym(RTLD_DEFAULT, "hipStreamDestroy");
        memcpy_async = (int (*)(void *, const void *, size_t, int, void *))dlsym(RTLD_DEFAULT, "hipMemcpyAsync");
        return malloc_ && free_ && memcpy_ && stream_create && stream_sync && stream_destroy && memcpy_async;
    }
};

bool write_ppm(const std::string &name, const std::vector<unsigned char> &rgba, uint32_t W, uint32_t H) {
    FILE *f = std::fopen(name.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "P6\n%u %u\n255\n", W, H);
    for (size_t p = 0; p < (size_t)W * H; ++p) std::fwrite(&rgba[p * 4], 1, 3, f);
    std::fclose(f);
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    bool moving = false, textured = false, variance = false, adaptive = false, light = false;
    uint32_t up_n = 0, up_d = 0;  // --upsample N/D
    for (; argc > 1 && std::strncmp(argv[1], "--", 2) == 0; --argc, ++argv) {
        if (std::strcmp(argv[1], "--moving") == 0) moving = true;
        else if (std::strcmp(argv[1], "--light") == 0) light = true;
        else if (std::strcmp(argv[1], "--textured") == 0) textured = true;
        else if (std::strcmp(argv[1], "--variance") == 0) variance = true;
        else if (std::strcmp(argv[1], "--adaptive") == 0) adaptive = true;
        else if (std::strcmp(argv[1], "--upsample") == 0 && argc > 2) {
            if (std::sscanf(argv[2], "%u/%u", &up_n, &up_d) != 2 || up_n < 1 || up_n > up_d || up_d > 4 * up_n) {
                std::fprintf(stderr, "flythrough: --upsample N/D needs 1 <= N <= D <= 4 N\n");
                return 1;
            }
            --argc, ++argv;
        }
        else {
            std::fprintf(stderr, "flythrough: unknown option %s\n", argv[1]);
            return 1;
        }
    }
    const std::string out = argc > 1 ? argv[1] : "fly";
    const uint32_t FW = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 256, FH = argc > 3 ? (uint32_t)std::atoi(argv[3]) : 256;
    const uint32_t frames = argc > 4 ? (uint32_t)std::atoi(argv[4]) : 8;
    const uint32_t full_spp = argc > 5 ? (uint32_t)std::atoi(argv[5]) : 4;
    // W x H and spp are what is rendered, accumulated and filtered: the low size under --upsample, else the full size FW x FH
    const bool upsample = up_n != 0;
    const uint32_t W = upsample ? (FW * up_n + up_d - 1) / up_d : FW, H = upsample ? (FH * up_n + up_d - 1) / up_d : FH;
    uint32_t spp = full_spp;
    if (upsample && full_spp * up_d * up_d / (up_n * up_n) >= 4) spp = full_spp * up_d * up_d / (up_n * up_n) / 4 * 4;
    if (upsample) std::printf("rendering %u x %u at %u spp for %u x %u at %u spp\n", W, H, spp, FW, FH, full_spp);
    const uint64_t seed = argc > 6 ? std::strtoull(argv[6], nullptr, 10) : 1;

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
    if (textured) {
        // 64 x 64 x 3: 8-texel checks in red and green, 4-texel stripes in blue
        std::vector<float> tex(64 * 64 * 3);
        for (uint32_t y = 0; y < 64; ++y)
            for (uint32_t x = 0; x < 64; ++x) {
                const float chk = (float)((x / 8 + y / 8) & 1u);
                float *t = &tex[(y * 64 + x) * 3];
                t[0] = 0.25f + 0.7f * chk, t[1] = 0.9f - 0.6f * chk, t[2] = 0.3f + 0.5f * (float)((x / 4) & 1u);
            }
        if (vmx_scene_bind_texture(scene, tex.data(), 64, 64, 3) != VMX_OK) {
            std::fprintf(stderr, "texture: %s\n", vmx_last_error());
            vmx_scene_destroy(scene);
            return 1;
        }
    }
    Hip hip;
    if (!hip.load()) {
        std::fprintf(stderr, "the HIP runtime's entries were not found\n");
        vmx_scene_destroy(scene);
        return 1;
    }
    const size_t npix = (size_t)W * H;
    vmx_temporal *temporal = nullptr;
    vmx_filter *filter = nullptr;
    void *stream = nullptr, *d_frame = nullptr, *d_rec = nullptr, *d_acc = nullptr, *d_rgba8 = nullptr, *d_hist = nullptr;
    // --moving: the positions of this frame and of the one before, the motion records, the other accumulator and its outputs
    const uint32_t ntris = (uint32_t)(pos.size() / 9);
    vmx_temporal *plain = nullptr;
    void *d_pos[2] = {nullptr, nullptr}, *d_motion = nullptr, *d_acc_plain = nullptr, *d_hist_plain = nullptr;
    void *d_albedo = nullptr;  // --textured: the frame's albedo plane, float4 per pixel
    void *d_var = nullptr;     // --variance: the variance of each pixel's luminance, one float per pixel
    void *d_change = nullptr;  // --adaptive: each pixel's change ratio r, one float per pixel
    // --upsample: the handle, the full-size G-buffer and the filtered low frame (RGBAZ: the upsampler's input)
    vmx_upsample *upsampler = nullptr;
    void *d_rec_full = nullptr, *d_filtered = nullptr;
    const size_t full_pix = (size_t)FW * FH;
    std::vector<float> var(variance ? (size_t)W * H : 0), change(adaptive ? (size_t)W * H : 0);
    std::vector<float> moved = pos, hist_plain(moving ? (size_t)W * H : 0);
    std::vector<unsigned char> rgba(full_pix * 4);
    std::vector<float> hist(npix);
    int rc = VMX_OK;
    bool io_ok = true;
    bool hip_ok = hip.stream_create(&stream) == 0 && hip.malloc_(&d_frame, npix * 20) == 0 && hip.malloc_(&d_rec, npix * 64) == 0 &&
                  hip.malloc_(&d_acc, npix * 20) == 0 && hip.malloc_(&d_rgba8, full_pix * 4) == 0 && hip.malloc_(&d_hist, npix * 4) == 0;
    if (hip_ok) rc = vmx_temporal_create_ex(0, W, H, variance ? VMX_TEMPORAL_MOMENTS : 0u, &temporal);
    if (hip_ok && rc == VMX_OK) rc = vmx_filter_create(0, W, H, &filter);
    if (upsample && hip_ok && rc == VMX_OK) {
        hip_ok = hip.malloc_(&d_rec_full, full_pix * 64) == 0 && hip.malloc_(&d_filtered, npix * 20) == 0;
        if (hip_ok) rc = vmx_upsample_create(0, W, H, FW, FH, &upsampler);
    }
    if (textured && hip_ok && rc == VMX_OK) hip_ok = hip.malloc_(&d_albedo, npix * 16) == 0;
    if (variance && hip_ok && rc == VMX_OK) hip_ok = hip.malloc_(&d_var, npix * 4) == 0;
    if (adaptive && hip_ok && rc == VMX_OK) hip_ok = hip.malloc_(&d_change, npix * 4) == 0;
    if ((moving || light) && hip_ok && rc == VMX_OK) hip_ok = hip.malloc_(&d_motion, npix * sizeof(vmx_motion)) == 0;
    // --light: the sphere table of this frame and of the one before
    std::vector<vmx_sphere> lights[2];
    if (light) {
        uint32_t count = 0;
        const vmx_sphere *def = vmx_default_spheres(&count);
        lights[0].assign(def, def + count), lights[1] = lights[0];
    }
    if (moving && hip_ok && rc == VMX_OK) {
        hip_ok = hip.malloc_(&d_pos[0], pos.size() * 4) == 0 && hip.malloc_(&d_pos[1], pos.size() * 4) == 0 &&
                 hip.malloc_(&d_acc_plain, npix * 20) == 0 &&
                 hip.malloc_(&d_hist_plain, npix * 4) == 0 && hip.memcpy_(d_pos[0], pos.data(), pos.size() * 4, 1) == 0;
        if (hip_ok) rc = vmx_temporal_create(0, W, H, &plain);
    }
    // rgba8 of a device frame of n pixels (vmx_quantize_device), or of d_rgba8 as it stands, on the host
    auto fetch = [&](const void *d_rgbaz, size_t n) {
        if (d_rgbaz && (rc = vmx_quantize_device(d_rgbaz, n, d_rgba8, nullptr, 0, stream)) != VMX_OK) return false;
        return (hip_ok = hip.stream_sync(stream) == 0 && hip.memcpy_(rgba.data(), d_rgba8, n * 4, 2) == 0);
    };
    // where the filter's result goes: straight to rgba8, or, under --upsample, to the RGBAZ frame the upsampler reads
    void *const f5 = upsample ? d_filtered : nullptr, *const f4 = upsample ? nullptr : d_rgba8;
    for (uint32_t i = 0; hip_ok && rc == VMX_OK && i < frames; ++i) {
        vmx_camera cam;
        std::memset(&cam, 0, sizeof(cam));
        cam.position[0] = 6.0f * (float)i, cam.position[1] = 420, cam.position[2] = 1900;  // a slow pan to the right ...
        cam.rotation_deg[1] = 0.15f * (float)i;                                             // ... while turning
        cam.back_distance = 6.0f;  // renderEngine.cpp:135
        cam.back_size[0] = 3.6f, cam.back_size[1] = 3.6f * (float)FH / (float)FW;
        cam.image_res[0] = W, cam.image_res[1] = H;
        cam.rays_per_pixel = spp;
        vmx_opts opts;
        std::memset(&opts, 0, sizeof(opts));
        opts.seed = seed + i;
        opts.sampling = VMX_SAMPLING_CORRECTED;
        vmx_stats st;
        const bool update = moving && i > 0;  // (frame 0 shows the scene as it was made: d_pos[0])
        if (update) {
            // the block (triangles 4..7) by (30, 0, 40) per frame: a translation, so the previous normals are not needed
            for (uint32_t t = 4; t < 8; ++t)
                for (uint32_t v = 0; v < 3; ++v)
                    moved[t * 9 + v * 3] = pos[t * 9 + v * 3] + 30.f * (float)i, moved[t * 9 + v * 3 + 2] = pos[t * 9 + v * 3 + 2] + 40.f * (float)i;
            // (hipMemcpyHostToDevice = 1; d_pos[i & 1] was last read two frames ago, on this stream)
            if (!(hip_ok = hip.memcpy_async(d_pos[i & 1], moved.data(), moved.size() * 4, 1, stream) == 0 && hip.stream_sync(stream) == 0))
                break;
            if ((rc = vmx_scene_update_device(scene, d_pos[i & 1], nullptr, nullptr, ntris, VMX_UPDATE_REFIT, stream)) != VMX_OK) break;
        }
        const bool relit = light && i >= 8;
        if (relit) {
            // sphere 0 is the small emitter, sphere 1 the big one (vmx_default_spheres)
            std::vector<vmx_sphere> &now = lights[i & 1];
            now = lights[0], now[0] = vmx_default_spheres(nullptr)[0], now[1] = vmx_default_spheres(nullptr)[1];
            now[0].centre[0] += 3.f * (float)(i - 7), now[0].centre[2] += 2.f * (float)(i - 7);
            for (float &c : now[1].colour) c *= 0.25f;
            if ((rc = vmx_scene_set_spheres(scene, now.data(), (uint32_t)now.size())) != VMX_OK) break;
        }
        if ((rc = vmx_raycast_camera_device(scene, &cam, &opts, 0, d_rec, 0, stream)) != VMX_OK) break;
        if (update && (rc = vmx_motion_device(d_rec, (uint32_t)npix, d_pos[i & 1], d_pos[(i & 1) ^ 1], nullptr, ntris, d_motion, 0,
                                              stream)) != VMX_OK)
            break;
        if (relit && (rc = vmx_motion_spheres_device(d_rec, (uint32_t)npix, cam.position, lights[i & 1].data(),
                                                     lights[(i & 1) ^ 1].data(), (uint32_t)lights[0].size(),
                                                     update ? d_motion : nullptr, d_motion, stream)) != VMX_OK)
            break;
        const void *motion = update || relit ? d_motion : nullptr;
        if ((rc = vmx_render_device(scene, &cam, &opts, d_frame, stream, &st)) != VMX_OK) break;
        if (adaptive) {  // (d_var is NULL without --variance, as a handle without moments wants it)
            if ((rc = vmx_temporal_accumulate_adaptive_device(temporal, &cam, d_rec, motion, d_frame, d_acc,
                                                              nullptr, d_hist, d_var, d_change, nullptr, nullptr, nullptr,
                                                              stream)) != VMX_OK)
                break;
        } else if (variance) {
            if ((rc = vmx_temporal_accumulate_variance_device(temporal, &cam, d_rec, motion, d_frame, d_acc,
                                                              nullptr, d_hist, d_var, nullptr, nullptr, stream)) != VMX_OK)
                break;
        } else if ((rc = vmx_temporal_accumulate_motion_device(temporal, &cam, d_rec, motion, d_frame, d_acc,
                                                               nullptr, d_hist, nullptr, stream)) != VMX_OK)
            break;
        if (moving && (rc = vmx_temporal_accumulate_device(plain, &cam, d_rec, d_frame, d_acc_plain, nullptr, d_hist_plain, nullptr,
                                                           stream)) != VMX_OK)
            break;
        if ((rc = vmx_filter_set_guide_device(filter, d_rec, stream)) != VMX_OK) break;
        if (textured) {
            const uint32_t albedo_samples = spp < 8 ? 4 * (spp / 4) : 4;  // (at most the frame's own samples)
            if ((rc = vmx_albedo_camera_device(scene, &cam, &opts, 0, albedo_samples, d_albedo, stream)) != VMX_OK) break;
            if (i + 1 == frames) {  // the plain filter's picture of the same frame, for comparison
                if ((rc = vmx_filter_apply_device(filter, d_acc, nullptr, d_rgba8, nullptr, stream)) != VMX_OK) break;
                if (fetch(nullptr, npix) && !write_ppm(out + "_plain.ppm", rgba, W, H)) {
                    std::fprintf(stderr, "flythrough: cannot write %s_plain.ppm\n", out.c_str());
                    io_ok = false;
                }
                if (!hip_ok) break;
            }
            if (variance) {
                if ((rc = vmx_filter_apply_variance_device(filter, d_acc, d_var, d_albedo, f5, f4, nullptr,
                                                           VMX_SIGMA_LUMINANCE_DEFAULT, stream)) != VMX_OK)
                    break;
            } else if ((rc = vmx_filter_apply_demodulated_device(filter, d_acc, d_albedo, f5, f4, nullptr, stream)) != VMX_OK)
                break;
        } else if (variance) {
            if ((rc = vmx_filter_apply_variance_device(filter, d_acc, d_var, nullptr, f5, f4, nullptr,
                                                       VMX_SIGMA_LUMINANCE_DEFAULT, stream)) != VMX_OK)
                break;
        } else if ((rc = vmx_filter_apply_device(filter, d_acc, f5, f4, nullptr, stream)) != VMX_OK)
            break;
        if (upsample) {
            vmx_camera full = cam;  // the same field on FW x FH pixels; a G-buffer is one camera ray per pixel
            full.image_res[0] = FW, full.image_res[1] = FH;
            full.rays_per_pixel = full_spp;
            if ((rc = vmx_raycast_camera_device(scene, &full, &opts, 0, d_rec_full, 0, stream)) != VMX_OK) break;
            if ((rc = vmx_upsample_set_guides_device(upsampler, d_rec, d_rec_full, stream)) != VMX_OK) break;
            if ((rc = vmx_upsample_apply_device(upsampler, d_filtered, nullptr, d_rgba8, nullptr, stream)) != VMX_OK) break;
        }
        if (!(hip_ok = hip.stream_sync(stream) == 0 && hip.memcpy_(hist.data(), d_hist, npix * 4, 2) == 0)) break;
        double mean = 0;
        for (float n : hist) mean += n;
        if (variance) {
            if (!(hip_ok = hip.memcpy_(var.data(), d_var, npix * 4, 2) == 0)) break;
            double mean_var = 0;
            for (float v : var) mean_var += v;
            std::printf("frame %u: mean luminance variance %.6f\n", i, mean_var / (double)npix);
        }
        if (adaptive) {
            if (!(hip_ok = hip.memcpy_(change.data(), d_change, npix * 4, 2) == 0)) break;
            size_t cut = 0;
            for (float r : change) cut += r > 1.f;
            std::printf("frame %u: adaptive, r > 1 in %.2f %% of the pixels\n", i, 100.0 * (double)cut / (double)npix);
        }
        if (moving) {
            if (!(hip_ok = hip.memcpy_(hist_plain.data(), d_hist_plain, npix * 4, 2) == 0)) break;
            double mean_plain = 0;
            for (float n : hist_plain) mean_plain += n;
            std::printf("frame %u: block at +%.0f x +%.0f z, camera x %.0f, %.2f ms device, mean history %.2f frames with motion "
                        "records, %.2f without\n", i, 30.0 * i, 40.0 * i, cam.position[0], st.ms_device, mean / (double)npix,
                        mean_plain / (double)npix);
        } else
            std::printf("frame %u: camera x %.0f, y-rotation %.2f deg, %.2f ms device, mean history %.2f frames\n", i,
                        cam.position[0], cam.rotation_deg[1], st.ms_device, mean / (double)npix);
        if (i + 1 == frames) {
            // (the filtered and, under --upsample, reconstructed frame is full size; the other two are the rendered size)
            const std::pair<const char *, const void *> files[3] = {{"_out.ppm", nullptr}, {"_acc.ppm", d_acc}, {"_raw.ppm", d_frame}};
            for (const auto &f : files)
                if (fetch(f.second, f.second ? npix : full_pix) && !write_ppm(out + f.first, rgba, f.second ? W : FW, f.second ? H : FH)) {
                    std::fprintf(stderr, "flythrough: cannot write %s%s\n", out.c_str(), f.first);
                    io_ok = false;
                }
        }
    }
    if (rc != VMX_OK) std::fprintf(stderr, "flythrough: %s\n", vmx_last_error());
    if (!hip_ok) std::fprintf(stderr, "flythrough: a HIP runtime call failed\n");
    if (stream) hip.stream_sync(stream);
    if (upsampler) vmx_upsample_destroy(upsampler);
    if (filter) vmx_filter_destroy(filter);
    if (temporal) vmx_temporal_destroy(temporal);
    if (plain) vmx_temporal_destroy(plain);
    for (void *p : {d_frame, d_rec, d_acc, d_rgba8, d_hist, d_pos[0], d_pos[1], d_motion, d_acc_plain, d_hist_plain, d_albedo, d_var, d_change, d_rec_full, d_filtered})
        if (p) hip.free_(p);
    if (stream) hip.stream_destroy(stream);
    vmx_scene_destroy(scene);
    return rc != VMX_OK || !hip_ok ? 1 : io_ok ? 0 : 2;
}
