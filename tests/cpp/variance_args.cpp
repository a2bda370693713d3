// variance_args.cpp — the argument checks of vmx_temporal_create_ex, vmx_temporal_accumulate_variance_device and
// vmx_filter_apply_variance_device, which run on the host before any device call, driven from a stand-alone program so that
// the host sanitizers see them (in the pattern of motion_args.cpp: build the library with -Xarch_host
// -fsanitize=address,undefined and link this against it).  Needs no GPU: every call here is refused before the device is
// looked at.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "vermilion_hip.h"

static int failures = 0;

static void expect(int rc, int want, const char *what, const char *text) {
    const char *err = vmx_last_error();
    if (rc != want || (text && !std::strstr(err, text))) {
        std::fprintf(stderr, "FAIL %s: rc %d (want %d), error \"%s\" (want \"%s\")\n", what, rc, want, err, text ? text : "");
        ++failures;
    }
}

int main() {
    std::vector<float> buf(8192);
    char *p = (char *)(((uintptr_t)buf.data() + 15) & ~(uintptr_t)15);
    const int inv = VMX_ERR_INVALID;
    vmx_temporal *t = nullptr;
    expect(vmx_temporal_create_ex(0, 8, 8, 2u, &t), inv, "flags", "unknown flags");
    expect(vmx_temporal_create_ex(0, 8, 8, VMX_TEMPORAL_MOMENTS | 0x80000000u, &t), inv, "flags", "unknown flags");
    expect(vmx_temporal_create_ex(0, 0, 8, VMX_TEMPORAL_MOMENTS, &t), inv, "size", "resolution must be non-zero");
    expect(vmx_temporal_create_ex(0, 8, 8, VMX_TEMPORAL_MOMENTS, nullptr), inv, "out", "NULL out");
    expect(vmx_temporal_create_ex(1 << 20, 8, 8, VMX_TEMPORAL_MOMENTS, &t), VMX_ERR_NO_DEVICE, "device", nullptr);

    vmx_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.back_distance = 6.f, cam.back_size[0] = 3.6f, cam.back_size[1] = 2.4f;
    cam.image_res[0] = 8, cam.image_res[1] = 8, cam.rays_per_pixel = 16;
    vmx_variance_params vp;
    expect(vmx_variance_default_params(&vp), VMX_OK, "defaults", nullptr);
    expect(vmx_variance_default_params(nullptr), inv, "defaults", "NULL out");
    if (sizeof(vp) != 32 || vp.min_history != 4.f || vp.normal_squarings != 5 || vp.sigma_depth != 0.1f) {
        std::fprintf(stderr, "FAIL vmx_variance_params defaults\n");
        ++failures;
    }
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (void *mv : {(void *)nullptr, (void *)p}) {
        expect(vmx_temporal_accumulate_variance_device(nullptr, &cam, p, mv, p, p, nullptr, nullptr, p, nullptr, &vp, nullptr), inv,
               "handle", "NULL handle");
        expect(vmx_temporal_accumulate_variance_device(nullptr, &cam, p, mv, p, nullptr, nullptr, nullptr, p, nullptr, nullptr, nullptr),
               inv, "the variance is an output", "NULL handle");
        expect(vmx_temporal_accumulate_variance_device(nullptr, &cam, p, mv, p, p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
               inv, "variance", "NULL d_variance");
        expect(vmx_temporal_accumulate_variance_device(nullptr, &cam, p, mv, p, p, nullptr, nullptr, p + 2, nullptr, nullptr, nullptr),
               inv, "variance alignment", "d_variance must be 4-byte aligned");
        expect(vmx_temporal_accumulate_variance_device(nullptr, nullptr, p, mv, p, p, nullptr, nullptr, p, nullptr, nullptr, nullptr), inv,
               "camera", "NULL camera");
    }
    for (float mh : {nan, inf, 0.5f, -1.f}) {
        vmx_variance_params bad = vp;
        bad.min_history = mh;
        expect(vmx_temporal_accumulate_variance_device(nullptr, &cam, p, nullptr, p, p, nullptr, nullptr, p, nullptr, &bad, nullptr), inv,
               "min_history", "min_history");
    }
    for (float sd : {nan, inf, 0.f, -0.1f}) {
        vmx_variance_params bad = vp;
        bad.sigma_depth = sd;
        expect(vmx_temporal_accumulate_variance_device(nullptr, &cam, p, nullptr, p, p, nullptr, nullptr, p, nullptr, &bad, nullptr), inv,
               "sigma_depth", "sigma_depth");
    }
    {
        vmx_variance_params bad = vp;
        bad.normal_squarings = 9;
        expect(vmx_temporal_accumulate_variance_device(nullptr, &cam, p, nullptr, p, p, nullptr, nullptr, p, nullptr, &bad, nullptr), inv,
               "normal_squarings", "normal_squarings");
        bad = vp;
        bad.reserved[4] = 1;
        expect(vmx_temporal_accumulate_variance_device(nullptr, &cam, p, nullptr, p, p, nullptr, nullptr, p, nullptr, &bad, nullptr), inv,
               "reserved", "reserved");
    }
    for (void *alb : {(void *)nullptr, (void *)p}) {
        expect(vmx_filter_apply_variance_device(nullptr, p, p, alb, p, nullptr, nullptr, 4.f, nullptr), inv, "handle", "NULL handle");
        for (float sl : {nan, inf, 0.f, -4.f})
            expect(vmx_filter_apply_variance_device(nullptr, p, p, alb, p, nullptr, nullptr, sl, nullptr), inv, "sigma_luminance",
                   "sigma_luminance must be finite and > 0");
        expect(vmx_filter_apply_variance_device(nullptr, nullptr, p, alb, p, nullptr, nullptr, 4.f, nullptr), inv, "in", "NULL d_in_rgbaz");
        expect(vmx_filter_apply_variance_device(nullptr, p, nullptr, alb, p, nullptr, nullptr, 4.f, nullptr), inv, "variance",
               "NULL d_variance");
        expect(vmx_filter_apply_variance_device(nullptr, p, p, alb, nullptr, nullptr, nullptr, 4.f, nullptr), inv, "outputs", "no output");
        expect(vmx_filter_apply_variance_device(nullptr, p, p + 1, alb, p, nullptr, nullptr, 4.f, nullptr), inv, "variance alignment",
               "d_variance must be 4-byte aligned");
    }
    expect(vmx_filter_apply_variance_device(nullptr, p, p, p + 4, p, nullptr, nullptr, 4.f, nullptr), inv, "albedo alignment",
           "d_albedo must be 16-byte aligned");
    if (failures) return 1;
    std::printf("variance argument checks: clean\n");
    return 0;
}
