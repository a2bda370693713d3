// adaptive_args.cpp — the argument checks of vmx_adaptive_default_params and vmx_temporal_accumulate_adaptive_device, which
// run on the host before any device call, driven from a stand-alone program so that the host sanitizers see them (in the
// pattern of variance_args.cpp: build the library with -Xarch_host -fsanitize=address,undefined and link this against it).
// Needs no GPU: every call here is refused before the device is looked at.
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
    vmx_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.back_distance = 6.f, cam.back_size[0] = 3.6f, cam.back_size[1] = 2.4f;
    cam.image_res[0] = 8, cam.image_res[1] = 8, cam.rays_per_pixel = 16;
    vmx_adaptive_params ap;
    expect(vmx_adaptive_default_params(&ap), VMX_OK, "defaults", nullptr);
    expect(vmx_adaptive_default_params(nullptr), inv, "defaults", "NULL out");
    if (sizeof(ap) != 32 || ap.gamma != 3.f || ap.min_support != 4.f || ap.normal_squarings != 5 || ap.sigma_depth != 0.1f) {
        std::fprintf(stderr, "FAIL vmx_adaptive_params defaults\n");
        ++failures;
    }
    vmx_variance_params vp;
    expect(vmx_variance_default_params(&vp), VMX_OK, "variance defaults", nullptr);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    auto call = [&](const vmx_camera *c, void *rayhit, void *mv, void *in, void *out, void *var, void *chg,
                    const vmx_variance_params *v, const vmx_adaptive_params *a) {
        return vmx_temporal_accumulate_adaptive_device(nullptr, c, rayhit, mv, in, out, nullptr, nullptr, var, chg, nullptr, v, a, nullptr);
    };
    for (void *mv : {(void *)nullptr, (void *)p}) {
        for (void *var : {(void *)nullptr, (void *)p}) {
            expect(call(&cam, p, mv, p, p, var, p, &vp, &ap), inv, "handle", "NULL handle");
            expect(call(&cam, p, mv, p, p, var, nullptr, nullptr, nullptr), inv, "handle", "NULL handle");
            expect(call(nullptr, p, mv, p, p, var, p, nullptr, nullptr), inv, "camera", "NULL camera");
            expect(call(&cam, nullptr, mv, p, p, var, p, nullptr, nullptr), inv, "rayhit", "NULL d_rayhit");
            expect(call(&cam, p, mv, nullptr, p, var, p, nullptr, nullptr), inv, "in", "NULL d_in_rgbaz");
            expect(call(&cam, p, mv, p, p, var, p + 2, nullptr, nullptr), inv, "change alignment", "d_change must be 4-byte aligned");
        }
        expect(call(&cam, p, mv, p, nullptr, p, nullptr, nullptr, nullptr), inv, "the variance is an output", "NULL handle");
        expect(call(&cam, p, mv, p, nullptr, nullptr, p, nullptr, nullptr), inv, "the change plane is none", "no output");
        expect(call(&cam, p, mv, p, p, p + 1, p + 1, nullptr, nullptr), inv, "variance alignment first", "d_variance must be 4-byte aligned");
    }
    for (float g : {nan, inf, 0.f, -3.f}) {
        vmx_adaptive_params bad = ap;
        bad.gamma = g;
        expect(call(&cam, p, nullptr, p, p, nullptr, nullptr, nullptr, &bad), inv, "gamma", "gamma");
    }
    for (float ms : {nan, inf, 0.5f, -1.f}) {
        vmx_adaptive_params bad = ap;
        bad.min_support = ms;
        expect(call(&cam, p, nullptr, p, p, nullptr, nullptr, nullptr, &bad), inv, "min_support", "min_support");
    }
    for (float sd : {nan, inf, 0.f, -0.1f}) {
        vmx_adaptive_params bad = ap;
        bad.sigma_depth = sd;
        expect(call(&cam, p, nullptr, p, p, nullptr, nullptr, nullptr, &bad), inv, "sigma_depth", "sigma_depth");
    }
    {
        vmx_adaptive_params bad = ap;
        bad.normal_squarings = 9;
        expect(call(&cam, p, nullptr, p, p, nullptr, nullptr, nullptr, &bad), inv, "normal_squarings", "normal_squarings");
        bad = ap;
        bad.reserved[3] = 1;
        expect(call(&cam, p, nullptr, p, p, nullptr, nullptr, nullptr, &bad), inv, "reserved", "vmx_adaptive_params: reserved");
        // the variance parameters come before the adaptive ones
        vmx_variance_params vbad = vp;
        vbad.min_history = 0.5f;
        bad = ap;
        bad.gamma = 0.f;
        expect(call(&cam, p, nullptr, p, p, nullptr, nullptr, &vbad, &bad), inv, "order", "vmx_variance_params");
        bad = ap;
        bad.gamma = 3e38f;  // (gamma*gamma overflows to +inf: the call that cuts nothing)
        expect(call(&cam, p, nullptr, p, p, nullptr, nullptr, nullptr, &bad), inv, "huge gamma", "NULL handle");
    }
    if (failures) return 1;
    std::printf("adaptive argument checks: clean\n");
    return 0;
}
