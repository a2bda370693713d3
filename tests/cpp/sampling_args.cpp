// sampling_args.cpp — the argument checks of the adaptive sampling entries (vmx_progressive_begin_ex, _state_device,
// _step_selected_device, _error_device, _select_device, _step_adaptive, vmx_sampling_default_params) that run on the host
// before any device call, driven from a stand-alone program so that the host sanitizers see them (in the pattern of
// adaptive_args.cpp: build the library with -Xarch_host -fsanitize=address,undefined and link this against it).
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
    std::vector<float> buf(256);
    char *p = (char *)(((uintptr_t)buf.data() + 15) & ~(uintptr_t)15);
    const int inv = VMX_ERR_INVALID;
    vmx_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.back_distance = 6.f, cam.back_size[0] = 3.6f, cam.back_size[1] = 2.4f;
    cam.image_res[0] = 8, cam.image_res[1] = 8, cam.rays_per_pixel = 16;
    vmx_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    vmx_sampling_params sp;
    expect(vmx_sampling_default_params(&sp), VMX_OK, "defaults", nullptr);
    expect(vmx_sampling_default_params(nullptr), inv, "defaults", "NULL out");
    if (sizeof(sp) != 32 || !(sp.threshold >= 0.25f && sp.threshold <= 2.f) || !(sp.floor >= 0.01f && sp.floor <= 0.2f) ||
        sp.min_samples != 8 || sp.radius != 1 || sp.reserved[0] || sp.reserved[1] || sp.reserved[2] || sp.reserved[3]) {
        std::fprintf(stderr, "FAIL vmx_sampling_params defaults\n");
        ++failures;
    }
    static_assert(VMX_PROGRESSIVE_MOMENTS == 1u, "the flag's value");

    // begin_ex: pointers, then the flags, then the frame, the scene last
    vmx_progressive *h = nullptr;
    for (uint32_t flags : {2u, 3u, 0x80000000u}) expect(vmx_progressive_begin_ex(nullptr, &cam, &opts, flags, nullptr, &h), inv, "flags", "unknown flag");
    for (uint32_t flags : {0u, VMX_PROGRESSIVE_MOMENTS}) {
        expect(vmx_progressive_begin_ex(nullptr, nullptr, &opts, flags, nullptr, &h), inv, "cam", "NULL argument");
        expect(vmx_progressive_begin_ex(nullptr, &cam, nullptr, flags, nullptr, &h), inv, "opts", "NULL argument");
        expect(vmx_progressive_begin_ex(nullptr, &cam, &opts, flags, nullptr, nullptr), inv, "out", "NULL out");
        expect(vmx_progressive_begin_ex(nullptr, &cam, &opts, flags, nullptr, &h), inv, "scene", "NULL scene");
        vmx_camera bad = cam;
        bad.rays_per_pixel = 3;
        expect(vmx_progressive_begin_ex(nullptr, &bad, &opts, flags, nullptr, &h), inv, "frame", "rays_per_pixel < 4");
    }

    expect(vmx_progressive_state_device(nullptr, nullptr, nullptr), inv, "state outputs", "no output");
    expect(vmx_progressive_state_device(nullptr, p, p + 16), inv, "state handle", "NULL handle");
    expect(vmx_progressive_state_device(nullptr, p, nullptr), inv, "state handle", "NULL handle");
    expect(vmx_progressive_state_device(nullptr, nullptr, p), inv, "state handle", "NULL handle");
    for (int off : {1, 2, 3}) {
        expect(vmx_progressive_state_device(nullptr, p + off, nullptr), inv, "sums alignment", "4-byte aligned");
        expect(vmx_progressive_state_device(nullptr, p, p + 16 + off), inv, "counts alignment", "4-byte aligned");
    }
    expect(vmx_progressive_state_device(nullptr, p, p), inv, "state overlap", "d_sums and d_counts overlap");
    expect(vmx_progressive_state_device(nullptr, p, p + 12), inv, "state overlap", "d_sums and d_counts overlap");

    expect(vmx_progressive_step_selected_device(nullptr, 4, nullptr, nullptr, nullptr), inv, "select map", "NULL d_select");
    expect(vmx_progressive_step_selected_device(nullptr, 4, p + 1, nullptr, nullptr), inv, "step handle", "NULL handle");

    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    auto all_three = [&](const vmx_sampling_params *prm, const char *what, const char *text) {
        expect(vmx_progressive_error_device(nullptr, prm, p, nullptr), inv, what, text);
        expect(vmx_progressive_select_device(nullptr, prm, p, nullptr), inv, what, text);
        expect(vmx_progressive_step_adaptive(nullptr, 4, prm, nullptr, nullptr), inv, what, text);
    };
    all_three(nullptr, "handle", "NULL handle");
    all_three(&sp, "handle", "NULL handle");
    for (float t : {nan, inf, -inf, -0.5f}) {
        vmx_sampling_params bad = sp;
        bad.threshold = t;
        all_three(&bad, "threshold", "threshold");
    }
    for (float f : {nan, inf, 0.f, -0.1f}) {
        vmx_sampling_params bad = sp;
        bad.floor = f;
        all_three(&bad, "floor", "floor");
    }
    for (uint32_t m : {0u, 1u}) {
        vmx_sampling_params bad = sp;
        bad.min_samples = m;
        all_three(&bad, "min_samples", "min_samples");
    }
    for (uint32_t r : {4u, 0xFFFFFFFFu}) {
        vmx_sampling_params bad = sp;
        bad.radius = r;
        all_three(&bad, "radius", "radius");
    }
    for (int i = 0; i < 4; ++i) {
        vmx_sampling_params bad = sp;
        bad.reserved[i] = 1;
        all_three(&bad, "reserved", "vmx_sampling_params: reserved");
    }
    {
        // the edges of the ranges are accepted: the call goes on to the handle
        vmx_sampling_params edge = sp;
        edge.threshold = 0.f, edge.min_samples = 2, edge.radius = 0;
        all_three(&edge, "edges", "NULL handle");
        edge.radius = 3, edge.min_samples = 0xFFFFFFFFu;
        all_three(&edge, "edges", "NULL handle");
        // the parameters come before the pointers
        vmx_sampling_params bad = sp;
        bad.floor = 0.f;
        expect(vmx_progressive_error_device(nullptr, &bad, nullptr, nullptr), inv, "order", "vmx_sampling_params");
        expect(vmx_progressive_select_device(nullptr, &bad, nullptr, nullptr), inv, "order", "vmx_sampling_params");
    }
    expect(vmx_progressive_error_device(nullptr, nullptr, nullptr, nullptr), inv, "error outputs", "no output");
    expect(vmx_progressive_error_device(nullptr, nullptr, nullptr, p), inv, "error handle", "NULL handle");
    expect(vmx_progressive_error_device(nullptr, nullptr, p, p + 4), inv, "error handle", "NULL handle");
    for (int off : {1, 2, 3}) {
        expect(vmx_progressive_error_device(nullptr, nullptr, p + off, nullptr), inv, "error alignment", "4-byte aligned");
        expect(vmx_progressive_error_device(nullptr, nullptr, p, p + 64 + off), inv, "variance alignment", "4-byte aligned");
    }
    expect(vmx_progressive_error_device(nullptr, nullptr, p, p), inv, "error overlap", "d_error and d_variance overlap");
    expect(vmx_progressive_select_device(nullptr, nullptr, nullptr, p), inv, "select map", "NULL d_select");
    for (int off : {1, 2, 3}) {
        expect(vmx_progressive_select_device(nullptr, nullptr, p + off, nullptr), inv, "a byte map needs no alignment", "NULL handle");
        expect(vmx_progressive_select_device(nullptr, nullptr, p, p + 64 + off), inv, "count alignment", "d_count must be 4-byte aligned");
    }
    expect(vmx_progressive_select_device(nullptr, nullptr, p + 6, p + 4), inv, "select overlap", "d_select and d_count overlap");
    expect(vmx_progressive_select_device(nullptr, nullptr, p + 8, p + 4), inv, "select handle", "NULL handle");
    if (failures) return 1;
    std::printf("sampling argument checks: clean\n");
    return 0;
}
