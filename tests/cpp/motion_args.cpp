// motion_args.cpp — the argument checks of vmx_motion_device and vmx_temporal_accumulate_motion_device, which run on the
// host before any device call, driven from a stand-alone program so that the host sanitizers see them
// (tools/host_asan_args.sh builds the library with -Xarch_host -fsanitize=address,undefined and links this against it).
// Needs no GPU: every call here is refused, or has nothing to do, before the device is looked at.
#include <cstdint>
#include <cstdio>
#include <cstring>
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
    char *rec = p, *out = p + 64 * 8, *now = p + 4096, *prev = p + 4096 + 36, *nrm = p + 4096 + 72;
    const int inv = VMX_ERR_INVALID;
    expect(vmx_motion_device(nullptr, 8, now, prev, nrm, 1, out, 0, nullptr), inv, "rayhit", "NULL d_rayhit");
    expect(vmx_motion_device(rec, 8, nullptr, prev, nrm, 1, out, 0, nullptr), inv, "pos_now", "NULL d_pos_now");
    expect(vmx_motion_device(rec, 8, now, nullptr, nrm, 1, out, 0, nullptr), inv, "pos_prev", "NULL d_pos_prev");
    expect(vmx_motion_device(rec, 8, now, prev, nrm, 1, nullptr, 0, nullptr), inv, "out", "NULL d_out");
    expect(vmx_motion_device(rec, 8, now, prev, nrm, 0, out, 0, nullptr), inv, "ntris", "ntris must be non-zero");
    expect(vmx_motion_device(rec + 4, 8, now, prev, nrm, 1, out, 0, nullptr), inv, "rayhit alignment", "16-byte aligned");
    expect(vmx_motion_device(rec, 8, now, prev, nrm, 1, out + 8, 0, nullptr), inv, "out alignment", "16-byte aligned");
    expect(vmx_motion_device(rec, 8, now + 2, prev, nrm, 1, out, 0, nullptr), inv, "pos alignment", "4-byte aligned");
    expect(vmx_motion_device(rec, 8, now, prev, nrm + 1, 1, out, 0, nullptr), inv, "nrm alignment", "4-byte aligned");
    expect(vmx_motion_device(rec, 0x80000000u, now, prev, nrm, 1, out, 0, nullptr), inv, "n", "2^31 - 1");
    // the largest n and ntris there are: the overlap check's products must not wrap (pointers far apart still overlap)
    expect(vmx_motion_device(rec, 0x7fffffffu, now, prev, nrm, 0xffffffffu, out, 0, nullptr), inv, "huge", "d_out overlaps");
    expect(vmx_motion_device(rec, 8, now, prev, nrm, 1, rec, 0, nullptr), inv, "in place", "d_out overlaps");
    expect(vmx_motion_device(rec, 8, now, prev, nrm, 1, p + 4144, 0, nullptr), inv, "over pos_prev", "d_out overlaps");
    expect(vmx_motion_device(rec, 8, now, prev, nrm, 1, p + 4176, 0, nullptr), inv, "over nrm_prev", "d_out overlaps");
    expect(vmx_motion_device(rec, 0, now, prev, nullptr, 1, out, 0, nullptr), VMX_OK, "n == 0", nullptr);
    expect(vmx_motion_device(rec, 8, now, prev, nullptr, 1, out, 1 << 20, nullptr), VMX_ERR_NO_DEVICE, "device", nullptr);

    vmx_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.back_distance = 6.f, cam.back_size[0] = 3.6f, cam.back_size[1] = 2.4f;
    cam.image_res[0] = 8, cam.image_res[1] = 8, cam.rays_per_pixel = 16;
    vmx_temporal_params prm;
    expect(vmx_temporal_default_params(&prm), VMX_OK, "defaults", nullptr);
    for (void *mv : {(void *)nullptr, (void *)p}) {
        expect(vmx_temporal_accumulate_motion_device(nullptr, &cam, p, mv, p, p, nullptr, nullptr, &prm, nullptr), inv, "handle",
               "NULL handle");
        expect(vmx_temporal_accumulate_motion_device(nullptr, nullptr, p, mv, p, p, nullptr, nullptr, nullptr, nullptr), inv, "camera",
               "NULL camera");
        expect(vmx_temporal_accumulate_motion_device(nullptr, &cam, nullptr, mv, p, p, nullptr, nullptr, nullptr, nullptr), inv,
               "rayhit", "NULL d_rayhit");
        expect(vmx_temporal_accumulate_motion_device(nullptr, &cam, p, mv, p, nullptr, nullptr, nullptr, nullptr, nullptr), inv,
               "outputs", "no output");
    }
    expect(vmx_temporal_accumulate_motion_device(nullptr, &cam, p, p + 8, p, p, nullptr, nullptr, nullptr, nullptr), inv,
           "motion alignment", "d_motion must be 16-byte aligned");
    expect(vmx_temporal_accumulate_device(nullptr, &cam, p, p, p, nullptr, nullptr, nullptr, nullptr), inv, "old entry", "NULL handle");
    if (failures) return 1;
    std::printf("motion argument checks: clean\n");
    return 0;
}
