// api_image.inc — part of vmx_api.cpp: the argument checks the image-space entries share (vmx_filter_*, vmx_upsample_*,
// vmx_temporal_*, vmx_motion_device, the filtered previews).  Each entry keeps its own list of checks, in the order its
// header documents; what a check is made of is here.

// ---- handles ------------------------------------------------------------------------------------------------------------
// `device` exists; it becomes the current device
static int device_checks(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(VMX_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(VMX_ERR_NO_DEVICE, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    return VMX_OK;
}

// what every vmx_*_create of a handle for width x height images checks before it allocates (the size bound is
// make_frame's: the kernels index pixels, and five floats per pixel, in 32 bits)
static int image_handle_checks(int device, uint32_t width, uint32_t height) {
    if (width == 0 || height == 0) return fail(VMX_ERR_INVALID, "image resolution must be non-zero");
    if ((uint64_t)width * height > 0x7fffffffull / 8) return fail(VMX_ERR_INVALID, "image too large");
    return device_checks(device);
}

// ---- buffers that may not overlap -----------------------------------------------------------------------------------------
struct Span {
    const void *p;
    size_t bytes;
};

// a NULL pointer (an output or input the call does without) meets nothing
static bool spans_meet(const Span &a, const Span &b) {
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    return x && y && x < y + b.bytes && y < x + a.bytes;
}

static bool meets_any(const Span &a, std::initializer_list<Span> others) {
    for (const Span &b : others)
        if (spans_meet(a, b)) return true;
    return false;
}

// ---- vmx_*_params ---------------------------------------------------------------------------------------------------------
static bool finite_positive(float x) { return std::isfinite(x) && x > 0.f; }
static bool squarings_ok(uint32_t normal_squarings) { return normal_squarings <= 8; }
template <size_t N>
static bool reserved_zero(const uint32_t (&words)[N]) {
    return std::all_of(words, words + N, [](uint32_t r) { return r == 0; });
}

// vmx_*_default_params
template <typename P>
static int default_params(P *out, const P &defaults) {
    if (!out) return fail(VMX_ERR_INVALID, "NULL out");
    *out = defaults;
    return VMX_OK;
}

static const vmx_variance_params kVarianceDefaults = {4.f, 5u, 0.1f, {0u, 0u, 0u, 0u, 0u}};

// NULL selects the defaults; anything out of range is refused before any launch (as filter_params, temporal_params and
// upsample_params next to their entries)
static int variance_params(const vmx_variance_params *in, vmx_variance_params &out) {
    out = in ? *in : kVarianceDefaults;
    if (!(std::isfinite(out.min_history) && out.min_history >= 1.f))
        return fail(VMX_ERR_INVALID, "vmx_variance_params: min_history must be finite and >= 1");
    if (!squarings_ok(out.normal_squarings)) return fail(VMX_ERR_INVALID, "vmx_variance_params: normal_squarings must be 0..8");
    if (!finite_positive(out.sigma_depth)) return fail(VMX_ERR_INVALID, "vmx_variance_params: sigma_depth must be finite and > 0");
    if (!reserved_zero(out.reserved)) return fail(VMX_ERR_INVALID, "vmx_variance_params: reserved words must be 0");
    return VMX_OK;
}

extern "C" int vmx_variance_default_params(vmx_variance_params *out) { return default_params(out, kVarianceDefaults); }

static const vmx_adaptive_params kAdaptiveDefaults = {3.f, 4.f, 5u, 0.1f, {0u, 0u, 0u, 0u}};

static int adaptive_params(const vmx_adaptive_params *in, vmx_adaptive_params &out) {
    out = in ? *in : kAdaptiveDefaults;
    if (!finite_positive(out.gamma)) return fail(VMX_ERR_INVALID, "vmx_adaptive_params: gamma must be finite and > 0");
    if (!(std::isfinite(out.min_support) && out.min_support >= 1.f))
        return fail(VMX_ERR_INVALID, "vmx_adaptive_params: min_support must be finite and >= 1");
    if (!squarings_ok(out.normal_squarings)) return fail(VMX_ERR_INVALID, "vmx_adaptive_params: normal_squarings must be 0..8");
    if (!finite_positive(out.sigma_depth)) return fail(VMX_ERR_INVALID, "vmx_adaptive_params: sigma_depth must be finite and > 0");
    if (!reserved_zero(out.reserved)) return fail(VMX_ERR_INVALID, "vmx_adaptive_params: reserved words must be 0");
    return VMX_OK;
}
