// vmx_image.inc — what the image-space passes share (vmx_filter.inc, vmx_upsample.inc, vmx_temporal.inc, vmx_variance.inc):
// the block of 32 x 8 pixels and its way through LDS, the guide's tap terms, and how such a kernel is launched.  Included
// by vmx_kernels.hip (inside its namespace) before them.  Every helper is inlined: a kernel built on them is the
// instruction stream it was with the helper's body written out (tools/isa_compare.py, profiles/image_refactor_isa.txt).
// With -ffp-contract=off every operation below rounds once, in the order written, as the restatements in tests/*_spec.py.
constexpr uint32_t kFilterBX = 32, kFilterBY = 8, kFilterBlock = kFilterBX * kFilterBY;

// one lane per pixel: a wave is two image rows of 32 pixels.  (bx0, by0) the block's first pixel, (x, y) the lane's,
// p its index, live: on the image
struct ImageTile {
    uint32_t bx0, by0, x, y, p;
    bool live;
};

__device__ __forceinline__ ImageTile image_tile(uint32_t W, uint32_t H) {
    // (a one-dimensional grid of blocks, row-major over the image: the second grid dimension ends at 65535)
    const uint32_t nbx = (W + kFilterBX - 1) / kFilterBX;
    const uint32_t by = blockIdx.x / nbx, bx = blockIdx.x - by * nbx;
    ImageTile t;
    t.bx0 = bx * kFilterBX, t.by0 = by * kFilterBY;
    t.x = t.bx0 + (threadIdx.x & (kFilterBX - 1));
    t.y = t.by0 + threadIdx.x / kFilterBX;
    t.live = t.x < W && t.y < H;
    t.p = t.y * W + t.x;  // (W * H <= 2^28: the size check of make_frame and of every handle's create)
    return t;
}

// The block's 256 RGBAZ pixels are eight runs of 160 floats in the image: row r is the run of 5 * (its pixels in the
// image) floats at ((by0 + r) * W + bx0) * 5.  They pass through s_px (kFilterBlock * 5 words, pixel i at i * 5: an odd
// stride, no bank conflict) as dword accesses of consecutive lanes to consecutive addresses, five per lane, instead of
// five of stride 20.  Word c * kFilterBlock + lane: its index i in s_px and its place in the image, false if off it
__device__ __forceinline__ bool tile_word(uint32_t c, uint32_t W, uint32_t H, uint32_t bx0, uint32_t by0, uint32_t &i, size_t &at) {
    const uint32_t run = min(kFilterBX, W - bx0) * 5;
    i = c * kFilterBlock + threadIdx.x;
    const uint32_t r = i / (kFilterBX * 5), col = i - r * (kFilterBX * 5);
    at = ((size_t)(by0 + r) * W + bx0) * 5 + col;
    return by0 + r < H && col < run;
}

__device__ __forceinline__ void tile_load_rgbaz(float *s_px, const float *in, uint32_t W, uint32_t H, uint32_t bx0, uint32_t by0) {
#pragma unroll
    for (uint32_t c = 0; c < 5; ++c) {
        uint32_t i;
        size_t at;
        if (tile_word(c, W, H, bx0, by0, i, at)) s_px[i] = in[at];
    }
}

// (after a barrier: every lane's pixel is in s_px)
__device__ __forceinline__ void tile_store_rgbaz(const float *s_px, float *out, uint32_t W, uint32_t H, uint32_t bx0, uint32_t by0) {
#pragma unroll
    for (uint32_t c = 0; c < 5; ++c) {
        uint32_t i;
        size_t at;
        if (tile_word(c, W, H, bx0, by0, i, at)) out[at] = s_px[i];
    }
}

// ---- a tap q against the centre p, both as guide records (n.xyz, z), z < 0 a miss ---------------------------------------
// the normal weight: max(0, n_p . n_q)^(2^squarings).  M: normal_squarings as a constant, or -1: `squarings` is read
template <int M>
__device__ __forceinline__ float guide_normal_weight(const float4 &gp, const float4 &gq, uint32_t squarings) {
    float d = gp.x * gq.x + gp.y * gq.y + gp.z * gq.z;
    d = d > 0.f ? d : 0.f;
    if (M >= 0) {
#pragma unroll
        for (int i = 0; i < M; ++i) d = d * d;
    } else {
        for (uint32_t i = 0; i < squarings; ++i) d = d * d;
    }
    return d;
}

// the weight's numerator and the depth term of its denominator: (b * d, 1 + t^2) between hits, (b, 1) between misses; b
// the tap's kernel weight, d its normal weight, isz = 1 / (sigma_depth * z_p)
__device__ __forceinline__ void guide_depth_terms(float b, float d, const float4 &gp, const float4 &gq, bool hitp, float isz,
                                                  float &num, float &g) {
    const float t = (gp.w - gq.w) * isz;
    num = hitp ? b * d : b;
    g = hitp ? 1.f + t * t : 1.f;
}

// a tap counts only if inside, in the centre's hit state, and its weight positive and finite (a NaN fails both comparisons)
__device__ __forceinline__ bool tap_counts(bool inside, const float4 &gq, bool hitp, float w) {
    return inside && ((gq.w >= 0.f) == hitp) && w > 0.f && w <= 3.402823466e+38f;
}

__device__ __forceinline__ float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// ---- launching ---------------------------------------------------------------------------------------------------------
static dim3 image_grid(uint32_t W, uint32_t H) { return dim3(((W + kFilterBX - 1) / kFilterBX) * ((H + kFilterBY - 1) / kFilterBY)); }

// kernel_of(M) for normal_squarings as the constant the kernels are built for (the default, 5) or -1: read from the pass
template <typename F>
static auto for_squarings(uint32_t squarings, F kernel_of) {
    return squarings == 5 ? kernel_of(std::integral_constant<int, 5>{}) : kernel_of(std::integral_constant<int, -1>{});
}

// one block per tile of the pass's width x height (none: nothing is launched)
template <typename Pass>
static int launch_image(void (*kernel)(Pass), const Pass &a, void *stream) {
    if (a.width == 0 || a.height == 0) return 0;
    hipLaunchKernelGGL(kernel, image_grid(a.width, a.height), dim3(kFilterBlock), 0, (hipStream_t)stream, a);
    return launch_status();
}
