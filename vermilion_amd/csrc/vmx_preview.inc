// vmx_preview.inc — the displayable frame of a progressive render (vmx_progressive_preview / _preview_device).
// Included by vmx_kernels.hip (inside its namespace).
//
//   k_preview  one lane per local pixel, 256 pixels per block.  k_resolve writes a pixel only once it is complete; this
//              kernel shows the per-pixel state as it stands and changes none of it:
//                finished pixel (cursor >= kmax)  the five floats k_resolve wrote for it, copied
//                unfinished pixel, n >= 1 samples k_resolve's pixel write (resolved_pixel) of its current (acc, n)
//                no sample yet                    (0, 0, 0, 1, 0)
//              and, in the same launch, the rgba8 form of those values (k_quantize's arithmetic).
//              A pixel is 20 bytes: a lane storing its own five floats would put five dword stores of stride 20 on
//              every 128-byte line.  The block's 256 pixels are one contiguous run of 1280 floats, so they pass through
//              LDS: the finished frame's run comes in (only in blocks that hold a finished pixel) and the result goes
//              out as dword accesses of consecutive lanes to consecutive addresses: 24 B read (state, or cursor and
//              frame) and 20 / 24 B written per pixel.  A lane's five LDS words are at 5 * lane: an odd stride, no bank conflict.
constexpr uint32_t kPreviewBlock = 256;

__global__ void __launch_bounds__(kPreviewBlock) k_preview(PixelStateDev px, uint32_t npix, uint32_t kmax,
                                                           const float *__restrict__ finished, float *__restrict__ out,
                                                           uchar4 *__restrict__ rgba8) {
    __shared__ float s_px[kPreviewBlock * 5];
    const uint32_t base = blockIdx.x * kPreviewBlock;  // (npix * 5 < 2^31 / 8 * 5: make_frame's size check)
    const uint32_t nb = min(kPreviewBlock, npix - base);
    const bool live = threadIdx.x < nb;
    const uint32_t lp = base + threadIdx.x;
    const bool done = live && (px.cursor[lp] & ~kCursorStrided) >= kmax;
    // the finished frame's run is read only where the block has a finished pixel: a frame without one costs its state alone
    if (__syncthreads_or(done)) {
        const float *src = finished + (size_t)base * 5;
#pragma unroll
        for (uint32_t c = 0; c < 5; ++c) {
            const uint32_t i = c * kPreviewBlock + threadIdx.x;
            if (i < nb * 5) s_px[i] = src[i];  // (an unfinished pixel's slot holds whatever the buffer held: replaced below)
        }
        __syncthreads();
    }
    if (live) {
        float *v = s_px + threadIdx.x * 5;
        if (!done) {
            const uint32_t n = px.count[lp];
            if (n == 0) {
                v[0] = 0.f, v[1] = 0.f, v[2] = 0.f, v[3] = 1.f, v[4] = 0.f;
            } else {
                resolved_pixel(((const float4 *)px.accum)[lp], n, v);
            }
        }
        if (rgba8) rgba8[lp] = quantized_pixel(v);
    }
    if (!out) return;
    __syncthreads();
    float *dst = out + (size_t)base * 5;
#pragma unroll
    for (uint32_t c = 0; c < 5; ++c) {
        const uint32_t i = c * kPreviewBlock + threadIdx.x;
        if (i < nb * 5) dst[i] = s_px[i];
    }
}

int launch_preview(PixelStateDev px, uint32_t npix, uint32_t kmax, const float *finished, float *out_rgbaz, void *rgba8,
                   void *stream) {
    if (npix == 0) return 0;
    hipLaunchKernelGGL(k_preview, dim3((npix + kPreviewBlock - 1) / kPreviewBlock), dim3(kPreviewBlock), 0,
                       (hipStream_t)stream, px, npix, kmax, finished, out_rgbaz, (uchar4 *)rgba8);
    return launch_status();
}
