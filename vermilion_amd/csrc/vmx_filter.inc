// vmx_filter.inc — G-buffer-guided edge-avoiding a-trous filter of frames and progressive previews (vmx_filter_*,
// vmx_progressive_preview_filtered*).  Included by vmx_kernels.hip (inside its namespace, after vmx_image.inc: the tile,
// the tap terms and the launch are there).  The arithmetic is stated
// in include/vermilion_hip.h and restated in tests/filter_spec.py; with -ffp-contract=off every operation below rounds
// once, in the order written, and `/` is the correctly rounded division with denormals kept: bit for bit the restatement.
//
//   k_filter_guide  one lane per pixel: the 64-byte vmx_rayhit becomes the 16-byte guide record (n.xyz, z); z = -1 and
//                   n = 0 where the ray missed ("a hit" is z >= 0 from here on).
//   k_atrous        one iteration, one lane per pixel of an image_tile: each of a wave's tap loads is two runs of 32
//                   consecutive 16-byte records at every step size.  The 25 taps
//                   are unrolled; the centre's guide and colour stay in registers; hit / miss and every skip rule are
//                   selects, not branches (a tap outside the image loads the centre's records and is selected away).
//                   IN: where the colours come from — 0 a float4 plane (every iteration but the first), 1 the RGBAZ
//                   frame, 2 the per-pixel state of a progressive render, shown as k_preview shows it.
//                   LAST: the iteration that writes the caller's buffers (atrous_write_last).  Else the result goes to
//                   the other float4 plane.
//                   M: normal_squarings as a constant (the default, 5) or -1: read from the pass.
//                   DEMOD (vmx_filter_apply_demodulated_device; LAST only): the result is multiplied by the pixel's own
//                   albedo before it leaves, each channel clamped from below (filter_albedo).
//   k_demod_divide  the demodulated call's pre-pass, one lane per pixel, dense: frame / albedo (or the pixel state as
//                   k_preview shows it / albedo) into the float4 plane the first iteration then reads as IN = 0.  Measured
//                   against dividing per tap inside the first iteration at 1920x1080 (profiles/demod_bench.txt): 436 us
//                   against 477 for a five-iteration call on a frame, 119 against 299 for a single iteration, 441 against
//                   1080 for a filtered preview — the per-tap forms of the first iteration need 300+ VGPRs.  The
//                   existing instantiations are the instruction streams they were without the parameter.
__global__ void __launch_bounds__(256) k_filter_guide(const float4 *__restrict__ rayhit, uint32_t npix,
                                                      float4 *__restrict__ guide) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const float4 *r = rayhit + (size_t)p * 4;  // (location, distance) (normal, tri_id) (uv, tri_t, flags) (colour, pad)
    const float4 a = r[0], b = r[1], c = r[2];
    const bool hit = (__float_as_uint(c.w) & 1u) != 0;
    guide[p] = hit ? make_float4(b.x, b.y, b.z, a.w) : make_float4(0.f, 0.f, 0.f, -1.f);
}

// pixel q of the filter's first input: the five floats of the frame, or what k_preview shows for that pixel's state
template <bool STATE>
__device__ __forceinline__ void filter_src_pixel(const FilterSrc &s, uint32_t q, float *v) {
    if (!STATE) {
        const float *f = s.frame + (size_t)q * 5;
        v[0] = f[0], v[1] = f[1], v[2] = f[2], v[3] = f[3], v[4] = f[4];
    } else if ((s.px.cursor[q] & ~kCursorStrided) >= s.kmax) {
        const float *f = s.finished + (size_t)q * 5;
        v[0] = f[0], v[1] = f[1], v[2] = f[2], v[3] = f[3], v[4] = f[4];
    } else {
        const uint32_t n = s.px.count[q];
        if (n == 0) {
            v[0] = 0.f, v[1] = 0.f, v[2] = 0.f, v[3] = 1.f, v[4] = 0.f;
        } else {
            resolved_pixel(((const float4 *)s.px.accum)[q], n, v);
        }
    }
}

// pixel q's albedo as the demodulated filter divides and multiplies by it: VMX_ALBEDO_FLOOR unless above it and finite
constexpr float kAlbedoFloor = 0.0009765625f;  // VMX_ALBEDO_FLOOR = 2^-10
__device__ __forceinline__ void filter_albedo(const FilterPass &a, uint32_t q, float *am) {
    const float4 v = ((const float4 *)a.albedo)[q];
    am[0] = (v.x > kAlbedoFloor && v.x <= 3.402823466e+38f) ? v.x : kAlbedoFloor;
    am[1] = (v.y > kAlbedoFloor && v.y <= 3.402823466e+38f) ? v.y : kAlbedoFloor;
    am[2] = (v.z > kAlbedoFloor && v.z <= 3.402823466e+38f) ? v.z : kAlbedoFloor;
}

template <int IN>
__device__ __forceinline__ void filter_colour(const FilterPass &a, uint32_t q, float *c) {
    if (IN == 0) {
        const float4 v = ((const float4 *)a.in_plane)[q];
        c[0] = v.x, c[1] = v.y, c[2] = v.z;
    } else {
        float v[5];
        filter_src_pixel<IN == 2>(a.src, q, v);
        c[0] = v[0], c[1] = v[1], c[2] = v[2];
    }
}

template <bool STATE>
__global__ void __launch_bounds__(256) k_demod_divide(FilterPass a, uint32_t npix) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    float v[5], am[3];
    filter_src_pixel<STATE>(a.src, p, v);
    filter_albedo(a, p, am);
    ((float4 *)a.out_plane)[p] = make_float4(v[0] / am[0], v[1] / am[1], v[2] / am[2], 0.f);
}

// the last iteration's way out, for k_atrous and k_atrous_var: o.rgb with the alpha and depth of the first input (own
// pixel only) into the lane's five words of s_px, rgba8 from the same values, then the block's runs to out_rgbaz.
// STATE: the first input may be the per-pixel state of a progressive render (a.src.frame NULL)
template <bool STATE>
__device__ __forceinline__ void atrous_write_last(const FilterPass &a, const ImageTile &t, const float *o, float *s_px) {
    if (t.live) {
        float *v = s_px + threadIdx.x * 5;
        float src[5];
        if (!STATE || a.src.frame)
            filter_src_pixel<false>(a.src, t.p, src);
        else
            filter_src_pixel<true>(a.src, t.p, src);
        v[0] = o[0], v[1] = o[1], v[2] = o[2], v[3] = src[3], v[4] = src[4];  // alpha, depth: the input's bits
        if (a.rgba8) ((uchar4 *)a.rgba8)[t.p] = quantized_pixel(v);
    }
    if (!a.out_rgbaz) return;
    __syncthreads();
    tile_store_rgbaz(s_px, a.out_rgbaz, a.width, a.height, t.bx0, t.by0);
}

template <int IN, bool LAST, int M, bool DEMOD = false>
__global__ void __launch_bounds__(kFilterBlock) k_atrous(FilterPass a) {
    static_assert(!DEMOD || (LAST && IN == 0), "demodulation: the pre-pass divides, the last iteration (from a plane) multiplies");
    __shared__ float s_px[LAST ? kFilterBlock * 5 : 1];
    const uint32_t W = a.width, H = a.height;
    const ImageTile tile = image_tile(W, H);
    const uint32_t x = tile.x, y = tile.y, p = tile.p;
    float o[3] = {0.f, 0.f, 0.f};
    if (tile.live) {
        const float4 *guide = (const float4 *)a.guide;
        const float4 gp = guide[p];
        float cp[3];
        filter_colour<IN>(a, p, cp);
        const bool hitp = gp.w >= 0.f;
        const float isc2 = a.isc2;
        const float isz = 1.f / (a.kz * gp.w);
        const int step = (int)a.step;
        float sum0 = 0.f, sum1 = 0.f, sum2 = 0.f, sumw = 0.f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const float h5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
                const float hh = h5[dy + 2] * h5[dx + 2];
                const int qx = (int)x + dx * step, qy = (int)y + dy * step;
                const bool inside = (uint32_t)qx < W && (uint32_t)qy < H;
                const uint32_t q = inside ? (uint32_t)qy * W + (uint32_t)qx : p;
                const float4 gq = guide[q];
                float cq[3];
                filter_colour<IN>(a, q, cq);
                const float d = guide_normal_weight<M>(gp, gq, a.squarings);
                float num, g;
                guide_depth_terms(hh, d, gp, gq, hitp, isz, num, g);
                const float dr = cp[0] - cq[0], dg = cp[1] - cq[1], db = cp[2] - cq[2];
                const float e = dr * dr + dg * dg + db * db;
                const float w = num / (g * (1.f + e * isc2));
                const bool ok = tap_counts(inside, gq, hitp, w);
                sum0 = ok ? sum0 + w * cq[0] : sum0;
                sum1 = ok ? sum1 + w * cq[1] : sum1;
                sum2 = ok ? sum2 + w * cq[2] : sum2;
                sumw = ok ? sumw + w : sumw;
            }
        }
        const bool any = sumw > 0.f;
        o[0] = any ? sum0 / sumw : cp[0];
        o[1] = any ? sum1 / sumw : cp[1];
        o[2] = any ? sum2 / sumw : cp[2];
        if (DEMOD && LAST) {
            float am[3];
            filter_albedo(a, p, am);
            o[0] = o[0] * am[0], o[1] = o[1] * am[1], o[2] = o[2] * am[2];
        }
    }
    if (!LAST) {
        if (tile.live) ((float4 *)a.out_plane)[p] = make_float4(o[0], o[1], o[2], 0.f);
    } else {
        atrous_write_last<true>(a, tile, o, s_px);
    }
}

int launch_filter_guide(const void *rayhit, uint32_t npix, void *guide, void *stream) {
    if (npix == 0) return 0;
    hipLaunchKernelGGL(k_filter_guide, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float4 *)rayhit,
                       npix, (float4 *)guide);
    return launch_status();
}

template <int IN, bool LAST>
static auto atrous_kernel(const FilterPass &a) -> void (*)(FilterPass) {
    // demodulation touches the iteration that writes the result (k_demod_divide wrote the plane the first one reads)
    if constexpr (IN == 0 && LAST)
        if (a.albedo) return for_squarings(a.squarings, [](auto m) { return k_atrous<IN, LAST, decltype(m)::value, true>; });
    return for_squarings(a.squarings, [](auto m) { return k_atrous<IN, LAST, decltype(m)::value>; });
}

// the demodulated call's pre-pass: a.src / a.albedo into a.out_plane
int launch_demod_divide(const FilterPass &a, void *stream) {
    const uint32_t npix = a.width * a.height;
    if (npix == 0) return 0;
    if (a.src.frame)
        hipLaunchKernelGGL(k_demod_divide<false>, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, npix);
    else
        hipLaunchKernelGGL(k_demod_divide<true>, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, npix);
    return launch_status();
}

int launch_atrous(const FilterPass &a, void *stream) {
    const int in = !a.first ? 0 : (a.src.frame ? 1 : 2);
    if (a.last)
        return launch_image(in == 0 ? atrous_kernel<0, true>(a) : in == 1 ? atrous_kernel<1, true>(a) : atrous_kernel<2, true>(a), a, stream);
    return launch_image(in == 0 ? atrous_kernel<0, false>(a) : in == 1 ? atrous_kernel<1, false>(a) : atrous_kernel<2, false>(a), a, stream);
}
