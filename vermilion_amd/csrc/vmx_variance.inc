// vmx_variance.inc — variance-guided denoising: the per-pixel variance of a moments accumulator's luminance
// (vmx_temporal_accumulate_variance_device) and the a-trous filter whose colour stop it steers
// (vmx_filter_apply_variance_device).  Included by vmx_kernels.hip (inside its namespace, after vmx_image.inc and
// vmx_filter.inc: the tile, the tap terms, the filter's pixel helpers and atrous_write_last).  The arithmetic is stated
// in include/vermilion_hip.h and restated in tests/variance_spec.py; with -ffp-contract=off every operation below rounds once, in the order written, and `/` is the
// correctly rounded division with denormals kept: bit for bit the restatement.  No transcendentals.
//
//   k_variance       one lane per pixel of an image_tile.  It reads the state k_temporal<.., MOMENTS> just wrote:
//                    n' (the colour plane's .w, one dword), the guide and the moments.  A pixel with n' >= min_history
//                    leaves with its temporal variance; a wave none of whose lanes is younger skips the window
//                    altogether (one ballot).  The window is 7 x 7 over the same state, rows in a loop and the seven
//                    taps of a row unrolled: two loads per tap (guide float4, moments float2), the centre's guide and n'
//                    in registers, every skip rule a select (a tap outside the image loads the centre's records and is
//                    selected away, as in k_atrous).
//                    M: normal_squarings as a constant (the default, 5) or -1: read from the pass.
//   k_variance_pack  the variance-guided call's pre-pass, one lane per pixel, dense: (r, g, b, variance) of the frame —
//                    with DEMOD (r, g, b) / albedo and variance / (luminance of the albedo)^2 — into the float4 plane the
//                    first iteration reads; the plane's fourth word carries the variance through the iterations, so a
//                    tap stays two float4 loads (guide, plane).
//   k_atrous_var     one iteration of that call: k_atrous<0, LAST, M, DEMOD> with the colour stop replaced by
//                    dl*dl / (sigma_l^2 * vbar + eps), vbar the 3 x 3 gaussian of the centre's neighbours' variance (nine
//                    dword loads per pixel, not per tap), and the variance propagated as sum w^2 v / (sum w)^2.  The
//                    last iteration drops it and writes the caller's buffers as k_atrous<0, LAST> does.
constexpr float kVarianceEps = 1e-10f;  // VMX_VARIANCE_EPS

template <int M>
__global__ void __launch_bounds__(kFilterBlock) k_variance(VariancePass a) {
    const uint32_t W = a.width, H = a.height;
    const ImageTile tile = image_tile(W, H);
    const uint32_t x = tile.x, y = tile.y;
    const bool live = tile.live;
    const uint32_t p = live ? tile.p : 0u;  // (a lane off the image reads pixel 0)
    const size_t npix = (size_t)W * H;
    const float4 *st_c = (const float4 *)a.state, *st_g = st_c + npix;
    const float2 *st_m = (const float2 *)(st_g + 2 * npix);
    const float np = ((const float *)st_c)[(size_t)p * 4 + 3];
    const float2 mp = st_m[p];
    float vt = mp.y - mp.x * mp.x;
    vt = vt > 0.f ? vt : 0.f;
    float var = vt;
    const bool young = live && !(np >= a.min_history);
    if (__ballot(young) != 0ull) {  // (uniform over the wave)
        const float4 gp = st_g[p];
        const bool hitp = gp.w >= 0.f;
        const float isz = 1.f / (a.sigma_depth * gp.w);
        float s1 = 0.f, s2 = 0.f, sw = 0.f;
#pragma unroll 1
        for (int dy = -3; dy <= 3; ++dy) {
            const int qy = (int)y + dy;
#pragma unroll
            for (int dx = -3; dx <= 3; ++dx) {
                const int qx = (int)x + dx;
                const bool inside = live && (uint32_t)qx < W && (uint32_t)qy < H;
                const uint32_t q = inside ? (uint32_t)qy * W + (uint32_t)qx : p;
                const float4 gq = st_g[q];
                const float2 mq = st_m[q];
                const float d = guide_normal_weight<M>(gp, gq, a.squarings);
                const float t = (gp.w - gq.w) * isz;
                const float w = hitp ? d / (1.f + t * t) : 1.f;
                const bool ok = tap_counts(inside, gq, hitp, w);
                s1 = ok ? s1 + w * mq.x : s1;
                s2 = ok ? s2 + w * mq.y : s2;
                sw = ok ? sw + w : sw;
            }
        }
        const float a1 = s1 / sw, a2 = s2 / sw;
        float vs = a2 - a1 * a1;
        vs = vs > 0.f ? vs : 0.f;
        const float spatial = sw > 0.f ? vs * (a.min_history / np) : vt;
        var = young ? spatial : vt;
    }
    if (live) a.variance[p] = var;
}

int launch_variance(const VariancePass &a, void *stream) {
    return launch_image(for_squarings(a.squarings, [](auto m) { return k_variance<decltype(m)::value>; }), a, stream);
}

template <bool DEMOD>
__global__ void __launch_bounds__(256) k_variance_pack(FilterPass a, const float *__restrict__ variance, uint32_t npix) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    float v[5];
    filter_src_pixel<false>(a.src, p, v);
    float var = variance[p];
    if (DEMOD) {
        float am[3];
        filter_albedo(a, p, am);
        const float la = luminance(am[0], am[1], am[2]);
        v[0] = v[0] / am[0], v[1] = v[1] / am[1], v[2] = v[2] / am[2];
        var = var / (la * la);
    }
    ((float4 *)a.out_plane)[p] = make_float4(v[0], v[1], v[2], var);
}

template <bool LAST, int M, bool DEMOD>
__global__ void __launch_bounds__(kFilterBlock) k_atrous_var(FilterPass a) {
    __shared__ float s_px[LAST ? kFilterBlock * 5 : 1];
    const uint32_t W = a.width, H = a.height;
    const ImageTile tile = image_tile(W, H);
    const uint32_t x = tile.x, y = tile.y, p = tile.p;
    float o[3] = {0.f, 0.f, 0.f}, vo = 0.f;
    if (tile.live) {
        const float4 *guide = (const float4 *)a.guide, *plane = (const float4 *)a.in_plane;
        const float4 gp = guide[p], cp = plane[p];
        const bool hitp = gp.w >= 0.f;
        const float isz = 1.f / (a.kz * gp.w);
        const int step = (int)a.step;
        // the 3 x 3 gaussian of the variance around p, at one pixel's distance whatever the step
        float vbar = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const float k3[3] = {0.25f, 0.5f, 0.25f};
                const int qx = (int)x + dx, qy = (int)y + dy;
                const bool inside = (uint32_t)qx < W && (uint32_t)qy < H;
                const uint32_t q = inside ? (uint32_t)qy * W + (uint32_t)qx : p;
                vbar = vbar + (k3[dy + 1] * k3[dx + 1]) * ((const float *)plane)[(size_t)q * 4 + 3];
            }
        }
        const float den = a.sl2 * vbar + kVarianceEps;
        const float lp = luminance(cp.x, cp.y, cp.z);
        float sum0 = 0.f, sum1 = 0.f, sum2 = 0.f, sumv = 0.f, sumw = 0.f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const float h5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
                const float hh = h5[dy + 2] * h5[dx + 2];
                const int qx = (int)x + dx * step, qy = (int)y + dy * step;
                const bool inside = (uint32_t)qx < W && (uint32_t)qy < H;
                const uint32_t q = inside ? (uint32_t)qy * W + (uint32_t)qx : p;
                const float4 gq = guide[q], cq = plane[q];
                const float d = guide_normal_weight<M>(gp, gq, a.squarings);
                float num, g;
                guide_depth_terms(hh, d, gp, gq, hitp, isz, num, g);
                const float dl = lp - luminance(cq.x, cq.y, cq.z);
                const float w = num / (g * (1.f + (dl * dl) / den));
                const bool ok = tap_counts(inside, gq, hitp, w);
                sum0 = ok ? sum0 + w * cq.x : sum0;
                sum1 = ok ? sum1 + w * cq.y : sum1;
                sum2 = ok ? sum2 + w * cq.z : sum2;
                sumv = ok ? sumv + (w * w) * cq.w : sumv;
                sumw = ok ? sumw + w : sumw;
            }
        }
        const bool any = sumw > 0.f;
        o[0] = any ? sum0 / sumw : cp.x;
        o[1] = any ? sum1 / sumw : cp.y;
        o[2] = any ? sum2 / sumw : cp.z;
        vo = any ? sumv / (sumw * sumw) : cp.w;
        if (DEMOD && LAST) {
            float am[3];
            filter_albedo(a, p, am);
            o[0] = o[0] * am[0], o[1] = o[1] * am[1], o[2] = o[2] * am[2];
        }
    }
    if (!LAST) {
        if (tile.live) ((float4 *)a.out_plane)[p] = make_float4(o[0], o[1], o[2], vo);
    } else {
        atrous_write_last<false>(a, tile, o, s_px);  // (the variance-guided call takes frames only)
    }
}

int launch_variance_pack(const FilterPass &a, const float *variance, void *stream) {
    const uint32_t npix = a.width * a.height;
    if (npix == 0) return 0;
    if (a.albedo)
        hipLaunchKernelGGL(k_variance_pack<true>, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, variance, npix);
    else
        hipLaunchKernelGGL(k_variance_pack<false>, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, variance, npix);
    return launch_status();
}

template <bool LAST, bool DEMOD>
static auto atrous_var_kernel(const FilterPass &a) {
    return for_squarings(a.squarings, [](auto m) { return k_atrous_var<LAST, decltype(m)::value, DEMOD>; });
}

int launch_atrous_var(const FilterPass &a, void *stream) {
    return launch_image(!a.last ? atrous_var_kernel<false, false>(a) : a.albedo ? atrous_var_kernel<true, true>(a) : atrous_var_kernel<true, false>(a),
                        a, stream);
}
