// vmx_adaptive.inc — adaptive temporal accumulation: the reprojected history is tested against the new frame over a 7 x 7
// window of like surface, and where the two window means differ by more than the input's noise explains, the history
// length is cut before the blend (vmx_temporal_accumulate_adaptive_device).  Included by vmx_kernels.hip (inside its
// namespace, after vmx_image.inc and vmx_temporal.inc: the tile, the guide's normal weight, temporal_proj).  The
// arithmetic is stated in include/vermilion_hip.h and restated in tests/adaptive_spec.py; with -ffp-contract=off every
// operation below rounds once, in the order written, and `/` is the correctly rounded division with denormals kept: bit
// for bit the restatement.  No transcendentals.  A first call is k_temporal<true, ..> itself: these kernels never see one.
//
//   k_temporal_gather  k_temporal's reprojection with no blend, one lane per pixel of an image_tile: the four taps of
//                      vmx_temporal.inc restated (the same loads, selects and order: k_temporal's instantiations stay the
//                      instruction streams they are), then (hh.rgb, any ? nh : 0) to the handle's reprojection plane —
//                      a fourth word > 0 IS `any`, since every history length is >= 1 — and (g1, g2) behind it on a
//                      moments handle.  It also writes the two planes of the new state that depend on the record alone,
//                      the guide (n.xyz, z) and X: k_rectify reads its taps' guide from there, packed, one float4 each.
//   k_rectify          one lane per pixel of an image_tile.  The block stages 38 x 14 pixels (the tile and a halo of 3) in
//                      LDS as eleven planes of one word — the input's r, g, b, the reprojection's (hh.rgb, nh), the guide's
//                      (n.xyz, z): lanes of a row at consecutive words, the two rows of a wave 38 words apart, so no access
//                      of the 49 taps meets a bank conflict; 23408 B, six blocks per CU.  A pixel outside the image is
//                      staged as a miss without history (z = -1, nh = 0), which the tap test rejects.  Rows in a loop, the
//                      seven taps of a row unrolled, every skip rule a select; 1 / (sigma_depth * z_p) is per pixel, the
//                      division of a tap's weight is the restatement's and stays.  Then k_temporal's tail: the blend
//                      with the cut history length, the colour plane (and moments) of the new state, rgba8, history_len,
//                      d_change, and the output frame through the staging words (tile_store_rgbaz).
//                      M: normal_squarings as a constant (the default, 5) or -1: read from the pass.
//   k_adaptive_store   a call in place only: k_rectify's taps read the input of neighbouring blocks, so it may not replace
//                      it; it leaves the frame alone and this dense pass copies r, g, b from the new state afterwards
//                      (alpha and depth are the input's bits already).
constexpr float kAdaptiveEps = 1e-10f;  // VMX_ADAPTIVE_EPS
constexpr int kRectHalo = 3;
constexpr uint32_t kRectW = kFilterBX + 2 * kRectHalo, kRectH = kFilterBY + 2 * kRectHalo, kRectN = kRectW * kRectH;
constexpr uint32_t kRectPlanes = 11;  // c.r c.g c.b  hh.r hh.g hh.b nh  n.x n.y n.z z
static_assert(kRectPlanes * kRectN >= kFilterBlock * 5, "k_rectify: the output tile passes through the staging words");

template <bool MOTION, bool MOMENTS>
__global__ void __launch_bounds__(kFilterBlock) k_temporal_gather(AdaptivePass a) {
    const uint32_t W = a.t.width, H = a.t.height;
    const ImageTile tile = image_tile(W, H);
    if (!tile.live) return;
    const uint32_t x = tile.x, y = tile.y, p = tile.p;
    const float4 *r = (const float4 *)a.t.rayhit + (size_t)p * 4;  // (location, distance) (normal, tri_id) (uv, tri_t, flags)
    const float4 ra = r[0], rb = r[1], rc = r[2];
    const bool hit = (__float_as_uint(rc.w) & 1u) != 0;
    const size_t npix = (size_t)W * H;
    float Xhx = ra.x, Xhy = ra.y, Xhz = ra.z, mnx = rb.x, mny = rb.y, mnz = rb.z;
    if (MOTION) {
        const float4 *m = (const float4 *)a.t.motion + (size_t)p * 2;  // (prev_location, flags) (prev_normal, pad)
        const float4 ma = m[0], mb = m[1];
        Xhx = ma.x, Xhy = ma.y, Xhz = ma.z, mnx = mb.x, mny = mb.y, mnz = mb.z;
    }
    const float fw = (float)W, fh = (float)H;
    const TemporalProj pc = temporal_proj(a.t.cam, ra.x, ra.y, ra.z, fw, fh);
    const TemporalProj ph = temporal_proj(a.t.hist_cam, Xhx, Xhy, Xhz, fw, fh);
    const float gx = (float)x + (ph.u - pc.u);
    const float gy = (float)y + (ph.w - pc.w);
    const bool inrange = hit && ph.front && gx >= -1.f && gx < fw && gy >= -1.f && gy < fh;
    const float x0 = floorf(gx), y0 = floorf(gy);
    const float fx = gx - x0, fy = gy - y0;
    const int x0i = (int)(inrange ? x0 : 0.f), y0i = (int)(inrange ? y0 : 0.f);
    const float zz = a.t.tol2 * (ra.w * ra.w);
    const float4 *old_c = (const float4 *)a.t.old_state, *old_g = old_c + npix, *old_x = old_g + npix;
    const float2 *old_m = (const float2 *)(old_x + npix);
    float sum0 = 0.f, sum1 = 0.f, sum2 = 0.f, sumn = 0.f, sumw = 0.f, summ1 = 0.f, summ2 = 0.f;
#pragma unroll
    for (int dy = 0; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = 0; dx <= 1; ++dx) {
            const int qx = x0i + dx, qy = y0i + dy;
            const bool inside = (uint32_t)qx < W && (uint32_t)qy < H;
            const uint32_t q = inside ? (uint32_t)qy * W + (uint32_t)qx : p;
            const float4 hc = old_c[q], hg = old_g[q], hx = old_x[q];
            const float wx = dx ? fx : 1.f - fx, wy = dy ? fy : 1.f - fy;
            const float wt = wx * wy;
            const float d = (mnx * hg.x + mny * hg.y) + mnz * hg.z;
            const float ex = Xhx - hx.x, ey = Xhy - hx.y, ez = Xhz - hx.z;
            const float pd = (mnx * ex + mny * ey) + mnz * ez;
            const bool ok = inrange && inside && hg.w >= 0.f && d >= a.t.normal_min && pd * pd <= zz && wt > 0.f;
            sum0 = ok ? sum0 + wt * hc.x : sum0;
            sum1 = ok ? sum1 + wt * hc.y : sum1;
            sum2 = ok ? sum2 + wt * hc.z : sum2;
            sumn = ok ? sumn + wt * hc.w : sumn;
            if (MOMENTS) {
                const float2 hm = old_m[q];
                summ1 = ok ? summ1 + wt * hm.x : summ1;
                summ2 = ok ? summ2 + wt * hm.y : summ2;
            }
            sumw = ok ? sumw + wt : sumw;
        }
    }
    const bool any = sumw > 0.f;
    const float h0 = sum0 / sumw, h1 = sum1 / sumw, h2 = sum2 / sumw, nh = sumn / sumw;
    float4 *plane = (float4 *)a.plane;
    plane[p] = any ? make_float4(h0, h1, h2, nh) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (MOMENTS) {
        const float g1 = summ1 / sumw, g2 = summ2 / sumw;
        ((float2 *)(plane + npix))[p] = any ? make_float2(g1, g2) : make_float2(0.f, 0.f);
    }
    float4 *new_g = (float4 *)a.t.new_state + npix, *new_x = new_g + npix;
    new_g[p] = hit ? make_float4(rb.x, rb.y, rb.z, ra.w) : make_float4(0.f, 0.f, 0.f, -1.f);
    new_x[p] = make_float4(ra.x, ra.y, ra.z, 0.f);
}

template <bool MOMENTS, int M>
__global__ void __launch_bounds__(kFilterBlock) k_rectify(AdaptivePass a) {
    __shared__ float s_all[kRectPlanes * kRectN];
    const uint32_t W = a.t.width, H = a.t.height;
    const ImageTile tile = image_tile(W, H);
    const uint32_t p = tile.p;
    const size_t npix = (size_t)W * H;
    const float4 *plane = (const float4 *)a.plane;
    float4 *new_c = (float4 *)a.t.new_state;
    const float4 *new_g = new_c + npix;
    for (uint32_t i = threadIdx.x; i < kRectN; i += kFilterBlock) {
        const uint32_t ry = i / kRectW, rx = i - ry * kRectW;
        const int qx = (int)(tile.bx0 + rx) - kRectHalo, qy = (int)(tile.by0 + ry) - kRectHalo;
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;
        float4 hq = make_float4(0.f, 0.f, 0.f, 0.f), gq = make_float4(0.f, 0.f, 0.f, -1.f);
        if ((uint32_t)qx < W && (uint32_t)qy < H) {
            const uint32_t q = (uint32_t)qy * W + (uint32_t)qx;
            const float *in = a.t.in_rgbaz + (size_t)q * 5;
            c0 = in[0], c1 = in[1], c2 = in[2];
            hq = plane[q], gq = new_g[q];
        }
        s_all[0 * kRectN + i] = c0, s_all[1 * kRectN + i] = c1, s_all[2 * kRectN + i] = c2;
        s_all[3 * kRectN + i] = hq.x, s_all[4 * kRectN + i] = hq.y, s_all[5 * kRectN + i] = hq.z, s_all[6 * kRectN + i] = hq.w;
        s_all[7 * kRectN + i] = gq.x, s_all[8 * kRectN + i] = gq.y, s_all[9 * kRectN + i] = gq.z, s_all[10 * kRectN + i] = gq.w;
    }
    __syncthreads();
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (tile.live) {
        const uint32_t li = (threadIdx.x / kFilterBX + kRectHalo) * kRectW + (threadIdx.x & (kFilterBX - 1)) + kRectHalo;
        const float c0 = s_all[0 * kRectN + li], c1 = s_all[1 * kRectN + li], c2 = s_all[2 * kRectN + li];
        const float h0 = s_all[3 * kRectN + li], h1 = s_all[4 * kRectN + li], h2 = s_all[5 * kRectN + li];
        const float nh = s_all[6 * kRectN + li];
        const float4 gp = make_float4(s_all[7 * kRectN + li], s_all[8 * kRectN + li], s_all[9 * kRectN + li], s_all[10 * kRectN + li]);
        const bool any = nh > 0.f;  // (a miss reprojects nothing: it has no history either)
        const float isz = 1.f / (a.sigma_depth * gp.w);
        float sw = 0.f, sww = 0.f;
        float sc0 = 0.f, sc1 = 0.f, sc2 = 0.f, scc0 = 0.f, scc1 = 0.f, scc2 = 0.f, sh0 = 0.f, sh1 = 0.f, sh2 = 0.f;
#pragma unroll 1
        for (int dy = -kRectHalo; dy <= kRectHalo; ++dy) {
            const uint32_t row = (uint32_t)((int)li + dy * (int)kRectW);
#pragma unroll
            for (int dx = -kRectHalo; dx <= kRectHalo; ++dx) {
                const uint32_t q = (uint32_t)((int)row + dx);
                const float4 gq = make_float4(s_all[7 * kRectN + q], s_all[8 * kRectN + q], s_all[9 * kRectN + q], s_all[10 * kRectN + q]);
                const float q0 = s_all[0 * kRectN + q], q1 = s_all[1 * kRectN + q], q2 = s_all[2 * kRectN + q];
                const float d = guide_normal_weight<M>(gp, gq, a.squarings);
                const float t = (gp.w - gq.w) * isz;
                const float w = d / (1.f + t * t);
                const bool ok = gq.w >= 0.f && s_all[6 * kRectN + q] > 0.f && w > 0.f && w <= 3.402823466e+38f;
                sw = ok ? sw + w : sw;
                sww = ok ? sww + w * w : sww;
                sc0 = ok ? sc0 + w * q0 : sc0;
                scc0 = ok ? scc0 + w * (q0 * q0) : scc0;
                sh0 = ok ? sh0 + w * s_all[3 * kRectN + q] : sh0;
                sc1 = ok ? sc1 + w * q1 : sc1;
                scc1 = ok ? scc1 + w * (q1 * q1) : scc1;
                sh1 = ok ? sh1 + w * s_all[4 * kRectN + q] : sh1;
                sc2 = ok ? sc2 + w * q2 : sc2;
                scc2 = ok ? scc2 + w * (q2 * q2) : scc2;
                sh2 = ok ? sh2 + w * s_all[5 * kRectN + q] : sh2;
            }
        }
        const bool support = sw > 0.f && sw * sw >= a.min_support * sww;
        const float share = sww / (sw * sw);
        float k[3];
        {
            const float sc[3] = {sc0, sc1, sc2}, scc[3] = {scc0, scc1, scc2}, sh[3] = {sh0, sh1, sh2};
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float mc = sc[j] / sw, mh = sh[j] / sw;
                float var = scc[j] / sw - mc * mc;
                var = var > 0.f ? var : 0.f;
                const float s2 = (2.f * var) * share + kAdaptiveEps;
                const float dm = mc - mh;
                k[j] = (dm * dm) / s2;
            }
        }
        float K = k[0];
        if (k[1] > K) K = k[1];
        if (k[2] > K) K = k[2];
        const float ratio = K / a.gamma2;
        const bool cut = support && ratio > 1.f;  // (false for NaN)
        const float nhe = cut ? nh / ratio : nh;
        const float t = nhe + 1.f;
        const float n1 = t < a.t.max_history ? t : a.t.max_history;
        const float al = 1.f / n1;
        const float o0 = any ? h0 + (c0 - h0) * al : c0;
        const float o1 = any ? h1 + (c1 - h1) * al : c1;
        const float o2 = any ? h2 + (c2 - h2) * al : c2;
        const float n_new = any ? n1 : 1.f;
        new_c[p] = make_float4(o0, o1, o2, n_new);
        if (MOMENTS) {
            const float lum = luminance(c0, c1, c2);
            const float2 g = ((const float2 *)(plane + npix))[p];
            const float m1 = any ? g.x + (lum - g.x) * al : lum;
            const float m2 = any ? g.y + (lum * lum - g.y) * al : lum * lum;
            ((float2 *)(new_c + 3 * npix))[p] = make_float2(m1, m2);
        }
        const float *in = a.t.in_rgbaz + (size_t)p * 5;
        v[0] = o0, v[1] = o1, v[2] = o2, v[3] = in[3], v[4] = in[4];  // (alpha and depth, the input's bits)
        if (a.t.rgba8) ((uchar4 *)a.t.rgba8)[p] = quantized_pixel(v);
        if (a.t.history_len) a.t.history_len[p] = n_new;
        if (a.change) a.change[p] = any && support ? ratio : 0.f;
    }
    if (!a.t.out_rgbaz) return;
    __syncthreads();  // (every tap has been read: the staging words become the tile's output pixels)
    {
        float *s = s_all + threadIdx.x * 5;
        s[0] = v[0], s[1] = v[1], s[2] = v[2], s[3] = v[3], s[4] = v[4];
    }
    __syncthreads();
    tile_store_rgbaz(s_all, a.t.out_rgbaz, W, H, tile.bx0, tile.by0);
}

__global__ void __launch_bounds__(256) k_adaptive_store(const float4 *__restrict__ colour, float *__restrict__ out, uint32_t npix) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const float4 c = colour[p];
    float *o = out + (size_t)p * 5;
    o[0] = c.x, o[1] = c.y, o[2] = c.z;
}

template <bool MOMENTS>
static auto rectify_kernel(const AdaptivePass &a) {
    return for_squarings(a.squarings, [](auto m) { return k_rectify<MOMENTS, decltype(m)::value>; });
}

// the two passes of a call that is no first call: a.t as launch_temporal takes it, a.t.out_rgbaz NULL for a call in place
// (store_in_place: the frame, then written from the new state)
int launch_adaptive(const AdaptivePass &a, float *store_in_place, void *stream) {
    const uint32_t W = a.t.width, H = a.t.height;
    if (W == 0 || H == 0) return 0;
    void (*gather)(AdaptivePass);
    if (a.t.moments)
        gather = a.t.motion ? k_temporal_gather<true, true> : k_temporal_gather<false, true>;
    else
        gather = a.t.motion ? k_temporal_gather<true, false> : k_temporal_gather<false, false>;
    void (*rectify)(AdaptivePass) = a.t.moments ? rectify_kernel<true>(a) : rectify_kernel<false>(a);
    hipLaunchKernelGGL(gather, image_grid(W, H), dim3(kFilterBlock), 0, (hipStream_t)stream, a);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(rectify, image_grid(W, H), dim3(kFilterBlock), 0, (hipStream_t)stream, a);
    if (int rc = launch_status()) return rc;
    if (store_in_place) {
        const uint32_t npix = W * H;
        hipLaunchKernelGGL(k_adaptive_store, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float4 *)a.t.new_state,
                           store_in_place, npix);
        return launch_status();
    }
    return 0;
}
