// vmx_upsample.inc — G-buffer-guided upsampling of a low-resolution frame under a full-size G-buffer (vmx_upsample_*).
// Included by vmx_kernels.hip (inside its namespace), after vmx_image.inc (the tile, the tap terms, the launch) and
// vmx_filter.inc, whose k_filter_guide packs both guides.  The
// arithmetic is stated in include/vermilion_hip.h ("guided upsampling") and restated in tests/upsample_spec.py; with
// -ffp-contract=off every operation below rounds once, in the order written, and `/` is the correctly rounded division
// with denormals kept: bit for bit the restatement.
//
//   k_upsample  one lane per full pixel of an image_tile.  The four taps are unrolled;
//               hit / miss, the skip rules and the anchor are selects, not branches (a tap outside the low image loads
//               tap (0, 0)'s records and is selected away).  The low frame and guide are NOT staged in LDS: a block's
//               32 x 8 full pixels touch at most 33 x 9 low pixels of 36 bytes (17 x 5 at ratio 1/2), about 10 KB, which
//               stays in the CU's 32 KiB vector cache between the lanes that share it, and lanes next to each other read
//               the same or the next 16-byte guide record, so a wave's tap load is one or two runs of consecutive
//               records as in k_atrous.  The call is bound by what it must move per full pixel (16 B guide read, 24 B
//               written) against at most 36 B per low pixel, read from HBM once; staging would add a barrier and, for
//               the ratios that are no integer, a per-block footprint computed twice, to save cache hits.
//               The block's pixels leave through LDS (tile_store_rgbaz); rgba8 from the same values.
//               M: normal_squarings as a constant (the default, 5) or -1: read from the pass.
template <int M>
__global__ void __launch_bounds__(kFilterBlock) k_upsample(UpsamplePass a) {
    __shared__ float s_px[kFilterBlock * 5];
    const uint32_t W = a.width, H = a.height, lw = a.low_width, lh = a.low_height;
    const ImageTile tile = image_tile(W, H);
    const uint32_t x = tile.x, y = tile.y, p = tile.p;
    if (tile.live) {
        const float4 *glo = (const float4 *)a.guide_low;
        const float4 gp = ((const float4 *)a.guide_full)[p];
        const float rx = (float)lw / (float)W, ry = (float)lh / (float)H;
        const float u = (float)x * rx, v = (float)y * ry;
        // (the min acts only where rounding lifts u to lw, beyond 2^21 pixels across: tap (0, 0) is inside the low image)
        const uint32_t X0 = min((uint32_t)(int)floorf(u), lw - 1), Y0 = min((uint32_t)(int)floorf(v), lh - 1);
        const float fx = u - (float)X0, fy = v - (float)Y0;
        const bool hitp = gp.w >= 0.f;
        const float isz = 1.f / (a.sigma_depth * gp.w);
        float sum0 = 0.f, sum1 = 0.f, sum2 = 0.f, sumw = 0.f, best = -1.f;
        uint32_t anchor = Y0 * lw + X0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const bool inside = X0 + i < lw && Y0 + j < lh;
                const uint32_t q = inside ? (Y0 + j) * lw + (X0 + i) : Y0 * lw + X0;
                const float b = (j ? fy : 1.f - fy) * (i ? fx : 1.f - fx);
                const bool better = inside && b > best;
                best = better ? b : best;
                anchor = better ? q : anchor;
                const float4 gq = glo[q];
                const float *cq = a.low + (size_t)q * 5;
                const float c0 = cq[0], c1 = cq[1], c2 = cq[2];
                const float d = guide_normal_weight<M>(gp, gq, a.squarings);
                float num, g;
                guide_depth_terms(b, d, gp, gq, hitp, isz, num, g);
                const float w = num / g;
                const bool ok = tap_counts(inside, gq, hitp, w);
                sum0 = ok ? sum0 + w * c0 : sum0;
                sum1 = ok ? sum1 + w * c1 : sum1;
                sum2 = ok ? sum2 + w * c2 : sum2;
                sumw = ok ? sumw + w : sumw;
            }
        }
        const float *la = a.low + (size_t)anchor * 5;
        const float l0 = la[0], l1 = la[1], l2 = la[2], l3 = la[3], l4 = la[4];
        const bool any = sumw > 0.f;
        float *o = s_px + threadIdx.x * 5;
        o[0] = any ? sum0 / sumw : l0;
        o[1] = any ? sum1 / sumw : l1;
        o[2] = any ? sum2 / sumw : l2;
        o[3] = l3, o[4] = l4;  // alpha, depth: the anchor's bits
        if (a.rgba8) ((uchar4 *)a.rgba8)[p] = quantized_pixel(o);
    }
    if (!a.out_rgbaz) return;
    __syncthreads();
    tile_store_rgbaz(s_px, a.out_rgbaz, W, H, tile.bx0, tile.by0);
}

int launch_upsample(const UpsamplePass &a, void *stream) {
    return launch_image(for_squarings(a.squarings, [](auto m) { return k_upsample<decltype(m)::value>; }), a, stream);
}
