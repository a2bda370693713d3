// vmx_temporal.inc — temporal accumulation: the previous accumulated frame reprojected into the new camera through the
// new frame's G-buffer, stale history rejected by normal and plane distance, the new frame blended in (vmx_temporal_*).
// Included by vmx_kernels.hip (inside its namespace, after vmx_image.inc: the tile and its way through LDS).  The
// arithmetic is stated in include/vermilion_hip.h and restated in tests/temporal_spec.py; with -ffp-contract=off every
// operation below rounds once, in the order written, and `/` is the correctly rounded division with denormals kept: bit
// for bit the restatement.
//
//   k_temporal  one call, one lane per pixel of an image_tile.  The block's input pixels come in through LDS
//               (tile_load_rgbaz) and the output pixels leave through the same words (tile_store_rgbaz); alpha and depth
//               are never touched there, so they pass through bitwise, and a call in place reads a run before any lane
//               of the block replaces it.
//               The record is read as three float4s (as k_filter_guide reads it).  The state is three float4 planes,
//               (c_h.rgb, n_h) (n.xyz, z) (X.xyz, -): each of the four taps is three loads of 16 bytes per lane from the
//               old buffer, neighbouring lanes at neighbouring addresses wherever the reprojection is coherent; the new
//               state goes to the other buffer.  Miss, out-of-range and every skip rule are selects, not branches (a tap
//               that cannot count loads the lane's own pixel and is selected away); there are no transcendentals.
//               FIRST: the call after create or reset — it reads no state and no history camera.
//               MOTION: vmx_temporal_accumulate_motion_device with records — two more float4 loads per lane, (Xh, flags)
//               (nh, -) of vmx_motion.inc: the history is looked up where the surface point was (proj of Xh in the
//               previous camera) and tested against what was there (nh, Xh); without it Xh, nh are the record's own X, n_p
//               and the instantiation is the one there was before motion records.  A first call ignores them.
//               MOMENTS: vmx_temporal_accumulate_variance_device — a fourth state plane of float2 (m1, m2), the first and
//               second moment of the input's luminance: one float2 load per tap (same ok, same wt as the colour) and one
//               float2 store; k_variance (vmx_variance.inc) turns them into a variance.  Without it the instantiations
//               are the instruction streams they were before the parameter.
struct TemporalProj {
    float u, w;
    bool front;
};

__device__ __forceinline__ TemporalProj temporal_proj(const TemporalCam &cam, float X, float Y, float Z, float fw, float fh) {
    const float vx = X - cam.px, vy = Y - cam.py, vz = Z - cam.pz;
    const float c0 = (cam.m[0] * vx + cam.m[1] * vy) + cam.m[2] * vz;
    const float c1 = (cam.m[3] * vx + cam.m[4] * vy) + cam.m[5] * vz;
    const float c2 = (cam.m[6] * vx + cam.m[7] * vy) + cam.m[8] * vz;
    const float t = cam.film_dist / (-c2);
    TemporalProj r;
    r.u = ((c0 * t) / cam.sensor_x + 0.5f) * fw;
    r.w = ((-(c1 * t)) / cam.sensor_y + 0.5f) * fh;
    r.front = c2 < 0.f;
    return r;
}

template <bool FIRST, bool MOTION, bool MOMENTS = false>
__global__ void __launch_bounds__(kFilterBlock) k_temporal(TemporalPass a) {
    __shared__ float s_px[kFilterBlock * 5];
    const uint32_t W = a.width, H = a.height;
    const ImageTile tile = image_tile(W, H);
    const uint32_t x = tile.x, y = tile.y, p = tile.p;
    tile_load_rgbaz(s_px, a.in_rgbaz, W, H, tile.bx0, tile.by0);
    __syncthreads();
    if (tile.live) {
        float *v = s_px + threadIdx.x * 5;
        const float c0 = v[0], c1 = v[1], c2 = v[2];
        const float4 *r = (const float4 *)a.rayhit + (size_t)p * 4;  // (location, distance) (normal, tri_id) (uv, tri_t, flags)
        const float4 ra = r[0], rb = r[1], rc = r[2];
        const bool hit = (__float_as_uint(rc.w) & 1u) != 0;
        const size_t npix = (size_t)W * H;
        float o0 = c0, o1 = c1, o2 = c2, n_new = 1.f;
        const float lum = MOMENTS ? luminance(c0, c1, c2) : 0.f;
        float m1 = lum, m2 = lum * lum;
        if (!FIRST) {
            float Xhx = ra.x, Xhy = ra.y, Xhz = ra.z, mnx = rb.x, mny = rb.y, mnz = rb.z;
            if (MOTION) {
                const float4 *m = (const float4 *)a.motion + (size_t)p * 2;  // (prev_location, flags) (prev_normal, pad)
                const float4 ma = m[0], mb = m[1];
                Xhx = ma.x, Xhy = ma.y, Xhz = ma.z, mnx = mb.x, mny = mb.y, mnz = mb.z;
            }
            const float fw = (float)W, fh = (float)H;
            const TemporalProj pc = temporal_proj(a.cam, ra.x, ra.y, ra.z, fw, fh);
            const TemporalProj ph = temporal_proj(a.hist_cam, Xhx, Xhy, Xhz, fw, fh);
            const float gx = (float)x + (ph.u - pc.u);
            const float gy = (float)y + (ph.w - pc.w);
            // (false for NaN; a miss takes no tap at all)
            const bool inrange = hit && ph.front && gx >= -1.f && gx < fw && gy >= -1.f && gy < fh;
            const float x0 = floorf(gx), y0 = floorf(gy);
            const float fx = gx - x0, fy = gy - y0;
            const int x0i = (int)(inrange ? x0 : 0.f), y0i = (int)(inrange ? y0 : 0.f);
            const float zz = a.tol2 * (ra.w * ra.w);
            const float4 *old_c = (const float4 *)a.old_state, *old_g = old_c + npix, *old_x = old_g + npix;
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
                    const bool ok = inrange && inside && hg.w >= 0.f && d >= a.normal_min && pd * pd <= zz && wt > 0.f;
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
            const float t = nh + 1.f;
            const float n1 = t < a.max_history ? t : a.max_history;
            const float al = 1.f / n1;
            o0 = any ? h0 + (c0 - h0) * al : c0;
            o1 = any ? h1 + (c1 - h1) * al : c1;
            o2 = any ? h2 + (c2 - h2) * al : c2;
            n_new = any ? n1 : 1.f;
            if (MOMENTS) {
                const float g1 = summ1 / sumw, g2 = summ2 / sumw;
                m1 = any ? g1 + (lum - g1) * al : m1;
                m2 = any ? g2 + (lum * lum - g2) * al : m2;
            }
        }
        float4 *new_c = (float4 *)a.new_state, *new_g = new_c + npix, *new_x = new_g + npix;
        new_c[p] = make_float4(o0, o1, o2, n_new);
        new_g[p] = hit ? make_float4(rb.x, rb.y, rb.z, ra.w) : make_float4(0.f, 0.f, 0.f, -1.f);
        new_x[p] = make_float4(ra.x, ra.y, ra.z, 0.f);
        if (MOMENTS) ((float2 *)(new_x + npix))[p] = make_float2(m1, m2);
        v[0] = o0, v[1] = o1, v[2] = o2;  // (v[3], v[4]: alpha and depth, the input's bits)
        if (a.rgba8) ((uchar4 *)a.rgba8)[p] = quantized_pixel(v);
        if (a.history_len) a.history_len[p] = n_new;
    }
    if (!a.out_rgbaz) return;
    __syncthreads();
    tile_store_rgbaz(s_px, a.out_rgbaz, W, H, tile.bx0, tile.by0);
}

int launch_temporal(const TemporalPass &a, void *stream) {
    if (a.moments)
        return launch_image(a.first ? k_temporal<true, false, true> : a.motion ? k_temporal<false, true, true> : k_temporal<false, false, true>,
                            a, stream);
    return launch_image(a.first ? k_temporal<true, false> : a.motion ? k_temporal<false, true> : k_temporal<false, false>, a, stream);
}
