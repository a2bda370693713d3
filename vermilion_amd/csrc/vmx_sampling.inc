// vmx_sampling.inc — adaptive sampling of a progressive handle: which pixels a step traces.  Included by vmx_kernels.hip
// (inside its namespace, after vmx_image.inc: the tile, luminance).  The arithmetic is stated in include/vermilion_hip.h and
// restated in tests/sampling_spec.py; with -ffp-contract=off every operation below rounds once, in the order written, `/`
// and sqrtf are correctly rounded and denormals are kept: bit for bit the restatement.
//
//   k_list_words       one lane per slot of a pixel list: the wave's ballot of "this slot's pixel stays" and its popcount,
//                      one word per 64 slots.  SELECT: the pixel is unfinished and its byte of the selection map is set (a
//                      selected step: the handle's master list -> the step's active list); else: the pixel is unfinished
//                      (after a step: the master list without the pixels that completed).  path_compact.hip scans the
//                      popcounts and scatters (launch_list_compact): the order of the list is kept, and with it the tile
//                      order that keeps camera waves coherent.
//   k_sampling_error   dense, one lane per local pixel: the relative standard error e of the pixel's mean luminance and the
//                      variance of that mean, from the handle's state (sums, m2, count).
//   k_sampling_select  one lane per pixel of an image_tile.  The block computes e for its 38 x 14 pixels (the tile and a
//                      halo of 3) straight from the state — 24 B per pixel — into one LDS plane (2128 B); a pixel outside
//                      the local image is staged as -1, which no threshold >= 0 lets through.  Then the window test over
//                      (2 * radius + 1)^2 taps, the map's byte, and the number of selected pixels by one atomic per wave.
//   k_list_words_budget, k_budget   budgeted steps of a light-sampled handle (stated in the header's "light sampling in
//                      progressive handles"; restated in tests/budget_spec.py): the word-map form of k_list_words, and the
//                      per-pixel sample budgets, staged and windowed as k_sampling_select.
constexpr float kSamplingNoEstimate = 3.402823466e+38f;  // e of a pixel with fewer than two samples

// (e, var) of one pixel; n its count, acc its (r, g, b sums, m2)
__device__ __forceinline__ float sampling_error(const float4 &acc, uint32_t n, float floor, float &var) {
    var = 0.f;
    if (n < 2) return kSamplingNoEstimate;
    const float fn = (float)n;
    const float m1 = luminance(acc.x, acc.y, acc.z) / fn;
    float v = acc.w / fn - m1 * m1;
    v = v > 0.f ? v : 0.f;  // (a NaN gives 0)
    var = v / (fn - 1.f);
    return sqrtf(var) / (fabsf(m1) + floor);
}

template <bool SELECT>
__global__ void __launch_bounds__(256)
k_list_words(const unsigned int *__restrict__ list, uint32_t n, const unsigned char *__restrict__ select,
             const unsigned int *__restrict__ cursor, uint32_t kmax, unsigned long long *__restrict__ mask,
             unsigned int *__restrict__ cnt) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;  // (the grid covers whole words: ceil(n / 64) * 64 slots at least)
    bool stays = false;
    if (slot < n) {
        const uint32_t lp = list[slot];
        stays = cursor[lp] < kmax;
        if (SELECT) stays = stays && select[lp] != 0;
    }
    const unsigned long long bits = __ballot(stays);
    if ((threadIdx.x & 63u) == 0 && slot < ((n + 63u) & ~63u)) {
        mask[slot >> 6] = bits;
        cnt[slot >> 6] = (uint32_t)__popcll(bits);
    }
}

__global__ void __launch_bounds__(256) k_sampling_error(SamplingPass a, float *__restrict__ error, float *__restrict__ variance) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.width * a.height) return;
    float var;
    const float e = sampling_error(((const float4 *)a.px.accum)[p], a.px.count[p], a.floor, var);
    if (error) error[p] = e;
    if (variance) variance[p] = var;
}

constexpr int kSelectHalo = 3;
constexpr uint32_t kSelectW = kFilterBX + 2 * kSelectHalo, kSelectH = kFilterBY + 2 * kSelectHalo, kSelectN = kSelectW * kSelectH;

__global__ void __launch_bounds__(kFilterBlock) k_sampling_select(SamplingPass a, unsigned char *__restrict__ select,
                                                                  unsigned int *__restrict__ count) {
    __shared__ float s_e[kSelectN];
    const uint32_t W = a.width, H = a.height;
    const ImageTile tile = image_tile(W, H);
    for (uint32_t i = threadIdx.x; i < kSelectN; i += kFilterBlock) {
        const uint32_t ry = i / kSelectW, rx = i - ry * kSelectW;
        const int qx = (int)(tile.bx0 + rx) - kSelectHalo, qy = (int)(tile.by0 + ry) - kSelectHalo;
        float e = -1.f;
        if ((uint32_t)qx < W && (uint32_t)qy < H) {
            const uint32_t q = (uint32_t)qy * W + (uint32_t)qx;
            float var;
            e = sampling_error(((const float4 *)a.px.accum)[q], a.px.count[q], a.floor, var);
        }
        s_e[i] = e;
    }
    __syncthreads();
    bool sel = false;
    if (tile.live) {
        const uint32_t p = tile.p;
        const uint32_t li = (threadIdx.x / kFilterBX + kSelectHalo) * kSelectW + (threadIdx.x & (kFilterBX - 1)) + kSelectHalo;
        const int r = (int)a.radius;  // (0..3: within the halo)
        bool above = false;
        for (int dy = -r; dy <= r; ++dy)
            for (int dx = -r; dx <= r; ++dx) above = above || s_e[(uint32_t)((int)li + dy * (int)kSelectW + dx)] > a.threshold;
        sel = a.px.cursor[p] < a.kmax && (a.px.count[p] < a.min_samples || above);
        select[p] = sel ? 1 : 0;
    }
    const unsigned long long bits = __ballot(sel);
    if (count && (threadIdx.x & 63u) == 0 && bits) atomicAdd(count, (unsigned int)__popcll(bits));
}

// k_list_words over a word map: the slot stays if its pixel is unfinished and has a budget (a budgeted step: the handle's
// master list -> the step's list).  A kernel of its own: the byte-map forms above stay what they compile to.
__global__ void __launch_bounds__(256)
k_list_words_budget(const unsigned int *__restrict__ list, uint32_t n, const unsigned int *__restrict__ budget,
                    const unsigned int *__restrict__ cursor, uint32_t kmax, unsigned long long *__restrict__ mask,
                    unsigned int *__restrict__ cnt) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    bool stays = false;
    if (slot < n) {
        const uint32_t lp = list[slot];
        stays = cursor[lp] < kmax && budget[lp] != 0;
    }
    const unsigned long long bits = __ballot(stays);
    if ((threadIdx.x & 63u) == 0 && slot < ((n + 63u) & ~63u)) {
        mask[slot >> 6] = bits;
        cnt[slot >> 6] = (uint32_t)__popcll(bits);
    }
}

// k_budget: one lane per pixel of an image_tile, staged as k_sampling_select stages its window.  E is the largest e of the
// window (x > E ? x : E from 0: a NaN never wins, and the -1 of a tap outside the image never does); a pixel whose E is
// above the threshold asks for the samples that bring its standard error down to it, n (E / threshold)^2 - n, within
// [1, cap].  budget[p] != 0 exactly where k_sampling_select writes 1.  The budgets' sum: a wave reduction, one atomic per
// wave.
__global__ void __launch_bounds__(kFilterBlock) k_budget(BudgetPass b, unsigned int *__restrict__ budget,
                                                         unsigned long long *__restrict__ total) {
    __shared__ float s_e[kSelectN];
    const SamplingPass &a = b.a;
    const uint32_t W = a.width, H = a.height;
    const ImageTile tile = image_tile(W, H);
    for (uint32_t i = threadIdx.x; i < kSelectN; i += kFilterBlock) {
        const uint32_t ry = i / kSelectW, rx = i - ry * kSelectW;
        const int qx = (int)(tile.bx0 + rx) - kSelectHalo, qy = (int)(tile.by0 + ry) - kSelectHalo;
        float e = -1.f;
        if ((uint32_t)qx < W && (uint32_t)qy < H) {
            const uint32_t q = (uint32_t)qy * W + (uint32_t)qx;
            float var;
            e = sampling_error(((const float4 *)a.px.accum)[q], a.px.count[q], a.floor, var);
        }
        s_e[i] = e;
    }
    __syncthreads();
    uint32_t out = 0;
    if (tile.live) {
        const uint32_t p = tile.p;
        const uint32_t n = a.px.count[p];
        if (a.px.cursor[p] < a.kmax) {
            uint32_t want = 0;
            if (n < a.min_samples) {
                want = a.min_samples - n;
            } else {
                const uint32_t li = (threadIdx.x / kFilterBX + kSelectHalo) * kSelectW + (threadIdx.x & (kFilterBX - 1)) + kSelectHalo;
                const int r = (int)a.radius;  // (0..3: within the halo)
                float E = 0.f;
                for (int dy = -r; dy <= r; ++dy)
                    for (int dx = -r; dx <= r; ++dx) {
                        const float x = s_e[(uint32_t)((int)li + dy * (int)kSelectW + dx)];
                        E = x > E ? x : E;
                    }
                if (E > a.threshold) {
                    const float fn = (float)n;
                    const float q = E / a.threshold;
                    const float t = (fn * q) * q;
                    const float d = ceilf(t) - fn;
                    want = d >= (float)b.cap ? b.cap : (d >= 1.f ? (uint32_t)d : 1u);
                }
            }
            const uint32_t room = n < a.kmax ? a.kmax - n : 0u;
            out = min(min(want, b.cap), room);
        }
        budget[p] = out;
    }
    const uint32_t sum = wave_sum(out);
    if (total && (threadIdx.x & 63u) == 0 && sum) atomicAdd(total, (unsigned long long)sum);
}

int launch_sampling_budget(const BudgetPass &b, unsigned int *budget, unsigned long long *total, void *stream) {
    if (b.a.width == 0 || b.a.height == 0) return 0;
    hipLaunchKernelGGL(k_budget, image_grid(b.a.width, b.a.height), dim3(kFilterBlock), 0, (hipStream_t)stream, b, budget, total);
    return launch_status();
}

int launch_list_words_budget(const unsigned int *list, uint32_t n, const unsigned int *budget, const unsigned int *cursor, uint32_t kmax,
                             unsigned long long *mask, unsigned int *cnt, void *stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_list_words_budget, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, list, n, budget, cursor, kmax, mask,
                       cnt);
    return launch_status();
}

int launch_list_words(const unsigned int *list, uint32_t n, const unsigned char *select, const unsigned int *cursor, uint32_t kmax,
                      unsigned long long *mask, unsigned int *cnt, void *stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(select ? k_list_words<true> : k_list_words<false>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, list,
                       n, select, cursor, kmax, mask, cnt);
    return launch_status();
}

int launch_sampling_error(const SamplingPass &a, float *error, float *variance, void *stream) {
    const uint32_t npix = a.width * a.height;
    if (npix == 0) return 0;
    hipLaunchKernelGGL(k_sampling_error, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, error, variance);
    return launch_status();
}

int launch_sampling_select(const SamplingPass &a, unsigned char *select, unsigned int *count, void *stream) {
    if (a.width == 0 || a.height == 0) return 0;
    hipLaunchKernelGGL(k_sampling_select, image_grid(a.width, a.height), dim3(kFilterBlock), 0, (hipStream_t)stream, a, select, count);
    return launch_status();
}
