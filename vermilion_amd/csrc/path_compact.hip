// path_compact.hip — order-preserving compaction of the camera paths that have to be traced (VMX_SAMPLING_ELIDE_DEAD).
//
// k_raygen<1> decides per path whether its radiance is provably zero (vmx_kernels.hip: step_is_dead) and leaves,
// per wave of 64 consecutive path ids, one word of live bits and its popcount.  Here: exclusive scan of the popcounts
// (hipcub), then every live path id is written to its place — neighbours stay neighbours, so a traversal wave still
// holds samples of one pixel (or of a few neighbouring ones).
// The same scan serves a pass that fuses its claimed pixels (k_slot_scatter): the ordered lists of the pass's unclaimed
// and claimed slots from one word of "unclaimed" bits per 64 slots.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "vmx_kernels.h"

namespace vmx {
namespace {

__global__ void __launch_bounds__(256)
k_live_scatter(const unsigned long long *__restrict__ live_mask, const unsigned int *__restrict__ offs, uint32_t nwords,
               unsigned int *__restrict__ ids, unsigned int *__restrict__ count) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < nwords; w += waves) {
        const unsigned long long bits = live_mask[w];
        const uint32_t off = offs[w];
        if ((bits >> lane) & 1ull) ids[off + (uint32_t)__popcll(bits & ((1ull << lane) - 1ull))] = w * 64u + lane;
        if (w + 1 == nwords && lane == 0) *count = off + (uint32_t)__popcll(bits);
    }
}

// the two ordered lists of a pass that fuses its claimed pixels: of the slots below n_active, those whose bit is set
// (offs: the exclusive scan of the words' popcounts) and the others — the claimed ones, whose rank is what is left of
// the slot's index
__global__ void __launch_bounds__(256)
k_slot_scatter(const unsigned long long *__restrict__ mask, const unsigned int *__restrict__ offs, uint32_t nwords, uint32_t n_active,
               unsigned int *__restrict__ set_ids, unsigned int *__restrict__ clear_ids, unsigned int *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < nwords; w += waves) {
        const unsigned long long bits = mask[w];
        const uint32_t off = offs[w], slot = w * 64u + lane;
        const uint32_t before = off + (uint32_t)__popcll(bits & ((1ull << lane) - 1ull));  // set bits below this slot
        if ((bits >> lane) & 1ull) set_ids[before] = slot;
        else if (slot < n_active) clear_ids[slot - before] = slot;
        if (w + 1 == nwords && lane == 0) {
            const uint32_t n_set = off + (uint32_t)__popcll(bits);
            counts[0] = n_set, counts[1] = n_active - n_set;
        }
    }
}

// a pixel list compacted in order (a progressive handle's master list by a selection map, or by "still takes samples"):
// slot i of `src` goes to its rank among the set bits
__global__ void __launch_bounds__(256)
k_list_scatter(const unsigned long long *__restrict__ mask, const unsigned int *__restrict__ offs, uint32_t nwords,
               const unsigned int *__restrict__ src, unsigned int *__restrict__ dst, unsigned int *__restrict__ count) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < nwords; w += waves) {
        const unsigned long long bits = mask[w];
        const uint32_t off = offs[w];
        // (a set bit is a slot below the list's length: launch_list_words)
        if ((bits >> lane) & 1ull) dst[off + (uint32_t)__popcll(bits & ((1ull << lane) - 1ull))] = src[w * 64u + lane];
        if (w + 1 == nwords && lane == 0) *count = off + (uint32_t)__popcll(bits);
    }
}

// a budgeted step's sample counts, one per slot of its pixel list and one behind the last: what the step's items are
// scanned from.  *len is the list's length on the device (launch_list_compact); slots at or past it count 0
__global__ void __launch_bounds__(256)
k_item_counts(const unsigned int *__restrict__ list, const unsigned int *__restrict__ len, uint32_t n_max,
              const unsigned int *__restrict__ budget, const unsigned int *__restrict__ cursor, uint32_t kmax, uint32_t B,
              unsigned int *__restrict__ cnt) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    if (slot > n_max) return;
    uint32_t c = 0;
    if (slot < n_max && slot < *len) {
        const uint32_t lp = list[slot];
        const uint32_t at = cursor[lp];
        c = min(min(budget[lp], B), at < kmax ? kmax - at : 0u);
    }
    cnt[slot] = c;
}

}  // namespace

size_t item_base_tmp_bytes(uint32_t n_max) {
    size_t bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (unsigned int *)nullptr, (unsigned int *)nullptr, (int)n_max + 1, nullptr);
    return bytes;
}

int launch_item_base(const unsigned int *list, const unsigned int *len, uint32_t n_max, const unsigned int *budget,
                     const unsigned int *cursor, uint32_t kmax, uint32_t B, unsigned int *cnt, unsigned int *base, void *tmp,
                     size_t tmp_bytes, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_item_counts, dim3((n_max + 1 + 255) / 256), dim3(256), 0, s, list, len, n_max, budget, cursor, kmax, B, cnt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return (int)hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cnt, base, (int)n_max + 1, s);
}

size_t live_compact_tmp_bytes(uint32_t nwords) {
    size_t bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (unsigned int *)nullptr, (unsigned int *)nullptr, (int)nwords, nullptr);
    return bytes;
}

int launch_live_compact(const unsigned long long *live_mask, const unsigned int *live_cnt, uint32_t nwords,
                        unsigned int *offs, unsigned int *ids, unsigned int *count, void *tmp, size_t tmp_bytes, uint32_t cus, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (nwords == 0) return (int)hipMemsetAsync(count, 0, 4, s);
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, live_cnt, offs, (int)nwords, s);
    if (e != hipSuccess) return (int)e;
    const uint32_t grid = strided_grid((nwords + 3) / 4, cus, 16);
    hipLaunchKernelGGL(k_live_scatter, dim3(grid), dim3(256), 0, s, live_mask, offs, nwords, ids, count);
    return (int)hipGetLastError();
}

int launch_slot_lists(const unsigned long long *mask, const unsigned int *cnt, uint32_t nwords, uint32_t n_active, unsigned int *offs,
                      unsigned int *unclaimed, unsigned int *claimed, unsigned int *counts, void *tmp, size_t tmp_bytes, uint32_t cus, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (nwords == 0) return (int)hipMemsetAsync(counts, 0, 8, s);
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cnt, offs, (int)nwords, s);
    if (e != hipSuccess) return (int)e;
    const uint32_t grid = strided_grid((nwords + 3) / 4, cus, 16);
    hipLaunchKernelGGL(k_slot_scatter, dim3(grid), dim3(256), 0, s, mask, offs, nwords, n_active, unclaimed, claimed, counts);
    return (int)hipGetLastError();
}

int launch_list_compact(const unsigned long long *mask, const unsigned int *cnt, uint32_t nwords, unsigned int *offs,
                        const unsigned int *src, unsigned int *dst, unsigned int *count, void *tmp, size_t tmp_bytes, uint32_t cus, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (nwords == 0) return (int)hipMemsetAsync(count, 0, 4, s);
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cnt, offs, (int)nwords, s);
    if (e != hipSuccess) return (int)e;
    const uint32_t grid = strided_grid((nwords + 3) / 4, cus, 16);
    hipLaunchKernelGGL(k_list_scatter, dim3(grid), dim3(256), 0, s, mask, offs, nwords, src, dst, count);
    return (int)hipGetLastError();
}

}  // namespace vmx
