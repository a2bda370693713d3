// pass_schedule.h — the pure decisions of the render host loop (api_render.inc: render_pass): how many samples a pass
// takes and the form it runs in.  Host only, plain C++, no HIP call: arithmetic on a handful of integers, which
// tests/cpp/pass_schedule_test.cpp runs without a GPU (tests/test_pass_schedule.py).
#pragma once
#include <algorithm>
#include <cstdint>

#include "vmx_device.h"  // FrameDev: kmax, quarter, nmin, early_stop

namespace vmx {

// passes below this many path slots run in the fused kernel (no per-generation launches): 4 M (1, 16 and 64 M were
// all slower on early-stop frames in round 1; a full 7.4 M-path pass takes 5.1 ms fused, 3.6 ms split).  The passes
// that FOLLOW the first one of an early-stop frame are different: many slots, few of them valid (pixels that stopped
// a stratum take 3 of up to 1024) — they run fused up to 32 M slots (round 3: 13.6 -> 12.9 ms before the pass merge)
constexpr uint64_t kHybridPaths = 4ull << 20, kHybridLeftover = 32ull << 20;

// the schedule's state between passes
struct PassSchedule {
    uint32_t n_uniform = 0;  // samples every active pixel has taken while no early stop was possible
    uint32_t k_fixed = 0;    // fixed-spp mode: samples issued so far
    // a progressive handle after its first selected step (api_sampling.inc): its pixels hold different counts, k_fixed means
    // nothing any more, a pass takes min(smax, cap) samples and the kernels' k < kmax clipping ends each pixel on its own
    bool ragged = false;
    uint64_t last_pass_pixels = 0, last_pass_breaks = 0;  // early-stop statistics of the previous pass
};

struct PassPlan {
    uint32_t S;     // samples per active pixel
    uint32_t lead;  // FrameDev::lead of the pass
    bool finished;  // a fixed-count frame has issued all its samples: no pass (S = 0)
};

// The next pass of a frame: every active pixel takes up to S samples, never above `cap` (a progressive step's remaining
// allowance; 0xFFFFFFFF: none).  smax: the most a pass takes, smax_alloc: what the buffers are sized for, per pixel of
// the n_pad_max padded slots.  Advances n_uniform / k_fixed; the caller files the pass's feedback in last_pass_*.
inline PassPlan plan_pass(PassSchedule &st, const FrameDev &fr, uint32_t smax, uint32_t smax_alloc, uint32_t n_active,
                          uint32_t n_pad_max, uint32_t cap) {
    PassPlan p{0, 0, false};
    if (fr.early_stop) {
        // no sample can trigger the early-stop rule before n = nmin+1 (pathtracer.cpp:292):
        // up to there whole groups of samples are issued without speculation, after that one at a time
        if (st.n_uniform < fr.nmin + 1 && st.n_uniform < fr.kmax) {
            p.S = std::min({fr.nmin + 1 - st.n_uniform, smax, fr.kmax - st.n_uniform, cap});
            st.n_uniform += p.S;
            // Most pixels stop on the first test (sample nmin) and then on the first sample of every
            // following stratum: when the whole group fits in one pass, those first samples ride
            // along in it (sample_index / k_resolve), which saves a pass (measured 20.0 -> 17.5 ms)
            const uint32_t strata_after = fr.quarter ? fr.kmax / fr.quarter - 1u : 0u;
            if (p.S == fr.nmin + 1 && p.S <= fr.quarter && strata_after > 0 && p.S + strata_after <= std::min(smax, cap)) {
                p.lead = p.S;
                p.S += strata_after;
            }
        } else {
            // Past that point a pixel may stop after any sample.  While most pixels are still
            // active one sample per pass is issued (nothing speculative); once the active set is
            // small, many samples per pixel are issued at once and k_resolve discards what
            // follows an early stop (same frame, fewer launch-bound passes).  Pixels that keep
            // sampling almost never stop later, so the speculation is deep (up to 8 M paths).
            // Speculation only pays for pixels that keep sampling: it is used when fewer than
            // 1 in 8 of the active pixels stopped a stratum in the previous pass.
            constexpr uint64_t spec = 16ull << 20, spec_cap = 1024;  // measured: 45 ms -> 31 ms vs (1 M, 16)
            // A pixel that has just stopped a stratum gets the first samples of all following
            // strata in one pass (sample_index in the kernels): 3 paths cover it to the end of
            // the frame if it keeps stopping, as most do (measured: 6 -> 4 passes, 26 -> 21 ms).
            p.S = std::max(1u, fr.kmax / std::max(fr.quarter, 1u) - 1u);
            // ... or when so few pixels are left that a pass of everything they can still take is small anyway (the
            // Sponza stand-in: 4,492 of 2 M pixels after the first pass — a pass of 3 paths each was an empty launch
            // chain of ~1 ms before the one that finished them; 13.8 -> 12.1 ms)
            if ((st.last_pass_pixels > 0 && st.last_pass_breaks * 8 < st.last_pass_pixels) || (uint64_t)n_active * 2 * spec_cap <= spec)
                p.S = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, spec / (2ull * n_active)), spec_cap);
            p.S = (uint32_t)std::min<uint64_t>(p.S, ((uint64_t)n_pad_max * smax_alloc) / ((n_active + 63u) & ~63u));
            p.S = std::max(std::min(p.S, cap), 1u);
        }
    } else if (st.ragged) {
        p.S = std::min(smax, cap);  // (the run ends when its list is empty: render_run)
    } else if (st.k_fixed >= fr.kmax) {
        p.finished = true;
    } else {
        p.S = std::min({smax, fr.kmax - st.k_fixed, cap});
        st.k_fixed += p.S;
    }
    return p;
}

// the form a pass runs in
enum class PassForm {
    Nee,       // light sampling: k_nee, whatever the pipeline
    Split,     // the split wavefront: pipeline 4, and pipeline 0 from kHybridPaths path slots on
    Fused,     // k_paths: pipeline 1, and the smaller passes of pipeline 0
    FirstGen,  // pipelines 2 and 3: the first-generation kernels (A/B library)
};

// slots: the pass's path slots, n_pad * S; frame_passes: passes of the frame before this one
inline PassForm pass_form(bool nee, uint32_t pipeline, uint64_t slots, bool early_stop, uint64_t frame_passes) {
    if (nee) return PassForm::Nee;
    if (pipeline == 4) return PassForm::Split;
    if (pipeline == 1) return PassForm::Fused;
    if (pipeline != 0) return PassForm::FirstGen;
    return slots >= ((early_stop && frame_passes > 0) ? kHybridLeftover : kHybridPaths) ? PassForm::Split : PassForm::Fused;
}

}  // namespace vmx
