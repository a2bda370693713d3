// Stand-alone driver of vermilion_amd/csrc/pass_schedule.h for tests/test_pass_schedule.py: runs the scripted passes it reads
// from stdin through plan_pass / pass_form and prints what they decide, one line per command.
//   frame <spp> <early_stop>                       the frame's numbers, as make_frame derives them; a new schedule state
//   job <smax> <smax_alloc> <n_pad_max> <pipeline> <nee> <ragged>
//   state <n_uniform> <k_fixed> <last_pass_pixels> <last_pass_breaks>
//   pass <n_active> <cap> <breaks>                 plans a pass: prints "S lead form", or "finished"; then files the
//                                                  pass's feedback (n_active pixels, `breaks` of them stopped a stratum)
//   form <nee> <pipeline> <slots> <early_stop> <frame_passes>      prints the form alone
// cap 0 stands for "no cap" (0xFFFFFFFF).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>

#include "pass_schedule.h"

using namespace vmx;

static const char *name(PassForm f) {
    switch (f) {
    case PassForm::Nee: return "nee";
    case PassForm::Split: return "split";
    case PassForm::Fused: return "fused";
    default: return "firstgen";
    }
}

int main() {
    FrameDev fr;
    std::memset(&fr, 0, sizeof(fr));
    PassSchedule st;
    uint32_t smax = 1, smax_alloc = 1, n_pad_max = 64, pipeline = 0;
    int nee = 0;
    uint64_t frame_passes = 0;
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "frame") {
            uint32_t spp;
            std::cin >> spp >> fr.early_stop;
            fr.spp = spp, fr.quarter = spp / 4, fr.kmax = 4 * (spp / 4);
            fr.nmin = (uint32_t)std::floor(std::sqrt((double)spp));
            st = PassSchedule{};
            frame_passes = 0;
        } else if (cmd == "job") {
            int ragged;
            std::cin >> smax >> smax_alloc >> n_pad_max >> pipeline >> nee >> ragged;
            st.ragged = ragged != 0;
        } else if (cmd == "state") {
            std::cin >> st.n_uniform >> st.k_fixed >> st.last_pass_pixels >> st.last_pass_breaks;
        } else if (cmd == "pass") {
            uint32_t n_active, cap;
            uint64_t breaks;
            std::cin >> n_active >> cap >> breaks;
            const PassPlan p = plan_pass(st, fr, smax, smax_alloc, n_active, n_pad_max, cap ? cap : 0xFFFFFFFFu);
            if (p.finished) {
                std::printf("finished\n");
                continue;
            }
            const uint64_t n_pad = (n_active + 63u) & ~63u;
            std::printf("%u %u %s\n", p.S, p.lead, name(pass_form(nee != 0, pipeline, n_pad * p.S, fr.early_stop != 0, frame_passes)));
            st.last_pass_pixels = n_active, st.last_pass_breaks = breaks;
            ++frame_passes;
        } else if (cmd == "form") {
            uint32_t f_nee, f_pipeline, f_early;
            uint64_t slots, passes;
            std::cin >> f_nee >> f_pipeline >> slots >> f_early >> passes;
            std::printf("%s\n", name(pass_form(f_nee != 0, f_pipeline, slots, f_early != 0, passes)));
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
        if (!std::cin) {
            std::fprintf(stderr, "bad arguments of %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
