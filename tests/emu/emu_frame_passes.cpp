// emu_frame_passes.cpp — TEST INFRASTRUCTURE: the pass planner of the frame layer (lzf_frame_jobs::split_passes,
// rust-lz-fear_amd/csrc/frame_jobs.h) compiled with g++ for the CPU tests of tests/test_frame_passes_cpu.py.  The product never
// loads it.
#include <cstdint>
#include <utility>
#include <vector>
#include "../../rust-lz-fear_amd/csrc/frame_jobs.h"

extern "C" {
// passes of need[0..n) under `budget`; group_end may be NULL.  Writes (first, second) of every pass to out[0..2 * max_passes) and
// returns the number of passes.
uint32_t lzf_emu_split_passes(const uint64_t* need, uint32_t n, uint64_t budget, const uint32_t* group_end, uint32_t* out, uint32_t max_passes) {
    std::vector<size_t> nd(need, need + n);
    std::vector<std::pair<uint32_t, uint32_t>> passes;
    passes.emplace_back(7u, 7u);            // (the planner clears what it is given)
    lzf_frame_jobs::split_passes(nd.data(), n, (size_t)budget, group_end, passes);
    for (size_t i = 0; i < passes.size() && i < max_passes; ++i) { out[2 * i] = passes[i].first; out[2 * i + 1] = passes[i].second; }
    return (uint32_t)passes.size();
}
}
