// emu_verify_dispatch.cpp — TEST INFRASTRUCTURE: verify_plan and verify_layout (rust-lz-fear_amd/csrc/lzf_dispatch.h) compiled with g++
// for tests/test_verify_cases_cpu.py.  The product never loads it.
#include <cstdint>
#include "../../rust-lz-fear_amd/csrc/lzf_dispatch.h"

namespace d = lzf_dispatch;

extern "C" {
// mode: the analysis knob (0 by rule, else d::kForced / d::kOff as given).  out: try_seg, min_in, by_len;  strs: the two launch strings
void lzf_emu_verify_plan(uint32_t cu, uint32_t lds, uint32_t mode, uint32_t n, uint64_t max_in, uint32_t* out, const char** strs) {
    d::Geometry g; g.cu = cu; g.lds = lds;
    d::Knobs k;
    if (mode == 1u) k.verify_seg = d::kForced;
    if (mode == 2u) k.verify_seg = d::kOff;
    const d::VerifyPlan p = d::verify_plan(g, k, n, max_in);
    out[0] = p.try_seg; out[1] = p.min_in; out[2] = p.by_len;
    strs[0] = p.seg_launch; strs[1] = p.last_launch;
}
// out: the size layout's total, o_tile_base, o_job_min, total, maxtile
void lzf_emu_verify_layout(uint32_t n, uint64_t max_in, uint64_t* out) {
    const d::VerifyLayout l = d::verify_layout(n, max_in);
    out[0] = l.s.total; out[1] = l.o_tile_base; out[2] = l.o_job_min; out[3] = l.total; out[4] = l.s.d.maxtile;
    out[5] = d::size_layout(n, max_in).total;
}
}
