// emu_size_dispatch.cpp — TEST INFRASTRUCTURE: the size call's dispatch rule (rust-lz-fear_amd/csrc/lzf_dispatch.h: size_plan,
// size_layout) compiled with g++ for tests/test_size_tiles_cpu.py.  The product never loads it.
#include <cstdint>
#include "../../rust-lz-fear_amd/csrc/lzf_dispatch.h"

namespace d = lzf_dispatch;

extern "C" {
// kn: size_seg mode, size_seg_min_in, size_force (~0 in [0..1]: the product's default).  out: try_seg, min_in, by_len, last
void lzf_emu_size_plan(uint32_t cu, uint32_t lds, const uint32_t* kn, uint32_t n, uint64_t max_in, uint32_t* out, const char** strs) {
    d::Geometry g; g.cu = cu; g.lds = lds;
    d::Knobs k;
    if (kn[0] != ~0u) k.size_seg = kn[0];
    if (kn[1] != ~0u) k.size_seg_min_in = kn[1];
    k.size_force = kn[2];
    const d::SizePlan p = d::size_plan(g, k, n, max_in);
    out[0] = p.try_seg; out[1] = p.min_in; out[2] = p.by_len; out[3] = p.last;
    strs[0] = p.seg_launch; strs[1] = p.last_launch;
}
// out: max_in, maxch, maxtile, the six offsets in the order they are taken, total
void lzf_emu_size_layout(uint32_t n, uint64_t max_in, uint64_t* out) {
    const d::SizeLayout l = d::size_layout(n, max_in);
    const uint64_t v[10] = {l.d.max_in, l.d.maxch, l.d.maxtile, l.o_st, l.o_xexit, l.o_vfrom, l.o_tile_sum, l.o_bits, l.o_by_len, l.total};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
}
uint64_t lzf_emu_size_max_scratch(void) { return d::kSizeMaxScratch; }
}
