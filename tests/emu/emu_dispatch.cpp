// emu_dispatch.cpp — TEST INFRASTRUCTURE: the dispatch rules of the two batch calls (rust-lz-fear_amd/csrc/lzf_dispatch.h) compiled
// with g++ for the CPU tests of tests/test_dispatch_cpu.py.  The product never loads it.
#include <cstdint>
#include "../../rust-lz-fear_amd/csrc/lzf_dispatch.h"

namespace d = lzf_dispatch;

namespace {
// kn (may be NULL = the product's defaults): [0] seg mode, [1] fed mode, [2] fed_min_in, [3] fed_open, [4] groups, [5..8] per cent per group,
// [9] decompress order, [10] compress order, [11] compress kernel, [12] team_max + 1 (0: default); ~0 in [0..2] and [9..11] leaves the default
d::Knobs knobs_of(const uint32_t* kn) {
    d::Knobs k;
    if (!kn) return k;
    if (kn[0] != ~0u) k.seg = kn[0];
    if (kn[1] != ~0u) k.fed = kn[1];
    if (kn[2] != ~0u) k.fed_min_in = kn[2];
    k.fed_open = kn[3] != 0u;
    k.seg_group_n = kn[4];
    for (int i = 0; i < 4; ++i) k.seg_group_pct[i] = kn[5 + i];
    if (kn[9] != ~0u) k.decompress_order = kn[9];
    if (kn[10] != ~0u) k.compress_order = kn[10];
    if (kn[11] != ~0u) k.compress_kernel = kn[11];
    if (kn[12]) k.team_max = (long)kn[12] - 1;
    return k;
}
d::Geometry geo_of(uint32_t cu, uint32_t lds) { d::Geometry g; g.cu = cu; g.lds = lds; return g; }
}  // namespace

extern "C" {
// out: want_order, try_seg, seg_min_in, seg_ring, groups, size[4], try_fed, last, seg_class;  strs: the launch strings of the three outcomes
void lzf_emu_decompress_plan(uint32_t cu, uint32_t lds, const uint32_t* kn, uint32_t n, uint64_t max_in, uint32_t* out, const char** strs) {
    const d::DecompressPlan p = d::decompress_plan(geo_of(cu, lds), knobs_of(kn), n, max_in);
    out[0] = p.want_order; out[1] = p.try_seg; out[2] = p.seg_min_in; out[3] = p.seg_ring; out[4] = p.groups.n;
    for (int i = 0; i < 4; ++i) out[5 + i] = p.groups.size[i];
    out[9] = p.try_fed; out[10] = p.last; out[11] = p.seg_class;
    strs[0] = p.seg_launch; strs[1] = p.fed_launch; strs[2] = p.last_launch;
}
// out: kinds, use_compact, use_team, fresh_only, want_order, general_skip
const char* lzf_emu_compress_plan(uint32_t cu, uint32_t lds, const uint32_t* kn, uint32_t n, uint32_t kinds, uint32_t* out) {
    const d::CompressPlan p = d::compress_plan(geo_of(cu, lds), knobs_of(kn), n, kinds);
    out[0] = p.kinds; out[1] = p.use_compact; out[2] = p.use_team; out[3] = p.fresh_only; out[4] = p.want_order; out[5] = p.general_skip;
    return p.launch;
}
// out: max_in, maxch, maxtile, rec_cap, the eleven offsets in the order they are taken, total
void lzf_emu_seg_layout(uint32_t n, uint64_t max_in, uint64_t* out) {
    const d::SegLayout l = d::seg_layout(n, max_in);
    const uint64_t v[16] = {l.d.max_in, l.d.maxch, l.d.maxtile, l.rec_cap, l.o_st, l.o_top, l.o_xexit, l.o_vfrom, l.o_tile_tok, l.o_tile_out, l.o_bits, l.o_recs,
                            l.o_order, l.o_by_len, l.o_est, l.total};
    for (int i = 0; i < 16; ++i) out[i] = v[i];
}
// out: max_in, maxch, maxtile, the five offsets, total
void lzf_emu_fed_layout(uint32_t n, uint64_t max_in, uint64_t* out) {
    const d::FedLayout l = d::fed_layout(n, max_in);
    const uint64_t v[9] = {l.d.max_in, l.d.maxch, l.d.maxtile, l.o_st, l.o_top, l.o_bits, l.o_ticket, l.o_state, l.total};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
}
const char* lzf_emu_launch_variant(void) { return d::kLaunchVariant; }
}
