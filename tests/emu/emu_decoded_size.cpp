// emu_decoded_size.cpp — TEST INFRASTRUCTURE: the size rules (rust-lz-fear_amd/csrc/lzf_size_rules.h) compiled with g++ and
// driven token by token for the CPU tests of tests/test_decoded_size_cpu.py.  The product never loads it.
#include <cstdint>
#include "../../rust-lz-fear_amd/csrc/lzf_size_rules.h"

extern "C" {
// decompress_raw's status and, when it is 0, output.len() in *out_len — no output byte is produced
int lzf_emu_decoded_size(const uint8_t* in, uint64_t len64, uint64_t prefix_len, uint64_t existing, uint64_t output_limit,
                         uint64_t* out_len) {
    const uint32_t len = (uint32_t)len64;
    auto rd1 = [&](uint32_t p) -> uint32_t { return in[p]; };
    auto rd4 = [&](uint32_t p) -> uint32_t {
        uint32_t v = 0;
        for (uint32_t i = 0; i < 4u && p + i < len; ++i) v |= (uint32_t)in[p + i] << (8u * i);
        return v;
    };
    auto ffrun = [&](uint32_t p) -> uint32_t { uint32_t n = 0; while (p + n < len && in[p + n] == 255u) ++n; return n; };
    uint64_t pos = existing;
    uint32_t tp = 0;
    while (tp < len) {
        lzf_size::Seq s;
        uint32_t next;
        if (!lzf_size::decode_token(tp, len, rd4, rd1, ffrun, s, next)) return lzf_size::UNEXPECTED_END;
        if (s.has) {
            const int code = lzf_size::check(pos + s.L, s.M, s.off, prefix_len, output_limit);
            if (code != lzf_size::OK) return code;
        }
        pos = lzf_size::advance(pos, s);
        tp = next;
    }
    *out_len = pos;
    return lzf_size::OK;
}
}
