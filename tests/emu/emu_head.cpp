// emu_head.cpp — TEST INFRASTRUCTURE: the head rules (rust-lz-fear_amd/csrc/lzf_head_rules.h) compiled with g++; the serial
// reference function head_block driven over one job for tests/test_head_cases_cpu.py.  The product never loads it.
// The readers and the writer count every access outside input[0, len), prefix[0, prefix_len), out[0, out_cap) for reads and
// out[existing, out_cap) for writes: *outside must come back 0.
// `out` is handed in from position out_origin on (out[r] = out_tail[r - out_origin]), so that a job with more than a GiB of existing
// output can be stated over its last bytes; nothing below out_origin may be touched either.
// trim != 0: the job goes through lzf_history_trim.h first — lengths relative to the moved origin, the result restored — as
// lzf_history_trim_batch / lzf_history_restore_batch and the `_host` call do it.
#include <cstdint>
#include "../../rust-lz-fear_amd/csrc/lzf_head_rules.h"
#include "../../rust-lz-fear_amd/csrc/lzf_history_trim.h"

extern "C" {
int lzf_emu_head(const uint8_t* in, uint64_t len64, const uint8_t* prefix, uint64_t prefix_len, uint8_t* out_tail,
                 uint64_t out_origin, uint64_t existing, uint64_t out_cap, uint64_t output_limit, int trim, uint64_t* out_len,
                 uint64_t* outside, uint64_t* shift_out) {
    const uint32_t len = (uint32_t)len64;
    uint64_t bad = 0;
    const uint64_t shift = trim ? lzf_trim::shift_of(existing, out_cap) : 0;
    if (shift) {
        existing -= shift; out_cap -= shift;
        output_limit = lzf_trim::limit_of(output_limit, shift);
    }
    *shift_out = shift;
    auto rd1 = [&](uint32_t p) -> uint32_t { if (p >= len) { ++bad; return 0u; } return in[p]; };
    auto rd4 = [&](uint32_t p) -> uint32_t {
        uint32_t v = 0;
        for (uint32_t i = 0; i < 4u && p + i < len; ++i) v |= (uint32_t)in[p + i] << (8u * i);
        return v;
    };
    auto ffrun = [&](uint32_t p) -> uint32_t { uint32_t n = 0; while (p + n < len && in[p + n] == 255u) ++n; return n; };
    auto pre1 = [&](uint64_t k) -> uint32_t { if (k >= prefix_len) { ++bad; return 0u; } return prefix[k]; };
    // positions of the (trimmed) job -> the memory handed in
    auto out1 = [&](uint64_t r) -> uint32_t { if (r >= out_cap || r + shift < out_origin) { ++bad; return 0u; } return out_tail[r + shift - out_origin]; };
    auto put1 = [&](uint64_t r, uint32_t b) { if (r >= out_cap || r < existing || r + shift < out_origin) { ++bad; return; } out_tail[r + shift - out_origin] = (uint8_t)b; };
    const lzf_head::Result v = lzf_head::head_block(len64, rd4, rd1, ffrun, pre1, prefix_len, out1, put1, existing, out_cap, output_limit);
    lzf_job_result r{v.out_len, v.status, 0u};
    lzf_trim::restore(r, shift);
    *out_len = r.out_len;
    *outside = bad;
    return r.status;
}
}
