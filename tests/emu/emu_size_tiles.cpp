// emu_size_tiles.cpp — TEST INFRASTRUCTURE: the tile rule of the size call's latency class (rust-lz-fear_amd/csrc/lzf_size_rules.h:
// TileSum, summarise, fold) compiled with g++ into a serial driver for tests/test_size_tiles_cpu.py.  The product never loads it.
#include <cstdint>
#include "../../rust-lz-fear_amd/csrc/lzf_size_rules.h"

extern "C" {
// The block's true tokens (decode_token from position 0 on) cut into tiles of `tile` compressed bytes by where they START, every
// tile summarised relative to its first token, the summaries folded.  Returns 1 = clean (*out_len = out_existing_len + total), 0 = not.
// sums (optional, room for len / tile + 1 entries of 4 words): the summaries, for the tests that look at them; *n_tiles their number.
int lzf_emu_size_tiles(const uint8_t* in, uint64_t len64, uint32_t tile, uint64_t prefix_len, uint64_t existing, uint64_t output_limit,
                       uint64_t* out_len, uint32_t* sums, uint32_t* n_tiles) {
    const uint32_t len = (uint32_t)len64;
    auto rd1 = [&](uint32_t p) -> uint32_t { return in[p]; };
    auto rd4 = [&](uint32_t p) -> uint32_t {
        uint32_t v = 0;
        for (uint32_t i = 0; i < 4u && p + i < len; ++i) v |= (uint32_t)in[p + i] << (8u * i);
        return v;
    };
    auto ffrun = [&](uint32_t p) -> uint32_t { uint32_t n = 0; while (p + n < len && in[p + n] == 255u) ++n; return n; };
    lzf_size::Fold f = lzf_size::fold_begin(existing);
    const uint32_t nt = tile ? (len + tile - 1u) / tile : (len ? 1u : 0u);
    uint32_t tp = 0;
    for (uint32_t t = 0; t < nt; ++t) {
        const uint64_t tend = tile ? (uint64_t)(t + 1u) * tile : (uint64_t)len;
        lzf_size::TileSum ts{0u, 0u, 0u, 0u};
        while (tp < len && tp < tend) {
            lzf_size::Seq s;
            uint32_t next;
            const bool ok = lzf_size::decode_token(tp, len, rd4, rd1, ffrun, s, next);
            lzf_size::summarise(ts, ts.sum, s, ok);
            tp = ok ? next : len;                  // (a token that does not decode ends the chain: its flag is all that counts)
        }
        if (sums) { sums[4u * t] = ts.sum; sums[4u * t + 1u] = ts.end; sums[4u * t + 2u] = ts.need; sums[4u * t + 3u] = ts.flags; }
        lzf_size::fold(f, ts, prefix_len, output_limit);
    }
    if (n_tiles) *n_tiles = nt;
    *out_len = f.base;
    return lzf_size::fold_end(f, existing) ? 1 : 0;
}
uint32_t lzf_emu_tile_len_clamp(void) { return lzf_size::kTileLenClamp; }
}
