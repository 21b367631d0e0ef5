// emu_fed_window.cpp — TEST INFRASTRUCTURE: the window loop of the bitmap-fed decompress kernel (lz4_decompress_fed.hip with
// lz4_decompress_feed_phase.inc and the batch loop of lz4_decompress_batch_phase.inc under LZF_FED_DECODE) on the CPU, over the
// window rules the kernel itself compiles (rust-lz-fear_amd/csrc/lzf_fed_window.h).  No bytes are copied: the emulator lists and
// verifies tokens and forms batches exactly as the kernel does, and checks what the rules have to guarantee:
//   * every pass of the loop makes progress (runs a batch, or asks for walk mode once);
//   * every token of the block's true chain is put into a batch exactly once, in order, and nothing else is;
// and it counts batches and windows, so that the chain-following windows can be set against the fixed rounds they replace.
// The bit map is made the way the hop parse leaves it: every 16 KiB chunk (chunks overlap by 2 KiB) walked from its own first byte.
//   g++ -O2 -std=c++17 -fPIC -shared -o libemu_fed_window.so tests/emu/emu_fed_window.cpp
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../rust-lz-fear_amd/csrc/lzf_fed_window.h"

namespace {

constexpr uint32_t kRing = 4096, kSpanMax = kRing / 3, kTokCap = 352, kTotClamp = 1u << 25;

struct Tok { uint32_t L, M, next; bool bad; };

// decompress.rs:61-71 without the copies: the token at p (p < len)
Tok decode(const uint8_t* in, uint32_t len, uint32_t p) {
    Tok t{0, 0, len, false};
    const uint32_t tok = in[p];
    uint32_t q = p + 1, L = tok >> 4;
    if (L == 15) { uint32_t b; do { if (q >= len) { t.bad = true; return t; } b = in[q++]; L += b; if (L > (1u << 30)) L = 1u << 30; } while (b == 255); }
    if (len - q < L) { t.bad = true; return t; }
    q += L; t.L = L;
    if (len - q < 2) return t;                       // the last literals
    q += 2;
    uint32_t M = tok & 15;
    if (M == 15) { uint32_t b; do { if (q >= len) { t.bad = true; return t; } b = in[q++]; M += b; if (M > (1u << 30)) M = 1u << 30; } while (b == 255); }
    t.M = M + 4; t.next = q;
    return t;
}

}  // namespace

// stats: [0] batches, [1] windows listed from the map, [2] windows walked, [3] sequences, [4] batches of fewer than 32 sequences,
//        [5] batches carried (left for the next window), [6] solo sequences, [7] true tokens of the block
// drop_chunk >= 0: that chunk's row of the bit map is cleared (a map that is wrong: the walk has to serve its share).
// log (optional, log_cap pairs): what the loop did, in order, as (kind, position) pairs — 0: a window listed from the map at cstart,
//        1: a window walked at cstart, 2: a batch left for the next window, its first token's position; *n_log = pairs that occurred.
// Returns 0: the block went through; 1: the chain itself fails (the kernel leaves the job to the pair kernel);
//        -1: a pass of the loop made no progress; -2: a batch took something that is not the next true token;
//        -3: true tokens were left out; -4: the block is not valid (the true chain cannot be walked).
extern "C" int lzf_emu_fed_window(const uint8_t* in, uint32_t len, int fixed, uint32_t carry, int drop_chunk, uint64_t* stats,
                                  uint32_t* log, uint32_t log_cap, uint32_t* n_log) {
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    uint32_t nl = 0;
    auto note = [&](uint32_t kind, uint32_t pos) { if (log && nl < log_cap) { log[2 * nl] = kind; log[2 * nl + 1] = pos; } ++nl; if (n_log) *n_log = nl; };
    if (n_log) *n_log = 0;
    if (len == 0) return 0;
    // ---- the true chain
    std::vector<uint32_t> truth;
    for (uint32_t p = 0; p < len;) { const Tok t = decode(in, len, p); if (t.bad) return -4; truth.push_back(p); p = t.next; }
    stats[7] = truth.size();
    // ---- the bit map: one row per chunk, the chain from the chunk's first byte
    const uint32_t nch = len <= (uint32_t)kFedwChunk ? 1u : 1u + (len - kFedwChunk + kFedwStride - 1u) / kFedwStride;
    const uint32_t words = kFedwChunk / 32;
    std::vector<uint32_t> bits((size_t)nch * words, 0u);
    for (uint32_t h = 0; h < nch; ++h) {
        if ((int)h == drop_chunk) continue;
        const uint32_t base = h * kFedwStride, end = base + kFedwChunk;
        for (uint32_t p = base; p < len && p < end;) {
            bits[(size_t)h * words + ((p - base) >> 5)] |= 1u << ((p - base) & 31u);
            const Tok t = decode(in, len, p);
            p = t.bad ? len : t.next;
        }
    }
    // ---- the window loop
    uint32_t expect = 0, taken = 0;
    bool walk = false;
    std::vector<uint16_t> toks(kTokCap);
    while (expect < len) {
        const uint32_t expect_in = expect;
        const uint32_t cstart = lzf_fedw_start(expect, fixed);
        uint32_t tc = 0;
        bool bail = false;
        ++stats[walk ? 2 : 1];
        note(walk ? 1u : 0u, cstart);
        if (!walk) {
            for (uint32_t lane = 0; lane < kFedwRound / 32 && !bail; ++lane) {
                const uint32_t wpos = cstart + lane * 32u;
                if (wpos >= len) break;
                const uint32_t h = lzf_fedw_chunk(wpos);
                if (h >= nch || lzf_fedw_word(wpos, h) >= words) return -2;
                uint32_t w = bits[(size_t)h * words + lzf_fedw_word(wpos, h)];
                if (expect >= wpos + 32u) w = 0u; else if (expect > wpos) w &= ~((1u << (expect - wpos)) - 1u);
                if (len - wpos < 32u) w &= (1u << (len - wpos)) - 1u;
                for (; w; w &= w - 1u) { if (tc >= kTokCap) { bail = true; break; } toks[tc++] = (uint16_t)(lane * 32u + (uint32_t)__builtin_ctz(w)); }
            }
            if (tc == 0) bail = true;
            if (bail) tc = 0;
        } else {
            for (uint32_t p = expect; p - cstart < (uint32_t)kFedwRound && p < len && tc < kTokCap;) {
                toks[tc++] = (uint16_t)(p - cstart);
                const Tok t = decode(in, len, p);
                if (t.bad) { bail = true; break; }
                p = t.next;
            }
            if (tc == 0) bail = true;
        }
        // ---- batches
        uint32_t tidx = 0;
        while (!bail && tidx < tc) {
            if (lzf_fedw_carry(tc, tidx, cstart + kFedwRound, len, fixed ? 0u : carry)) { ++stats[5]; note(2u, cstart + toks[tidx]); break; }
            const uint32_t nb_try = tc - tidx < (uint32_t)kFedwLanes ? tc - tidx : (uint32_t)kFedwLanes;
            uint32_t prev = expect, incl = 0, nb = nb_try, last_next = expect;
            std::vector<uint32_t> nexts(nb_try);
            for (uint32_t j = 0; j < nb_try; ++j) {
                const uint32_t tp = cstart + toks[tidx + j];
                const Tok t = decode(in, len, tp);
                if (t.bad || tp != prev) { bail = true; break; }             // the chain's links, before anything is written
                prev = t.next; nexts[j] = t.next;
                uint32_t tot = t.L + t.M; if (tot > kTotClamp) tot = kTotClamp;
                incl += tot;
                if (incl > kSpanMax && nb == nb_try) nb = j;
            }
            if (bail) break;
            const uint32_t n_seq = nb ? nb : 1u;                             // nb == 0: one solo sequence
            for (uint32_t j = 0; j < n_seq; ++j) {
                if (taken >= truth.size() || truth[taken] != cstart + toks[tidx + j]) return -2;
                ++taken;
            }
            last_next = nexts[n_seq - 1u];
            expect = last_next;
            ++stats[0]; stats[3] += n_seq;
            if (nb == 0) ++stats[6];
            if (n_seq < 32u) ++stats[4];
            tidx += n_seq;
        }
        if (bail) {
            if (walk) return 1;
            walk = true; continue;
        }
        walk = false;
        if (expect == expect_in) return -1;
    }
    return taken == truth.size() ? 0 : -3;
}
