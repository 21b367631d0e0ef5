// emu_fed_window.cpp — TEST INFRASTRUCTURE: the window loop of the bitmap-fed decompress kernel (lz4_decompress_fed.hip with
// lz4_decompress_feed_phase.inc and the batch loop of lz4_decompress_batch_phase.inc under LZF_FED_DECODE) on the CPU, over the
// window rules the kernel itself compiles (rust-lz-fear_amd/csrc/lzf_fed_window.h).  No bytes are copied: the emulator lists and
// verifies tokens and forms batches exactly as the kernel does, and checks what the rules have to guarantee:
//   * every pass of the loop makes progress (runs a batch, or asks for walk mode once);
//   * every token of the block's true chain is put into a batch exactly once, in order, and nothing else is;
// and it counts batches and windows, so that the chain-following windows can be set against the fixed rounds they replace.
// The bit map is made the way the hop parse leaves it: every 16 KiB chunk (chunks overlap by 2 KiB) walked from its own first byte.
// lzf_emu_fed_pieces runs the same loop PIECE BY PIECE, as a launch that cuts its jobs does (the piece rules of lzf_fed_window.h): what
// every piece does and the state it parks for the next one.
//   g++ -O2 -std=c++17 -fPIC -shared -o libemu_fed_window.so tests/emu/emu_fed_window.cpp
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../rust-lz-fear_amd/csrc/lzf_fed_window.h"

namespace {

constexpr uint32_t kRing = 4096, kSpanMax = kRing / 3, kTokCap = 352, kTotClamp = 1u << 25;

struct Tok { uint32_t L, M, next, off; bool bad; };

// decompress.rs:61-71 without the copies: the token at p (p < len); off = its match offset (M != 0)
Tok decode(const uint8_t* in, uint32_t len, uint32_t p) {
    Tok t{0, 0, len, 0, false};
    const uint32_t tok = in[p];
    uint32_t q = p + 1, L = tok >> 4;
    if (L == 15) { uint32_t b; do { if (q >= len) { t.bad = true; return t; } b = in[q++]; L += b; if (L > (1u << 30)) L = 1u << 30; } while (b == 255); }
    if (len - q < L) { t.bad = true; return t; }
    q += L; t.L = L;
    if (len - q < 2) return t;                       // the last literals
    t.off = (uint32_t)in[q] | ((uint32_t)in[q + 1] << 8);
    q += 2;
    uint32_t M = tok & 15;
    if (M == 15) { uint32_t b; do { if (q >= len) { t.bad = true; return t; } b = in[q++]; M += b; if (M > (1u << 30)) M = 1u << 30; } while (b == 255); }
    t.M = M + 4; t.next = q;
    return t;
}

// what the copy stage checks of a sequence before it writes it (lz4_decompress_batch_phase.inc: "errors"; the solo sequence's checks come
// to the same): lo = the output position of its literals.  A job with any of these is left to the pair kernel.
struct Copy { bool on; uint32_t plen, cap; uint64_t limit; };
bool copy_error(const Copy& c, const Tok& t, uint32_t lo) {
    if (lo > c.cap || c.cap - lo < t.L) return true;
    if (!t.M) return false;
    const uint32_t mo = lo + t.L;
    return (uint64_t)mo + t.M > c.limit || t.off == 0u || (t.off > mo && t.off - mo > c.plen) || c.cap - mo < t.M;
}

// what a pass over [expect, piece_end) came to
enum { kParked = 1, kParkedAtOnce = 2, kFinished = 3, kWalkFailed = 4, kStatus = 5 };

struct Loop {
    const uint8_t* in = nullptr; uint32_t len = 0; int fixed = 0; uint32_t carry = 0; Copy copy{false, 0u, 0u, 0u};
    std::vector<uint32_t> truth;         // the positions of the true chain's tokens, as far as it can be walked
    bool truth_whole = true;
    std::vector<uint32_t> bits; uint32_t nch = 0, words = kFedwChunk / 32;
    uint32_t expect = 0, o = 0, taken = 0;
    uint64_t* stats = nullptr; uint32_t* log = nullptr; uint32_t log_cap = 0; uint32_t* n_log = nullptr; uint32_t nl = 0;
    std::vector<uint16_t> toks = std::vector<uint16_t>(kTokCap);

    void note(uint32_t kind, uint32_t pos) { if (log && nl < log_cap) { log[2 * nl] = kind; log[2 * nl + 1] = pos; } ++nl; if (n_log) *n_log = nl; }
    void prepare(int drop_chunk) {
        for (uint32_t p = 0; p < len;) { const Tok t = decode(in, len, p); if (t.bad) { truth_whole = false; break; } truth.push_back(p); p = t.next; }
        stats[7] = truth.size();
        // the bit map: one row per chunk, the chain from the chunk's first byte
        nch = len <= (uint32_t)kFedwChunk ? 1u : 1u + (len - kFedwChunk + kFedwStride - 1u) / kFedwStride;
        bits.assign((size_t)nch * words, 0u);
        for (uint32_t h = 0; h < nch; ++h) {
            if ((int)h == drop_chunk) continue;
            const uint32_t base = h * kFedwStride, end = base + kFedwChunk;
            for (uint32_t p = base; p < len && p < end;) {
                bits[(size_t)h * words + ((p - base) >> 5)] |= 1u << ((p - base) & 31u);
                const Tok t = decode(in, len, p);
                p = t.bad ? len : t.next;
            }
        }
    }
    // The window loop from the state (expect, o) up to piece_end (the kernel's loop with its `expect >= piece_end` at the head).
    // Returns one of the enum above, or -1: a pass made no progress; -2: a batch took something that is not the next true token;
    // -5: the piece took a token that starts a window or more behind its end.  counts: [0] windows listed, [1] windows walked, [2] batches.
    int run(uint32_t piece_end, uint32_t* counts) {
        bool walk = false, first = true;
        while (expect < len) {
            if (expect >= piece_end) return first ? kParkedAtOnce : kParked;
            first = false;
            const uint32_t expect_in = expect;
            const uint32_t cstart = lzf_fedw_start(expect, fixed);
            uint32_t tc = 0;
            bool bail = false;
            ++stats[walk ? 2 : 1]; ++counts[walk ? 1 : 0];
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
                uint32_t prev = expect, incl = 0, nb = nb_try;
                std::vector<Tok> dec(nb_try);
                for (uint32_t j = 0; j < nb_try; ++j) {
                    const uint32_t tp = cstart + toks[tidx + j];
                    const Tok t = decode(in, len, tp);
                    if (t.bad || tp != prev) { bail = true; break; }             // the chain's links, before anything is written
                    prev = t.next; dec[j] = t;
                    uint32_t tot = t.L + t.M; if (tot > kTotClamp) tot = kTotClamp;
                    incl += tot;
                    if (incl > kSpanMax && nb == nb_try) nb = j;
                }
                if (bail) break;
                const uint32_t n_seq = nb ? nb : 1u;                             // nb == 0: one solo sequence
                uint32_t lo = o;
                for (uint32_t j = 0; j < n_seq; ++j) {
                    const uint32_t tp = cstart + toks[tidx + j];
                    if (taken + j >= truth.size() || truth[taken + j] != tp) return -2;
                    if (tp >= piece_end && tp - piece_end >= (uint32_t)kFedwRound) return -5;
                    if (copy.on && copy_error(copy, dec[j], lo)) { expect = dec[n_seq - 1u].next; return kStatus; }      // (nothing of the batch is written; `expect` has moved, nobody reads it again)
                    lo += dec[j].L + dec[j].M;
                }
                taken += n_seq; o = lo;
                expect = dec[n_seq - 1u].next;
                ++stats[0]; ++counts[2]; stats[3] += n_seq;
                if (nb == 0) ++stats[6];
                if (n_seq < 32u) ++stats[4];
                tidx += n_seq;
            }
            if (bail) {
                if (walk) return kWalkFailed;
                walk = true; continue;
            }
            walk = false;
            if (expect == expect_in) return -1;
        }
        return kFinished;
    }
};

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
    if (n_log) *n_log = 0;
    if (len == 0) return 0;
    Loop lp;
    lp.in = in; lp.len = len; lp.fixed = fixed; lp.carry = carry;
    lp.stats = stats; lp.log = log; lp.log_cap = log_cap; lp.n_log = n_log;
    lp.prepare(drop_chunk);
    if (!lp.truth_whole) return -4;
    uint32_t counts[3] = {0, 0, 0};
    const int r = lp.run(len, counts);
    if (r < 0) return r;
    if (r == kWalkFailed) return 1;
    return lp.taken == lp.truth.size() ? 0 : -3;
}

// The same loop piece by piece: a job of `pieces` pieces (lzf_fedw_piece_end), each taking the state (expect, o) its predecessor parked.
// prefix_len, existing_len, limit, cap: the job's, for the copy stage's checks (a match offset of 0 or beyond the output, the limit, the
// capacity end the job for this kernel).  carry: the longest batch left for the next window.
// expire_piece >= 1: the hand-over wait of that piece runs out.  THE RULE OF THE EXPIRY PATH (lz4_decompress_fed.hip: `if (f != piece) continue`
// behind the bounded wait): the piece skips — nothing written, no flag set — so the flag never reaches what the pieces behind it wait for and
// they expire too; the job stays !done for the pair kernel and its flag stays what the last piece that ran left (never kFedEnded).
// rec: [pieces][8] = what, expect, o, windows listed, windows walked, batches, true tokens taken, the `expect` the piece took; what:
//        0 the ticket passes (the job ended in an earlier piece: flag kFedEnded),
//        1 took the state, ran at least a window and parked, 2 parked at once (no token of the chain in its range: the state it took),
//        3 finished the job, 4 failed in walk mode, 5 a copy-stage check failed, 6 its wait expired;
//        expect, o: what the piece parked (1, 2), else what it took.
// sum: [0] the piece that ended the job for this kernel (3, 4, 5; ~0: none did), [1] done (the kernel finished the job), [2] the flag
//        after all pieces (pieces finished, or 0x80000000 = kFedEnded; pieces == 1: 0, the kernel does not touch it), [3] true tokens taken.
// log: as above, and (3, p) where piece p starts to run (what 1 .. 5).
// Returns 0, or -1 / -2 / -5 as Loop::run; -3: the job was finished with true tokens left out, or a finished piece is followed by work.
extern "C" int lzf_emu_fed_pieces(const uint8_t* in, uint32_t len, uint32_t pieces, uint32_t carry, uint32_t prefix_len, uint32_t existing_len,
                                  uint64_t limit, uint32_t cap, int expire_piece, uint32_t* rec, uint32_t* sum, uint64_t* stats,
                                  uint32_t* log, uint32_t log_cap, uint32_t* n_log) {
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    if (n_log) *n_log = 0;
    sum[0] = ~0u; sum[1] = 0; sum[2] = 0; sum[3] = 0;
    if (len == 0 || pieces == 0) return -3;
    Loop lp;
    lp.in = in; lp.len = len; lp.carry = carry; lp.copy = Copy{true, prefix_len, cap, limit};
    lp.stats = stats; lp.log = log; lp.log_cap = log_cap; lp.n_log = n_log;
    lp.prepare(-1);
    lp.o = existing_len;
    bool ended = false, expired = false;
    uint32_t flag = 0;
    for (uint32_t p = 0; p < pieces; ++p) {
        uint32_t* r = rec + 8u * p;
        for (int i = 0; i < 8; ++i) r[i] = 0;
        r[1] = lp.expect; r[2] = lp.o; r[7] = lp.expect;
        if (ended) continue;                                         // (what 0)
        if (expired || (expire_piece >= 1 && (int)p == expire_piece)) { expired = true; r[0] = 6u; continue; }
        lp.note(3u, p);
        const uint32_t taken0 = lp.taken;
        const int w = lp.run(lzf_fedw_piece_end(len, pieces, p), r + 3);
        if (w < 0) return w;
        r[0] = (uint32_t)w; r[6] = lp.taken - taken0;
        if (w == kParked || w == kParkedAtOnce) {
            if (p + 1u == pieces) return -3;                         // (the last piece ends at len: it cannot park)
            r[1] = lp.expect; r[2] = lp.o; flag = p + 1u;
            continue;
        }
        ended = true; sum[0] = p;
        if (pieces > 1u) flag = 0x80000000u;
        if (w == kFinished) { if (lp.taken != lp.truth.size() || !lp.truth_whole) return -3; sum[1] = 1u; }
    }
    sum[2] = flag; sum[3] = lp.taken;
    return 0;
}

// the piece rules of lzf_fed_window.h, for the tests of the ticket map
extern "C" uint32_t lzf_emu_fedw_piece_end(uint32_t len, uint32_t pieces, uint32_t p) { return lzf_fedw_piece_end(len, pieces, p); }
extern "C" uint32_t lzf_emu_fedw_group_jobs(uint32_t n, uint32_t g, uint32_t ng) { return lzf_fedw_group_jobs(n, g, ng); }
extern "C" uint32_t lzf_emu_fedw_ticket_piece(uint32_t tk, uint32_t n_g) { return lzf_fedw_ticket_piece(tk, n_g); }
extern "C" uint32_t lzf_emu_fedw_ticket_rank(uint32_t tk, uint32_t piece, uint32_t n_g, uint32_t g, uint32_t ng) { return lzf_fedw_ticket_rank(tk, piece, n_g, g, ng); }
