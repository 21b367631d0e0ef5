// lzf_verify_rules.h — "does this block decode to exactly these bytes?" without decoding, as __host__ __device__ code on top of
// lzf_size_rules.h: which output position of a sequence does not hold the expected byte, and the verdict of a whole job.
//
// The job is the decoder's (include/lzfear_hip.h): out[0, existing) is history, trusted as in the decode; out[existing, out_cap)
// holds the EXPECTED bytes; out is only read.  Against a known plaintext E there is no data dependence between sequences:
//   the decoder's output equals E on [0, p) exactly when for every position r < p a literal byte equals E[r] and a match byte
//   satisfies E[r] == E[r - off] (a source in front of out[0] comes from the prefix's tail);
//   if every position below r passes, decoded[r - off] == E[r - off], so the test at r is the decoder's own byte;
//   hence the first position that fails is the first position where the real decode differs from E — overlapping matches
//   (off < M) included, with no special case.
// Positions are sums of lengths, which the size rules give; so every sequence can be tested on its own, by any lane, in any order
// (lz4_verify.hip: lane j tests sequence j of a round, long runs go 16 bytes a lane over the whole wave), and the smallest failing
// position is the answer.  The status precedes the bytes: a block with a DecodeError reports that error whatever E holds, so the
// walk always runs to the block's end.  verify_block below is the one definition of the result; the CPU tests run it
// (tests/emu/emu_verify.cpp) against decode-then-compare by the oracle, and the kernel is held to it.
#ifndef LZF_VERIFY_RULES_H
#define LZF_VERIFY_RULES_H

#include "lzf_size_rules.h"

namespace lzf_verify {

enum : int { CONTRACT = 6, MISMATCH = 8 };            // LZF_CONTRACT, LZF_MISMATCH of include/lzfear_hip.h
constexpr uint64_t kNone = ~0ull;                     // "no position fails"
constexpr uint64_t kMaxLen = 0x7FFFFF00ull;           // the size call's contract (lzf_copy_helpers.h: kMaxPosB): lengths from here on are LZF_CONTRACT

// Where the literals of the token at `tp` start in the input: behind the token and the length bytes of L (15 + 255 n + last: n + 1 bytes).
LZF_SIZE_HD uint32_t literals_at(uint32_t tp, uint32_t L) { return tp + 1u + (L >= 15u ? (L - 15u) / 255u + 1u : 0u); }

// How many of the n bytes at output position r0 lie below out_cap: positions at or beyond out_cap are not compared (the length
// rule of conclude() speaks for them).
LZF_SIZE_HD uint64_t below_cap(uint64_t r0, uint64_t n, uint64_t out_cap) { return r0 >= out_cap ? 0ull : (n < out_cap - r0 ? n : out_cap - r0); }

// One sequence `s` that passed lzf_size::check, its first literal at output position `pos` (existing output included) and its
// literals at input position `lit_at`.  Readers: in1(p) the input byte at p, pre1(k) prefix[k], out1(r) out[r] (r < out_cap).
// Returns the first output position of the sequence whose byte is not the expected one, or kNone.  A match source that starts in
// the prefix and runs into out is followed across out[0].
template <class RI, class RP, class RO>
LZF_SIZE_HD uint64_t first_mismatch(const lzf_size::Seq& s, uint64_t pos, uint32_t lit_at, RI in1, RP pre1, RO out1,
                                    uint64_t prefix_len, uint64_t out_cap) {
    const uint64_t nl = below_cap(pos, s.L, out_cap);
    for (uint64_t i = 0; i < nl; ++i)
        if (in1(lit_at + (uint32_t)i) != out1(pos + i)) return pos + i;
    if (!s.has) return kNone;
    const uint64_t mo = pos + s.L, nm = below_cap(mo, s.M, out_cap);
    for (uint64_t i = 0; i < nm; ++i) {
        const uint64_t r = mo + i;
        const uint32_t src = r >= s.off ? out1(r - s.off) : pre1(prefix_len - (s.off - r));      // (check: off - mo <= prefix_len)
        if (src != out1(r)) return r;
    }
    return kNone;
}

// The verdict of a job whose walk ended with `status` and output.len() `n`, `bad` the smallest failing position (kNone: none).
//   a DecodeError (or LZF_CONTRACT) first: a malformed block is malformed whatever the bytes; out_len unspecified
//   LZF_MISMATCH with the first differing position, or — the compared bytes equal, the lengths not — min(n, out_cap)
//   LZF_OK with n == out_cap
struct Verdict { int status; uint64_t out_len; };
LZF_SIZE_HD Verdict conclude(int status, uint64_t n, uint64_t bad, uint64_t out_cap) {
    if (status != lzf_size::OK) return Verdict{status, n};
    if (bad != kNone) return Verdict{MISMATCH, bad};
    if (n != out_cap) return Verdict{MISMATCH, n < out_cap ? n : out_cap};
    return Verdict{lzf_size::OK, n};
}

// The serial reference: walk the tokens with the size rules, compare every clean sequence until one fails, conclude.  Readers of the
// input as lzf_size::decode_token wants them (rd4, rd1, ffrun), of the prefix and of out as first_mismatch wants them.
template <class R4, class R1, class RF, class RP, class RO>
LZF_SIZE_HD Verdict verify_block(uint64_t input_len, R4 rd4, R1 rd1, RF ffrun, RP pre1, uint64_t prefix_len, RO out1,
                                 uint64_t existing, uint64_t out_cap, uint64_t output_limit) {
    if (input_len >= kMaxLen || existing >= kMaxLen || prefix_len >= kMaxLen) return Verdict{CONTRACT, existing};
    const uint32_t len = (uint32_t)input_len;
    uint64_t pos = existing, bad = kNone;
    uint32_t tp = 0;
    while (tp < len) {
        lzf_size::Seq s;
        uint32_t next;
        if (!lzf_size::decode_token(tp, len, rd4, rd1, ffrun, s, next)) return Verdict{lzf_size::UNEXPECTED_END, pos};
        if (s.has) {
            const int code = lzf_size::check(pos + s.L, s.M, s.off, prefix_len, output_limit);
            if (code != lzf_size::OK) return Verdict{code, pos};
        }
        if (bad == kNone) bad = first_mismatch(s, pos, literals_at(tp, s.L), rd1, pre1, out1, prefix_len, out_cap);
        pos = lzf_size::advance(pos, s);
        tp = next;
    }
    return conclude(lzf_size::OK, pos, bad, out_cap);
}

}  // namespace lzf_verify

#endif  // LZF_VERIFY_RULES_H
