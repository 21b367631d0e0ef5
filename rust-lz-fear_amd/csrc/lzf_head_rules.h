// lzf_head_rules.h — "the first bytes of this block": raw::decompress_raw (src/raw/decompress.rs:58-99) with one added rule, as
// __host__ __device__ code on top of lzf_size_rules.h.
//
// The job is the decoder's (include/lzfear_hip.h); out_cap is the TARGET, the absolute output length (existing output included) at
// which decoding stops.  With `pos` = output.len() at the top of an iteration of the reference's loop (:61), the position of the
// sequence's first literal:
//   stop     the loop ends with Ok in front of the first sequence whose pos >= target; that sequence and everything behind it is
//            never looked at, malformed or not;
//   checks   a sequence with pos < target is taken whole, as the reference takes it: token and length bytes, UnexpectedEnd (the whole
//            literal run must be in the input: lzf_size::decode_token), the limit test :72-74, the offset tests :83-89 — also
//            where its literals alone reach the target.  The first failing sequence in stream order wins;
//   writes   of such a sequence the bytes at positions below the target are written, the rest are dropped (clamp below);
//   result   LZF_OK with out_len = min(n, target), n the length the loop ended with; a codec status 1..4 (out_len unspecified).
// A position depends on lengths only, so the stop is known from the size rules before a byte is moved, and the clamp is the same
// arithmetic as the verify call's below_cap.  head_block below is the one definition of the result; the CPU tests run it
// (tests/emu/emu_head.cpp) against the oracle's decode cut at the target, and the kernel (lz4_decode_head.hip) is held to it and
// uses the same clamp.
#ifndef LZF_HEAD_RULES_H
#define LZF_HEAD_RULES_H

#include "lzf_size_rules.h"

namespace lzf_head {

enum : int { CONTRACT = 6 };                          // LZF_CONTRACT of include/lzfear_hip.h
constexpr uint64_t kMaxLen = 0x7FFFFF00ull;           // the decoder's contract (lzf_copy_helpers.h: kMaxPosB): lengths from here on are LZF_CONTRACT

// Where the literals of the token at `tp` start in the input: behind the token and the length bytes of L (15 + 255 n + last: n + 1 bytes).
LZF_SIZE_HD uint32_t literals_at(uint32_t tp, uint32_t L) { return tp + 1u + (L >= 15u ? (L - 15u) / 255u + 1u : 0u); }

// Does the walk stop in front of a sequence whose first literal sits at `pos`?
LZF_SIZE_HD bool stops(uint64_t pos, uint64_t target) { return pos >= target; }

// How many of the n bytes at output position r0 lie below the target.
LZF_SIZE_HD uint64_t below(uint64_t r0, uint64_t n, uint64_t target) { return r0 >= target ? 0ull : (n < target - r0 ? n : target - r0); }

// The clamp of a sequence that starts below the target and passed its checks: nl of its literal bytes and nm of its match bytes
// are written.  (nl < L implies nm == 0: the match starts behind the literals.)
struct Clamp { uint32_t nl; uint64_t nm; };
LZF_SIZE_HD Clamp clamp(uint64_t pos, const lzf_size::Seq& s, uint64_t target) {
    return Clamp{(uint32_t)below(pos, s.L, target), s.has ? below(pos + s.L, s.M, target) : 0ull};
}

// The length a job reports: the walk ended at output.len() n.  (A target below the existing output: nothing is done, and the
// existing length is the answer.)
LZF_SIZE_HD uint64_t reported(uint64_t n, uint64_t target, uint64_t existing) {
    const uint64_t m = n < target ? n : target;
    return m < existing ? existing : m;
}

// The serial reference.  Readers of the input as lzf_size::decode_token wants them (rd4, rd1, ffrun); pre1(k) = prefix[k];
// out1(r) = out[r] for r below the position being written (history, and what this walk wrote); put1(r, byte) writes out[r],
// existing <= r < target.
struct Result { int status; uint64_t out_len; };
template <class R4, class R1, class RF, class RP, class RO, class WO>
LZF_SIZE_HD Result head_block(uint64_t input_len, R4 rd4, R1 rd1, RF ffrun, RP pre1, uint64_t prefix_len, RO out1, WO put1,
                              uint64_t existing, uint64_t target, uint64_t output_limit) {
    if (input_len >= kMaxLen || existing >= kMaxLen || prefix_len >= kMaxLen) return Result{CONTRACT, existing};
    const uint32_t len = (uint32_t)input_len;
    uint64_t pos = existing;
    uint32_t tp = 0;
    while (tp < len && !stops(pos, target)) {
        lzf_size::Seq s;
        uint32_t next;
        if (!lzf_size::decode_token(tp, len, rd4, rd1, ffrun, s, next)) return Result{lzf_size::UNEXPECTED_END, pos};
        const uint64_t mo = pos + s.L;
        if (s.has) {
            const int code = lzf_size::check(mo, s.M, s.off, prefix_len, output_limit);
            if (code != lzf_size::OK) return Result{code, pos};
        }
        const Clamp c = clamp(pos, s, target);
        const uint32_t lit_at = literals_at(tp, s.L);
        for (uint32_t i = 0; i < c.nl; ++i) put1(pos + i, rd1(lit_at + i));
        for (uint64_t i = 0; i < c.nm; ++i) {
            const uint64_t r = mo + i;
            put1(r, r >= s.off ? out1(r - s.off) : pre1(prefix_len - (s.off - r)));      // (check: off - mo <= prefix_len)
        }
        pos = lzf_size::advance(pos, s);
        tp = next;
    }
    return Result{lzf_size::OK, reported(pos, target, existing)};
}

}  // namespace lzf_head

#endif  // LZF_HEAD_RULES_H
