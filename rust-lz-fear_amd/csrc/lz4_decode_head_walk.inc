// lz4_decode_head_walk.inc — the head walk of ONE job (lzf_head_rules.h: head_block), shared by lzf_decode_head_kernel
// (lz4_decode_head.hip: the job is the caller's) and lzf_frame_head_kernel (frame_device_head.hip: the job of a frame's compressed
// block); textual include inside the kernel, as the decompress kernels share their stages, so that the LDS buffers stay the
// kernel's.  lz4_decode_head.hip's header has the walk's description; the copies are lz4_decode_head_copies.inc's.
// Expects in scope: lane; the job — in, pre, out (global pointers), input_len, plen, existing, limit, cap (the target); the parse
// stage's LDS cbuf / nxt / tokex / toks with cbuf_a / nxt_a / ex_a and S, TOKCAP, STAGE, kChunk, kCB, kExStride; and, to be left
// with the result, int status (LZF_OK) and uint64_t o (= existing: output.len()).
        if (input_len >= kMaxPosB || existing >= kMaxPosB || plen >= kMaxPosB) {
            status = LZF_CONTRACT;
        } else {
            const uint32_t len = (uint32_t)input_len;
            const DecodeJob jv{in, nullptr, nullptr, len, 0u, 0u, 0ull, 0u};      // what the parse stage reads of a job: its input
            uint32_t cstart = 0;                       // a true token position (or len)
            // readers of the input in HBM / L2 for the one token looked at ahead of a chunk (wave-uniform addresses)
            auto g1 = [&](uint32_t p) -> uint32_t { return (uint32_t)in[p]; };
            auto g4 = [&](uint32_t p) -> uint32_t {
                if (len - p >= 4u) return ld4(in + p);
                uint32_t v = 0;
                for (uint32_t i = 0; p + i < len; ++i) v |= (uint32_t)in[p + i] << (8u * i);
                return v;
            };
            auto gff = [&](uint32_t p) -> uint32_t {           // 0xFF bytes from p on, eight at a time
                uint32_t n = 0;
                while (len - (p + n) >= 8u && ld8(in + p + n) == ~0ull) n += 8u;
                while (p + n < len && in[p + n] == 255u) ++n;
                return n;
            };
            // the walk ends in front of the first sequence at or beyond the target: nothing of it is read
            while (cstart < len && status == LZF_OK && !lzf_head::stops(o, cap)) {
                // a token that reaches beyond the chunk: decoded ahead of the parse as in the size kernel, moved by the whole wave
                {
                    const uint32_t w = g4(cstart);
                    if ((w & 0xFFF0u) == 0xFFF0u || (w & 15u) == 15u) {
                        lzf_size::Seq s;
                        uint32_t next;
                        if (!lzf_size::decode_token(cstart, len, g4, g1, gff, s, next)) { status = LZF_UNEXPECTED_END; break; }
                        if (next - cstart > kChunk) {
                            const int code = s.has ? lzf_size::check(o + s.L, s.M, s.off, plen, limit) : LZF_OK;
                            if (code != LZF_OK) { status = code; break; }
                            const lzf_head::Clamp c = lzf_head::clamp(o, s, cap);
                            wave_copy_apart(out + o, in + lzf_head::literals_at(cstart, s.L), c.nl, lane);
                            wave_store_fence();
                            if (c.nm) {
                                wave_match(out, pre, plen, o + s.L, s.off, c.nm, lane);
                                wave_store_fence();
                            }
                            o = lzf_size::advance(o, s);
                            cstart = next;
                            continue;
                        }
                    }
                }
#define LZF_TOK_T uint16_t
#define LZF_THOP_RECORD thop_loop_record
#include "lz4_decompress_parse_phase.inc"
#undef LZF_THOP_RECORD
#undef LZF_TOK_T
                // the staged chunk's readers, and how many bytes from p on are 0xFF (no further than len); here the run ends within a chunk
                auto rdb = [&](uint32_t q) -> uint32_t { return sb.rdb(q); };
                auto rd4 = [&](uint32_t q) -> uint32_t { return sb.rd4(q); };
                auto ffrun = [&](uint32_t p) -> uint32_t {
                    uint32_t n = 0;
                    while (p + n < len && rdb(p + n) == 255u) ++n;
                    return n;
                };
                bool stopped = false;
                for (uint32_t tidx = 0; tidx < Tc; tidx += kWave) {
                    const bool listed = lane < Tc - tidx;
                    // lanes past the list decode the round's first token again (masked off below)
                    const uint32_t tp = cstart + toks[listed ? tidx + lane : tidx];
                    lzf_size::Seq s;
                    uint32_t next;
                    (void)lzf_size::decode_token(tp, len, rd4, rdb, ffrun, s, next);     // listed tokens are whole: the parse read them
                    const uint64_t tot = listed ? (uint64_t)s.L + s.M : 0ull;
                    // the size kernel's rule for the 32-bit scan (an L of 2^24 needs more than 64 K length bytes: such a token is longer
                    // than a chunk and was taken ahead of the parse above, never listed)
                    const bool wide = __ballot(listed && s.M >= (1ull << 24)) != 0ull;
                    const uint64_t incl = wave_scan_add64(tot, wide);
                    const uint64_t lpos = o + (incl - tot), mo = lpos + s.L;             // output.len() in front of / behind this lane's literals
                    const bool act = listed && !lzf_head::stops(lpos, cap);              // (positions rise: the live lanes come first)
                    const int code = act && s.has ? lzf_size::check(mo, s.M, s.off, plen, limit) : LZF_OK;
                    const uint32_t e = first_lane(__ballot(code != LZF_OK));
                    if (e < 64u) { status = __builtin_amdgcn_readlane(code, e); break; }
                    // the round is clean: the copies
                    lzf_head::Clamp c = lzf_head::clamp(lpos, s, cap);
                    if (!act) { c.nl = 0u; c.nm = 0ull; }
                    const uint32_t lit_at = lzf_head::literals_at(tp, s.L);
                    const bool from_pre = (uint64_t)s.off > mo;                          // the source starts in the prefix's tail
                    const uint64_t back = from_pre ? (uint64_t)s.off - mo : 0ull;
                    // a match nothing of this round feeds: wholly in the prefix, or ending in front of the round's first byte
                    const bool own_m = c.nm != 0ull && c.nm <= kOwn && (from_pre ? c.nm <= back : mo - s.off + c.nm <= o);
                    if (__ballot(own_m) != 0ull) wave_store_fence();                     // their sources: what earlier rounds wrote
                    if (c.nl != 0u && c.nl <= kOwn) lane_copy(out + lpos, in + lit_at, c.nl);
                    if (own_m) lane_copy(out + mo, from_pre ? pre + (plen - back) : (cgu8*)out + (mo - s.off), (uint32_t)c.nm);
                    for (unsigned long long m = __ballot(c.nl > kOwn); m; m &= m - 1ull) {
                        const uint32_t l = (uint32_t)__builtin_ctzll(m);
                        wave_copy_apart(out + readlane64(lpos, l), in + (uint32_t)__builtin_amdgcn_readlane(lit_at, l),
                                        (uint32_t)__builtin_amdgcn_readlane(c.nl, l), lane);
                    }
                    const unsigned long long later = __ballot(c.nm != 0ull && !own_m);
                    if (later) wave_store_fence();
                    for (unsigned long long m = later; m; m &= m - 1ull) {
                        const uint32_t l = (uint32_t)__builtin_ctzll(m);
                        wave_match(out, pre, plen, readlane64(mo, l), (uint32_t)__builtin_amdgcn_readlane(s.off, l), readlane64(c.nm, l), lane);
                        wave_store_fence();
                    }
                    o += readlane64(incl, 63);
                    if (__ballot(listed && !act) != 0ull) { stopped = true; break; }     // (o is at or beyond the target now)
                }
                if (status == LZF_OK && !stopped && !lzf_head::stops(o, cap) && cerr != LZF_OK) status = cerr;
                cstart = cend;
            }
        }
