// lz4_decompress_feed_phase.inc — the FEED stage of the bitmap-fed decompress kernels (lz4_decompress_fed.hip): what the PARSE
// stage of lz4_decompress_parse_phase.inc produces for a chunk — the token list of the chunk — taken from the token bit map the
// hop parse of the segmented pipeline wrote for the whole batch (lzf_seg_parse_kernel + lzf_seg_seam_kernel,
// lz4_decompress_seg.hip) instead of being worked out in the kernel.  Textual include inside the kernel's round loop.
//
// A ROUND is kRound = 32 * W bytes of compressed input at a kRound-aligned position (W bit-map words, one per lane).  Rounds
// subdivide the 2 KiB tiles of the segmented pipeline, so a round lies inside ONE chunk's share of the bit map (kernels.h).
//
// Nothing of the bit map is trusted: the listed tokens are accepted only as a VERIFIED CHAIN.  The first token of the job
// must sit at position 0, and every listed token must sit where its predecessor ends — worked out from the predecessor's own
// bytes (decompress.rs:61-71 without the copies); the carry between batches and rounds is `expect`.  By induction the accepted
// tokens are exactly the tokens decompress_raw visits.  The copy stage checks the links of a batch as it decodes the batch's
// tokens (lz4_decompress_batch_phase.inc, LZF_FED_DECODE), before it writes anything of the batch; here only the list is made.
// Anything else (a missing or an extra bit, a token whose body leaves the input: UnexpectedEnd) ends the job for this kernel
// with `bail`: it is left to the pair kernel, which decodes it from its first byte and reports the reference's status.
//
// Expects in scope: lane, in, len, cstart (round start), cbuf / cbuf_a (kCB staged bytes), toks (uint16_t[TOKCAP]),
// fed_bits / fed_vf (the job's rows of seg_ctx::bits / ::vfrom), expect (uniform), the constants W, TOKCAP, kRound, kCB.
// Leaves: Tc (tokens listed for this round, 0 when the chain jumps over it), bail (uniform), and the lambda rdb for the copy
// stage.  Token-list entry = the token's offset in the round (< kRound), two aligned bytes.
// (Three-byte entries of offset and pre-decoded lengths were measured: 97.5 -> 110 ms per call, misaligned DS accesses.)
            uint32_t Tc = 0;
            bool bail = false;
            // byte of the input at absolute position q >= cstart (LDS while staged; asm on purpose, see lz4_decompress_parse_phase.inc)
            auto rdb = [&](uint32_t q) -> uint32_t {
                const uint32_t r = q - cstart;
                if (r < kCB) return lds_ld8(cbuf_a + r);
                return (uint32_t)in[q];
            };
            if (expect < cstart + kRound) {
                // ---- F0. stage in[cstart, cstart + kCB) (zeros beyond the input) and fetch the round's words of the bit map
                // (Asking for the next round one round ahead — held in registers, or one load per 64 bytes to bring its lines into
                // L2 — changed nothing at five or at six waves per SIMD: the other wavefronts already cover this round trip,
                // profiles/fed_residency_prefetch.txt section 3.)
                {
                    const uint32_t avail = len - cstart < kCB ? len - cstart : kCB;
                    cgu8* g = in + cstart;
                    constexpr uint32_t kPieces = (kCB + 1023u) / 1024u;
                    u32x4 v[kPieces];
#pragma unroll
                    for (uint32_t k = 0; k < kPieces; ++k) {
                        const uint32_t i = k * 1024u + lane * 16u;
                        v[k] = u32x4{0, 0, 0, 0};
                        if (i + 16u <= avail) v[k] = ld16(g + i);
                        else if (i < avail) { for (uint32_t t = 0; i + t < avail; ++t) v[k][(t >> 2) & 3u] |= (uint32_t)g[i + t] << ((t & 3u) * 8u); }
                    }
                    // the chunk of the segmented parse this round belongs to (kernels.h: chunk 0 owns the first kSegChunk bytes, chunk
                    // h >= 1 the kSegStride bytes from h * kSegStride + kSegOverlap on) and the round's first word in that chunk's row
                    const uint32_t h = cstart < kSegChunk ? 0u : 1u + (cstart - kSegChunk) / kSegStride;
                    uint32_t w = 0;
                    if (lane < (uint32_t)W) {
                        w = fed_bits[(size_t)h * kSegChunkWords + ((cstart - h * kSegStride) >> 5) + lane];
                        const uint32_t vf = fed_vf[h];
                        const uint32_t wpos = cstart + lane * 32u;             // position of bit 0
                        if (vf == 0xFFFFFFFFu || vf >= wpos + 32u) w = 0u;     // the chunk's marks are the true tokens from vf on
                        else if (vf > wpos) w &= ~((1u << (vf - wpos)) - 1u);
                        if (wpos >= len) w = 0u;
                        else if (len - wpos < 32u) w &= (1u << (len - wpos)) - 1u;
                    }
#pragma unroll
                    for (uint32_t k = 0; k < kPieces; ++k) {
                        const uint32_t i = k * 1024u + lane * 16u;
                        if (i < kCB) *reinterpret_cast<u32x4*>(&cbuf[i]) = v[k];
                    }
                    PHASE(6);
                    // ---- F1. bit map -> token positions in stream order
                    const uint32_t cnt = (uint32_t)__popc(w);
                    const uint32_t incl = wave_scan_add(cnt);
                    uint32_t k = incl - cnt;
                    Tc = __builtin_amdgcn_readlane(incl, 63);                  // <= kRound / 3 + 1 would hold for a true chain; TOKCAP >= kRound is not needed:
                    if (Tc > (uint32_t)TOKCAP) { bail = true; Tc = 0; }        // more marks than any chain has (tokens are >= 1 byte apart only in a damaged map)
                    else while (w) { const uint32_t b = (uint32_t)__builtin_ctz(w); toks[k++] = lane * 32u + b; w &= w - 1u; }
                }
                PHASE(7);
                if (Tc == 0u && !bail) bail = true;                            // the chain enters this round but no token is marked in it
                if (bail) Tc = 0;
            }
