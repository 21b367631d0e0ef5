// frame_deliver_body.inc — the body of the frame layer's delivery kernels (frame_device.hip; textual include inside the kernel,
// as the decompress kernels share their stages): lzf_frame_deliver_kernel with LZF_DELIVER_COUNT_ONLY 0, and the size query's
// lzf_frame_size_deliver_kernel with LZF_DELIVER_COUNT_ONLY 1 — the same stops fix the same status, out_len and consumed, and
// nothing else is written: no copy lists, no content checksum (the kernel has no r_ / l_ / h_ arrays).  With LZF_DELIVER_INDEX 1
// on top of counting only it is lzf_frame_block_index_kernel: the same per-block decisions, written out as the frame's block
// index (lzf_block_index.h's fill_entry) instead of the frame's results.  The rounds then go on behind the stop: every block
// gets its entry, the ones behind the stop with the frame's length as their place.
// Expects in scope: frames, blks, jobs, res, sums, d_status, d_out_len, d_consumed and, when not counting only, r_src / r_dst /
// r_len, l_src / l_dst / l_len, h_len / h_check; in index mode x_index / x_cap / d_n_listed instead of d_status / d_out_len /
// d_consumed.
    const DFrameDesc F = frames[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    const bool linked = (F.flags & kLinked) != 0;
    uint64_t w = 0, consumed = F.scan_consumed;
    int st = LZF_OK;
    bool stopped = false;
#if LZF_DELIVER_INDEX
    lzf_frame_block* const x_out = x_index ? x_index[F.frame] : nullptr;
    const uint64_t x_room = x_out ? x_cap[F.frame] : 0ull;
#endif
    for (uint32_t base = 0; base < F.nb; base += 64u) {
        const uint32_t i = base + lane;
        const bool act = i < F.nb;
        uint64_t n = 0, end_off = 0;
        int code = 0;
        const uint8_t* src = nullptr;
#if LZF_DELIVER_INDEX
        DBlkDesc x_b{};
#endif
        if (act) {
            const DBlkDesc b = blks[F.blk0 + i];
#if LZF_DELIVER_INDEX
            x_b = b;
#endif
            end_off = b.end_off; src = b.src;
            if (b.sum_idx != kNone && sums[b.sum_idx] != b.want_sum) code = LZF_F_BLOCK_CHECKSUM_FAIL;
            else if (b.job != kNone) {
                const lzf_job_result r = res[b.job];
                if (r.status != LZF_OK) code = r.status;
                else n = r.out_len - (linked ? jobs[b.job].out_existing_len : 0ull);   // linked: the chain step set the stream's length before the job
            } else n = b.len;
            if (!code && n > F.bmax) code = LZF_F_BLOCK_SIZE_OVERFLOW;
        }
        const uint64_t incl = wave_incl_scan(n, lane);
        const uint64_t at = w + (incl - n);                     // where the block goes in the caller's output
        const bool cap = act && !code && (at > F.out_cap || F.out_cap - at < n);
        const bool zero = act && !code && !cap && n == 0;
        const uint64_t stops = __ballot(act && (code || cap || zero));
        const uint32_t first = stops ? (uint32_t)__builtin_ctzll(stops) : 64u;
#if !LZF_DELIVER_COUNT_ONLY
        if (!linked && act) {
            const bool give = lane < first;
            r_src[F.blk0 + i] = src; r_dst[F.blk0 + i] = F.dst + (give ? at : 0ull); r_len[F.blk0 + i] = give ? n : 0ull;
        }
#endif
#if LZF_DELIVER_INDEX
        {   // every block's entry: its place in front of the stop, the frame's length (the stopping block's place) behind it
            const uint64_t at_stop = __shfl(at, (int)(first & 63u), 64);
            if (act && i < x_room) {
                const bool has_sum = x_b.sum_idx != kNone;
                const lzf_bindex::Place place = lzf_bindex::place_of(stopped, lane, first);
                x_out[i] = lzf_bindex::fill_entry(x_b.end_off - (has_sum ? 4u : 0u) - x_b.len, x_b.len, x_b.job == kNone, has_sum, x_b.want_sum, linked,
                                                  F.bmax, code, n, at, stopped ? w : at_stop, place);
            }
        }
        if (stopped) continue;
#endif
        if (stops) {
            const int c = __shfl(code, (int)first, 64);
            const int cp = __shfl((int)cap, (int)first, 64);
            w = __shfl(at, (int)first, 64);
            consumed = __shfl(end_off, (int)first, 64);
            st = c ? c : cp ? LZF_OUT_CAPACITY : LZF_OK;
            stopped = true;
#if LZF_DELIVER_INDEX
            continue;
#else
            break;
#endif
        }
        w += __shfl(incl, 63, 64);
    }
    if (lane != 0) return;
#if LZF_DELIVER_INDEX
    if (d_n_listed) d_n_listed[F.frame] = F.nb;
#else
#if !LZF_DELIVER_COUNT_ONLY
    if (linked && F.nb) { l_src[F.link_idx] = F.stream; l_dst[F.link_idx] = F.dst; l_len[F.link_idx] = w; }
#endif
    d_out_len[F.frame] = w;
    if (stopped) { d_status[F.frame] = st; d_consumed[F.frame] = consumed; }
    else { d_status[F.frame] = F.scan_err; d_consumed[F.frame] = F.scan_consumed; }
#if !LZF_DELIVER_COUNT_ONLY
    if (F.hash_idx != kNone) {
        const bool check = !stopped && (F.flags & kCheckContent);
        h_len[F.hash_idx] = check ? w : 0ull; h_check[F.hash_idx] = check ? 1u : 0u;
    }
#endif
#endif  // !LZF_DELIVER_INDEX
