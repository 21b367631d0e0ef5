// lzf_history_trim.h — a decode job whose existing output is long, restated over the last 64 KiB of it, as
// __host__ __device__ code.
//
// An LZ4 offset is a u16 (src/raw/decompress.rs:76), so of prefix ++ out[0, E) only the last 65 535 bytes can ever be a match
// source, and once E >= 65 535 the prefix is out of reach altogether (kernels.h: kSegPrefixReach).  Every rule of decompress_raw
// compares output.len() with output_limit (:72-74) or with an offset (:83-89).  So a job whose origin is moved forward by
// `shift` bytes — out, out_existing_len, out_cap and output_limit all relative to it — decodes the same bytes to the same
// addresses with the same status, and its output.len() is `shift` short.  That is how jobs with more history than the decode
// kernels' 31-bit positions hold (lzf_copy_helpers.h: kMaxPosB) are run: trimmed where they are made — the frame layer's chain step of
// linked-block streams (lzf_chain_step.h: lzf_chain_decompress_step_trimmed), the `_host` entry points (capi_host.cpp), lzf_history_trim_batch for raw callers
// (aux_kernels.hip) — and their results restored.  The CPU tests compile this header with g++ (tests/emu/emu_history_trim.cpp).
//
//   E < 2^30, or E > out_cap   shift = 0: the job as it is (a short history behaves as ever; the second is the decoder's LZF_CONTRACT)
//   otherwise                  shift = (E - 65 536) & ~15, so 65 536 <= E - shift <= 65 551
// A multiple of 16 keeps out & 15: the output ring's bias (DecodeJob::rb) and every alignment class stay what they were.  A frame
// block adds at most 4 MiB + its input to a stream, so a linked stream is trimmed long before its length reaches kMaxPosB.
// output_limit saturates at 0: with limit < shift the untrimmed job fails MemoryLimitExceeded at its first match (:72-74: E + M >
// limit), and so does the trimmed one, whose 65 536 bytes and more of history alone exceed a limit of 0.
#ifndef LZF_HISTORY_TRIM_H
#define LZF_HISTORY_TRIM_H

#include <stdint.h>
#include "../../include/lzfear_hip.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define LZF_TRIM_HD __host__ __device__ __forceinline__
#else
#define LZF_TRIM_HD inline
#endif

namespace lzf_trim {

constexpr uint64_t kThreshold = 1ull << 30;      // existing output from which a job is trimmed
constexpr uint64_t kKeep = 65536;                // what stays of it, rounded up to the next 16: every offset's reach and one byte

// How far the origin of a job with `existing` bytes of output and `out_cap` bytes of room moves forward.
LZF_TRIM_HD uint64_t shift_of(uint64_t existing, uint64_t out_cap) {
    if (existing < kThreshold || existing > out_cap) return 0;
    return (existing - kKeep) & ~15ull;
}
// The lengths of a job relative to `shift` (out_cap >= existing >= shift whenever shift != 0).
LZF_TRIM_HD uint64_t limit_of(uint64_t output_limit, uint64_t shift) { return output_limit > shift ? output_limit - shift : 0; }

// The trimmed job; *shift is what restore() adds back.  input, input_len, prefix and prefix_len are untouched.
LZF_TRIM_HD lzf_decompress_job trim(const lzf_decompress_job& job, uint64_t* shift) {
    const uint64_t s = shift_of(job.out_existing_len, job.out_cap);
    lzf_decompress_job t = job;
    if (s) {
        t.out = job.out ? job.out + s : job.out;      // (the size calls take jobs without output)
        t.out_existing_len = job.out_existing_len - s;
        t.out_cap = job.out_cap - s;
        t.output_limit = limit_of(job.output_limit, s);
    }
    *shift = s;
    return t;
}
// A result of the trimmed job as the untrimmed job's (out_len is unspecified on an error and stays what it is).  The verify call's
// LZF_MISMATCH (8) carries a position in out_len: it moves back with the origin like a length.
LZF_TRIM_HD void restore(lzf_job_result& r, uint64_t shift) {
    if (r.status == LZF_OK || r.status == 8) r.out_len += shift;
}

}  // namespace lzf_trim

#endif  // LZF_HISTORY_TRIM_H
