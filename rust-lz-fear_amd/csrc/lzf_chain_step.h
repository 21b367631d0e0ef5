// lzf_chain_step.h — the step between two blocks of a linked-block stream (lzfear_hip.h: lzf_chain_decompress_step and
// lzf_chain_decompress_step_trimmed), shared by the decode (aux_kernels.hip: the two lzf_chain_decompress_step*_kernel) and by the frame layer's size query (frame_device_decode.hip:
// lzf_chain_size_step_kernel).  kCountOnly: the stream's history is carried as a length alone — a stored block adds its
// length and copies nothing; every length put into the next job is the decode's.
//
// A stream's length is 64-bit and absolute in lzf_chain_state; the decode kernels hold 31-bit positions.  So from 1 GiB of history on
// a job is handed out trimmed (lzf_history_trim.h): its origin `shift` bytes into the stream's buffer, its lengths relative to that.
// The shift is a function of the length the job was made from, which is still cs.length when the job's result is read: the finish
// adds it back, and no state is kept for it.  That is kTrim: the step of lzf_chain_decompress_step_trimmed and of the frame layer.
// kTrim = false is lzf_chain_decompress_step, whose jobs carry the whole stream as history at every length, as they always did.
#pragma once
#include "lzf_device.h"
#include "lzf_history_trim.h"

namespace lzf {

// One workgroup per linked-block stream, between two decode steps.
template <bool kCountOnly, bool kTrim>
__device__ __forceinline__ void chain_step(const lzf_chain_step* __restrict__ steps, lzf_chain_state* __restrict__ state,
                                           uint32_t n, lzf_decompress_job* __restrict__ jobs,
                                           const lzf_job_result* __restrict__ results) {
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const lzf_chain_step st = steps[i];
    __shared__ lzf_chain_state cs_in;                              // read once: lane 0 stores the new state below while other waves may not have started
    if (threadIdx.x == 0) cs_in = state[i];
    __syncthreads();
    lzf_chain_state cs = cs_in;
    if (st.prev_job != 0xFFFFFFFFu && !cs.dead) {                 // finish the previous step (decompress.rs:253-269: the output joins the history)
        const lzf_job_result r = results[st.prev_job];
        if (r.status != LZF_OK) cs.dead = 1u;
        else {
            const uint64_t out_len = r.out_len + (kTrim ? lzf_trim::shift_of(cs.length, ~0ull) : 0ull);      // (the job's room was never below its history)
            if (out_len - cs.length > st.block_maxsize) cs.dead = 1u;        // decompress.rs:272-274 BlockSizeOverflow ends the stream
            cs.length = out_len;
        }
    }
    if (st.job != 0xFFFFFFFFu) {
        if (threadIdx.x == 0) {
            lzf_decompress_job& j = jobs[st.job];
            if (cs.dead) { j.input_len = 0; j.out_existing_len = 0; j.out_cap = 0; j.output_limit = 0; }
            else {
                const uint64_t shift = kTrim ? lzf_trim::shift_of(cs.length, ~0ull) : 0ull, e = cs.length - shift;      // below 1 GiB: 0, and `out` stays the host's
                if (shift && !kCountOnly) j.out = st.out + shift;
                j.out_existing_len = e; j.out_cap = e + st.block_maxsize + j.input_len; j.output_limit = e + st.block_maxsize;
            }
        }
    } else if (st.stored_len && !cs.dead) {                       // decompress.rs:250: a stored block is appended as it is
        if (!kCountOnly) {
            cgu8* s = as_global(st.stored_src);
            gu8* d = as_global(st.out) + cs.length;
            for (uint64_t t = threadIdx.x; t < st.stored_len; t += blockDim.x) d[t] = s[t];
        }
        cs.length += st.stored_len;
    }
    if (threadIdx.x == 0) state[i] = cs;
}

}  // namespace lzf
