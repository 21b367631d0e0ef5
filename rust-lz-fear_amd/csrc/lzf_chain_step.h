// lzf_chain_step.h — the step between two blocks of a linked-block stream (lzfear_hip.h: lzf_chain_decompress_step), shared by
// the decode (aux_kernels.hip: lzf_chain_decompress_step_kernel) and by the frame layer's size query (frame_device.hip:
// lzf_chain_size_step_kernel).  kCountOnly: the stream's history is carried as a length alone — a stored block adds its
// length and copies nothing; every length put into the next job is the decode's.
#pragma once
#include "lzf_device.h"

namespace lzf {

// One workgroup per linked-block stream, between two decode steps.
template <bool kCountOnly>
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
            if (r.out_len - cs.length > st.block_maxsize) cs.dead = 1u;      // decompress.rs:272-274 BlockSizeOverflow ends the stream
            cs.length = r.out_len;
        }
    }
    if (st.job != 0xFFFFFFFFu) {
        if (threadIdx.x == 0) {
            lzf_decompress_job& j = jobs[st.job];
            if (cs.dead) { j.input_len = 0; j.out_existing_len = 0; j.out_cap = 0; j.output_limit = 0; }
            else { j.out_existing_len = cs.length; j.out_cap = cs.length + st.block_maxsize + j.input_len; j.output_limit = cs.length + st.block_maxsize; }
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
