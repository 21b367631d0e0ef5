// lz4_seg_order.hip — the launch orders of the segmented pipeline (kernels.h: by_len, by_tok, order) and the pause between two groups.
#include "lzf_device.h"
#include "kernels.h"

namespace lzf {

// =====================================================================================================================
// order of the resolve stage's workgroups (kernels.h): one workgroup, n_jobs <= 1024
// =====================================================================================================================
__global__ __launch_bounds__(1024) void lzf_seg_by_len_kernel(seg_ctx c) {
    __shared__ uint32_t cost[1024];
    const uint32_t i = threadIdx.x, n = c.n_jobs;
    if (n > 1024u) return;                                        // (one workgroup ranks the call: the dispatch never asks for more, lzf_dispatch.h kSegRankMax)
    if (i < n) { const uint64_t l = c.jobs[i].input_len; cost[i] = l > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)l; }
    __syncthreads();
    if (i >= n) return;
    const uint32_t mine = cost[i];
    uint32_t r = 0;
    for (uint32_t k = 0; k < n; ++k) { const uint32_t o = cost[k]; r += (o > mine || (o == mine && k < i)) ? 1u : 0u; }
    c.by_len[r] = i;
}
// Grouped calls: one wavefront that does nothing for `ticks` of the device's wall clock (capi_drivers.hip converts from microseconds by the rate the runtime reports).  It sits on the caller's stream between a group's
// records stage and the next one's: the group's resolve stage starts on another stream (an event away: a few microseconds later), and
// its workgroups — 32+ KiB of LDS each — should find the compute units empty rather than squeeze in between the next records stage's
// (measured at 980 blocks: 15.4 ms with such a pause, 17.0 without).
__global__ __launch_bounds__(64) void lzf_seg_pause_kernel(uint32_t ticks) {
    const uint64_t t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
// Grouped calls: the jobs of the call by their sequences, most first — by_tok[rank] = job; consecutive ranks form the groups that go
// through the last two stages together (sizes gs.x .. gs.w, zero = no such group) — and, where the resolve stage orders its
// workgroups (c.order), every group's order at once: a group's jobs are ranks off .. off + size - 1, dealt out in rows of n_cu
// like lzf_seg_order_kernel does for a whole call.
__global__ __launch_bounds__(1024) void lzf_seg_rank_kernel(seg_ctx c, uint32_t* __restrict__ by_tok, uint4 gs) {
    __shared__ uint32_t cost[1024];
    const uint32_t i = threadIdx.x, n = c.n_jobs;
    if (n > 1024u) return;
    if (i < n) { const seg_job s = c.st[i]; cost[i] = (s.eligible && !s.failed) ? s.ntok : 0u; }
    __syncthreads();
    if (i >= n) return;
    const uint32_t mine = cost[i];
    uint32_t r = 0;
    for (uint32_t k = 0; k < n; ++k) { const uint32_t o = cost[k]; r += (o > mine || (o == mine && k < i)) ? 1u : 0u; }
    by_tok[r] = i;
    if (!c.order) return;
    const uint32_t sz[4] = {gs.x, gs.y, gs.z, gs.w};
    uint32_t off = 0, gn = 0;
    for (uint32_t k = 0; k < 4u; ++k) { if (r >= off + sz[k]) off += sz[k]; else { gn = sz[k]; break; } }
    if (!gn) return;
    const uint32_t rr = r - off;
    const uint32_t ncu = c.n_cu ? c.n_cu : 256u;
    const uint32_t row = rr / ncu, col = rr % ncu;
    const uint32_t rowlen = gn - row * ncu < ncu ? gn - row * ncu : ncu;
    c.order[off + row * ncu + ((row & 1u) ? rowlen - 1u - col : col)] = i;
}
__global__ __launch_bounds__(1024) void lzf_seg_order_kernel(seg_ctx c) {
    __shared__ uint32_t cost[1024];
    const uint32_t i = threadIdx.x, n = c.g_n;                     // (the ranks of this launch's group)
    if (n > 1024u) return;
    const uint32_t job = i < n ? (c.grouped ? seg_job_of(c, i) : i) : 0u;
    if (i < n) { const seg_job s = c.st[job]; cost[i] = (s.eligible && !s.failed) ? s.ntok : 0u; }
    __syncthreads();
    if (i >= n) return;
    const uint32_t mine = cost[i];
    uint32_t r = 0;
    for (uint32_t k = 0; k < n; ++k) { const uint32_t o = cost[k]; r += (o > mine || (o == mine && k < i)) ? 1u : 0u; }
    const uint32_t ncu = c.n_cu ? c.n_cu : 256u;
    const uint32_t row = r / ncu, col = r % ncu;
    const uint32_t rowlen = n - row * ncu < ncu ? n - row * ncu : ncu;
    c.order[c.g_off + row * ncu + ((row & 1u) ? rowlen - 1u - col : col)] = job;
}

}  // namespace lzf
