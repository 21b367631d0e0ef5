// emu_compress_plan.cpp — TEST INFRASTRUCTURE: the compress plan of the frame layer (lzf_frame_jobs::compress_plan and
// fill_compress_job, rust-lz-fear_amd/csrc/frame_jobs.h) compiled with g++ for the CPU tests of tests/test_compress_plan_cpu.py.
// The product never loads it.
#include <cstdint>
#include <vector>
#include "../../rust-lz-fear_amd/csrc/frame_jobs.h"

extern "C" {
// One plan kept between the calls below (the tests are single-threaded).
static lzf_frame_jobs::CPlan g_plan;

// Plans n frames; returns the number of jobs, or -1 where the plan refuses.  *n_steps = step_off's entries - 1.
int64_t lzf_emu_compress_plan(uint32_t n, const uint64_t* in_len, const int32_t* status0, uint64_t bs, uint64_t dict_len, int indep,
                              uint64_t* n_steps, uint64_t* max_nb, uint32_t* n_linked, uint64_t* slots) {
    std::vector<size_t> len(in_len, in_len + n);
    std::vector<int> st(status0, status0 + n);
    if (!lzf_frame_jobs::compress_plan(n, len.data(), st.data(), (size_t)bs, (size_t)dict_len, indep != 0, g_plan)) return -1;
    *n_steps = g_plan.step_off.size() - 1; *max_nb = g_plan.max_nb; *n_linked = g_plan.n_linked; *slots = g_plan.slots;
    return (int64_t)g_plan.jobs.size();
}
// step_off[0 .. n_steps]
void lzf_emu_compress_plan_steps(uint64_t* step_off) { for (size_t k = 0; k < g_plan.step_off.size(); ++k) step_off[k] = g_plan.step_off[k]; }
// per frame: nb[f] and, at out[first .. first + nb), the job of every block in block order; job_of has room for every job
void lzf_emu_compress_plan_frames(uint64_t* nb, uint64_t* job_of) {
    size_t at = 0;
    for (size_t f = 0; f < g_plan.nb.size(); ++f) {
        nb[f] = g_plan.nb[f];
        for (size_t k = 0; k < g_plan.nb[f]; ++k) job_of[at++] = (uint64_t)(&g_plan.of((uint32_t)f, k) - g_plan.jobs.data());
    }
}
// job q as 9 words: frame, block, W.off, W.n, W.lo, W.hist, W.add, slot, table; and, as 6 more, the lzf_compress_job that
// fill_compress_job makes of it from input = 1000, out = 2000, table = 3000: input_len, cursor, out_cap, table_kind, flags with
// and without the read-only template
void lzf_emu_compress_plan_job(uint64_t q, uint64_t* w) {
    const lzf_frame_jobs::CJob& r = g_plan.jobs[q];
    w[0] = r.frame; w[1] = r.block; w[2] = r.W.off; w[3] = r.W.n; w[4] = r.W.lo; w[5] = r.W.hist; w[6] = r.W.add; w[7] = r.slot; w[8] = r.table;
    lzf_compress_job j, k;
    lzf_frame_jobs::fill_compress_job(j, r, reinterpret_cast<const uint8_t*>(1000), reinterpret_cast<uint8_t*>(2000), reinterpret_cast<void*>(3000), true);
    lzf_frame_jobs::fill_compress_job(k, r, reinterpret_cast<const uint8_t*>(1000), reinterpret_cast<uint8_t*>(2000), reinterpret_cast<void*>(3000), false);
    const bool addr = j.input == reinterpret_cast<const uint8_t*>(1000) && j.out == reinterpret_cast<uint8_t*>(2000) && j.table == reinterpret_cast<void*>(3000);
    w[9] = j.input_len; w[10] = j.cursor; w[11] = j.out_cap; w[12] = addr ? j.table_kind : ~0ull; w[13] = j.flags; w[14] = k.flags;
}
}
