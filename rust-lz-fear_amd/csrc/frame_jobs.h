// frame_jobs.h — the decode jobs of one pass of frames, shared by lzf_frame_decompress_many (frame.cpp: frames in host
// memory, uploaded) and lzf_frame_decompress_device_many (frame_device_decode.hip: frames in device memory); at the end the
// compress jobs of one pass (input windows, launch order, output slots, tables), shared the same way by lzf_frame_compress_many
// and lzf_frame_compress_device_many.
//
// Layout of decompress.rs:238-269 on the device: an independent frame's compressed blocks each get an output slot of
// block_out_bound + input length (the limit plus what the literals may overshoot); a linked frame is one stream
// buffer that lzf_chain_decompress_step grows block after block, with the dictionary as every job's prefix (:239-245).
// Stored blocks get no job: independent ones are read straight from the input, linked ones are appended by the chain step.
//
// split_passes is the one planner of the memory budget: the four *_many drivers cut their frames into passes with it.
#ifndef LZF_FRAME_JOBS_H
#define LZF_FRAME_JOBS_H

#include <cassert>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>
#include "../../include/lzfear_frame.h"
#include "lzf_frame_scan.h"

namespace lzf_frame_jobs {

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
using lzf_scan::block_out_bound;    // the most a block of `len` compressed bytes can decode to (lzf_frame_scan.h)

// The passes of a call under a memory budget: frames [0, n), frame f asking for need[f] bytes, go through in passes [first, second)
// of whole groups, in order.  Groups are taken greedily while the running sum stays within the budget; the first group of a pass
// is always taken, so a group over the budget alone is a pass of its own (the caller sees that from the pass and `need`).
// group_end[f] = one past the last frame of f's group, for every f; NULL: every frame is its own group.
inline void split_passes(const size_t* need, uint32_t n, size_t budget, const uint32_t* group_end,
                         std::vector<std::pair<uint32_t, uint32_t>>& passes) {
    passes.clear();
    for (uint32_t f0 = 0; f0 < n;) {
        size_t sum = 0; uint32_t f1 = f0;
        while (f1 < n) {
            const uint32_t e = group_end ? group_end[f1] : f1 + 1;
            assert(e > f1 && e <= n);                             // a group ends behind its frames and inside the call
            size_t add = 0;
            for (uint32_t f = f1; f < e; ++f) add += need[f];
            if (f1 != f0 && (add > budget || sum > budget - add)) break;
            sum += add; f1 = e;
        }
        passes.emplace_back(f0, f1);
        f0 = f1;
    }
}

struct BlockRef { const uint8_t* src; uint32_t len; bool compressed; };    // src: device address of the block's bytes
struct Frame {
    bool linked = false;
    size_t bmax = 0, consumed = 0;                // consumed: the frame's input bytes (linked stream room, see layout)
    std::vector<BlockRef> blocks;
    // filled by layout / build
    size_t out_off = 0, out_size = 0;             // linked: the stream's output buffer
    uint32_t chain = 0;                           // linked: index among the linked streams
    std::vector<size_t> job;                      // per block: job index or SIZE_MAX (stored)
    std::vector<size_t> slot;                     // independent: offset of the block's output slot
};
struct Plan {
    std::vector<lzf_decompress_job> jobs;         // ordered by step: step 0 = every block of the independent frames + block 0 of the linked streams
    std::vector<size_t> step_off;                 // jobs of step k are [step_off[k], step_off[k + 1])
    std::vector<lzf_chain_step> csteps;           // n_steps x n_chain
    size_t out_total = 0, n_steps = 1;
    uint32_t n_chain = 0;
};

// Output offsets of every frame, in frame order.
inline void layout(const std::vector<Frame*>& fs, Plan& p) {
    size_t max_steps = 0;
    for (Frame* F : fs) {
        const size_t nb = F->blocks.size();
        F->job.assign(nb, SIZE_MAX); F->slot.assign(nb, 0);
        if (F->linked) {
            size_t bound = 0;
            for (const BlockRef& b : F->blocks) bound += b.compressed ? block_out_bound(F->bmax, b.len) : b.len;
            // a block may run past its limit by its literals before the stream is stopped: room for that
            if (nb) { F->chain = p.n_chain++; F->out_off = p.out_total; F->out_size = bound + F->consumed + 64; p.out_total = up256(p.out_total + F->out_size); if (nb > max_steps) max_steps = nb; }
        } else {
            for (size_t i = 0; i < nb; ++i) if (F->blocks[i].compressed) { F->slot[i] = p.out_total; p.out_total = up256(p.out_total + block_out_bound(F->bmax, F->blocks[i].len) + F->blocks[i].len); }
        }
    }
    p.n_steps = max_steps > 1 ? max_steps : 1;
}

// Jobs and chain steps against the output allocation `dout` (p.out_total bytes) and the device dictionary.  With `sizes_only`
// (lzf_frame_decompressed_size_device) there is neither: every length is set as for the decode, every output and dictionary
// address stays NULL.
inline void build(const std::vector<Frame*>& fs, Plan& p, uint8_t* dout, const uint8_t* d_dict, size_t dict_len, bool sizes_only = false) {
    p.jobs.clear(); p.step_off.clear();
    p.csteps.assign((size_t)p.n_chain * p.n_steps, lzf_chain_step{});
    for (size_t k = 0; k < p.n_steps; ++k) {
        p.step_off.push_back(p.jobs.size());
        for (Frame* Fp : fs) {
            Frame& F = *Fp;
            const size_t nb = F.blocks.size(), bmax = F.bmax;
            auto add_job = [&](size_t i) {
                lzf_decompress_job j;
                memset(&j, 0, sizeof j);
                j.input = F.blocks[i].src; j.input_len = F.blocks[i].len;
                j.prefix = sizes_only ? nullptr : d_dict; j.prefix_len = dict_len;                // :239-245
                const size_t lim = bmax;                                                          // :248
                if (F.linked) { j.out = sizes_only ? nullptr : dout + F.out_off; j.out_cap = lim + F.blocks[i].len; j.output_limit = lim; }   // (patched per step)
                else { j.out = sizes_only ? nullptr : dout + F.slot[i]; j.out_cap = block_out_bound(bmax, F.blocks[i].len) + F.blocks[i].len; j.output_limit = lim; }
                F.job[i] = p.jobs.size(); p.jobs.push_back(j);
            };
            if (!F.linked) { if (k == 0) for (size_t i = 0; i < nb; ++i) if (F.blocks[i].compressed) add_job(i); continue; }
            if (!nb) continue;
            lzf_chain_step& st = p.csteps[k * p.n_chain + F.chain];
            memset(&st, 0, sizeof st);
            st.prev_job = (k > 0 && k - 1 < nb && F.blocks[k - 1].compressed) ? (uint32_t)F.job[k - 1] : UINT32_MAX;
            st.job = UINT32_MAX; st.out = sizes_only ? nullptr : dout + F.out_off; st.block_maxsize = bmax;
            if (k < nb) {
                if (F.blocks[k].compressed) { add_job(k); st.job = (uint32_t)F.job[k]; }
                else { st.stored_len = F.blocks[k].len; st.stored_src = F.blocks[k].src; }
            }
        }
    }
    p.step_off.push_back(p.jobs.size());
}

// the largest input of the jobs of step k (lzf_decompress_batch_sized's bound: the host built the jobs, it knows their sizes)
inline uint64_t step_max_input(const Plan& p, size_t k) {
    uint64_t m = 0;
    for (size_t q = p.step_off[k]; q < p.step_off[k + 1]; ++q) if (p.jobs[q].input_len > m) m = p.jobs[q].input_len;
    return m;
}

// ---- the compress side: every block's input window (src/framed/compress.rs:217-275), shared by lzf_frame_compress_many
//      (frame.cpp) and lzf_frame_compress_device_many (frame_device_compress.hip)
// Block k's payload is data[off, off + n).  Its job compresses S[lo, lo + hist + n) from cursor `hist`, where
//   linked blocks (:271-275): S = dict ++ data and the history is the last <= 64 KiB of what came before it (block 0: the whole
//     dictionary); `add` is what the window forgot since the block before: the stream's table.offset(add) is due before it.
//     Every non-final block is a whole block of >= 64 KiB, so from block 1 on the window lies inside data (lo >= dict_len);
//   independent blocks with a dictionary (:218,:268): S = dict ++ this block alone, lo = 0, hist = dict_len;
//   independent blocks without one: S = data, lo = off, hist = 0.
struct CWindow { size_t off, n, lo, hist; uint64_t add; };
// appends the windows of one input's blocks to w
inline void compress_windows(size_t in_len, size_t bs, size_t dict_len, bool indep, std::vector<CWindow>& w) {
    const size_t nb = (in_len + bs - 1) / bs;
    size_t lo = 0, len = dict_len;                        // linked: the history is S[lo, lo + len)
    uint64_t pending = 0;
    for (size_t k = 0; k < nb; ++k) {
        const size_t off = k * bs, n = in_len - off < bs ? in_len - off : bs;
        if (indep) { w.push_back(dict_len ? CWindow{off, n, 0, dict_len, 0} : CWindow{off, n, off, 0, 0}); continue; }
        w.push_back(CWindow{off, n, lo, len, pending});
        len += n;
        pending = 0;
        if (len > LZF_WINDOW_SIZE) { const size_t forget = len - LZF_WINDOW_SIZE; pending = forget; lo += forget; len = LZF_WINDOW_SIZE; }
    }
}

// The compress jobs of one pass of frames, free of addresses: the twin of Plan / build above, for both compress drivers.
// A frame takes part when the driver's status for it is LZF_OK up front; the others get no job.  Independent blocks go in frame
// order, one step; linked streams go step-major (block k of every stream that has one in step k: streams run in lock-step, with
// lzf_table_offset_batch of `W.add` on table `table` before the step).  Every job's output slot is as long as its block (:242),
// the slots stand one behind the other in job order.
struct CJob { uint32_t frame, block; CWindow W; size_t slot; uint32_t table; };      // table: linked: the stream's index among the linked streams
struct CPlan {
    std::vector<size_t> nb;               // per frame: its blocks, 0 where it takes no part
    std::vector<CJob> jobs;               // launch order
    std::vector<size_t> step_off;         // jobs of step k are [step_off[k], step_off[k + 1])
    std::vector<size_t> first, job_of;    // frame f's block k is job job_of[first[f] + k] (first: n + 1 entries)
    size_t max_nb = 0, slots = 0;         // slots: the bytes of all output slots
    uint32_t n_linked = 0;
    const CJob& of(uint32_t f, size_t k) const { return jobs[job_of[first[f] + k]]; }
};
// false: more jobs than a launch takes (nothing is planned)
inline bool compress_plan(uint32_t n, const size_t* in_len, const int* status0, size_t bs, size_t dict_len, bool indep, CPlan& p) {
    p = CPlan{};
    p.nb.assign(n, 0); p.first.assign((size_t)n + 1, 0);
    std::vector<uint32_t> table(n, 0);
    size_t total = 0;
    for (uint32_t f = 0; f < n; ++f) {
        p.first[f] = total;
        if (status0[f] != LZF_OK) continue;
        p.nb[f] = (in_len[f] + bs - 1) / bs; total += p.nb[f];
        if (p.nb[f] > p.max_nb) p.max_nb = p.nb[f];
        if (!indep && p.nb[f]) table[f] = p.n_linked++;
    }
    p.first[n] = total;
    if (total > 0x7FFFFFFFull) return false;
    std::vector<CWindow> win;             // in frame order: frame f's at first[f]
    win.reserve(total);
    for (uint32_t f = 0; f < n; ++f) if (p.nb[f]) compress_windows(in_len[f], bs, dict_len, indep, win);
    p.jobs.reserve(total); p.job_of.resize(total);
    auto add_job = [&](uint32_t f, size_t k) {
        const CWindow& W = win[p.first[f] + k];
        p.job_of[p.first[f] + k] = p.jobs.size();
        p.jobs.push_back(CJob{f, (uint32_t)k, W, p.slots, table[f]});
        p.slots += W.n;
    };
    if (indep) {
        for (uint32_t f = 0; f < n; ++f) for (size_t k = 0; k < p.nb[f]; ++k) add_job(f, k);
        p.step_off = {0, total};
    } else {
        for (size_t k = 0; k < p.max_nb; ++k) {
            p.step_off.push_back(p.jobs.size());
            for (uint32_t f = 0; f < n; ++f) if (k < p.nb[f]) add_job(f, k);
        }
        p.step_off.push_back(total);
    }
    return true;
}
// The job of record r: `input` = where S[W.lo] stands, `out` = the job's slot, `table` = its stream's table or the call's template
// (NULL: a fresh one); readonly_template: an independent block's template.clone() (:220,:270).
inline void fill_compress_job(lzf_compress_job& j, const CJob& r, const uint8_t* input, uint8_t* out, void* table, bool readonly_template) {
    memset(&j, 0, sizeof j);
    j.input = input; j.input_len = r.W.hist + r.W.n; j.cursor = r.W.hist;      // :222,:243
    j.out = out; j.out_cap = r.W.n;                                            // :242
    j.table = table; j.table_kind = LZF_TABLE_U32;                             // :202
    if (readonly_template) j.flags = LZF_CJOB_TABLE_READONLY;
}

// lzf_frame_set_memory_budget's value (0: half of the free device memory), read under the frame layer's lock (frame.cpp)
size_t memory_budget();

}  // namespace lzf_frame_jobs

#endif  // LZF_FRAME_JOBS_H
