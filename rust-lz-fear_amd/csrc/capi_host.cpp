// capi_host.cpp — the host-buffer entry points of include/lzfear_hip.h: stage -> launch -> copy back.  Synchronous.  Every job's
// bytes travel through the pinned slab of host_staging.h in 4 MiB pieces (worker threads memcpy, one asynchronous DMA per piece),
// device scratch is kept between calls; the only per-job host work is the layout arithmetic.  Also here: EncoderTable on host
// tables and compress2 for any writer.  No kernel is launched from this file: it calls the device entry points of capi.hip.
#include <vector>
#include "capi_internal.h"
#include "host_staging.h"
#include "lzf_history_trim.h"

using namespace lzf_capi;
using lzf_host::Seg; using lzf_host::Staging;

namespace {
// What the batch wrappers share: the staging lock, the device slots (0 bytes going up, 1 bytes coming back, 3 job array, 4 results),
// the job array's way up and the results' way back.
template <class Job> struct HostCall {
    Staging& sg = Staging::get();
    std::lock_guard<std::mutex> guard{sg.lock()};
    hipStream_t cs = nullptr;
    uint8_t* din = nullptr; uint8_t* dout = nullptr; Job* djobs = nullptr; lzf_job_result* dres = nullptr;
    uint32_t n = 0;
    // with_out: the call has a slab coming back.  LZF_E_HIP when a slot, the stream or the pinned slab is not to be had.
    int open(uint32_t n_jobs, size_t in_bytes, size_t out_bytes, bool with_out) {
        n = n_jobs;
        cs = sg.stream(0);
        din = static_cast<uint8_t*>(sg.device(0, in_bytes));
        if (with_out) dout = static_cast<uint8_t*>(sg.device(1, out_bytes));
        djobs = static_cast<Job*>(sg.device(3, sizeof(Job) * n));
        dres = static_cast<lzf_job_result*>(sg.device(4, sizeof(lzf_job_result) * n));
        if (!cs || !din || (with_out && !dout) || !djobs || !dres || !sg.pinned(in_bytes > out_bytes ? in_bytes : out_bytes)) return fail_hip(hipErrorOutOfMemory, "staging memory");
        return LZF_OK;
    }
    // the bytes of `up` and the job array go up; the compute stream waits for both
    int send(const std::vector<Seg>& up, size_t in_total, const std::vector<Job>& dj) {
        HIP_TRY(sg.upload(up, in_total, din));
        HIP_TRY(hipMemcpyAsync(djobs, dj.data(), sizeof(Job) * n, hipMemcpyHostToDevice, cs));
        HIP_TRY(sg.join_copies(cs));
        return LZF_OK;
    }
    // rc: what the device entry point returned (a failure: nothing may still run when the caller's buffers go away); else the results come back
    int fetch(int rc, lzf_job_result* results) {
        if (rc != LZF_OK) { (void)hipDeviceSynchronize(); return rc; }
        HIP_TRY(hipMemcpyAsync(results, dres, sizeof(lzf_job_result) * n, hipMemcpyDeviceToHost, cs));
        HIP_TRY(hipStreamSynchronize(cs));
        return LZF_OK;
    }
};
}  // namespace

extern "C" {

int lzf_compress_batch_host(const lzf_compress_job* jobs, lzf_job_result* results, uint32_t n_jobs) {
    if (n_jobs == 0) return LZF_OK;
    if (!jobs || !results) { g_last_error = "lzf_compress_batch_host: NULL argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    // layout: one slab [inputs | tables] going up, one slab [outputs] coming back
    std::vector<size_t> in_off(n_jobs), out_off(n_jobs), tab_off(n_jobs);
    size_t in_total = 0, out_total = 0;
    uint32_t kinds = 0;
    std::vector<Seg> up;
    static_assert(sizeof(lzf_u32_table) == sizeof(lzf_u16_table), "table structs share a slab slot size");
    for (uint32_t i = 0; i < n_jobs; ++i) {
        if (jobs[i].table_kind > LZF_TABLE_U16) { g_last_error = "bad table_kind"; return LZF_E_INVALID; }
        kinds |= jobs[i].table_kind == LZF_TABLE_U32 ? LZF_KINDS_U32 : LZF_KINDS_U16;
        in_off[i] = in_total; in_total = align_up(in_total + jobs[i].input_len, 256);
        if (jobs[i].input_len) up.push_back({in_off[i], const_cast<uint8_t*>(jobs[i].input), (size_t)jobs[i].input_len});
    }
    for (uint32_t i = 0; i < n_jobs; ++i) {
        tab_off[i] = in_total;
        if (jobs[i].table) { up.push_back({tab_off[i], static_cast<uint8_t*>(jobs[i].table), sizeof(lzf_u32_table)}); in_total = align_up(in_total + sizeof(lzf_u32_table), 256); }
    }
    for (uint32_t i = 0; i < n_jobs; ++i) { out_off[i] = out_total; out_total = align_up(out_total + jobs[i].out_cap, 256); }
    HostCall<lzf_compress_job> h;
    if ((rc = h.open(n_jobs, in_total, out_total, true)) != LZF_OK) return rc;
    std::vector<lzf_compress_job> dj(jobs, jobs + n_jobs);
    for (uint32_t i = 0; i < n_jobs; ++i) {
        dj[i].input = h.din + in_off[i];
        dj[i].out = h.dout + out_off[i];
        if (jobs[i].table) dj[i].table = h.din + tab_off[i];
    }
    if ((rc = h.send(up, in_total, dj)) != LZF_OK) return rc;
    if ((rc = h.fetch(lzf_compress_batch(h.djobs, h.dres, n_jobs, kinds, h.cs), results)) != LZF_OK) return rc;
    std::vector<Seg> down;
    for (uint32_t i = 0; i < n_jobs; ++i) {
        if (results[i].status == LZF_OK && results[i].out_len) down.push_back({out_off[i], jobs[i].out, (size_t)results[i].out_len});
        if (jobs[i].table && !(jobs[i].flags & LZF_CJOB_TABLE_READONLY) && results[i].status != LZF_CONTRACT)
            HIP_TRY(hipMemcpyAsync(jobs[i].table, h.din + tab_off[i], sizeof(lzf_u32_table), hipMemcpyDeviceToHost, h.cs));
    }
    HIP_TRY(h.sg.download(down, out_total, h.dout, h.cs));
    HIP_TRY(hipStreamSynchronize(h.cs));
    return LZF_OK;
}

int lzf_compressed_size_batch_host(const lzf_compress_job* jobs, lzf_job_result* results, uint32_t n_jobs) {
    if (n_jobs == 0) return LZF_OK;
    if (!jobs || !results) { g_last_error = "lzf_compressed_size_batch_host: NULL argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    // one slab [inputs | tables] going up; `out` is not read by the size call and stays what it is (never dereferenced), out_cap is honoured
    std::vector<size_t> in_off(n_jobs), tab_off(n_jobs);
    size_t in_total = 0;
    uint32_t kinds = 0;
    std::vector<Seg> up;
    for (uint32_t i = 0; i < n_jobs; ++i) {
        if (jobs[i].table_kind > LZF_TABLE_U16) { g_last_error = "bad table_kind"; return LZF_E_INVALID; }
        if (jobs[i].input_len && !jobs[i].input) { g_last_error = "lzf_compressed_size_batch_host: NULL input"; return LZF_E_INVALID; }
        kinds |= jobs[i].table_kind == LZF_TABLE_U32 ? LZF_KINDS_U32 : LZF_KINDS_U16;
        in_off[i] = in_total; in_total = align_up(in_total + jobs[i].input_len, 256);
        if (jobs[i].input_len) up.push_back({in_off[i], const_cast<uint8_t*>(jobs[i].input), (size_t)jobs[i].input_len});
    }
    for (uint32_t i = 0; i < n_jobs; ++i) {
        tab_off[i] = in_total;
        if (jobs[i].table) { up.push_back({tab_off[i], static_cast<uint8_t*>(jobs[i].table), sizeof(lzf_u32_table)}); in_total = align_up(in_total + sizeof(lzf_u32_table), 256); }
    }
    HostCall<lzf_compress_job> h;
    if ((rc = h.open(n_jobs, in_total ? in_total : 256, 0, false)) != LZF_OK) return rc;
    std::vector<lzf_compress_job> dj(jobs, jobs + n_jobs);
    for (uint32_t i = 0; i < n_jobs; ++i) {
        dj[i].input = h.din + in_off[i];
        if (jobs[i].table) dj[i].table = h.din + tab_off[i];
    }
    if ((rc = h.send(up, in_total, dj)) != LZF_OK) return rc;
    if ((rc = h.fetch(lzf_compressed_size_batch(h.djobs, h.dres, n_jobs, kinds, h.cs), results)) != LZF_OK) return rc;
    for (uint32_t i = 0; i < n_jobs; ++i)         // a writable table comes back as lzf_compress_batch_host leaves it
        if (jobs[i].table && !(jobs[i].flags & LZF_CJOB_TABLE_READONLY) && results[i].status != LZF_CONTRACT)
            HIP_TRY(hipMemcpyAsync(jobs[i].table, h.din + tab_off[i], sizeof(lzf_u32_table), hipMemcpyDeviceToHost, h.cs));
    HIP_TRY(hipStreamSynchronize(h.cs));
    return LZF_OK;
}

int lzf_decompress_batch_host(const lzf_decompress_job* jobs, lzf_job_result* results, uint32_t n_jobs) {
    if (n_jobs == 0) return LZF_OK;
    if (!jobs || !results) { g_last_error = "lzf_decompress_batch_host: NULL argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    // Long existing output is trimmed here, where the jobs are host structs (lzf_history_trim.h): of a history of 1 GiB and more only
    // the last 64 KiB are staged and given room on the device; the results are restored on the way out.
    std::vector<lzf_decompress_job> trimmed(n_jobs);
    std::vector<uint64_t> shift(n_jobs);
    for (uint32_t i = 0; i < n_jobs; ++i) {
        if (jobs[i].out_existing_len > jobs[i].out_cap) { g_last_error = "out_existing_len > out_cap"; return LZF_E_INVALID; }
        trimmed[i] = lzf_trim::trim(jobs[i], &shift[i]);
    }
    jobs = trimmed.data();
    // one slab going up: [inputs | prefixes | existing output]; the output slab is laid out the same way for the way back
    std::vector<size_t> in_off(n_jobs), pre_off(n_jobs), out_off(n_jobs);
    size_t in_total = 0, out_total = 0;
    uint64_t max_in = 0;
    std::vector<Seg> up, up_out;
    for (uint32_t i = 0; i < n_jobs; ++i) {
        in_off[i] = in_total; in_total = align_up(in_total + jobs[i].input_len, 256);
        if (jobs[i].input_len) up.push_back({in_off[i], const_cast<uint8_t*>(jobs[i].input), (size_t)jobs[i].input_len});
        if (jobs[i].input_len > max_in) max_in = jobs[i].input_len;
    }
    for (uint32_t i = 0; i < n_jobs; ++i) {
        pre_off[i] = in_total; in_total = align_up(in_total + jobs[i].prefix_len, 256);
        if (jobs[i].prefix_len) up.push_back({pre_off[i], const_cast<uint8_t*>(jobs[i].prefix), (size_t)jobs[i].prefix_len});
    }
    for (uint32_t i = 0; i < n_jobs; ++i) {
        out_off[i] = out_total; out_total = align_up(out_total + jobs[i].out_cap, 256);
        if (jobs[i].out_existing_len) up_out.push_back({out_off[i], jobs[i].out, (size_t)jobs[i].out_existing_len});
    }
    HostCall<lzf_decompress_job> h;
    if ((rc = h.open(n_jobs, in_total, out_total, true)) != LZF_OK) return rc;
    std::vector<lzf_decompress_job> dj(jobs, jobs + n_jobs);
    for (uint32_t i = 0; i < n_jobs; ++i) {
        dj[i].input = h.din + in_off[i];
        dj[i].prefix = h.din + pre_off[i];
        dj[i].out = h.dout + out_off[i];
    }
    if (!up_out.empty()) {                          // (the slab is used for one move at a time: existing output first, and wait for it)
        HIP_TRY(h.sg.upload(up_out, out_total, h.dout));
        HIP_TRY(h.sg.join_copies(h.cs));
        HIP_TRY(hipStreamSynchronize(h.cs));
    }
    if ((rc = h.send(up, in_total, dj)) != LZF_OK) return rc;
    if ((rc = h.fetch(lzf_decompress_batch_sized(h.djobs, h.dres, n_jobs, max_in, h.cs), results)) != LZF_OK) return rc;
    std::vector<Seg> down;
    for (uint32_t i = 0; i < n_jobs; ++i) {
        uint64_t n = results[i].out_len;
        if (n > jobs[i].out_cap) n = jobs[i].out_cap;
        if (n > jobs[i].out_existing_len)
            down.push_back({out_off[i] + (size_t)jobs[i].out_existing_len, jobs[i].out + jobs[i].out_existing_len, (size_t)(n - jobs[i].out_existing_len)});
    }
    HIP_TRY(h.sg.download(down, out_total, h.dout, h.cs));
    for (uint32_t i = 0; i < n_jobs; ++i) lzf_trim::restore(results[i], shift[i]);
    return LZF_OK;
}

int lzf_decompressed_size_batch_host(const lzf_decompress_job* jobs, lzf_job_result* results, uint32_t n_jobs) {
    if (n_jobs == 0) return LZF_OK;
    if (!jobs || !results) { g_last_error = "lzf_decompressed_size_batch_host: NULL argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    // the inputs go up; prefix, out and out_cap are not read by the size call and stay what they are (never dereferenced)
    std::vector<size_t> in_off(n_jobs);
    size_t in_total = 0;
    uint64_t max_in = 0;
    std::vector<Seg> up;
    for (uint32_t i = 0; i < n_jobs; ++i) {
        in_off[i] = in_total; in_total = align_up(in_total + jobs[i].input_len, 256);
        if (jobs[i].input_len) {
            if (!jobs[i].input) { g_last_error = "lzf_decompressed_size_batch_host: NULL input"; return LZF_E_INVALID; }
            up.push_back({in_off[i], const_cast<uint8_t*>(jobs[i].input), (size_t)jobs[i].input_len});
        }
        if (jobs[i].input_len > max_in) max_in = jobs[i].input_len;
    }
    HostCall<lzf_decompress_job> h;
    if ((rc = h.open(n_jobs, in_total ? in_total : 256, 0, false)) != LZF_OK) return rc;
    std::vector<lzf_decompress_job> dj(n_jobs);
    std::vector<uint64_t> shift(n_jobs);
    for (uint32_t i = 0; i < n_jobs; ++i) {         // (long existing output trimmed as in lzf_decompress_batch_host: any length is answered)
        lzf_decompress_job j = jobs[i];
        if (j.out_cap < j.out_existing_len) j.out_cap = j.out_existing_len;      // out_cap is ignored by this call: it must not hold the trim back
        dj[i] = lzf_trim::trim(j, &shift[i]);
        dj[i].input = h.din + in_off[i];
    }
    if ((rc = h.send(up, in_total, dj)) != LZF_OK) return rc;
    if ((rc = h.fetch(lzf_decompressed_size_batch(h.djobs, h.dres, n_jobs, max_in, h.cs), results)) != LZF_OK) return rc;
    for (uint32_t i = 0; i < n_jobs; ++i) lzf_trim::restore(results[i], shift[i]);
    return LZF_OK;
}

int lzf_decompress_verify_batch_host(const lzf_decompress_job* jobs, lzf_job_result* results, uint32_t n_jobs) {
    if (n_jobs == 0) return LZF_OK;
    if (!jobs || !results) { g_last_error = "lzf_decompress_verify_batch_host: NULL argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    // long existing output trimmed as in lzf_decompress_batch_host; one slab going up: [inputs | prefixes | out[0, out_cap): history and expected bytes]
    std::vector<lzf_decompress_job> dj(n_jobs);
    std::vector<uint64_t> shift(n_jobs);
    std::vector<size_t> in_off(n_jobs), pre_off(n_jobs), out_off(n_jobs);
    size_t in_total = 0;
    uint64_t max_in = 0;
    std::vector<Seg> up;
    for (uint32_t i = 0; i < n_jobs; ++i) {
        dj[i] = lzf_trim::trim(jobs[i], &shift[i]);
        if ((dj[i].input_len && !dj[i].input) || (dj[i].prefix_len && !dj[i].prefix) || (dj[i].out_cap && !dj[i].out)) {
            g_last_error = "lzf_decompress_verify_batch_host: NULL buffer with a length"; return LZF_E_INVALID;
        }
        in_off[i] = in_total; in_total = align_up(in_total + dj[i].input_len, 256);
        if (dj[i].input_len) up.push_back({in_off[i], const_cast<uint8_t*>(dj[i].input), (size_t)dj[i].input_len});
        if (dj[i].input_len > max_in) max_in = dj[i].input_len;
    }
    for (uint32_t i = 0; i < n_jobs; ++i) {
        pre_off[i] = in_total; in_total = align_up(in_total + dj[i].prefix_len, 256);
        if (dj[i].prefix_len) up.push_back({pre_off[i], const_cast<uint8_t*>(dj[i].prefix), (size_t)dj[i].prefix_len});
    }
    for (uint32_t i = 0; i < n_jobs; ++i) {
        out_off[i] = in_total; in_total = align_up(in_total + dj[i].out_cap, 256);
        if (dj[i].out_cap) up.push_back({out_off[i], dj[i].out, (size_t)dj[i].out_cap});
    }
    HostCall<lzf_decompress_job> h;
    if ((rc = h.open(n_jobs, in_total ? in_total : 256, 0, false)) != LZF_OK) return rc;
    for (uint32_t i = 0; i < n_jobs; ++i) {
        dj[i].input = h.din + in_off[i];
        dj[i].prefix = h.din + pre_off[i];
        dj[i].out = h.din + out_off[i];
    }
    if ((rc = h.send(up, in_total, dj)) != LZF_OK) return rc;
    if ((rc = h.fetch(lzf_decompress_verify_batch(h.djobs, h.dres, n_jobs, max_in, h.cs), results)) != LZF_OK) return rc;
    for (uint32_t i = 0; i < n_jobs; ++i) lzf_trim::restore(results[i], shift[i]);      // (a mismatch's position comes back absolute as well)
    return LZF_OK;
}

// The head call on host buffers.  Of a job's existing output at most the last 65 535 bytes can be a match source (an offset is a
// u16), so that tail is all that goes up: the job is restated with its origin `shift` = out_existing_len - 65 535 bytes further on,
// by lzf_history_trim.h's rule for the lengths (which is also the long-history trim: any out_existing_len below the target is
// answered).  A job whose target does not lie beyond its existing output goes up as it is, without bytes: the device call answers
// it without reading any.  The room on the device is what the block can decode to (255 bytes per input byte), not the target.
int lzf_decompress_head_batch_host(const lzf_decompress_job* jobs, lzf_job_result* results, uint32_t n_jobs) {
    if (n_jobs == 0) return LZF_OK;
    if (!jobs || !results) { g_last_error = "lzf_decompress_head_batch_host: NULL argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    constexpr uint64_t kReach = 65535;
    std::vector<uint64_t> shift(n_jobs), keep(n_jobs), room(n_jobs);
    std::vector<size_t> in_off(n_jobs), pre_off(n_jobs), out_off(n_jobs);
    size_t in_total = 0, out_total = 0;
    std::vector<Seg> up, up_out;
    for (uint32_t i = 0; i < n_jobs; ++i) {
        const lzf_decompress_job& j = jobs[i];
        const bool work = j.out_cap > j.out_existing_len;
        if ((j.input_len && !j.input) || (j.prefix_len && !j.prefix) || (work && !j.out)) {
            g_last_error = "lzf_decompress_head_batch_host: NULL buffer with a length"; return LZF_E_INVALID;
        }
        keep[i] = work ? (j.out_existing_len < kReach ? j.out_existing_len : kReach) : 0;
        shift[i] = work ? j.out_existing_len - keep[i] : 0;
        const uint64_t want = work ? j.out_cap - j.out_existing_len : 0, most = 255ull * j.input_len + 64u;
        room[i] = want < most ? want : most;
        in_off[i] = in_total; in_total = align_up(in_total + j.input_len, 256);
        if (j.input_len) up.push_back({in_off[i], const_cast<uint8_t*>(j.input), (size_t)j.input_len});
    }
    for (uint32_t i = 0; i < n_jobs; ++i) {
        pre_off[i] = in_total; in_total = align_up(in_total + jobs[i].prefix_len, 256);
        if (jobs[i].prefix_len) up.push_back({pre_off[i], const_cast<uint8_t*>(jobs[i].prefix), (size_t)jobs[i].prefix_len});
    }
    for (uint32_t i = 0; i < n_jobs; ++i) {
        out_off[i] = out_total; out_total = align_up(out_total + keep[i] + room[i], 256);
        if (keep[i]) up_out.push_back({out_off[i], jobs[i].out + shift[i], (size_t)keep[i]});
    }
    HostCall<lzf_decompress_job> h;
    if ((rc = h.open(n_jobs, in_total ? in_total : 256, out_total ? out_total : 256, true)) != LZF_OK) return rc;
    std::vector<lzf_decompress_job> dj(jobs, jobs + n_jobs);
    for (uint32_t i = 0; i < n_jobs; ++i) {
        dj[i].input = h.din + in_off[i];
        dj[i].prefix = h.din + pre_off[i];
        dj[i].out = h.dout + out_off[i];
        if (jobs[i].out_cap > jobs[i].out_existing_len) {
            dj[i].out_existing_len = keep[i];
            dj[i].out_cap = jobs[i].out_cap - shift[i];
            dj[i].output_limit = lzf_trim::limit_of(jobs[i].output_limit, shift[i]);
        }
    }
    if (!up_out.empty()) {                          // (the slab is used for one move at a time: existing output first, and wait for it)
        HIP_TRY(h.sg.upload(up_out, out_total, h.dout));
        HIP_TRY(h.sg.join_copies(h.cs));
        HIP_TRY(hipStreamSynchronize(h.cs));
    }
    if ((rc = h.send(up, in_total, dj)) != LZF_OK) return rc;
    if ((rc = h.fetch(lzf_decompress_head_batch(h.djobs, h.dres, n_jobs, h.cs), results)) != LZF_OK) return rc;
    std::vector<Seg> down;
    for (uint32_t i = 0; i < n_jobs; ++i) {
        if (results[i].status != LZF_OK) continue;
        const uint64_t n = results[i].out_len;      // relative to the moved origin
        if (n > keep[i] && jobs[i].out_cap > jobs[i].out_existing_len)
            down.push_back({out_off[i] + (size_t)keep[i], jobs[i].out + jobs[i].out_existing_len, (size_t)(n - keep[i])});
        lzf_trim::restore(results[i], shift[i]);
    }
    HIP_TRY(h.sg.download(down, out_total, h.dout, h.cs));
    return LZF_OK;
}

// ---- EncoderTable on host tables (src/raw/compress/mod.rs:40-61, :64-74, :88-99) --------------------------------------
int lzf_table_replace_host(void* table, uint32_t table_kind, const uint8_t* input, uint64_t input_len, uint64_t pos, uint64_t* previous) {
    if (!table || (!input && input_len) || table_kind > LZF_TABLE_U16) { g_last_error = "lzf_table_replace_host: bad argument"; return LZF_E_INVALID; }
    if (pos > input_len) return LZF_CONTRACT;                         // &input[offset..] panics
    const uint64_t rem = input_len - pos;
    if (table_kind == LZF_TABLE_U32) {
        lzf_u32_table* t = static_cast<lzf_u32_table*>(table);
        const uint64_t o = pos + t->offset;
        if (o > 0xFFFFFFFFull || o < pos) return LZF_CONTRACT;         // :67 try_into().expect
        uint64_t v = 0;
        if (rem >= 8) memcpy(&v, input + pos, 8);                      // :43 input.get(..8) or 0 (little-endian host = little-endian GPU)
        const uint32_t slot = (uint32_t)(((v << 24) * 889523592379ull) >> 52);
        const uint32_t old = t->dict[slot];
        t->dict[slot] = (uint32_t)o;
        if (previous) *previous = old > t->offset ? old - t->offset : 0;
    } else {
        lzf_u16_table* t = static_cast<lzf_u16_table*>(table);
        const uint64_t o = pos + t->offset;
        if (o > 0xFFFFull || o < pos) return LZF_CONTRACT;             // :92
        if (rem < 4) return LZF_CONTRACT;                               // :59 read_u32 on a short slice panics
        uint32_t v; memcpy(&v, input + pos, 4);
        const uint32_t slot = (uint32_t)(v * 2654435761u) >> 19;
        const uint16_t old = t->dict[slot];
        t->dict[slot] = (uint16_t)o;
        if (previous) *previous = old > t->offset ? old - t->offset : 0;
    }
    return LZF_OK;
}

int lzf_table_offset_host(void* table, uint32_t table_kind, uint64_t add) {
    if (!table || table_kind > LZF_TABLE_U16) { g_last_error = "lzf_table_offset_host: bad argument"; return LZF_E_INVALID; }
    if (table_kind == LZF_TABLE_U32) static_cast<lzf_u32_table*>(table)->offset += add;
    else static_cast<lzf_u16_table*>(table)->offset += add;
    return LZF_OK;
}

// ---- compress2 for any writer: device compress against the worst-case bound, then the reference's write calls replayed ----
int lzf_compress2_host_writer(const uint8_t* input, uint64_t input_len, uint64_t cursor, void* table, uint32_t table_kind,
                              lzf_write_all_fn write_all, void* ctx, int* writer_error) {
    if ((!input && input_len) || !write_all || table_kind > LZF_TABLE_U16) { g_last_error = "lzf_compress2_host_writer: bad argument"; return LZF_E_INVALID; }
    if (writer_error) *writer_error = 0;
    const uint64_t payload = cursor < input_len ? input_len - cursor : 0;
    const uint64_t bound = payload + payload / 255 + 16;
    std::vector<uint8_t> out(bound);
    static_assert(sizeof(lzf_u32_table) == sizeof(lzf_u16_table), "one scratch copy serves both table kinds");
    std::vector<uint8_t> t0(sizeof(lzf_u32_table), 0), t1;
    if (table) memcpy(t0.data(), table, t0.size());                    // (the state on entry: a refused write needs a second run from it)
    t1 = t0;
    lzf_compress_job job{};
    job.input = input; job.input_len = input_len; job.cursor = cursor;
    job.out = out.data(); job.out_cap = bound; job.table = table ? t1.data() : nullptr; job.table_kind = table_kind;
    lzf_job_result res{};
    int rc = lzf_compress_batch_host(&job, &res, 1);
    if (rc != LZF_OK) return rc;
    if (res.status != LZF_OK) return res.status;                       // LZF_CONTRACT (the bound cannot be exceeded)
    const uint8_t* p = out.data();
    const uint8_t* const end = p + res.out_len;
    // one call of the writer; false = refused
    int werr = 0;
    auto put = [&](const uint8_t* d, size_t n) -> bool { if (n == 0) return true; werr = write_all(ctx, d, n); return werr == 0; };
    // the tail of a length (mod.rs:243-260) as it sits in the stream at q: k 0xFF bytes and the remainder byte
    auto put_tail = [&](const uint8_t*& q) -> bool {
        size_t k = 0; while (q[k] == 0xFF) ++k;
        for (size_t i = 0; i < k / 4; ++i) { if (!put(q, 4)) return false; q += 4; }
        for (size_t i = 0; i < k % 4; ++i) { if (!put(q, 1)) return false; q += 1; }
        if (!put(q, 1)) return false;
        q += 1;
        return true;
    };
    bool refused = false;
    const uint8_t* group = p;
    while (p < end && !refused) {
        group = p;
        const uint8_t tok = *p;
        const uint8_t* q = p + 1;
        if (!put(p, 1)) { refused = true; break; }                      // writer.write_u8(token)
        size_t L = tok >> 4;
        if (L == 15) { const uint8_t* t = q; while (*t == 0xFF) { L += 255; ++t; } L += *t; if (!put_tail(q)) { refused = true; break; } }
        if (!put(q, L)) { refused = true; break; }                      // writer.write_all(literal)
        q += L;
        if (q >= end) { p = q; break; }                                 // the literal-only section that ends the block (:182-189)
        if (!put(q, 2)) { refused = true; break; }                      // write_u16::<LE>(offset)
        q += 2;
        if ((tok & 15) == 15) { if (!put_tail(q)) { refused = true; break; } }
        p = q;
    }
    if (!refused) {
        if (table) memcpy(table, t1.data(), t1.size());
        return LZF_OK;
    }
    if (writer_error) *writer_error = werr;
    if (table) {
        // the table as the reference leaves it: after the search of the refused sequence, i.e. compress2 into a sink that
        // takes everything in front of that sequence and not the sequence itself
        const uint8_t* q = group; const uint8_t tok = *q++; size_t L = tok >> 4;
        if (L == 15) { while (*q == 0xFF) { L += 255; ++q; } L += *q++; }
        q += L;
        if (q < end) { q += 2; if ((tok & 15) == 15) { while (*q == 0xFF) ++q; ++q; } }
        const uint64_t gsize = (uint64_t)(q - group);
        t1 = t0;
        job.out_cap = (uint64_t)(group - out.data()) + gsize - 1;
        job.table = t1.data();
        rc = lzf_compress_batch_host(&job, &res, 1);
        if (rc != LZF_OK) return rc;
        memcpy(table, t1.data(), t1.size());
    }
    return LZF_OUTPUT_FULL;
}

int lzf_xxh32_batch_host(const uint8_t* const* ptrs, const uint64_t* lens, uint32_t* out, uint32_t n) {
    if (n == 0) return LZF_OK;
    if (!ptrs || !lens || !out) { g_last_error = "lzf_xxh32_batch_host: NULL argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    std::vector<Seg> up; std::vector<const uint8_t*> dp(n);
    size_t total = 0;
    for (uint32_t i = 0; i < n; ++i) { if (lens[i]) up.push_back({total, const_cast<uint8_t*>(ptrs[i]), (size_t)lens[i]}); dp[i] = reinterpret_cast<const uint8_t*>(total); total = align_up(total + lens[i], 256); }
    Staging& sg = Staging::get();
    std::lock_guard<std::mutex> guard(sg.lock());
    hipStream_t cs = sg.stream(0);
    uint8_t* const din = static_cast<uint8_t*>(sg.device(0, total));
    const size_t lp = 0, ll = align_up(sizeof(void*) * n, 256), lo = ll + align_up(sizeof(uint64_t) * n, 256);
    uint8_t* const dl = static_cast<uint8_t*>(sg.device(5, lo + sizeof(uint32_t) * n));
    if (!cs || !din || !dl || !sg.pinned(total)) return fail_hip(hipErrorOutOfMemory, "staging memory");
    for (uint32_t i = 0; i < n; ++i) dp[i] = din + reinterpret_cast<size_t>(dp[i]);
    HIP_TRY(sg.upload(up, total, din));
    HIP_TRY(hipMemcpyAsync(dl + lp, dp.data(), sizeof(void*) * n, hipMemcpyHostToDevice, cs));
    HIP_TRY(hipMemcpyAsync(dl + ll, lens, sizeof(uint64_t) * n, hipMemcpyHostToDevice, cs));
    HIP_TRY(sg.join_copies(cs));
    rc = lzf_xxh32_batch(reinterpret_cast<const uint8_t* const*>(dl + lp), reinterpret_cast<const uint64_t*>(dl + ll), reinterpret_cast<uint32_t*>(dl + lo), n, cs);
    if (rc != LZF_OK) { (void)hipDeviceSynchronize(); return rc; }
    HIP_TRY(hipMemcpyAsync(out, dl + lo, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipStreamSynchronize(cs));
    return LZF_OK;
}

}  // extern "C"
