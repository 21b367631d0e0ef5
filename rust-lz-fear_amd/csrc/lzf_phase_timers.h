// lzf_phase_timers.h — the SECTION TIMERS of the decompress kernels (analysis builds; nothing in the product build).  A kernel
// declares `PhaseTimers ph;`, calls ph.start() where its timed stretch begins, PHASE(i) where section i ends (0-5: the copy
// stage's, lz4_decompress_batch_phase.inc, 0 being what lies between batches; 6 stage + bit map, 7 bit map -> list:
// lz4_decompress_feed_phase.inc) and ph.report(results[jid]) behind its own stores to the result.
//   -DLZF_DBG_PHASE_SEL=k   cycles in section k alone, >> 10, in results[].reserved  (tools/build_phase_variants.py: pair, fed)
//   -DLZF_PHASE_TIMING      sections 0-5 at once, 10 bits each in units of 2^20 cycles: bits 0-31 of the pack above bit 32 of
//                           results[].out_len, the rest in `reserved`  (tools/diag_blocks.py: the batched kernel)
#pragma once
#include "lzf_device.h"

namespace lzf {
namespace {
#if defined(LZF_DBG_PHASE_SEL)
struct PhaseTimers {
    long long t = 0, acc = 0;
    __device__ __forceinline__ void start() { t = clock64(); }
    __device__ __forceinline__ void mark(int i) { const long long tn = clock64(); if (i == LZF_DBG_PHASE_SEL) acc += tn - t; t = tn; }
    __device__ __forceinline__ void report(lzf_job_result& r) const { r.reserved = (uint32_t)(acc >> 10); }
};
#define PHASE(i) ph.mark(i)
#elif defined(LZF_PHASE_TIMING)
struct PhaseTimers {
    long long t = 0, tph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    __device__ __forceinline__ void start() { t = clock64(); }
    __device__ __forceinline__ void mark(int i) { const long long tn = clock64(); tph[i] += tn - t; t = tn; }
    __device__ __forceinline__ void report(lzf_job_result& r) const {
        unsigned long long pk = 0;
        for (int i = 0; i < 6; ++i) { unsigned long long u = (unsigned long long)(tph[i] >> 20); if (u > 1023) u = 1023; pk |= u << (10 * i); }
        r.out_len = (r.out_len & 0xFFFFFFFFull) | ((pk & 0xFFFFFFFFull) << 32);
        r.reserved = (uint32_t)(pk >> 32);
    }
};
#define PHASE(i) ph.mark(i)
#else
struct PhaseTimers { __device__ __forceinline__ void start() {} };
#define PHASE(i) do { } while (0)
#endif
}  // namespace
}  // namespace lzf
