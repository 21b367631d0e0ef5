// lzf_out_ring.h — the output ring of the batched decompress kernels and THE rule by which a byte range of it is moved to or from `out`: head
// bytes up to a 16-byte address, 16-byte vector accesses, tail bytes.
//   lzf_ring_split   the (head, vector, tail) split of a range; plain constexpr code that the kernels and a CPU test compile
//                    (tests/emu/emu_ring_split.cpp, against the model tests/alignment_cases.py::ring_flush_split)
//   OutRing<RING>    the most recent RING bytes of output in LDS: ring index == output address mod RING (rb = out & 15 is the bias), so 16-byte
//                    pieces of the ring line up with 16-byte pieces of HBM.  idx (RIDX), fill, flush; flush_lines (the fed kernel's deferred
//                    flush: the whole 16-byte pieces of a range, the rest left to the caller).
// The stager of lzf_seg_resolve_pair_kernel (lz4_seg_resolve.hip) keeps a written-out copy of the split, which names this one.
#ifndef LZF_OUT_RING_H
#define LZF_OUT_RING_H

#include <stdint.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define LZF_RING_HD __host__ __device__
#else
#define LZF_RING_HD
#endif
struct lzf_ring_parts { uint32_t head, vec, tail; };      // bytes, 16-byte pieces, bytes

// out[a, b) of a buffer whose address & 15 is rb (for biased positions y = x + rb: rb = 0): head = the bytes below the first 16-byte address,
// clamped to the range; vec = the whole 16-byte pieces behind the head; tail = what is left (0..15).  (Unbiased positions with the bias
// apart, as the three kernels have always worked it out: as a function of (a + rb, b + rb) alone it changed their code — profiles/copy_stage_one_ring.txt.)
LZF_RING_HD constexpr lzf_ring_parts lzf_ring_split(uint32_t a, uint32_t b, uint32_t rb) {
    uint32_t nh = (16u - ((a + rb) & 15u)) & 15u;
    if (nh > b - a) nh = b - a;
    a += nh;
    const uint32_t nv = (b - a) >> 4;
    a += nv << 4;
    return lzf_ring_parts{nh, nv, b - a};
}

#if defined(__HIPCC__)
#include "lzf_device.h"

namespace lzf {
namespace {

// rg.idx(x) spelled for the stages' loops, over the `rg` in scope.  A macro on purpose: a call, even of a forced-inline member, is opaque to the
// compiler's passes in front of its inliner, and rg.idx(x) in the copy stage changed the code of all three kernels (profiles/copy_stage_one_ring.txt).
#define RIDX(x) (((x) + rg.rb) & (rg.kRing - 1u))
// Unbiased output positions throughout (a, b, x are offsets into `out`); one wavefront, every lane calls.
template <int RING>
struct OutRing {
    static_assert(RING >= 16 && (RING & (RING - 1)) == 0, "ring index = address mod RING");
    static constexpr uint32_t kRing = RING;
    uint8_t* ring;          // LDS, 16-byte aligned
    gu8* out;
    uint32_t rb;            // out & 15
    uint32_t lane;
    uint32_t lds;           // lds_addr(ring)
    __device__ __forceinline__ uint32_t idx(uint32_t x) const { const OutRing& rg = *this; return RIDX(x); }
    __device__ __forceinline__ uint8_t& at(uint32_t x) const { return ring[idx(x)]; }
    // FLUSH: out[a, b) <- ring; else ring <- out[a, b)   (b - a <= RING; the caller made out[a, b) visible)
    template <bool FLUSH>
    __device__ __forceinline__ void move(uint32_t a, uint32_t b) const {
        const lzf_ring_parts s = lzf_ring_split(a, b, rb);
        if (lane < s.head) { if (FLUSH) out[a + lane] = at(a + lane); else at(a + lane) = out[a + lane]; }
        a += s.head;
        for (uint32_t c = lane; c < s.vec; c += kWave) {
            LZF_GLOBAL u32x4* const g = reinterpret_cast<LZF_GLOBAL u32x4*>(out + a + 16u * c);
            u32x4* const r = reinterpret_cast<u32x4*>(&at(a + 16u * c));
            if (FLUSH) *g = *r; else *r = *g;
        }
        a += s.vec << 4;
        if (lane < s.tail) { if (FLUSH) out[a + lane] = at(a + lane); else at(a + lane) = out[a + lane]; }
    }
    __device__ __forceinline__ void fill(uint32_t a, uint32_t b) const { move<false>(a, b); }
    __device__ __forceinline__ void flush(uint32_t a, uint32_t b) const { move<true>(a, b); }
    // out[a, e) <- ring for the whole 16-byte pieces of [a, b) only; returns e, the last 16-byte address at or below b (biased), from where the
    // caller keeps the rest pending (the fed kernel's deferred flush: a range that starts on such an address — every one but the first — has
    // no head and no tail, and a 16-byte line of `out` is written once).  a, b uniform.  A range that does not reach its first 16-byte address
    // stays pending as a whole (e == a).
    __device__ __forceinline__ uint32_t flush_lines(uint32_t a, uint32_t b) const {
        const uint32_t nh = (0u - (a + rb)) & 15u;
        if (nh != 0u) {
            if (b - a < nh) return a;
            if (lane < nh) out[a + lane] = at(a + lane);
            a += nh;
        }
        const uint32_t nv = (b - a) >> 4;
        for (uint32_t c = lane; c < nv; c += kWave)
            *reinterpret_cast<LZF_GLOBAL u32x4*>(out + a + 16u * c) = *reinterpret_cast<u32x4*>(&at(a + 16u * c));
        return a + (nv << 4);
    }
    // (analysis, LZF_DBG_SKIP & 128: the flush's ring reads and address work with no store issued — what the stores themselves cost)
    __device__ __forceinline__ void flush_dry(uint32_t a, uint32_t b) const {
        const lzf_ring_parts s = lzf_ring_split(a, b, rb);
        if (lane < s.head) { const uint32_t v = at(a + lane); asm volatile("" :: "v"(v), "v"(out + a + lane)); }
        a += s.head;
        for (uint32_t c = lane; c < s.vec; c += kWave) {
            const u32x4 v = *reinterpret_cast<u32x4*>(&at(a + 16u * c));
            asm volatile("" :: "v"(v), "v"(out + a + 16u * c));
        }
        a += s.vec << 4;
        if (lane < s.tail) { const uint32_t v = at(a + lane); asm volatile("" :: "v"(v), "v"(out + a + lane)); }
    }
};

}  // namespace
}  // namespace lzf
#endif  // __HIPCC__
#endif  // LZF_OUT_RING_H
