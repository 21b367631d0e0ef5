// frame_device_head.hip — lzf_frame_head_device: the first bytes of every frame held in device memory (frame_device_common.h has
// the map; lzf_frame_head_rules.h has the rule and the one definition of the result).
//
// lzf_frame_head_kernel, one wavefront per frame, frames drawn from a 4-byte ticket by as many workgroups as the device holds at
// once.  The wave runs lzf_frame_scan.h's header parse and the walk's step uniformly (every lane reads the same few bytes,
// bytewise: frames start at any address), and takes every block entered in front of the target:
//   a stored block      moved wave-wide, 16 bytes a lane, the end bytewise, no further than the target;
//   a compressed block  the head walk of the raw call (lz4_decode_head_walk.inc, the body lzf_decode_head_kernel runs), on the job
//                       lzf_frame_head::block_job states: an independent block into out + pos with the dictionary as prefix, a
//                       linked block behind the frame's pos bytes of output.
// In front of every step that reads what the wave wrote — a linked block reading the block before it, a compressed block behind
// a stored one — the wave waits for its own stores (wave_store_fence).  Block checksums are stepped over, not verified.
// The host reads nothing back: it packs the call's four arrays into one upload, enqueues the kernel and returns once the upload has
// left host memory.  There is no class of many wavefronts and no launch order: a frame costs what its target asks for, and a
// target that spans many blocks is decoded at one wavefront's rate — correct, and not meant to be fast (profiles/frame_head.txt).
// No load leaves in[0, in_len), dict[0, dict_len) or out[0, target); no store leaves out[0, target).
#include <atomic>
#include "frame_device_common.h"
#include "lzf_device.h"
#include "kernels.h"
#include "lzf_copy_helpers.h"
#include "lzf_parse_helpers.h"
#include "lzf_frame_head_rules.h"

namespace lzf {
namespace {
static_assert(lzf_head::kMaxLen == kMaxPosB && lzf_head::CONTRACT == LZF_CONTRACT, "lzf_head_rules.h restates these");
static_assert(lzf_scan::INPUT_ERROR == LZF_F_INPUT_ERROR && lzf_scan::BLOCK_SIZE_OVERFLOW == LZF_F_BLOCK_SIZE_OVERFLOW, "lzf_frame_scan.h restates these");
constexpr uint32_t kOwn = 64;            // bytes of a run a lane moves by itself   (the raw head kernel's values: lz4_decode_head.hip)
constexpr uint32_t kStep = 1024;         // bytes the wave moves per step: 16 a lane

#include "lz4_decode_head_copies.inc"

// a value every lane holds alike, moved to the scalar side (the walk's branches are then uniform for the compiler too)
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return (uint64_t)rfl((uint32_t)v) | ((uint64_t)rfl((uint32_t)(v >> 32)) << 32); }

template <int S, int TOKCAP>
__global__ __launch_bounds__(64) void lzf_frame_head_kernel(const uint8_t* const* __restrict__ f_in, const uint64_t* __restrict__ f_len,
                                                            uint8_t* const* __restrict__ f_out, const uint64_t* __restrict__ f_target,
                                                            const uint8_t* dict, uint64_t dict_len, uint32_t n_frames, uint32_t* __restrict__ ticket,
                                                            uint64_t* __restrict__ d_out_len, int32_t* __restrict__ d_status) {
    constexpr bool STAGE = true;
    constexpr uint32_t kChunk = 64u * S;               // compressed bytes whose tokens one parse covers
    constexpr uint32_t kCB = kChunk + 64u;             // staged bytes: the chunk + room for token bodies
    static_assert(kChunk <= 65536, "token positions are stored as u16 offsets into the chunk");
    static_assert(kCB % 16 == 0, "chunk buffer is filled in 16-byte pieces");
    __shared__ __attribute__((aligned(16))) uint8_t cbuf[kCB];
    __shared__ __attribute__((aligned(16))) uint8_t nxt[kChunk];
    constexpr uint32_t kExStride = (uint32_t)S + 4u;
    constexpr uint32_t kTokBytes = ((uint32_t)TOKCAP + 64u) * 2u;
    constexpr uint32_t kExBytes = 64u * kExStride;
    __shared__ __attribute__((aligned(16))) uint8_t tokex[kTokBytes > kExBytes ? kTokBytes : kExBytes];
    uint16_t* const toks = reinterpret_cast<uint16_t*>(tokex);
    const uint32_t lane = threadIdx.x;
    const uint32_t cbuf_a = lds_addr(cbuf), nxt_a = lds_addr(nxt), ex_a = lds_addr(tokex);

    for (;;) {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(ticket, 1u);
        t = rfl(t);
        if (t >= n_frames) break;
        const uint32_t f = t;
        cgu8* const fin = as_global(f_in[f]);
        gu8* const fout = as_global(f_out[f]);
        const uint64_t flen = f_len[f], target = f_target[f];
        int fst = LZF_OK;
        uint64_t pos = 0;                              // bytes delivered in front of the block being entered
        if (lzf_frame_head::contract(target)) {
            fst = LZF_CONTRACT;
        } else {
            lzf_scan::Header h = lzf_scan::read_header((const uint8_t*)fin, flen);
            h.status = (int)rfl((uint32_t)h.status); h.header_len = rfl(h.header_len); h.flags = (uint8_t)rfl(h.flags); h.bd = (uint8_t)rfl(h.bd);
            h.block_maxsize = uni64(h.block_maxsize);
            if (h.status != lzf_scan::OK) {
                fst = h.status;
            } else {
                const bool linked = (h.flags & lzf_scan::FL_INDEP) == 0;
                const uint64_t bmax = h.block_maxsize;
                uint64_t r = h.header_len;
                while (!lzf_head::stops(pos, target)) {
                    const lzf_frame_head::Next x = lzf_frame_head::next_block((const uint8_t*)fin, flen, r, h);
                    if (!rfl((uint32_t)x.found)) { fst = (int)rfl((uint32_t)x.status); break; }      // the EndMark (LZF_OK), or the walk's error
                    const uint64_t b_off = uni64(x.b.off);
                    const uint32_t b_len = rfl(x.b.len);
                    r = uni64(x.b.end_off);
                    uint64_t n = b_len;
                    if (!rfl(x.b.compressed)) {
                        wave_copy_apart(fout + pos, fin + b_off, lzf_head::below(pos, n, target), lane);
                    } else {
                        const lzf_frame_head::BlockJob j = lzf_frame_head::block_job(linked, pos, bmax, target);
                        cgu8* __restrict__ in = fin + b_off;
                        cgu8* pre = as_global(dict);
                        gu8* out = fout + j.shift;
                        const uint64_t input_len = b_len, plen = dict_len, existing = j.existing, limit = j.limit, cap = j.target;
                        int status = LZF_OK;
                        uint64_t o = existing;             // output.len()
                        wave_store_fence();                // (a linked block reads what the blocks before it wrote)
#include "lz4_decode_head_walk.inc"
                        if (status != LZF_OK) { fst = status; break; }
                        n = lzf_head::reported(o, cap, existing) - existing;
                    }
                    if (lzf_frame_head::reaches(pos, n, target)) { pos = target; break; }
                    const lzf_frame_head::Behind s = lzf_frame_head::behind_block(n, bmax);
                    if (s.ends) { fst = s.status; break; }
                    pos += n;
                }
            }
        }
        if (lane == 0) {
            d_out_len[f] = pos < target ? pos : target;
            d_status[f] = fst;
        }
    }
}

constexpr auto k_frame_head = lzf_frame_head_kernel<48, 768>;
}  // namespace
}  // namespace lzf

using namespace lzf_fdev;

namespace {
// workgroups of the kernel the current device holds at once (asked once per device)
int resident_workgroups(hipStream_t st, uint32_t* room) {
    static std::atomic<uint32_t> known[64];
    int dev = 0;
    DEV_TRY(hipGetDevice(&dev));
    const bool keep = dev >= 0 && dev < 64;
    uint32_t v = keep ? known[dev].load(std::memory_order_relaxed) : 0u;
    if (!v) {
        int per = 0, cu = 0;
        DEV_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, lzf::k_frame_head, 64, 0));
        DEV_TRY(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev));
        v = (uint32_t)(per > 0 ? per : 1) * (uint32_t)(cu > 0 ? cu : 1);
        if (keep) known[dev].store(v, std::memory_order_relaxed);
    }
    *room = v;
    return LZF_OK;
}
}  // namespace

extern "C" int lzf_frame_head_device(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len, const uint8_t* d_dict, size_t dict_len,
                                     uint8_t* const* d_out, const size_t* target, uint64_t* d_out_len, int32_t* d_status, void* hip_stream) {
    if (n_frames && (!d_in || !in_len || !d_out || !target || !d_out_len || !d_status)) return LZF_E_INVALID;
    for (uint32_t f = 0; f < n_frames; ++f) if ((in_len[f] && !d_in[f]) || (target[f] && !d_out[f])) return LZF_E_INVALID;
    if (!d_dict) dict_len = 0;
    if (n_frames == 0) return LZF_OK;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    static_assert(sizeof(size_t) == 8 && sizeof(void*) == 8, "the four arrays travel as 64-bit words");
    uint32_t room = 0;
    RC_TRY(resident_workgroups(st, &room));
    Meta meta(st);                                   // [in | in_len | out | target], and the ticket behind them (zeroed)
    const size_t words = 8 * (size_t)n_frames;
    const size_t i_in = meta.add(d_in, words), i_len = meta.add(in_len, words), i_out = meta.add(d_out, words), i_target = meta.add(target, words);
    const size_t s_ticket = meta.room(4);
    RC_TRY(meta.upload(true));
    KERNEL(lzf::k_frame_head, dim3(n_frames < room ? n_frames : room), dim3(64), 0, st, meta.img<const uint8_t* const>(i_in), meta.img<const uint64_t>(i_len),
           meta.img<uint8_t* const>(i_out), meta.img<const uint64_t>(i_target), d_dict, (uint64_t)dict_len, n_frames, meta.scr<uint32_t>(s_ticket), d_out_len, d_status);
    return meta.wait();                              // the image has left host memory; the kernel runs on
}
