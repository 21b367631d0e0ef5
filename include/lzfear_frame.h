/*
 * lzfear_frame.h — C ABI of the host-side LZ4 *frame* layer that drives the GPU block codec
 * (SURVEY.md §8 row f1).  It mirrors lz-fear's `framed` module:
 *
 *   CompressionSettings + compress / compress_with_size   src/framed/compress.rs:36-157
 *   compress_internal (header, block loop, EndMark)       src/framed/compress.rs:160-282
 *   LZ4FrameReader::new / decode_block / decompress_frame src/framed/decompress.rs:102-288
 *   Flags / BlockDescriptor                               src/framed/header.rs:8-81
 *   MAGIC / INCOMPRESSIBLE / WINDOW_SIZE                  src/framed/mod.rs:16-20
 *
 * The reference calls the block codec once per block (compress.rs:243, decompress.rs:248); here
 * all independent blocks of a frame go to the GPU in ONE batch (lzf_compress_batch /
 * lzf_decompress_batch of lzfear_hip.h); linked-block frames are inherently sequential and run
 * block after block with the table / window carried between calls.
 * Buffers are host memory (except for the "frames in device memory" section below).  No CPU codec: the calls fail with LZF_E_NO_DEVICE without a GPU.
 * Checksums: the header checksum (a few bytes) is hashed on the host; block checksums are computed on the device for
 * all blocks of a call in one launch; content checksums on the device for frames up to 32 MiB and on host worker
 * threads, overlapping the kernels, for longer ones (XXH32 is one serial chain per buffer).
 */
#ifndef LZFEAR_FRAME_H
#define LZFEAR_FRAME_H

#include <stddef.h>
#include <stdint.h>
#include "lzfear_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* frame-level status codes (>= 16; block-level DecodeError codes 1..4 of lzfear_hip.h pass through
 * as `CodecError`, src/framed/decompress.rs:20-21) */
enum {
    LZF_F_INPUT_ERROR = 16,            /* DecompressionError::InputError (EOF), decompress.rs:18-19 */
    LZF_F_WRONG_MAGIC = 17,            /* :24-25 */
    LZF_F_HEADER_CHECKSUM_FAIL = 18,   /* :26-27 */
    LZF_F_BLOCK_CHECKSUM_FAIL = 19,    /* :28-29 */
    LZF_F_FRAME_CHECKSUM_FAIL = 20,    /* :30-31 */
    LZF_F_BLOCK_LENGTH_OVERFLOW = 21,  /* :32-33 */
    LZF_F_BLOCK_SIZE_OVERFLOW = 22,    /* :34-35 */
    LZF_F_UNIMPLEMENTED_BLOCKSIZE = 23,/* header::ParseError, header.rs:19-28 */
    LZF_F_UNSUPPORTED_VERSION = 24,
    LZF_F_RESERVED_FLAG_BITS = 25,
    LZF_F_RESERVED_BD_BITS = 26,
    LZF_F_INVALID_BLOCK_SIZE = 27,     /* CompressionError::InvalidBlockSize, compress.rs:21-22 */
    LZF_F_PANIC = 28                   /* BlockDescriptor::new unwrap() panic, header.rs:55 */
};
/* per-frame status of the *_many calls only: the frame alone asks for more device memory than the budget allows */
#define LZF_E_NO_MEMORY (-4)

#define LZF_MAGIC 0x184D2204u          /* src/framed/mod.rs:16 */
#define LZF_WINDOW_SIZE 65536u         /* src/framed/mod.rs:20 */

/* CompressionSettings (src/framed/compress.rs:36-55) plus the `content_size: Option<u64>` of
 * compress_internal (:160; compress_with_size passes Some(len), :148-157). */
typedef struct lzf_settings {
    int32_t independent_blocks;     /* default 1  (:47) */
    int32_t block_checksums;        /* default 0  (:48) */
    int32_t content_checksum;       /* default 1  (:49) */
    int32_t has_dictionary_id;      /* dictionary(id, d) sets it; dictionary_id_nonsense_override clears/sets it (:113-133) */
    uint64_t block_size;            /* default 4 MiB (:50); 64 KiB / 256 KiB / 1 MiB / 4 MiB */
    const uint8_t* dictionary;      /* NULL = None (:51) */
    uint64_t dictionary_len;
    uint32_t dictionary_id;
    int32_t has_content_size;
    uint64_t content_size;
} lzf_settings;

void lzf_settings_default(lzf_settings* s);                       /* Default::default(), :44-55 */
size_t lzf_frame_compress_bound(const lzf_settings* s, size_t in_len);

/* CompressionSettings::compress / compress_with_size_unchecked over memory buffers.
 * Returns LZF_OK, LZF_F_INVALID_BLOCK_SIZE, LZF_F_PANIC, LZF_OUT_CAPACITY or a negative LZF_E_*. */
int lzf_frame_compress(const lzf_settings* s, const uint8_t* in, size_t in_len,
                       uint8_t* out, size_t out_cap, size_t* out_len);

/* Parsed frame header (LZ4FrameReader::new + accessors :167-175). */
typedef struct lzf_frame_info {
    uint8_t flags;                  /* FLG byte */
    uint8_t bd;                     /* BD byte */
    uint16_t header_len;            /* bytes up to and including HC */
    uint32_t dictionary_id;
    int32_t has_dictionary_id;
    int32_t has_content_size;
    uint64_t content_size;
    uint64_t block_maxsize;
} lzf_frame_info;
int lzf_frame_read_header(const uint8_t* in, size_t in_len, lzf_frame_info* info);

/* decompress_frame (:284-288) with an optional dictionary (into_read_with_dictionary, :180).
 * Status is the inner error kind (what decode_block returns).  *out_len = bytes produced by the
 * blocks completed before the error; *consumed = bytes of `in` read. */
int lzf_frame_decompress(const uint8_t* in, size_t in_len, const uint8_t* dict, size_t dict_len,
                         uint8_t* out, size_t out_cap, size_t* out_len, size_t* consumed);

/* Many frames per call: every block of every frame goes into the same launches and stays on the device from the
 * first block to the last (independent-block frames: one launch; linked-block frames: block k of every stream in
 * launch k, no host round trip in between).  Same bytes and the same per-frame statuses as one
 * lzf_frame_compress / lzf_frame_decompress call per frame; status[f], out_len[f] (and consumed[f], may be NULL) are
 * per frame, the return value is LZF_OK or a negative LZF_E_* (device trouble, bad arguments).  All frames of a
 * compress call share `s` (and its dictionary), all frames of a decompress call the dictionary. */
int lzf_frame_compress_many(const lzf_settings* s, uint32_t n_frames, const uint8_t* const* in, const size_t* in_len,
                            uint8_t* const* out, const size_t* out_cap, size_t* out_len, int* status);
int lzf_frame_decompress_many(uint32_t n_frames, const uint8_t* const* in, const size_t* in_len,
                              const uint8_t* dict, size_t dict_len,
                              uint8_t* const* out, const size_t* out_cap, size_t* out_len, size_t* consumed, int* status);

/* Block-by-block reader: LZ4FrameReader (src/framed/decompress.rs:79-282) over a memory buffer that the caller keeps
 * alive.  lzf_frame_reader_new = LZ4FrameReader::new (:102-161, header errors as its return value, *r = NULL then);
 * lzf_frame_reader_decode_block = decode_block (:198-282): decodes the next block into out[0..out_cap) — *out_len = 0
 * with LZF_OK once the EndMark has been read (`finished`, :206-215; the content checksum is verified there) —
 * with `dict` as the reference's `dictionary` argument (:238-245; linked frames carry their own 64 KiB window, :253-269).
 * One block per call means one small launch per call: the *_many drivers above are the fast path, this is the
 * reference's streaming interface for callers that want it.  Needs out_cap >= block_maxsize + the block's compressed
 * size to never see LZF_OUT_CAPACITY. */
typedef struct lzf_frame_reader lzf_frame_reader;
int lzf_frame_reader_new(const uint8_t* in, size_t in_len, lzf_frame_reader** r);
void lzf_frame_reader_free(lzf_frame_reader* r);
void lzf_frame_reader_info(const lzf_frame_reader* r, lzf_frame_info* info);     /* block_size(), frame_size(), dictionary_id() :167-175 */
int lzf_frame_reader_decode_block(lzf_frame_reader* r, const uint8_t* dict, size_t dict_len,
                                  uint8_t* out, size_t out_cap, size_t* out_len);
int lzf_frame_reader_finished(const lzf_frame_reader* r);
size_t lzf_frame_reader_consumed(const lzf_frame_reader* r);                     /* bytes of `in` read so far */

/* Streaming frame WRITER: CompressionSettings::compress / compress_with_size_unchecked (src/framed/compress.rs:138-157) for a
 * caller that feeds the stream piece by piece and takes the frame piece by piece — bounded memory, any stream length.
 * compress_internal's loop (:221-276) reads `block_size` bytes per turn; here the bytes come through
 * lzf_frame_writer_write in any granularity and leave through `write_all` (see lzf_compress2_host_writer), in the
 * reference's order: header (:163-200) at the first write or at finish, per block the length word, the payload and the
 * optional block checksum (:244-263), EndMark and content checksum (:277-281) at finish.
 * Independent blocks: `blocks_per_launch` whole blocks (0 = 64) are buffered and compressed in one launch (with a
 * dictionary: each block behind its own copy of it and the seeded template table, :217-220,:265-270).
 * Linked blocks: one launch per block, the table and the last 64 KiB carried (:271-275).
 * settings->has_content_size / content_size = compress_with_size_unchecked's argument.  The dictionary is copied.
 * Byte-identical to lzf_frame_compress over the concatenated input.
 * Returns LZF_OK, LZF_F_INVALID_BLOCK_SIZE / LZF_F_PANIC (new), LZF_OUTPUT_FULL when the sink refused a write (its code:
 * lzf_frame_writer_sink_error; the writer is dead from then on), LZF_CONTRACT, or a negative LZF_E_*. */
typedef struct lzf_frame_writer lzf_frame_writer;
int lzf_frame_writer_new(const lzf_settings* s, lzf_write_all_fn write_all, void* ctx, uint32_t blocks_per_launch, lzf_frame_writer** w);
int lzf_frame_writer_write(lzf_frame_writer* w, const uint8_t* data, size_t len);
int lzf_frame_writer_finish(lzf_frame_writer* w);
int lzf_frame_writer_sink_error(const lzf_frame_writer* w);
void lzf_frame_writer_free(lzf_frame_writer* w);

/* ---- the host side of the drivers (host_staging.h): one pinned slab, kept device scratch, worker threads ---------- */
typedef struct lzf_frame_stats {
    uint64_t calls;                     /* *_many calls served */
    uint64_t device_block_hashes;       /* block checksums computed by lzf_xxh32_batch */
    uint64_t host_block_hashes;         /* ... by the host (lzf_frame_assemble only: its payloads are host memory) */
    uint64_t device_content_hashes;     /* content checksums: one device chain per frame (frames <= 32 MiB) */
    uint64_t host_content_hashes;       /* ... on the worker threads (longer frames) */
    uint64_t h2d_copies, d2h_copies;    /* DMA transfers issued through the pinned slab, and their bytes */
    uint64_t h2d_bytes, d2h_bytes;
    uint64_t pinned_bytes;              /* size of the pinned slab now */
} lzf_frame_stats;
void lzf_frame_get_stats(lzf_frame_stats* st);
/* The drivers keep their pinned slab and device scratch between calls (allocating gigabytes costs more than the
 * kernels); this gives everything back.  Calls are serialised per device (one slab per device). */
void lzf_frame_release_scratch(void);
/* Worker threads of the host staging (pageable <-> pinned copies, content hashes of long frames): n of them, 0 = default (12 on a
 * large host), LZF_HOST_THREADS_NONE = none at all — the calling thread does every copy itself (no hidden host
 * threads are REQUIRED; they are a throughput option).  The threads are created on first use and kept. */
#define LZF_HOST_THREADS_NONE 0xFFFFFFFFu
void lzf_frame_set_host_threads(uint32_t n);
/* Device memory one pass of lzf_frame_decompress_many / lzf_frame_compress_many may use (0 = half of what is free): more frames
 * than fit are processed in several passes; a frame that does not fit alone gets status LZF_E_NO_MEMORY (decompress) or is a
 * pass of its own (compress).  A frame in device memory that is over the budget decodes piece by piece through
 * lzf_frame_resume_device, whose scratch follows the room the caller gives, not the frame. */
void lzf_frame_set_memory_budget(size_t bytes);
/* Pinned host memory the staging may hold (0 = default: 2 GiB; at least two 4 MiB slots).  A pass that moves more than this
 * recycles the slab as a ring of 4 MiB slots — a slot is reused when the DMA that last read it has finished — so the pinned
 * footprint of a call is bounded whatever the size of the call.  Changing it gives the current slab back. */
void lzf_frame_set_pinned_limit(size_t bytes);

/* XXH32 on the host (header / content checksums; twox-hash XxHash32 in the reference). */
uint32_t lzf_xxh32(const uint8_t* p, size_t len, uint32_t seed);
/* Streaming form (the content hasher of a block-by-block reader, src/framed/decompress.rs:89,276-278).  lzf_xxh32_state is
 * declared in lzfear_hip.h: the device's lzf_xxh32_update_batch / lzf_xxh32_digest_batch take the same 48 bytes. */
void lzf_xxh32_reset(lzf_xxh32_state* st, uint32_t seed);
void lzf_xxh32_update(lzf_xxh32_state* st, const uint8_t* p, size_t len);
uint32_t lzf_xxh32_digest(const lzf_xxh32_state* st);

/* ---- frames in device memory ------------------------------------------------------------------------------------------
 * lzf_frame_decompress_many for frames that already live on the device (a tensor, shards a loader uploaded compressed),
 * decoded into device memory: decompress_frame (src/framed/decompress.rs:284-288) of every frame, with the header parse of
 * LZ4FrameReader::new (:102-161), the block walk and stop rules of decode_block (:198-282) and the dictionary / linked-block
 * window of :238-269 run on the device.
 *   d_in, in_len, d_out, out_cap: HOST arrays of n_frames entries; d_in[f] / d_out[f] are DEVICE addresses.  Frames may alias
 *     each other (one tensor may serve as many frames); outputs must not overlap each other or any input.  d_dict: device.
 *   d_out_len, d_consumed, d_status: DEVICE arrays of n_frames entries, written in stream order on `hip_stream` (a hipStream_t
 *     of the current device; NULL = the legacy default stream).
 * Per frame the results are those of lzf_frame_decompress_many on the same bytes: status, out_len bytes and consumed, also
 * LZF_OUT_CAPACITY at the same block when out_cap[f] is short, and LZF_E_NO_MEMORY for a frame that does not fit the memory
 * budget (lzf_frame_set_memory_budget) alone; with out_cap[f] >= lzf_frame_decompress_bound_device's bound no frame ends in
 * LZF_OUT_CAPACITY.  Nothing in d_out[f] beyond out_len[f] is written.
 * The host waits twice on the stream: for the per-frame scan summary and for the block table (24 bytes per block), which it
 * needs to plan the decode; it then enqueues block checksums, decode, delivery, the copy into d_out and the content checksums,
 * waits for its own small upload of job lists to leave host memory (it is first in the stream at that point), and returns.
 * No host memory of the call is read after it returns.  The waits make the call NOT graph-capturable.  Scratch comes from the
 * device's stream-ordered memory pool and is freed in stream order.  Frames go through in passes of the memory budget, with
 * the host driver's accounting.  No state is kept between calls and lzf_frame_stats is not touched; the calls do not take the
 * host drivers' lock, except to read the memory budget.
 * Checksums are computed on the device only: block checksums in one launch per pass; a content checksum is one serial XXH32
 * chain per frame (~1.3 GB/s each, many frames at once), so one huge frame with a content checksum is bounded by its chain.
 * Returns LZF_OK or a negative LZF_E_* (bad arguments, HIP failure, LZF_E_NO_DEVICE without a device: no CPU fallback). */
/* Per frame: the most its blocks can decode to.  For a frame whose header parses, this is the sum over the blocks the walk
 * finds of (compressed ? min(255*len + 16, block_maxsize) : len); 0 for a frame whose header fails.  Synchronous. */
int lzf_frame_decompress_bound_device(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len,
                                      size_t* out_bound, void* hip_stream);
/* lzf_frame_decompress_many for frames that live in device memory, decoded into device memory. */
int lzf_frame_decompress_device_many(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len,
                                     const uint8_t* d_dict, size_t dict_len,
                                     uint8_t* const* d_out, const size_t* out_cap,
                                     uint64_t* d_out_len, uint64_t* d_consumed, int32_t* d_status,
                                     void* hip_stream);
/* Per frame: what lzf_frame_decompress_device_many would report, found without decoding — no output memory is needed, none is
 * allocated.  Conventions of lzf_frame_decompress_device_many: d_in / in_len are HOST arrays, d_in[f] a DEVICE address; d_out_len,
 * d_consumed (may be NULL), d_status are DEVICE arrays written in stream order.
 *   d_out_len[f]   the out_len lzf_frame_decompress_device_many reports for the same bytes, a dictionary of dict_len bytes and
 *                  unlimited out_cap[f] — also the partial length of a frame that stops early (block checksum, codec error, a
 *                  block that decodes past block_maxsize, an empty block, truncated input).
 *   d_status[f]    that call's status, with ONE exception: the content checksum is not verified (it needs the content), so a
 *                  frame that would end in LZF_F_FRAME_CHECKSUM_FAIL reports LZF_OK.  Block checksums ARE verified: they
 *                  decide where delivery stops, hence the size.  Never LZF_OUT_CAPACITY and never LZF_E_NO_MEMORY: a frame
 *                  too large for the memory budget to decode still gets its size.
 *   d_consumed[f]  that call's consumed.
 * Only the dictionary's length matters (every block's decode may reach dict_len bytes behind its output); no dictionary bytes
 * are passed.  The host waits twice, as for the decode (scan summary, block table), then enqueues block checksums
 * (lzf_xxh32_batch), lzf_decompressed_size_batch over the blocks (linked frames in lock-step, history carried as a length) and
 * the decode's stop rules, waits for its own upload of job lists and returns.  Scratch (jobs, results, 24 bytes per block, and what
 * lzf_decompressed_size_batch takes for a call of few large blocks: about 1.2 bits per compressed byte of the largest block x blocks,
 * which a pool that is short of memory may refuse without changing any result) comes from the stream-ordered pool and does not
 * depend on the decoded sizes. */
int lzf_frame_decompressed_size_device(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len,
                                       size_t dict_len,
                                       uint64_t* d_out_len, uint64_t* d_consumed, int32_t* d_status,
                                       void* hip_stream);
/* "Does this frame deliver exactly these bytes?" per frame, WITHOUT decoding it: no output memory, no delivery copy.  For callers
 * who compress on the device and then free the only copy of the input — verify the frame first.  Conventions of
 * lzf_frame_decompressed_size_device: d_in / in_len / d_expected / expected_len are HOST arrays, d_in[f] and d_expected[f] DEVICE
 * addresses (d_expected[f] may be NULL where expected_len[f] is 0); d_at, d_consumed (may be NULL), d_status are DEVICE arrays
 * written in stream order; d_dict / dict_len: the dictionary in device memory, NULL = none.  Per frame, in this order:
 *   1. st = what lzf_frame_decompressed_size_device reports (block checksums verified, the content checksum not).  If it is not
 *      LZF_OK: d_status = st, d_at = that call's out_len.
 *   2. otherwise the delivered content, out_len bytes, is compared with d_expected[f][0, expected_len[f]): a first differing
 *      position, or lengths that differ, give LZF_MISMATCH with d_at = that position, or the shorter length.
 *   3. otherwise, where the reader reached the EndMark and the frame carries a content checksum, XXH32 of the EXPECTED bytes (the
 *      chain the compress call runs over its input, lzf_xxh32_batch: ~1.3 GB/s per frame, many frames at once) is compared with
 *      the stored word: LZF_F_FRAME_CHECKSUM_FAIL, d_at = out_len.
 *   4. otherwise LZF_OK, d_at = out_len.
 * d_consumed[f] is the size query's.  Behind the size query's own work every delivered block becomes one job of
 * lzf_decompress_verify_batch (include/lzfear_hip.h) — against known plaintext block k's history is the expected bytes in front of
 * it, so the blocks of a linked frame are verified side by side, in one call with every other frame's, with no lock-step — or,
 * stored, one compared range; one wavefront per frame takes the first failing block.  The host waits as the size query does and
 * no more.  Scratch: the size query's, plus 48 + 120 bytes per block and 4 per frame, from the stream-ordered pool; none of it
 * depends on the decoded sizes.  Only the expected bytes, the frames and the dictionary are read. */
int lzf_frame_verify_device(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len,
                            const uint8_t* d_dict, size_t dict_len,
                            const uint8_t* const* d_expected, const size_t* expected_len,
                            uint64_t* d_at, uint64_t* d_consumed, int32_t* d_status, void* hip_stream);
/* "What are the first target[f] bytes of this frame?" per frame, decoding no further: the frame form of lzf_decompress_head_batch
 * (include/lzfear_hip.h), for a record header, a dtype/shape preamble, a file magic out of thousands of frames.  Conventions of
 * lzf_frame_decompress_device_many: d_in / in_len / d_out / target are HOST arrays, d_in[f] / d_out[f] DEVICE addresses at any
 * alignment (d_out[f] may be NULL where target[f] is 0); frames may alias each other, outputs must not overlap each other or any
 * input; d_out_len / d_status are DEVICE arrays written in stream order; d_dict / dict_len: the dictionary in device memory,
 * NULL = none.  The rule (csrc/lzf_frame_head_rules.h, one definition for the kernel and the CPU tests), with pos = the bytes
 * delivered when the reader's decode_block is entered:
 *   - the header is parsed always, also for target 0; a header that fails gives its status with out_len 0;
 *   - the reader ends with LZF_OK in front of the first block entered at pos >= target[f]: that block's length word and everything
 *     behind it is never looked at, malformed or not;
 *   - a block entered at pos < target[f] is read as the reader reads it: the EndMark (its content checksum word must be there, else
 *     LZF_F_INPUT_ERROR, but is not compared) ends the frame with LZF_OK and out_len = pos — the frame ended first;
 *     LZF_F_BLOCK_SIZE_OVERFLOW for a length word above block_maxsize; LZF_F_INPUT_ERROR where the payload or its checksum word is
 *     cut off.  A stored block's bytes below the target are copied.  A compressed block goes through the head walk of
 *     lzf_decompress_head_batch on the job the decode states for it; a codec status 1..4 ends the frame with that status and
 *     out_len = pos, the length in front of the failing block (bytes below the target may have been written);
 *   - behind a block that ended in front of the target the reader's remaining stops apply: more than block_maxsize bytes is
 *     LZF_F_BLOCK_SIZE_OVERFLOW, an empty block ends the frame with LZF_OK, both with out_len = pos.  A block that reaches the
 *     target is asked neither question: an error at or behind the target is not seen, as in the raw call;
 *   - LZF_OK with out_len = min(pos reached, target[f]).  out_len < target[f]: the frame ended first; out_len == target[f] does not
 *     say whether more follows.  No byte at or beyond d_out[f] + target[f] is written.
 * THE CHECKSUM EXCEPTION: block checksums are stepped over and the content checksum is not compared.  The size, verify and decode
 * calls verify block checksums; this call is for reading a preamble, and hashing a 4 MiB block at ~1.3 GB/s to read 64 bytes of
 * it would cost 3 ms, the whole point of the call lost.  A frame whose block 0 is damaged reports LZF_OK here and the damaged
 * bytes, and LZF_F_BLOCK_CHECKSUM_FAIL from lzf_frame_decompressed_size_device.
 * Contract: a target of 2 GiB - 256 or more is LZF_CONTRACT for that frame with nothing read (a head is short; with that bound no
 * position of the walk leaves the decoder's 31-bit contract); a dictionary of that length is LZF_CONTRACT where a compressed block
 * is entered.
 * Cost: one wavefront per frame (lzf_frame_head_kernel), as many workgroups as the device holds at once drawing frames from a
 * 4-byte ticket; a frame costs what its target asks for, not what it holds, and a target that spans many blocks is decoded at one
 * wavefront's rate — correct, not meant to be fast.  The host packs the four arrays into one upload, enqueues the kernel, waits
 * only for that upload to leave host memory and returns: nothing is read back, nothing is scanned or planned.  Scratch: 32 bytes
 * per frame and the ticket, from the stream-ordered pool.
 * Measured on one MI355X against the parent commit's library decoding the frames whole and copying the heads
 * (lzf_frame_decompress_device_many + lzf_copy_ranges; profiles/frame_head.txt): 980 frames of one 4 MiB block 0.13 ms against
 * 20.5 at 64 bytes and 0.18 ms against 20.5 at 4 KiB; 49 frames of 20 x 4 MiB blocks 0.057 ms against 66.6 at 64 bytes; one linked
 * frame of 16 x 4 MiB 0.049 ms against 102.4 at 64 bytes and 53.4 ms against 102.5 at 4 MiB + 64; 30 000 frames of 64 KiB at 256
 * bytes 0.59 ms against 16.2.  CROSSOVER for the 980 frames, the smallest target of the sweep at which decoding whole and slicing
 * is not slower: 1 MiB (16.2 ms against 20.8 at 768 KiB, 25.9 ms against 20.9 at 1 MiB; the whole 4 MiB takes 85.3 ms against 21.9). */
int lzf_frame_head_device(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len,
                          const uint8_t* d_dict, size_t dict_len,
                          uint8_t* const* d_out, const size_t* target,
                          uint64_t* d_out_len, int32_t* d_status, void* hip_stream);
/* lzf_frame_compress_many for inputs that live in device memory, compressed into device memory: compress_internal
 * (src/framed/compress.rs:160-282) of every frame with the settings `s` (a host struct, shared by all frames as in
 * lzf_frame_compress_many: flags, dictionary id and content size of the header come from it).  s->dictionary must be NULL
 * (else LZF_E_INVALID: no host pointer reaches a kernel); the dictionary is d_dict / dict_len in device memory, NULL = none.
 *   d_in, in_len, d_out, out_cap: HOST arrays of n_frames entries; d_in[f] / d_out[f] are DEVICE addresses at any alignment.
 *     Inputs may alias each other; outputs must not overlap each other or any input.
 *   d_out_len, d_status: DEVICE arrays of n_frames entries, written in stream order on `hip_stream`.
 * Per frame the status, out_len and bytes are those of lzf_frame_compress_many with the same settings, dictionary bytes and
 * input: LZF_OUT_CAPACITY when out_cap[f] < lzf_frame_compress_bound(s, in_len[f]), LZF_F_INVALID_BLOCK_SIZE / LZF_F_PANIC on
 * every frame for a bad block size, and a block status other than LZF_OK / LZF_OUTPUT_FULL (stored raw) fails the frame with the
 * first such status in block order and out_len 0.  Nothing outside d_out[f][0, out_len) is written; a frame whose status is
 * not LZF_OK gets no writes at all.
 * The host plans the whole call from in_len[] and the settings and reads nothing back from the device: it enqueues the work,
 * waits for its own upload of job lists to leave host memory and returns; no host memory of the call is read after that.  Not
 * a goal: graph capture.  Scratch comes from the stream-ordered pool, freed in stream order.  Frames go through in passes of the
 * memory budget (lzf_frame_set_memory_budget) counted in scratch (output slots, dictionary copies, tables); a frame whose
 * scratch alone is over it is a pass of its own — the call never reports LZF_E_NO_MEMORY.  lzf_frame_stats is not touched and
 * no host-driver lock is taken, except to read the budget.  Checksums are computed on the device only: block checksums in one
 * launch per pass, content checksums over d_in[f] directly, one serial XXH32 chain per frame (~1.3 GB/s each, many frames at
 * once), so one huge frame with a content checksum is bounded by its chain.
 * Returns LZF_OK or a negative LZF_E_* (bad arguments, HIP failure, LZF_E_NO_DEVICE without a device: no CPU fallback). */
int lzf_frame_compress_device_many(const lzf_settings* s, uint32_t n_frames,
                                   const uint8_t* const* d_in, const size_t* in_len,
                                   const uint8_t* d_dict, size_t dict_len,
                                   uint8_t* const* d_out, const size_t* out_cap,
                                   uint64_t* d_out_len, int32_t* d_status, void* hip_stream);
/* lzf_frame_compressed_size_device is to lzf_frame_compress_device_many what lzf_frame_decompressed_size_device is to the decoder:
 * per frame the status and out_len that call reports for the same settings, dictionary bytes and input whenever out_cap[f] >=
 * lzf_frame_compress_bound — WITHOUT writing a frame.  It never reports LZF_OUT_CAPACITY; a bad block size gives
 * LZF_F_INVALID_BLOCK_SIZE / LZF_F_PANIC on every frame, and the first block status other than LZF_OK / LZF_OUTPUT_FULL, in
 * block order, fails the frame with out_len 0, as there.  Conventions of lzf_frame_compress_device_many: d_in / in_len are HOST
 * arrays of device addresses, d_out_len / d_status DEVICE arrays, s->dictionary must be NULL.
 * A frame's length does not depend on its checksums' VALUES, so no checksum is computed: neither lzf_xxh32_batch nor the serial
 * content chain is launched — with a content checksum in the settings the answer simply counts its 4 bytes.  The blocks go
 * through lzf_compressed_size_batch with out_cap = the block's length (the stored-block decision is the status), linked frames
 * in lock-step with lzf_table_offset_batch as in the compress call, and one wavefront per frame folds the block results into
 * the frame's length.  No output memory: the scratch is the compress call's WITHOUT its output slots — job lists, results, the
 * dictionary copies and the linked streams' tables, which are the call's own scratch tables — in passes of the memory budget.
 * Nothing of the caller's is written except d_out_len / d_status.  The host reads nothing back and waits only for its upload
 * of the job lists to leave host memory. */
int lzf_frame_compressed_size_device(const lzf_settings* s, uint32_t n_frames,
                                     const uint8_t* const* d_in, const size_t* in_len,
                                     const uint8_t* d_dict, size_t dict_len,
                                     uint64_t* d_out_len, int32_t* d_status, void* hip_stream);

/* ---- streams of back-to-back frames in device memory ------------------------------------------------------------------
 * "This also allows LZ4 frames to be concatenated back to back" (src/framed/mod.rs:6).  A content checksum is one serial XXH32
 * chain per frame, so a payload written as one frame per few MiB has one short chain per frame, and the chains run in
 * parallel.  A stream is in[0, len) holding zero or more frames back to back.  The rule is the loop a caller of
 * lzf_frame_decompress writes with `consumed`:
 *     pos = 0; out = 0; frames = 0; status = LZF_OK
 *     while pos < len:
 *         (st, n, c) = lzf_frame_decompress of in[pos, len) with the dictionary and the capacity out_cap - out
 *         out += n; pos += c
 *         if st != LZF_OK: status = st; break
 *         if the frame did not end at its EndMark: break         (the Read adapter's stop at an empty block: LZF_OK)
 *         frames += 1
 * Hence: an empty stream is LZF_OK, 0, 0, 0; 1-3 trailing bytes are LZF_F_INPUT_ERROR with consumed = len; 4 or more trailing
 * bytes that are not the magic (skippable and legacy frames too: the reference knows neither) are LZF_F_WRONG_MAGIC with
 * consumed = pos + 4; a truncated last frame is LZF_F_INPUT_ERROR with the output of its complete blocks; LZF_OUT_CAPACITY
 * comes at the block where the per-frame call with the remaining capacity reports it.
 *
 * lzf_frame_decompress_stream_device: conventions of lzf_frame_decompress_device_many.  d_in, in_len, d_out, out_cap are HOST
 * arrays of n_streams entries holding DEVICE addresses; streams may alias each other, outputs must not overlap each other or
 * any input.  d_out_len, d_consumed, d_status and d_n_frames (may be NULL; the frames that ended at their EndMark with LZF_OK)
 * are DEVICE arrays of n_streams entries, written in stream order on `hip_stream`.  One dictionary per call.  A frame that does
 * not fit the memory budget alone ends its stream with LZF_E_NO_MEMORY, the output of the frames before it stands.
 * Nothing outside d_out[s][0, out_cap[s]) is ever written, and nothing beyond out_len[s] — with one exception: when a stream
 * ends in LZF_F_FRAME_CHECKSUM_FAIL, the frames behind the failing one may have been placed already (the checksum is computed
 * from the delivered bytes), and [out_len, out_cap) is unspecified.
 * The host waits four times on the stream: for the frame count of every stream and for the frames' start offsets (the stream
 * scan, one lane per stream, run twice), then, as lzf_frame_decompress_device_many, for the per-frame scan summary and the
 * block table.  Where a frame goes is decided on the device: behind the decode a count-only delivery finds every frame's
 * length, one wavefront per stream prefixes them and applies the rule above, then the delivery, the copy and the content
 * checksums run as for single frames and a last kernel folds the frames' results into the streams'.  Frames go through in
 * passes of the memory budget; a stream may span passes.  Not graph-capturable.
 * lzf_frame_stream_bound_device: per stream the sum over the frames the walk finds of lzf_frame_decompress_bound_device's
 * bound; with out_cap[s] at least that no stream ends in LZF_OUT_CAPACITY.  Synchronous (three waits). */
int lzf_frame_stream_bound_device(uint32_t n_streams, const uint8_t* const* d_in, const size_t* in_len,
                                  size_t* out_bound, void* hip_stream);
int lzf_frame_decompress_stream_device(uint32_t n_streams, const uint8_t* const* d_in, const size_t* in_len,
                                       const uint8_t* d_dict, size_t dict_len,
                                       uint8_t* const* d_out, const size_t* out_cap,
                                       uint64_t* d_out_len, uint64_t* d_consumed, int32_t* d_status, uint64_t* d_n_frames,
                                       void* hip_stream);

/* ---- exact sizes and a frame index of streams, found without decoding --------------------------------------------------
 * lzf_frame_stream_decompressed_size_device is to lzf_frame_decompress_stream_device what lzf_frame_decompressed_size_device is
 * to lzf_frame_decompress_device_many: per stream the status, out_len, consumed and n_frames that call reports for the same
 * bytes, a dictionary of dict_len bytes and unlimited out_cap[s] — with the size query's ONE exception: the content checksum is
 * not verified, so a frame that would end its stream with LZF_F_FRAME_CHECKSUM_FAIL counts as LZF_OK and the stream goes on
 * behind it.  Never LZF_OUT_CAPACITY and never LZF_E_NO_MEMORY: no output slots, one pass whatever the memory budget is.
 * On request it also lists the frames.  Entry k of stream s describes the k-th frame the structural walk finds (the failing
 * last one included), with the frame size query's own results for in[in_off, len):
 *   out_off   the sum of out_len over the frames before it: where the decode call puts its output.
 *   flags     LZF_SFRAME_COMPLETE: the frame ended at its EndMark with LZF_OK.  The first frame without it ends the stream
 *             (its own out_len and consumed still count, as in the rule above); every frame behind that one has
 *             LZF_SFRAME_BEHIND_STOP and out_off = the stream's out_len: the walk found it, the decode call never reaches it.
 * A run of whole frames is itself a stream: in[in_off of frame i, in_off + consumed of frame j) decodes, with
 * lzf_frame_decompress_stream_device, to bytes [out_off of i, out_off + out_len of j) of the stream's output, and only the
 * content checksums of the frames i..j are then verified.  lzf_stream_index_locate finds i and j for a byte range.
 * Conventions of lzf_frame_decompress_stream_device: d_in, in_len are HOST arrays of n_streams entries holding DEVICE addresses;
 * streams may alias each other.  d_index / index_cap: HOST arrays of n_streams entries, d_index[s] the DEVICE address (8-byte
 * aligned) of room for index_cap[s] entries; at most index_cap[s] entries are written and nothing behind them; both NULL: sizes
 * only.  d_out_len, d_consumed, d_status, d_n_frames (may be NULL; the decode call's count) and d_n_listed (may be NULL; the
 * frames found, whatever the capacity — lzf_frame_stream_count_device's number) are DEVICE arrays of n_streams entries, written
 * in stream order on `hip_stream`.  The host waits four times, as for the decode: twice for the stream scan, then for the
 * per-frame scan summary and the block table; it then enqueues the frame size query's work over all frames, the fold of the
 * frames' results into the streams' (the decode call's own kernel) and one index kernel (one wavefront per stream: a prefix of
 * the lengths, the stop, the entries), waits for its own small upload and returns.  No host memory of the call is read after
 * it returns.  An empty call is LZF_OK; an empty stream is LZF_OK, 0, 0, 0 with 0 frames listed.  Not graph-capturable. */
#define LZF_STREAM_NO_CONTENT_SIZE 0xFFFFFFFFFFFFFFFFull
#define LZF_SFRAME_COMPLETE    1u   /* ended at its EndMark with LZF_OK (content checksum not verified) */
#define LZF_SFRAME_BEHIND_STOP 2u   /* the stream rule never reaches it: an earlier frame ended the stream */
typedef struct lzf_stream_frame {   /* 48 bytes */
    uint64_t in_off;        /* the frame is in[in_off, len) as its reader sees it */
    uint64_t consumed;      /* lzf_frame_decompressed_size_device's consumed for it: the next frame starts at in_off + consumed */
    uint64_t out_off;       /* where its output starts in the stream's output */
    uint64_t out_len;       /* lzf_frame_decompressed_size_device's out_len for it, with dict_len */
    uint64_t content_size;  /* the header's content size field; LZF_STREAM_NO_CONTENT_SIZE when absent or the header fails */
    int32_t  status;        /* lzf_frame_decompressed_size_device's status for it */
    uint32_t flags;         /* LZF_SFRAME_* */
} lzf_stream_frame;
/* Frames the walk finds per stream (the failing last one included): the entries the index call can list.  n_found: a HOST
 * array.  Synchronous, one wait (the stream scan's first launch). */
int lzf_frame_stream_count_device(uint32_t n_streams, const uint8_t* const* d_in, const size_t* in_len,
                                  size_t* n_found, void* hip_stream);
int lzf_frame_stream_decompressed_size_device(uint32_t n_streams, const uint8_t* const* d_in, const size_t* in_len,
                                              size_t dict_len,
                                              lzf_stream_frame* const* d_index, const size_t* index_cap,
                                              uint64_t* d_out_len, uint64_t* d_consumed, int32_t* d_status,
                                              uint64_t* d_n_frames, uint64_t* d_n_listed,
                                              void* hip_stream);
/* Host only, no device: frames [*first, *first + *count) of an index (a host copy of n entries) whose output meets the bytes
 * [a, b) of the stream's output: out_off < b && out_off + out_len > a, among the entries without LZF_SFRAME_BEHIND_STOP.  A
 * binary search.  a >= b, or no frame meets the range (n == 0, a range wholly behind the output): *count = 0.  The first and
 * the last frame of the result have bytes in the range: frames of zero length are never at its edges.  Byte ranges stay out of
 * the ABI: decode the frames, slice the output.  LZF_OK, or LZF_E_INVALID for a NULL argument. */
int lzf_stream_index_locate(const lzf_stream_frame* index, size_t n, uint64_t a, uint64_t b, size_t* first, size_t* count);

/* ---- the block index of a frame, and the decode of runs of its blocks ----------------------------------------------------
 * The stream index gives random access frame by frame; a frame of independent blocks (what compress writes by default: one
 * frame of 4 MiB blocks, src/framed/compress.rs:44-55) gives it block by block: every block decodes on its own, behind the
 * dictionary alone.  lzf_frame_block_index_device is lzf_frame_decompressed_size_device that also lists the blocks;
 * lzf_block_index_locate finds the blocks that hold a byte range; lzf_frame_decompress_blocks_device decodes runs of
 * consecutive blocks straight to their places.  Byte ranges stay out of the ABI: decode the blocks, slice the output.
 *
 * Entry k of frame f describes block k of the structural walk (lzf_frame_block_count_device's number; truncated input ends the
 * list where the walk ends; 0 entries for a frame whose header fails):
 *   in_off, in_len, want_sum, block_maxsize   where the payload lies in the frame, the checksum word behind it, the header's size
 *   out_off   the sum of out_len over the blocks before it: where the decode puts its output.
 *   out_len   the block's exact decoded length, a dictionary of dict_len bytes behind it (a stored block: in_len).  Unspecified
 *             where status is a codec error or LZF_F_BLOCK_CHECKSUM_FAIL, and behind a stop in a linked-block frame.
 *   status    what the block does to the reader on its own: LZF_OK, a codec error 1..4, LZF_F_BLOCK_CHECKSUM_FAIL, or
 *             LZF_F_BLOCK_SIZE_OVERFLOW (it decodes past block_maxsize).
 *   flags     LZF_FBLOCK_DELIVERED: the reader delivers the block: neither it nor a block before it stops the frame.  The first
 *             block without it is the stopping one (a status other than LZF_OK, or the empty block at which the Read adapter
 *             stops, which is LZF_OK): its status is the frame's, its out_off the frame's out_len.  Every block behind it has
 *             LZF_FBLOCK_BEHIND_STOP and out_off = the frame's out_len.  Every block of a linked-block frame has
 *             LZF_FBLOCK_LINKED: its sizes come from the size query's lock-step chain, and it decodes only behind the blocks
 *             before it.
 * Conventions of lzf_frame_decompressed_size_device: d_in / in_len are HOST arrays, d_in[f] a DEVICE address.  d_index /
 * index_cap: HOST arrays of n_frames entries, d_index[f] the DEVICE address (8-byte aligned) of room for index_cap[f] entries;
 * at most index_cap[f] entries are written and nothing behind them; both NULL: sizes only.  d_out_len, d_consumed (may be NULL)
 * and d_status are exactly what lzf_frame_decompressed_size_device reports for the same bytes and dict_len — its one exception
 * included: the content checksum is not verified; d_n_listed (may be NULL): the blocks found, whatever the capacity.  All four are
 * DEVICE arrays written in stream order.  The host waits as the size query does (scan summary, block table) and no more; behind
 * the size query's own work one more kernel, one wavefront per frame, runs the delivery's stop rules again and writes the
 * entries.  Not graph-capturable. */
#define LZF_FBLOCK_STORED      1u   /* stored raw: the run decode copies it */
#define LZF_FBLOCK_HAS_SUM     2u   /* a block checksum word follows the payload */
#define LZF_FBLOCK_LINKED      4u   /* linked-block frame: needs the blocks before it */
#define LZF_FBLOCK_DELIVERED   8u   /* the reader delivers this block: no stop at it or before it */
#define LZF_FBLOCK_BEHIND_STOP 16u  /* an earlier block stopped the frame; out_off = the frame's out_len */
typedef struct lzf_frame_block {    /* 48 bytes */
    uint64_t in_off;        /* payload start in the frame (behind the length word) */
    uint64_t out_off;       /* where the block's output starts in the frame's output */
    uint64_t out_len;       /* exact decoded length (stored: in_len); unspecified on a codec error */
    uint32_t in_len;        /* payload bytes */
    uint32_t want_sum;      /* the checksum word, 0 without HAS_SUM */
    uint32_t block_maxsize;
    int32_t  status;        /* what this block does to the reader: LZF_OK, 1..4, LZF_F_BLOCK_CHECKSUM_FAIL,
                               LZF_F_BLOCK_SIZE_OVERFLOW; the stopping block carries the frame's status */
    uint32_t flags;         /* LZF_FBLOCK_* */
    uint32_t reserved;      /* 0 */
} lzf_frame_block;
/* Blocks the structural walk finds per frame (0 for a header that fails): the entries the index call can list.  n_found: a HOST
 * array.  Synchronous, one wait (the scan summary). */
int lzf_frame_block_count_device(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len,
                                 size_t* n_found, void* hip_stream);
int lzf_frame_block_index_device(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len, size_t dict_len,
                                 lzf_frame_block* const* d_index, const size_t* index_cap,
                                 uint64_t* d_out_len, uint64_t* d_consumed, int32_t* d_status, uint64_t* d_n_listed,
                                 void* hip_stream);
/* Host only, no device: blocks [*first, *first + *count) of an index (a host copy of n entries) whose output meets the bytes
 * [a, b) of the frame's output, among the LZF_FBLOCK_DELIVERED entries.  lzf_stream_index_locate's search and semantics: a >= b,
 * n == 0 or a range wholly behind the delivered output give *count = 0; blocks of zero length are never at an edge of the
 * result.  LZF_OK, or LZF_E_INVALID for a NULL argument. */
int lzf_block_index_locate(const lzf_frame_block* index, size_t n, uint64_t a, uint64_t b, size_t* first, size_t* count);
/* Decodes runs of consecutive blocks.  Run r is count[r] consecutive entries of the index of the frame at d_in[r] (in_len[r]
 * bytes), given as HOST copies: runs[r] points at them.  Block k of the run is decoded to d_out[r] + (e[k].out_off -
 * e[0].out_off); the run's total is the sum of its out_len.  d_in, in_len, runs, count, d_out, out_cap: HOST arrays of n_runs
 * entries; d_in[r], d_out[r], d_dict: DEVICE addresses.  Runs may share a frame; outputs must not overlap each other or any
 * input.  d_out_len, d_status: DEVICE arrays of n_runs entries, written in stream order.
 * The host plans everything from the entries and reads nothing back: no wait except for its own upload of job lists.  A call
 * that holds an entry without LZF_FBLOCK_DELIVERED or with LZF_FBLOCK_LINKED (block k of a linked frame needs every block before
 * it: decode the frame), in_off + in_len (+ 4 with HAS_SUM) beyond in_len[r], in_len or out_len above block_maxsize, a stored
 * block whose out_len is not its in_len, or out_off values that are not contiguous enqueues nothing and returns LZF_E_INVALID.
 * out_cap[r] below the run's total gives that run LZF_OUT_CAPACITY, out_len 0 and no writes; count[r] == 0 is LZF_OK, 0.
 * Enqueued: the block checksums (lzf_xxh32_batch over the payloads, compared with the word read from the input on the device,
 * not with the entry's copy), the decode (lzf_decompress_batch_sized, every block at its final place with out_cap =
 * output_limit = out_len and d_dict as its prefix), the stored copies (lzf_copy_ranges) and one kernel, one wavefront per run,
 * that folds the results.  No output slots, no delivery copy, no passes of the memory budget; scratch (jobs, results, sums)
 * comes from the stream-ordered pool.
 *   d_status[r]   the first of, in block order: LZF_F_BLOCK_CHECKSUM_FAIL; a codec status 1..4; LZF_CONTRACT where a block's
 *                 result differs from its entry (another decoded length, or no room in out_len bytes: the index does not
 *                 describe these bytes).  LZF_OK otherwise.
 *   d_out_len[r]  the bytes of the blocks before that one, or the total on LZF_OK.
 * Nothing outside d_out[r][0, total) is ever written; behind a failing block [d_out_len, total) is unspecified.
 * The content checksum is NEVER verified by this call: it needs the whole content.  lzf_frame_decompress_device_many remains
 * the call that verifies it.  Not graph-capturable. */
int lzf_frame_decompress_blocks_device(uint32_t n_runs, const uint8_t* const* d_in, const size_t* in_len,
                                       const lzf_frame_block* const* runs, const size_t* count,
                                       const uint8_t* d_dict, size_t dict_len,
                                       uint8_t* const* d_out, const size_t* out_cap,
                                       uint64_t* d_out_len, int32_t* d_status, void* hip_stream);

/* ---- resumable decode of frames in device memory: the device counterpart of lzf_frame_reader -----------------------------
 * LZ4FrameReader::decode_block hands out one block at a time and into_read pulls a frame of any length through a fixed buffer
 * (src/framed/decompress.rs:198-288).  lzf_frame_resume_device is that reader for frames in device memory: a cursor per frame
 * that the caller comes back to.  One call decodes as many whole blocks as fit the room given, carries the 64 KiB window of a
 * linked-block frame (:238-269) and the running content hash between calls, verifies the content checksum at the EndMark like
 * lzf_frame_decompress_device_many, and treats "the input ends here" as COME BACK WITH MORE, not as an error.  So a frame whose
 * output slots are over the memory budget decodes piece by piece, a frame still arriving can be started, and a linked-block
 * frame decodes by runs with its content checksum verified.
 * Conventions of lzf_frame_decompress_device_many: d_in, in_len, d_out, out_cap are HOST arrays of n_frames entries holding
 * DEVICE addresses; d_out_len, d_consumed, d_status and d_phase are DEVICE arrays written in stream order; one dictionary per
 * call.  d_cursors: n_frames x lzf_frame_cursor_bytes() bytes of DEVICE memory, 16-byte aligned, cursor f at d_cursors + f x
 * lzf_frame_cursor_bytes().  A cursor is opaque; all zero = the start of a frame.  It holds the header's fields once parsed, the
 * input offset of the next unread item, the bytes delivered so far, the sticky status and phase, the content hash's
 * lzf_xxh32_state and, for linked-block frames, the reader's window: the last <= 64 KiB of (dictionary tail ++ everything
 * delivered), in two buffers used in turn.  The caller passes the same frame bytes (in_len may have grown), the same dictionary
 * and the same cursor on every call; d_out and out_cap are free to differ per call, and an output buffer may be reused once its
 * bytes are consumed.  Cursors of one call must not alias; calls that share a cursor must be ordered by the caller.
 * The rule of one call, per frame (csrc/lzf_frame_resume_rules.h, one definition for the kernels and the CPU tests):
 *   1. A cursor in phase LZF_RESUME_DONE delivers nothing: out_len 0, status and consumed as they were; no byte of the frame is read.
 *   2. A fresh cursor parses the header as LZ4FrameReader::new does.  A header error is DONE with that status and consumed, as
 *      the whole-frame call reports them; a header cut off by in_len is NEED_INPUT with consumed 0, and the cursor stays fresh.
 *   3. Blocks are taken in order, the reader's way: the length word (the EndMark ends the frame, step 6; a length above
 *      block_maxsize is LZF_F_BLOCK_SIZE_OVERFLOW: DONE, consumed behind the word), then the payload and its checksum word, which
 *      must lie inside in_len: a block that is cut off ends the call with NEED_INPUT in front of its length word.  A whole block
 *      is taken while its BOUND, compressed ? min(255 x len + 16, block_maxsize) : len (lzf_frame_decompress_bound_device's
 *      term), fits what is left of out_cap[f]; the first block that does not fit ends the call with LZF_RESUME_MORE in front of
 *      it.  The piece is the longest such run, decided from length words alone.  No length word behind the first block that
 *      does not fit or is cut off is read: a call's scan costs what its piece costs.  If the very first block of the call does
 *      not fit, the call reports LZF_OUT_CAPACITY with phase MORE, out_len 0 and the cursor untouched (consumed as it was): that
 *      status is not sticky, more room cures it.
 *   4. The piece's blocks go through the whole-frame call's stages: block checksums, the decode (independent blocks behind the
 *      dictionary, linked blocks behind the cursor's window and the piece so far, in lock-step), the delivery's stop rules
 *      (block checksum, codec status, more than block_maxsize bytes, the empty block).  The first stop in block order makes the
 *      frame DONE with its status and consumed = the end of the stopping block; the bytes of the blocks in front of it are
 *      delivered, packed, to d_out[f][0, out_len).  Nothing at or beyond d_out[f] + out_len is written.
 *   5. The delivered bytes update the content hash (lzf_xxh32_update_batch) and, for linked frames, the window.
 *   6. At the EndMark, with a content checksum in the header, the stored word is compared with the digest:
 *      LZF_F_FRAME_CHECKSUM_FAIL on a difference (the bytes of the call are delivered all the same).  A checksum word cut off by
 *      in_len is NEED_INPUT in front of the EndMark.  Then DONE.
 *   7. d_out_len[f]: the bytes of THIS call.  d_consumed[f]: the input offset the cursor now stands at, counted from the start
 *      of the frame — the start of the next unread item, which in NEED_INPUT is the start of the incomplete one.  d_status[f]:
 *      LZF_OK unless a rule above says otherwise.  d_phase[f]: LZF_RESUME_*.
 * THE CONTRACT: for capacities that are each at least the largest block bound of the frame and an in_len that grows to the full
 * length, the concatenation of the calls' outputs, the last status and the last consumed are exactly what
 * lzf_frame_decompress_device_many reports for the full bytes with unlimited capacity.  THE ONE DIFFERENCE: where in_len never
 * reaches the end of the frame, the frame rests in NEED_INPUT with LZF_OK — the bytes delivered are the whole-frame call's
 * out_len bytes for the cut input, but LZF_F_INPUT_ERROR is the caller's to report once it knows that no more input comes, and
 * consumed is the start of the incomplete item, not in_len.
 * The host waits twice on the stream, as the whole-frame call does: for a 64-byte summary per frame that the bounded walk
 * (one lane per frame, from the cursor's offset, reading the cursor itself: the host never reads a cursor) writes, and for the
 * block table of the pieces (24 bytes per block).  It then enqueues block checksums, decode, delivery, the copies, the hash
 * update, the digest and one kernel per call that moves the cursors and the windows, waits for its own upload of job lists
 * to leave host memory and returns.  Scratch comes from the stream-ordered pool and follows out_cap and the piece's input,
 * never the frame: the call never reports LZF_E_NO_MEMORY.  Pieces over the memory budget go through in passes; a piece over
 * it alone is a pass of its own.  No global state, no host-driver lock except to read the budget.  Not graph-capturable.
 * Every call pays the two waits, so small pieces are slow: tools/frame_resume_bench.py measures pieces against the whole-frame
 * call (profiles/frame_resume.txt).  Returns LZF_OK or a negative LZF_E_*. */
#define LZF_RESUME_MORE        0u  /* stopped in front of a block whose bound does not fit what is left of out_cap */
#define LZF_RESUME_NEED_INPUT  1u  /* in[0, in_len) ends inside the header, the next block (its checksum word included),
                                      or the content checksum: nothing of that item was consumed */
#define LZF_RESUME_DONE        2u  /* terminal: EndMark read and content checksum verified, the empty-block stop, or an
                                      error status; sticky */
size_t lzf_frame_cursor_bytes(void);         /* device bytes per cursor, a multiple of 256; all zero = start of a frame */
int lzf_frame_resume_device(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len,
                            const uint8_t* d_dict, size_t dict_len,
                            void* d_cursors,                      /* n_frames x lzf_frame_cursor_bytes(), DEVICE */
                            uint8_t* const* d_out, const size_t* out_cap,
                            uint64_t* d_out_len, uint64_t* d_consumed, int32_t* d_status, uint32_t* d_phase,
                            void* hip_stream);

/* ---- streaming frame writer in device memory ---------------------------------------------------------------------------------
 * The reference's compressor is incremental by construction: compress_internal (src/framed/compress.rs:221-276) reads
 * block_size bytes per turn and carries the table and the last 64 KiB.  lzf_frame_append_device is that writer for inputs in
 * device memory: a write cursor per frame that the caller comes back to with the next bytes of the stream.  A frame longer than
 * the memory the caller can spare for input plus bound, a frame whose bytes appear on the device over time and a linked-block
 * frame fed by runs are written this way; lzf_frame_resume_device reads them back the same way.
 * Conventions of lzf_frame_compress_device_many: d_in, in_len, flags, d_out, out_cap are HOST arrays of n_frames entries (device
 * addresses at any alignment); d_out_len, d_taken, d_status, d_phase are DEVICE arrays of n_frames entries, written in stream
 * order.  s->dictionary must be NULL (LZF_E_INVALID); one `s` and one dictionary per call, and the caller passes the same ones on
 * every call of a cursor.  d_cursors: n_frames x lzf_frame_wcursor_bytes() bytes of DEVICE memory, 16-byte aligned, cursor f at
 * d_cursors + f x lzf_frame_wcursor_bytes().  A cursor is opaque; all zero = nothing written yet.  It holds whether the header is
 * out, the bytes taken so far, the sticky status and phase, the content hash's lzf_xxh32_state and, for linked-block frames, the
 * stream's lzf_u32_table and the writer's window: the last 64 KiB of what was taken.  Cursors of one call must not alias; calls
 * that share a cursor are ordered by the caller; d_in[f] of one call may be reused once that call's work is done in stream order.
 * The rule of one call, per frame (csrc/lzf_frame_append_rules.h, one definition for the kernels, the host and the CPU tests):
 *   1. A cursor in phase LZF_APPEND_DONE writes nothing: out_len 0, taken 0, status as it was.
 *   2. A bad block size makes the frame DONE with LZF_F_INVALID_BLOCK_SIZE / LZF_F_PANIC, as in the whole call.
 *   3. What is taken is decided from host arguments alone.  With bs = s->block_size the offer d_in[f][0, in_len[f]) is cut as
 *      the reference cuts it: whole blocks of bs from its start, plus a shorter last block only under LZF_APPEND_FINISH.  The call
 *      takes the longest run of these blocks whose bytes t satisfy lzf_frame_compress_bound(s, t) <= out_cap[f] (the bound always
 *      counts header, EndMark and checksum words: slightly conservative for a cursor whose header is out).  d_taken[f] = t.
 *   4. If not even the first block fits — or, under FINISH with nothing to take, out_cap[f] < lzf_frame_compress_bound(s, 0) —
 *      the call reports LZF_OUT_CAPACITY with phase MORE and taken 0; the cursor is untouched and the status is not sticky.
 *   5. If fewer than bs bytes are offered without FINISH, nothing is taken or written, the cursor is untouched and the phase is
 *      NEED_INPUT: the caller offers those bytes again together with what follows them.
 *   6. A cursor whose header is not out writes the header first (:163-200; content size from `s`).  Every taken block then goes
 *      through the whole call's stages: independent blocks each behind the dictionary and the read-only template table; linked
 *      blocks in lock-step over the frames of the call, block 0 of a call behind the whole dictionary on a fresh cursor and
 *      behind the cursor's window otherwise, later blocks behind the caller's input, the stream's table (seeded from the template
 *      on a fresh cursor) carried by the cursor with table.offset(forget) (:271-275) applied between blocks and across the call
 *      boundary.  Per block: the length word (stored on LZF_OUTPUT_FULL), the payload, the optional block checksum.
 *   7. A block status other than LZF_OK / LZF_OUTPUT_FULL makes the frame DONE with the first such status in block order; no
 *      byte of this call is written for that frame, out_len and taken are 0.
 *   8. The taken bytes update the content hash; for linked frames the window becomes the last 64 KiB of the taken bytes.
 *   9. If FINISH is set and the whole offer was taken, the call writes the EndMark and, with a content checksum, the digest; DONE.
 *  10. Otherwise the phase is MORE if a block was left for lack of room, NEED_INPUT if only a part-block or nothing is left.
 *  11. Everything is packed into d_out[f][0, out_len); nothing at or beyond d_out[f] + out_len is written.
 * THE CONTRACT: for any cut of an input into offers (untaken tails offered again), any capacities of at least
 * lzf_frame_compress_bound(s, bs) and FINISH on the final offer, the concatenation of the calls' outputs is byte for byte the
 * frame lzf_frame_compress_device_many writes for the concatenated input with the same settings and dictionary, and the sum of
 * taken is the input's length.
 * The host plans from in_len, flags, out_cap and `s` alone: it never reads a cursor, reads nothing back, waits only for its own
 * upload of job lists to leave host memory and never reports LZF_E_NO_MEMORY.  So a DONE cursor costs the compression of its
 * offer and writes nothing.  Three kernels settle what depends on the cursor: a prepare kernel (block 0's history, job and table
 * offsets, the table of a fresh cursor), the append form of the assembly kernel (header only when it is not out, EndMark only
 * when finishing) and a commit kernel that alone moves the cursors and copies the windows.  Scratch comes from the
 * stream-ordered pool and follows the offer, never the frame; offers over the memory budget go through in passes.  Not
 * graph-capturable.  Measured on one MI355X (tools/frame_append_bench.py, profiles/frame_append.txt; medians of 5): one call with
 * FINISH costs the whole call (49 inputs of 20 x 4 MiB blocks 312.5 ms against lzf_frame_compress_device_many's 312.1; one linked input
 * of 16 x 4 MiB 1614.4 against 1613.5); the linked input in pieces of 1 / 4 blocks 1612.5 / 1614.6 ms; the independent inputs in pieces
 * of 1 / 4 / 16 blocks 2246.1 / 632.7 / 452.0 ms (few blocks per call leave the device idle: offer many); the 64 MiB linked input under a
 * 32 MiB budget through one reused 4 MiB input buffer 1614.2 ms with 8.1 MiB of pool scratch at its peak (whole: 1611.7 ms, 68.1 MiB).
 * Not timed: offers below one block, capacities that leave blocks behind, dictionaries, a producer slower than the writer.
 * Returns LZF_OK or a negative LZF_E_*. */
#define LZF_APPEND_MORE        0u  /* stopped in front of a block whose bound does not fit what is left of out_cap */
#define LZF_APPEND_NEED_INPUT  1u  /* what is left of the offer is less than one block and FINISH is not set */
#define LZF_APPEND_DONE        2u  /* EndMark (and content checksum) written, or an error status; sticky */
#define LZF_APPEND_FINISH      1u  /* flags[f]: the offer ends the stream (the reader's short read / EOF, :227-231) */
size_t lzf_frame_wcursor_bytes(void);        /* device bytes per cursor, a multiple of 256; all zero = nothing written yet */
int lzf_frame_append_device(const lzf_settings* s, uint32_t n_frames,
                            const uint8_t* const* d_in, const size_t* in_len, const uint32_t* flags,
                            const uint8_t* d_dict, size_t dict_len,
                            void* d_cursors,                      /* n_frames x lzf_frame_wcursor_bytes(), DEVICE */
                            uint8_t* const* d_out, const size_t* out_cap,
                            uint64_t* d_out_len, uint64_t* d_taken, int32_t* d_status, uint32_t* d_phase,
                            void* hip_stream);

/* lzf_frame_compress_stream_device: input s becomes max(1, ceil(in_len[s] / frame_bytes)) frames, written back to back into
 * d_out[s]: the bytes are the concatenation of lzf_frame_compress_many's output for each piece of frame_bytes bytes (the last
 * one shorter) with the same settings and dictionary.  With s->has_content_size every frame's header carries its own piece's
 * length; s->content_size is ignored.  frame_bytes == 0 or a non-NULL s->dictionary is LZF_E_INVALID.
 * Conventions of lzf_frame_compress_device_many; d_out_len, d_status: DEVICE arrays of n_streams entries.  out_cap[s] below
 * lzf_frame_compress_stream_bound (the sum of lzf_frame_compress_bound over the pieces; 0 for frame_bytes == 0) gives
 * LZF_OUT_CAPACITY and no writes; a block status other than LZF_OK / LZF_OUTPUT_FULL (stored raw) fails the whole stream with
 * the first such status in stream order, out_len 0 and no writes; otherwise nothing outside d_out[s][0, out_len) is written.
 * The host plans everything from in_len[] and reads nothing back: between the compression and the assembly one kernel, one
 * wavefront per stream, computes every frame's exact length from the job results, prefixes the lengths and sets every
 * frame's destination and the stream's out_len and status.  A pass of the memory budget holds whole streams (a stream that
 * is over the budget alone is a pass of its own), so that a failing stream has no byte written. */
size_t lzf_frame_compress_stream_bound(const lzf_settings* s, size_t frame_bytes, size_t in_len);
int lzf_frame_compress_stream_device(const lzf_settings* s, size_t frame_bytes, uint32_t n_streams,
                                     const uint8_t* const* d_in, const size_t* in_len,
                                     const uint8_t* d_dict, size_t dict_len,
                                     uint8_t* const* d_out, const size_t* out_cap,
                                     uint64_t* d_out_len, int32_t* d_status, void* hip_stream);
/* lzf_frame_compress_stream_size_device: the out_len / status lzf_frame_compress_stream_device reports for the same arguments
 * whenever out_cap[s] holds the bound — the sum over the pieces of frame_bytes, each piece a frame — without writing anything
 * (lzf_frame_compressed_size_device over the pieces, folded per stream by the compress call's own one-wavefront-per-stream
 * kernel).  Never LZF_OUT_CAPACITY; no checksum is computed, no output memory is taken. */
int lzf_frame_compress_stream_size_device(const lzf_settings* s, size_t frame_bytes, uint32_t n_streams,
                                          const uint8_t* const* d_in, const size_t* in_len,
                                          const uint8_t* d_dict, size_t dict_len,
                                          uint64_t* d_out_len, int32_t* d_status, void* hip_stream);

/* Frame assembly from already-compressed blocks (what rank 0 does after the RCCL all-gather of a
 * block-sharded compression): writes header, then for every block
 * [u32 len | stored-bit][bytes][xxh32]?, then EndMark and content checksum.
 *   comp_len[i] == UINT32_MAX  => block i is stored raw (compress2 returned LZF_OUTPUT_FULL)
 *   payload[i] points at comp_len[i] compressed bytes, or at the raw block when stored.
 * `raw_len[i]` is the uncompressed length of block i. */
int lzf_frame_assemble(const lzf_settings* s, uint32_t n_blocks, const uint8_t* const* payload,
                       const uint32_t* comp_len, const uint32_t* raw_len, uint32_t content_xxh32,
                       uint8_t* out, size_t out_cap, size_t* out_len);

#ifdef __cplusplus
}
#endif
#endif /* LZFEAR_FRAME_H */
