/*
 * lzfear_hip.h — C ABI of the MI355X (gfx950) LZ4 raw-block codec that drops in under
 * lz-fear's `raw` module.
 *
 * This is the boundary a Rust `-sys` crate would bind (INTEGRATION.md shows the `extern "C"`
 * block and the safe wrappers with the reference's own signatures).  Plain pointers and sizes
 * only; no C++ or torch types.  Each entry point cites the reference interface it replaces
 * (file:line in the lz-fear 0.2.0 tree).
 *
 * The reference calls its codec once per frame block (src/framed/compress.rs:243,
 * src/framed/decompress.rs:248).  The GPU boundary is the same call *batched over jobs*: one
 * job = one `compress2` / `decompress_raw` invocation, one wavefront (compress) or one
 * workgroup (decompress) each, many jobs per launch.
 *
 * Memory: every pointer in a job is a DEVICE pointer (HBM) unless the function name ends in
 * `_host`.  The library never retains pointers past a call and owns no global state besides
 * the staging memory of the `_host` helpers and the frame layer (one pinned slab and device
 * scratch, kept between calls; lzf_frame_release_scratch() of lzfear_frame.h frees them) and ONE process-wide setting: the batch
 * calls take their scratch from the device's default stream-ordered memory pool and raise that pool's release threshold
 * (hipMemPoolAttrReleaseThreshold) to "keep", once per device — without it every call would go back to the device allocator
 * and wait for whatever is running.  There is NO CPU fallback: every entry point
 * returns LZF_E_NO_DEVICE when no HIP device is usable.
 */
#ifndef LZFEAR_HIP_H
#define LZFEAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LZFEAR_ABI_VERSION 2

/* ---- per-job status (lzf_job_result.status) --------------------------------------------- */
enum {
    LZF_OK = 0,
    /* raw::DecodeError — src/raw/decompress.rs:8-17 */
    LZF_UNEXPECTED_END = 1,
    LZF_MEMORY_LIMIT_EXCEEDED = 2,
    LZF_ZERO_DEDUP_OFFSET = 3,
    LZF_INVALID_DEDUP_OFFSET = 4,
    /* compress2's writer refused a write: io::ErrorKind::ConnectionAborted from
     * NoPartialWrites — src/framed/compress.rs:294-314, matched at :250-255 */
    LZF_OUTPUT_FULL = 5,
    /* the reference would panic: assert at src/raw/compress/mod.rs:167, expect at :67/:92 */
    LZF_CONTRACT = 6,
    /* decode output buffer smaller than what the reference's Vec would have grown to
     * (literals are not limit-checked, src/raw/decompress.rs:63-67): give the job
     * out_cap >= output_limit + input_len and this never happens */
    LZF_OUT_CAPACITY = 7
};
#define LZF_MISMATCH 8   /* verify calls only: the block decodes cleanly, but not to the expected bytes */

/* ---- library-level return codes (negative) ---------------------------------------------- */
enum {
    LZF_E_NO_DEVICE = -1,     /* no HIP device / HIP runtime error at init */
    LZF_E_HIP = -2,           /* a HIP call failed; lzf_last_error() has the text */
    LZF_E_INVALID = -3        /* bad argument (NULL jobs with n_jobs > 0, ...) */
};

/* ---- encoder tables: src/raw/compress/mod.rs:27-36 (U32Table), :78-87 (U16Table) --------- */
#define LZF_TABLE_U32 0       /* 4096 x u32, payload limit u32::MAX (:75)  — what framed uses (:202) */
#define LZF_TABLE_U16 1       /* 8192 x u16, payload limit 65535   (:100) — raw API only        */

typedef struct lzf_u32_table { uint32_t dict[4096]; uint64_t offset; } lzf_u32_table;
typedef struct lzf_u16_table { uint16_t dict[8192]; uint64_t offset; } lzf_u16_table;

/* ---- jobs ------------------------------------------------------------------------------- */

/* One `compress2(input, cursor, &mut table, writer)` call — src/raw/compress/mod.rs:165-166.
 *   input[0..cursor) is addressable history (dictionary / previous-block window),
 *   input[cursor..input_len) is the payload.  The writer is a bounded sink of `out_cap` bytes
 *   with NoPartialWrites semantics (the frame layer passes out_cap = payload length,
 *   src/framed/compress.rs:242).
 *   table == NULL  <=>  `&mut T::default()` thrown away afterwards (independent blocks without
 *   a dictionary).  Otherwise it points at an lzf_u32_table / lzf_u16_table in device memory
 *   which is read at start and written back at the end (mutations survive LZF_OUTPUT_FULL,
 *   exactly like the reference's `&mut table`). */
typedef struct lzf_compress_job {
    const uint8_t* input;
    uint64_t input_len;
    uint64_t cursor;
    uint8_t* out;
    uint64_t out_cap;
    void* table;
    uint32_t table_kind;          /* LZF_TABLE_U32 | LZF_TABLE_U16 */
    uint32_t flags;               /* LZF_CJOB_* */
} lzf_compress_job;

#define LZF_CJOB_TABLE_READONLY 1u   /* do not write the table back: `template_table.clone()`
                                        per independent block, src/framed/compress.rs:220,270 */

/* One `decompress_raw(input, prefix, &mut output, output_limit)` call —
 * src/raw/decompress.rs:58-59.  `out[0..out_existing_len)` is the Vec's content on entry
 * (addressable history); decoded bytes are appended after it.  out_cap is the room the Vec may
 * grow to. */
typedef struct lzf_decompress_job {
    const uint8_t* input;
    uint64_t input_len;
    const uint8_t* prefix;
    uint64_t prefix_len;
    uint8_t* out;
    uint64_t out_existing_len;
    uint64_t out_cap;
    uint64_t output_limit;
} lzf_decompress_job;

typedef struct lzf_job_result {
    uint64_t out_len;             /* compress: bytes written; decompress: output.len() (incl. existing) */
    int32_t status;               /* LZF_OK ... LZF_OUT_CAPACITY; out_len is unspecified on error */
    uint32_t reserved;            /* diagnostic only: kilo-cycles the job's wavefront ran */
} lzf_job_result;

/* ---- library ---------------------------------------------------------------------------- */
int lzf_abi_version(void);
const char* lzf_last_error(void);
/* Number of usable HIP devices (>= 1) or LZF_E_NO_DEVICE. */
int lzf_device_count(void);

/* Batched raw::compress2 — src/raw/compress/mod.rs:165-238 for every job.
 * d_jobs / d_results are device arrays of n_jobs entries.  Asynchronous on `hip_stream`
 * (a hipStream_t; NULL = the legacy default stream) of the CURRENT device.
 * `table_kinds` says which table types occur in the batch (the job array lives in HBM, the
 * host cannot look): LZF_KINDS_U32, LZF_KINDS_U16 or both or'ed; 0 means "either".
 * Batches larger than the device holds at once are executed longest job first (an internal launch order: results[i]
 * always belongs to jobs[i]). */
#define LZF_KINDS_U32 1u
#define LZF_KINDS_U16 2u
/* optional promise, or'ed in: every U32 job of the batch has table == NULL or a LZF_CJOB_TABLE_READONLY table whose
 * offset is 0, and cursor <= input_len < 2 GiB (the independent-block jobs of src/framed/compress.rs:265-270).  Saves the
 * launch of the general kernel; a job that breaks the promise reports LZF_CONTRACT. */
#define LZF_KINDS_U32_FRESH_ONLY 4u
int lzf_compress_batch(const lzf_compress_job* d_jobs, lzf_job_result* d_results,
                       uint32_t n_jobs, uint32_t table_kinds, void* hip_stream);
/* raw::compress2's status and the number of bytes it would write, for every job, WITHOUT writing them: no output memory is
 * needed.  The parse is the compressor's own with the stores to the output left out, so the answer is exact.  Same job struct
 * as lzf_compress_batch (size, then compress, with one array).
 *   out      ignored and never dereferenced: NULL or a dangling pointer is fine.
 *   out_cap  IS honoured: status and out_len are what lzf_compress_batch writes for the job, LZF_OUTPUT_FULL at the same capacity
 *            included (out_len is then the bytes written before the refused sequence, as there).  A frame layer passes
 *            out_cap = the block's length and reads the stored-block decision from the status; pass UINT64_MAX for the pure size.
 *   table    a caller-owned table is read and written back exactly as lzf_compress_batch does — tables carry from block to
 *            block of a linked stream, so a size query over a chain needs the mutation.  LZF_CJOB_TABLE_READONLY is respected.
 *            To size and LATER COMPRESS a job that has a writable table, give the size call a COPY of the table: the
 *            compress call must start from the table as it was before the size call.
 *   reserved a diagnostic: the job's probe batches + sequences for a job the compact-table kernel answered, kilo-cycles otherwise.
 * table_kinds as above; LZF_KINDS_U32_FRESH_ONLY is the same promise, and a job that breaks it reports LZF_CONTRACT.  The call
 * launches the compact-table kernel and the general kernels in their dry forms whatever the job count (no latency class);
 * batches larger than the device holds at once may run in the compress call's launch order.  lzf_last_compress_launch is not
 * touched.  Asynchronous on `hip_stream`, no host wait; scratch (the launch order's) comes from the stream-ordered pool alone. */
int lzf_compressed_size_batch(const lzf_compress_job* d_jobs, lzf_job_result* d_results,
                              uint32_t n_jobs, uint32_t table_kinds, void* hip_stream);

/* Batched raw::decompress_raw — src/raw/decompress.rs:58-138 for every job.
 * Of out[0, out_existing_len) only the last 65 535 bytes are ever read (an offset is a u16, src/raw/decompress.rs:76), and with
 * that much existing output the prefix is never read at all.  The kernels hold 31-bit positions: a job whose input_len,
 * prefix_len or out_existing_len is 2 GiB - 256 or more reports LZF_CONTRACT.  For existing output there is a way around that
 * costs nothing: lzf_history_trim_batch below restates such jobs over the tail of their history. */
int lzf_decompress_batch(const lzf_decompress_job* d_jobs, lzf_job_result* d_results,
                         uint32_t n_jobs, void* hip_stream);
/* The same with what the caller knows about the batch: an upper bound of the jobs' input_len (the job array lives in HBM, the
 * library cannot look; ~0 = unknown, which is what lzf_decompress_batch passes).  Batches of up to four blocks per CU go through the
 * segmented pipeline (a block decoded by many wavefronts; blocks of 64 KiB .. 4 MiB + 32 KiB of input, with or without a prefix and
 * existing output below 2 GiB - 256: the blocks of linked-block and dictionary frames included), whose stream-ordered scratch — bit maps, tile sums and a 16-byte record per sequence, up to ~0.15 + 1.8 bytes per byte of
 * `max_input_len` and job, from the device's default memory pool, freed in stream order — is sized by this bound; with a bound below
 * 64 KiB the pipeline is skipped.  Results are identical either way. */
int lzf_decompress_batch_sized(const lzf_decompress_job* d_jobs, lzf_job_result* d_results,
                               uint32_t n_jobs, uint64_t max_input_len, void* hip_stream);
/* raw::decompress_raw's status and output.len() for every job WITHOUT decoding it: no output memory is needed.  Every DecodeError
 * depends on positions and lengths only, never on an output byte, so a pass that parses tokens and adds lengths answers exactly.
 * Same job struct as the decoder (size, then decode, with one array).  Read: input, input_len, prefix_len, out_existing_len,
 * output_limit.  `prefix`, `out` and `out_cap` are ignored and never dereferenced (NULL / 0 / dangling are fine).
 *   status   what decompress_raw returns, i.e. what lzf_decompress_batch writes for the job whenever its out_cap is large enough:
 *            LZF_OK or 1..4, never LZF_OUT_CAPACITY.  The first failing sequence in stream order wins; inside a sequence the
 *            reference's order (UnexpectedEnd, then the limit :72-74, then the offset checks :83-89; literals are not
 *            limit-checked).  LZF_CONTRACT where the decoder refuses the job: input_len, out_existing_len or prefix_len of 2 GiB - 256 or more.
 *            (That sentence describes jobs as they are handed in, untrimmed: after lzf_history_trim_batch no out_existing_len is that long.)
 *   out_len  on LZF_OK output.len(), out_existing_len included; unspecified on an error.  The decoder stops at 2 GiB of
 *            output; this call does not: a block that decodes to more (LZ4 expands up to 255 x) gets its true 64-bit length.
 *   reserved a diagnostic: kilo-cycles, as for the decoder, for a job the one-wave kernel answered; the number of 2 KiB tiles of the
 *            input for a job the latency class answered.
 * Two classes, picked by the call's size alone (lzf_last_size_launch says which ran); results are the same either way:
 *   * a call of up to 16 jobs per compute unit (4 096 on MI355X) whose max_input_len is 64 KiB or more takes the LATENCY CLASS
 *     first: a block is summed up by many wavefronts (the segmented pipeline's plan, parse and seam, then one wavefront per 2 KiB of
 *     input and one per job), which answers every job of 64 KiB .. 4 MiB + 32 KiB of input that decodes cleanly;
 *   * always last, one wavefront per job over the whole call, skipping what the class answered: every error status, every other size.
 * max_input_len: as for lzf_decompress_batch_sized (~0 = unknown: 4 MiB blocks at their worst case); it sizes the latency class's
 * scratch — bit maps, chunk exits and 16 bytes per tile: about 1.2 bits per byte of max_input_len and job, at most 3 GiB, 0.61 MiB
 * per job of unknown size.  A caller of many SMALL blocks should pass its bound: with ~0 a call of up to 16 jobs per CU enters the class
 * whatever its inputs are, takes that scratch and runs the class's front over jobs that are all below its window before the one-wave kernel
 * answers them (4 096 blocks of 500 bytes: 0.31 ms instead of 0.13, 2.4 GiB of pool memory; with the bound, 0.13 ms and a job counter).  The one-wave kernel's scratch is a job counter, and 4 bytes per job for the launch order of batches
 * larger than the device holds at once.  All of it is independent of the decoded sizes, comes from the stream-ordered pool and is
 * freed in stream order; a pool that refuses the class's scratch is no error — the one-wave kernel then answers the whole call.  The
 * call enqueues its kernels and returns; no host wait. */
int lzf_decompressed_size_batch(const lzf_decompress_job* d_jobs, lzf_job_result* d_results,
                                uint32_t n_jobs, uint64_t max_input_len, void* hip_stream);
/* "Does this block decode to exactly these bytes?" for every job, WITHOUT decoding it: no output memory beyond the expected bytes
 * the caller already holds, and nothing but d_results is written.  Against a known plaintext no sequence depends on another — a
 * literal byte must equal the expected byte, a match byte must equal the expected byte `offset` earlier — so the call is the size
 * call's walk plus compares, parallel inside a block.  Same job struct as the decoder and the size call (size, verify and decode
 * with one array):
 *   out[0, out_existing_len)        history, trusted as in the decode;
 *   out[out_existing_len, out_cap)  the EXPECTED bytes.  `out` is read, never written;
 *   prefix, output_limit            as in the decode.
 * The result, in this order of precedence:
 *   1. the size call's status for the job, if that is not LZF_OK (1..4, or LZF_CONTRACT under the size call's own conditions),
 *      whatever the bytes: a malformed block is malformed first.  out_len is unspecified.
 *   2. with n the decoded output.len() and p the first position in [out_existing_len, min(n, out_cap)) whose decoded byte differs
 *      from out[p]: LZF_MISMATCH if p exists or n != out_cap, with out_len = p if it exists, else min(n, out_cap).
 *   3. LZF_OK with out_len = n = out_cap.
 * LZF_OUT_CAPACITY is never reported.  No byte outside input[0, input_len), prefix[0, prefix_len) and out[0, out_cap) is read: a
 * buffer may end where its allocation ends.  The size call's two classes, picked by the call's size alone (lzf_last_verify_launch says
 * which ran; results are the same either way): a call of up to 16 jobs per compute unit whose max_input_len is 64 KiB or more takes
 * the LATENCY CLASS first — the size call's front and tile sums, then one wavefront per 2 KiB tile of input compares the tile's
 * sequences at their positions, for every job of 64 KiB .. 4 MiB + 32 KiB of input that decodes cleanly — and always last, one
 * wavefront per job over the whole call, skipping what the class answered.  Those thresholds are the size call's, inherited, not
 * measured for this call.  max_input_len as for the size call; the class's scratch is the size call's plus 8 bytes per tile and
 * per job, at most 3 GiB, from the stream-ordered pool, and a pool that refuses it is no error.  `reserved`: the number of tiles
 * for a job the class answered, kilo-cycles otherwise.
 * lzf_history_trim_batch / lzf_history_restore_batch work on these jobs unchanged — `out`, with its expected bytes, moves with the
 * origin, and the restore adds the shift to the position of an LZF_MISMATCH as it does to the length of an LZF_OK.
 * Asynchronous on `hip_stream`, no host wait. */
int lzf_decompress_verify_batch(const lzf_decompress_job* d_jobs, lzf_job_result* d_results,
                                uint32_t n_jobs, uint64_t max_input_len, void* hip_stream);
/* The HEAD of every job's block: decode until the output is `out_cap` bytes long and stop (liblz4's LZ4_decompress_safe_partial).
 * A record header, a dtype/shape preamble or a file magic out of thousands of blocks costs what the heads cost, not the blocks.
 * Same job struct as the decoder, the size call and the verify call (all four run from one array).  Here out_cap is the TARGET: the
 * absolute output length, out_existing_len included, at which decoding stops — as the verify call reads out_cap as the end of the
 * expected bytes.  input, prefix, out[0, out_existing_len) and output_limit mean what they mean to the decoder.
 * The result is that of the reference's loop (src/raw/decompress.rs:61-77) with one added rule; `pos` is output.len() at the top of
 * an iteration, the position of the sequence's first literal:
 *   stop     the loop ends with Ok in front of the first sequence whose pos >= out_cap.  That sequence and everything behind it
 *            is never looked at, malformed or not.
 *   checks   a sequence with pos < out_cap is taken whole, exactly as the reference takes it: token and length bytes,
 *            UnexpectedEnd (the whole literal run must be in the input), then the limit test :72-74, then the offset tests :83-89
 *            — also where its literals alone already reach the target.  The first failing sequence in stream order wins; inside a
 *            sequence the reference's order.
 *   writes   of such a sequence the bytes at positions below out_cap are written, the rest are dropped:
 *            out[out_existing_len, min(n, out_cap)) holds exactly the bytes the decoder would put there; no byte at or beyond
 *            out + out_cap and no byte below out + out_existing_len is ever written.
 *   status   LZF_OK with out_len = min(n, out_cap), n the length reached when the loop ended.  out_len < out_cap says the block
 *            ended first; out_len == out_cap does NOT say whether more follows (the size call answers that).  Codec statuses 1..4
 *            as above, out_len unspecified (bytes below out_cap may have been written).  LZF_CONTRACT under the decoder's
 *            conditions for lengths: input_len, out_existing_len or prefix_len of 2 GiB - 256 or more.  LZF_OUT_CAPACITY is never
 *            reported.
 * What follows from that:
 *   out_cap <= out_existing_len  is LZF_OK with out_len = out_existing_len, and no input byte is read;
 *   a target beyond the block's end is the full decode (by one wavefront: see below);
 *   an error in a sequence that starts at or behind the target is not seen — the price of reading only the head.  A caller who
 *   needs the block's status asks the size call.
 * No byte outside input[0, input_len), prefix[0, prefix_len) and out[0, out_cap) is read.
 * lzf_history_trim_batch / lzf_history_restore_batch work on these jobs unchanged: the target moves with the origin.  `reserved`:
 * kilo-cycles, as for the decoder.  Asynchronous on `hip_stream`, no host wait; the only scratch is a 4-byte job counter from the
 * stream-ordered pool.
 * One wavefront per job, whatever the target, and no class of many wavefronts for large targets: the stop saves the chunks behind
 * the target, the bytes in front of it come at one wavefront's rate.  A caller who wants most of a large block decodes it whole
 * (lzf_decompress_batch_sized) and slices.  Measured on one MI355X, 2026-10-21, against
 * lzf_decompress_batch_sized of the whole blocks + lzf_copy_ranges of the heads (tools/head_bench.py, profiles/head_decode.txt), 4 MiB
 * blocks: 980 blocks 0.24 ms against 15.1 at 64 bytes, 0.26 ms against 15.1 at 4 KiB; the CROSSOVER, from which decoding whole and
 * slicing is not slower, lies at a target of 768 KiB for 980 blocks (at 512 KiB the head call is still 1.4 x quicker) and at 512 KiB
 * for 49 blocks (at 384 KiB still 1.2 x quicker). */
int lzf_decompress_head_batch(const lzf_decompress_job* d_jobs, lzf_job_result* d_results,
                              uint32_t n_jobs, void* hip_stream);
/* Jobs with long existing output — a Vec that block after block is appended to, a linked stream — for the calls above.
 * decompress_raw compares output.len() with output_limit and with offsets only, and no offset reaches further back than 65 535
 * bytes, so a job may be restated with its origin `shift` bytes further on without changing a byte or a status:
 *   out_existing_len < 2^30, or > out_cap:  shift = 0, the job is copied as it is;
 *   otherwise  shift = (out_existing_len - 65 536) & ~15   (a multiple of 16: out keeps its alignment), and the trimmed job has
 *              out + shift, out_existing_len - shift, out_cap - shift and output_limit - shift (0 where the limit is below the
 *              shift: MemoryLimitExceeded at the first match either way); input, prefix and their lengths are copied.
 * lzf_history_trim_batch writes d_trimmed[i] and d_shift[i] for every job; d_trimmed must not be d_jobs (LZF_E_INVALID).  The
 * caller then runs lzf_decompress_batch(_sized) or lzf_decompressed_size_batch on d_trimmed, and lzf_history_restore_batch adds
 * d_shift[i] back to out_len of every result whose status is LZF_OK.  What stays out of contract: inputs and prefixes of
 * 2 GiB - 256 and more, and one job that itself decodes past 2 GiB - 256 of (trimmed) output.  Asynchronous on `hip_stream`.
 * The `_host` calls and lzf_chain_decompress_step_trimmed below apply the same rule themselves. */
int lzf_history_trim_batch(const lzf_decompress_job* d_jobs, lzf_decompress_job* d_trimmed,
                           uint64_t* d_shift, uint32_t n_jobs, void* hip_stream);
int lzf_history_restore_batch(lzf_job_result* d_results, const uint64_t* d_shift,
                              uint32_t n_jobs, void* hip_stream);
/* Diagnostic: the kernels the calling thread's last lzf_decompress_batch launched (the batch size picks them: the
 * segmented pipeline — one block decoded by many wavefronts — up to four blocks per CU, one workgroup per block beyond). */
const char* lzf_last_decompress_launch(void);
/* The same for the calling thread's last lzf_decompressed_size_batch: "latency: ..." when the latency class ran in front of the
 * one-wave kernel, the one-wave kernel's name alone otherwise (larger calls, small inputs, no scratch from the pool). */
const char* lzf_last_size_launch(void);
/* The same for the calling thread's last lzf_decompress_verify_batch: "latency: ..." when the latency class ran in front of the
 * one-wave kernel, the one-wave kernel's name alone otherwise. */
const char* lzf_last_verify_launch(void);
/* The same for the calling thread's last lzf_compress_batch: "lzf_compress_team_kernel" (the latency class: no more jobs than
 * compute units, a team of three wavefronts and a CU's LDS per block) or "lzf_compress_compact_kernel" (one wavefront per
 * block, 18 per CU), plus the general kernels that ran beside it for U16 / writable-table jobs. */
const char* lzf_last_compress_launch(void);

/* EncoderTable helpers on device tables.
 * lzf_table_seed_from_dictionary: the template-table loop of src/framed/compress.rs:202-211
 *   (`for window in dict.windows(8).step_by(3) { template_table.replace(dict, offset) }`).
 * lzf_table_offset: EncoderTable::offset — src/raw/compress/mod.rs:72-74 / :97-99. */
int lzf_table_seed_from_dictionary(lzf_u32_table* d_table, const uint8_t* d_dict,
                                   uint64_t dict_len, void* hip_stream);
int lzf_table_offset(void* d_table, uint32_t table_kind, uint64_t add, void* hip_stream);
/* The same for n tables in one launch (d_tables[i]->offset += d_adds[i]): the `table.offset(forget)` of every
 * linked-block stream of a batch between two blocks, src/framed/compress.rs:271-275. */
int lzf_table_offset_batch(void* const* d_tables, const uint64_t* d_adds, uint32_t n, uint32_t table_kind,
                           void* hip_stream);

/* Linked-block streams decoded without a host round trip per block (src/framed/decompress.rs:238-269 for many
 * streams at once).  A stream's output is one contiguous device buffer (history = everything decoded so far, which
 * covers the reference's 64 KiB carry-over window); before step k this call finishes step k-1 and prepares step k of
 * every stream:
 *   - prev_job[i] (index into d_jobs / d_results, or UINT32_MAX): if that job failed the stream is dead (its later
 *     jobs are emptied), else the stream's length becomes its out_len;
 *   - job[i] (or UINT32_MAX): d_jobs[job[i]].out_existing_len = length, out_cap = length + block_maxsize + input_len,
 *     output_limit = length + block_maxsize;
 *   - stored_len[i] > 0: a stored block — stored_src[i] is copied to the end of the stream's output instead.
 * d_state[i] = {length, dead flag} persists across the calls of one chain. */
typedef struct lzf_chain_state { uint64_t length; uint32_t dead; uint32_t reserved; } lzf_chain_state;
typedef struct lzf_chain_step {
    uint32_t prev_job;              /* job of the previous step, UINT32_MAX if none / stored */
    uint32_t job;                   /* job of this step, UINT32_MAX if none / stored */
    uint64_t stored_len;            /* > 0: this step is a stored block */
    const uint8_t* stored_src;
    uint8_t* out;                   /* the stream's output buffer */
    uint64_t block_maxsize;
} lzf_chain_step;
int lzf_chain_decompress_step(const lzf_chain_step* d_steps, lzf_chain_state* d_state, uint32_t n_streams,
                              lzf_decompress_job* d_jobs, const lzf_job_result* d_results, void* hip_stream);
/* The same step for streams of ANY length, and the one the frame layer uses.  lzf_chain_decompress_step gives every job the whole
 * stream as history, so a stream ends with LZF_CONTRACT (or LZF_OUT_CAPACITY) once it nears 2 GiB.  This call hands the job out
 * trimmed from length >= 2^30 on, as lzf_history_trim_batch does it: with shift = (length - 65 536) & ~15 the job's `out` becomes
 * the stream's out + shift and out_existing_len, out_cap and output_limit count from there; the job's out_len comes back short by
 * that shift, which the next call of the chain adds again (the shift is a function of the length alone, so nothing is kept for
 * it).  d_state stays absolute and 64-bit, and so does the place of a stored block.  Below 2^30 the two calls write the same
 * bytes (`out` of a job untouched).  A chain uses ONE of the two calls from its first step to its last. */
int lzf_chain_decompress_step_trimmed(const lzf_chain_step* d_steps, lzf_chain_state* d_state, uint32_t n_streams,
                                      lzf_decompress_job* d_jobs, const lzf_job_result* d_results, void* hip_stream);

/* Batched XXH32 (seed 0) of n device buffers: the per-block checksums of
 * src/framed/compress.rs:259-263 and src/framed/decompress.rs:228-235. */
int lzf_xxh32_batch(const uint8_t* const* d_ptrs, const uint64_t* d_lens, uint32_t* d_out,
                    uint32_t n, void* hip_stream);

/* Resumable XXH32: the content hasher of a block-by-block reader (src/framed/decompress.rs:89,276-278) for bytes that arrive in
 * device memory piece by piece.  lzf_xxh32_state is the host's streaming state (lzf_xxh32_reset / _update / _digest of
 * lzfear_frame.h) and, unchanged, the device layout: 48 bytes — the four accumulators, up to 15 bytes that do not fill a stripe
 * yet, their count, the seed, the bytes hashed so far.  A state written by lzf_xxh32_reset on the host and uploaded is a valid
 * start; a state downloaded after any number of device updates gives, through the host's lzf_xxh32_digest, the hash of the
 * concatenation, and a state the host has updated goes on on the device the same way.
 * lzf_xxh32_update_batch: d_states[i] takes d_lens[i] bytes at d_ptrs[i] (any alignment; a zero length changes nothing and its
 *   pointer is not read).  One wavefront per state, lzf_xxh32_batch's stripe loop from the saved accumulators: one serial chain
 *   per state, at the rate of that call's chain and no faster (profiles/frame_resume.txt).  States must not alias each other.
 * lzf_xxh32_digest_batch: d_out[i] = the hash of everything d_states[i] has taken; the states are not changed.
 * d_states, d_ptrs, d_lens, d_out: DEVICE arrays of n entries.  Asynchronous on `hip_stream`, no host wait, no scratch. */
typedef struct lzf_xxh32_state { uint32_t v[4]; uint8_t buf[16]; uint32_t fill; uint32_t seed; uint64_t total; } lzf_xxh32_state;
int lzf_xxh32_update_batch(lzf_xxh32_state* d_states, const uint8_t* const* d_ptrs, const uint64_t* d_lens,
                           uint32_t n, void* hip_stream);
int lzf_xxh32_digest_batch(const lzf_xxh32_state* d_states, uint32_t* d_out, uint32_t n, void* hip_stream);

/* Stored blocks: copies n device byte ranges (d_src[i] -> d_dst[i], d_len[i] bytes, each at most max_len) in one
 * launch — the raw-block moves of src/framed/compress.rs:250-255 and src/framed/decompress.rs:250 without going
 * through the host.  Ranges must not overlap each other. */
int lzf_copy_ranges(const uint8_t* const* d_src, uint8_t* const* d_dst, const uint64_t* d_len, uint32_t n,
                    uint64_t max_len, void* hip_stream);

/* ---- host-buffer convenience (synchronous; stages through device scratch) ---------------
 * Same semantics as the batch calls but every pointer in the jobs is a HOST pointer and
 * `results` is a host array.  `table` pointers are host lzf_*_table structs, updated in
 * place.  Used by the frame layer and by callers that have not moved their data to HBM.
 * The two decode-side calls trim long existing output themselves (see lzf_history_trim_batch): any out_existing_len <= out_cap
 * is accepted, only the last 64 KiB of it are staged, and out_len comes back absolute. */
int lzf_compress_batch_host(const lzf_compress_job* jobs, lzf_job_result* results, uint32_t n_jobs);
int lzf_decompress_batch_host(const lzf_decompress_job* jobs, lzf_job_result* results, uint32_t n_jobs);
/* lzf_decompressed_size_batch over host buffers: `input` of every job is a HOST pointer (staged to the device), `results` a
 * host array; prefix, out and out_cap are ignored as above.  Synchronous. */
int lzf_decompressed_size_batch_host(const lzf_decompress_job* jobs, lzf_job_result* results, uint32_t n_jobs);
/* lzf_decompress_verify_batch over host buffers: `input`, `prefix` and `out` of every job are HOST pointers; the input, the prefix
 * and out[0, out_cap) — history and expected bytes; of a history of 1 GiB and more its last 64 KiB — are staged to the device,
 * `results` is a host array.  out_len comes back absolute, for LZF_MISMATCH as well.  Synchronous. */
int lzf_decompress_verify_batch_host(const lzf_decompress_job* jobs, lzf_job_result* results, uint32_t n_jobs);
/* lzf_decompress_head_batch over host buffers: `input`, `prefix` and `out` of every job are HOST pointers.  The input, the prefix
 * and at most the last 65 535 bytes of out[0, out_existing_len) are staged to the device — existing output of any length below the
 * target is accepted, the long-history trim included — and only out[out_existing_len, out_len) comes back; nothing else of `out`
 * is touched.  Device room is what the block can decode to, never more than the target asks for.  `results` is a host array,
 * out_len comes back absolute.  Synchronous. */
int lzf_decompress_head_batch_host(const lzf_decompress_job* jobs, lzf_job_result* results, uint32_t n_jobs);
/* lzf_compressed_size_batch over host buffers: `input` and `table` of every job are HOST pointers (staged to the device; a
 * writable table is updated in place, as lzf_compress_batch_host does), `results` a host array; `out` is ignored, out_cap is
 * honoured as above.  Synchronous. */
int lzf_compressed_size_batch_host(const lzf_compress_job* jobs, lzf_job_result* results, uint32_t n_jobs);
/* EncoderTable::replace on a HOST table — src/raw/compress/mod.rs:19-25 (trait), :64-71 (U32Table), :88-96 (U16Table):
 * swaps `pos + table.offset` into the slot of hash(input[pos..]) and returns the previous entry minus table.offset,
 * saturating at 0 (stale entries read as position 0).  hash = hash_for_u32 (:40-51: 5 bytes of an 8-byte little-endian
 * read, slot 0 when fewer than 8 bytes remain) or hash_for_u16 (:58-61).  With lzf_table_offset's host twin below this
 * completes the trait for a crate that keeps `trait EncoderTable` and implements it on the C ABI's table structs.
 * Returns LZF_OK, or LZF_CONTRACT where the reference panics: pos + offset beyond the table's integer range (:67 / :92),
 * pos > input_len, or (U16) fewer than 4 bytes at pos (the slice read of :59). */
int lzf_table_replace_host(void* table, uint32_t table_kind, const uint8_t* input, uint64_t input_len, uint64_t pos,
                           uint64_t* previous);
/* EncoderTable::offset on a host table (mod.rs:72-74, :97-99). */
int lzf_table_offset_host(void* table, uint32_t table_kind, uint64_t add);

/* raw::compress2 with the reference's signature for ANY writer — src/raw/compress/mod.rs:165-166:
 *   pub fn compress2<W: Write, T: EncoderTable>(input: &[u8], cursor: usize, table: &mut T, mut writer: W)
 * `write_all(ctx, data, len)` stands for `writer.write_all(data)`: 0 = Ok(()), any other value = the writer's error, which
 * ends the call and is handed back in *writer_error (the Rust wrapper turns it into the io::Error again).  The block is
 * compressed on the device against LZ4's worst-case bound, then the reference's own sequence of write calls is replayed
 * from it — per sequence: the token byte, the literal length's tail (0xFF bytes four at a time, then one at a time, then
 * the remainder byte: mod.rs:243-260), the literals in one call, the two offset bytes, the match length's tail
 * (mod.rs:150-163); the final literal-only section likewise (:182-189).  A writer that refuses call k has seen exactly
 * the calls 0..k-1, as under the reference.  `table` (host memory, may be NULL = T::default() thrown away) ends in the
 * state the reference leaves it in: after the whole input, or — when the writer refuses — after the search of the
 * sequence whose write was refused (the reference mutates the table before it writes a sequence, :196-218 then :236).
 * Returns LZF_OK, LZF_OUTPUT_FULL (the writer refused), LZF_CONTRACT, or a negative library code.  Host buffers. */
typedef int (*lzf_write_all_fn)(void* ctx, const uint8_t* data, size_t len);
int lzf_compress2_host_writer(const uint8_t* input, uint64_t input_len, uint64_t cursor, void* table, uint32_t table_kind,
                              lzf_write_all_fn write_all, void* ctx, int* writer_error);

/* lzf_xxh32_batch over host buffers (staged to the device, hashed there; `out` is a host array). */
int lzf_xxh32_batch_host(const uint8_t* const* ptrs, const uint64_t* lens, uint32_t* out, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif /* LZFEAR_HIP_H */
