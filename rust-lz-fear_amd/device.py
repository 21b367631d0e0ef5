"""Device-resident batches for the C ABI: job arrays built with numpy, kept in HBM as torch
uint8 tensors.  torch is plumbing here (device memory + streams), not the product: the codec
is liblzfear_hip.so and every launch goes through its extern "C" entry points."""
import ctypes as C

import numpy as np
import torch

from . import ffi

CJOB = np.dtype([("input", "<u8"), ("input_len", "<u8"), ("cursor", "<u8"), ("out", "<u8"),
                 ("out_cap", "<u8"), ("table", "<u8"), ("table_kind", "<u4"), ("flags", "<u4")])
DJOB = np.dtype([("input", "<u8"), ("input_len", "<u8"), ("prefix", "<u8"), ("prefix_len", "<u8"),
                 ("out", "<u8"), ("out_existing_len", "<u8"), ("out_cap", "<u8"), ("output_limit", "<u8")])
RES = np.dtype([("out_len", "<u8"), ("status", "<i4"), ("reserved", "<u4")])
SFRAME = np.dtype([("in_off", "<u8"), ("consumed", "<u8"), ("out_off", "<u8"), ("out_len", "<u8"), ("content_size", "<u8"),
                   ("status", "<i4"), ("flags", "<u4")])          # lzf_stream_frame
FBLOCK = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("out_len", "<u8"), ("in_len", "<u4"), ("want_sum", "<u4"),
                   ("block_maxsize", "<u4"), ("status", "<i4"), ("flags", "<u4"), ("reserved", "<u4")])          # lzf_frame_block
assert CJOB.itemsize == 56 and DJOB.itemsize == 64 and RES.itemsize == 16 and SFRAME.itemsize == 48 and FBLOCK.itemsize == 48


def to_device(arr, device):
    """numpy (structured) array -> uint8 tensor in HBM."""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    return torch.from_numpy(raw.copy()).to(device)


def results_to_host(d_res, n):
    return d_res.cpu().numpy().view(RES)[:n]


def _stream_ptr(stream):
    if stream is None:
        stream = torch.cuda.current_stream()
    return stream.cuda_stream


def compress_batch(d_jobs, d_res, n, kinds=ffi.KINDS_U32, stream=None):
    ffi.check(ffi.lib().lzf_compress_batch(d_jobs.data_ptr(), d_res.data_ptr(), n, kinds, _stream_ptr(stream)))


def compressed_size_batch(d_jobs, d_res, n, kinds=ffi.KINDS_U32, stream=None):
    """lzf_compressed_size_batch: status and out_len of every compress job without writing its output.  The same job array as
    compress_batch: `out` is not looked at, out_cap is honoured (UINT64_MAX: the pure size), a writable table is written back —
    give the call a copy of a table that a later compress_batch is to start from."""
    ffi.check(ffi.lib().lzf_compressed_size_batch(d_jobs.data_ptr(), d_res.data_ptr(), n, kinds, _stream_ptr(stream)))


def decompress_batch(d_jobs, d_res, n, stream=None, max_input_len=None):
    """lzf_decompress_batch; with max_input_len (an upper bound of the jobs' input_len, which the caller of a device-resident
    job array usually knows) lzf_decompress_batch_sized: the segmented pipeline then sizes its scratch for that bound instead
    of for 4 MiB blocks at their worst case — a batch of small blocks allocates (and launches) next to nothing."""
    if max_input_len is None:
        ffi.check(ffi.lib().lzf_decompress_batch(d_jobs.data_ptr(), d_res.data_ptr(), n, _stream_ptr(stream)))
    else:
        ffi.check(ffi.lib().lzf_decompress_batch_sized(d_jobs.data_ptr(), d_res.data_ptr(), n, int(max_input_len), _stream_ptr(stream)))


def decompressed_size_batch(d_jobs, d_res, n, stream=None, max_input_len=None):
    """lzf_decompressed_size_batch: status and output.len() of every decode job without decoding it.  The same job array as
    decompress_batch; prefix, out and out_cap of the jobs are not looked at.  max_input_len: an upper bound of the jobs' input_len; a
    call of many small blocks should give it — without one a call of up to 16 jobs per CU takes the latency class's scratch (sized for
    4 MiB blocks) and front stages whatever its inputs are."""
    bound = (1 << 64) - 1 if max_input_len is None else int(max_input_len)
    ffi.check(ffi.lib().lzf_decompressed_size_batch(d_jobs.data_ptr(), d_res.data_ptr(), n, bound, _stream_ptr(stream)))


def history_trim_batch(d_jobs, d_trimmed, d_shift, n, stream=None):
    """lzf_history_trim_batch: d_trimmed[i] = job i restated over the last 64 KiB of its existing output (jobs with less than 1 GiB of it are
    copied), d_shift[i] = what lzf_history_restore_batch adds back.  d_trimmed must not be d_jobs; d_shift: n uint64 in device memory."""
    ffi.check(ffi.lib().lzf_history_trim_batch(d_jobs.data_ptr(), d_trimmed.data_ptr(), d_shift.data_ptr(), n, _stream_ptr(stream)))


def history_restore_batch(d_res, d_shift, n, stream=None):
    ffi.check(ffi.lib().lzf_history_restore_batch(d_res.data_ptr(), d_shift.data_ptr(), n, _stream_ptr(stream)))


def _with_long_history(call, d_jobs, d_res, n, stream, max_input_len):
    d_trimmed = torch.empty(n * DJOB.itemsize, dtype=torch.uint8, device=d_jobs.device)
    d_shift = torch.empty(n, dtype=torch.int64, device=d_jobs.device)
    history_trim_batch(d_jobs, d_trimmed, d_shift, n, stream)
    call(d_trimmed, d_res, n, stream=stream, max_input_len=max_input_len)
    history_restore_batch(d_res, d_shift, n, stream)
    return d_trimmed, d_shift


def decompress_batch_long_history(d_jobs, d_res, n, stream=None, max_input_len=None):
    """decompress_batch for jobs whose existing output may be long — tensors that are appended to past 2 GiB: trim, decode, restore, all on
    `stream`.  out_len comes back absolute.  Returns the two scratch tensors (the trimmed jobs, the shifts): keep them until the stream has
    run when it is not the current one."""
    return _with_long_history(decompress_batch, d_jobs, d_res, n, stream, max_input_len)


def decompressed_size_batch_long_history(d_jobs, d_res, n, stream=None, max_input_len=None):
    """decompressed_size_batch the same way: any out_existing_len <= out_cap is answered."""
    return _with_long_history(decompressed_size_batch, d_jobs, d_res, n, stream, max_input_len)


def last_size_launch():
    """lzf_last_size_launch: what this thread's last decompressed_size_batch launched ("latency: ..." = the class of few large blocks)."""
    return ffi.lib().lzf_last_size_launch().decode()


def decompress_verify_batch(d_jobs, d_res, n, stream=None, max_input_len=None):
    """lzf_decompress_verify_batch: does every decode job decode to exactly the bytes out[out_existing_len, out_cap) already holds?
    The same job array as decompress_batch; `out` is read, never written.  Per job LZF_OK with the length, ffi.MISMATCH with the first
    differing position (or the shorter length), or the status decompressed_size_batch reports — nothing is decoded."""
    bound = (1 << 64) - 1 if max_input_len is None else int(max_input_len)
    ffi.check(ffi.lib().lzf_decompress_verify_batch(d_jobs.data_ptr(), d_res.data_ptr(), n, bound, _stream_ptr(stream)))


def last_verify_launch():
    """lzf_last_verify_launch: what this thread's last decompress_verify_batch launched."""
    return ffi.lib().lzf_last_verify_launch().decode()


def decompress_head_batch(d_jobs, d_res, n, stream=None, max_input_len=None):
    """lzf_decompress_head_batch: the head of every decode job's block — decoding stops where the output is out_cap bytes long, out_cap
    being the target (out_existing_len included).  The same job array as decompress_batch.  Per job LZF_OK with out_len =
    min(decoded length, out_cap), or the codec status of a sequence that starts in front of the target; what lies behind it is not
    looked at.  (max_input_len: accepted for _with_long_history's sake; the call has no use for it.)"""
    ffi.check(ffi.lib().lzf_decompress_head_batch(d_jobs.data_ptr(), d_res.data_ptr(), n, _stream_ptr(stream)))


def decompress_head_batch_long_history(d_jobs, d_res, n, stream=None):
    """decompress_head_batch for jobs whose existing output may be 1 GiB and more: trim, decode the heads, restore, all on `stream`; the
    target moves with the origin and out_len comes back absolute.  Returns the two scratch tensors, as decompress_batch_long_history."""
    return _with_long_history(decompress_head_batch, d_jobs, d_res, n, stream, None)


def block_heads(blocks, nbytes, prefix=None, stream=None):
    """The first `nbytes` decoded bytes of every raw block in `blocks` (1-D uint8 CUDA tensors), `prefix` (a 1-D uint8 CUDA tensor) being
    every block's dictionary: (heads, lens, statuses) — heads a [n, nbytes] uint8 CUDA tensor (row i: the head of block i, zeros behind
    lens[i] bytes), lens int64 and statuses int32 CUDA tensors, all written in order on `stream`.  One lzf_decompress_head_batch: a
    block is decoded no further than the sequence that reaches nbytes.  No output limit is applied."""
    n = len(blocks)
    dev = blocks[0].device if n else torch.device("cuda", torch.cuda.current_device())
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        heads = torch.zeros((n, nbytes), dtype=torch.uint8, device=dev)
        if n == 0:
            return heads, torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
        for t in blocks:
            assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 1 and t.is_contiguous(), "blocks: 1-D contiguous uint8 CUDA tensors"
        j = np.zeros(n, dtype=DJOB)
        j["input"] = [t.data_ptr() for t in blocks]
        j["input_len"] = [t.numel() for t in blocks]
        if prefix is not None and prefix.numel():
            assert prefix.dtype == torch.uint8 and prefix.is_cuda and prefix.dim() == 1 and prefix.is_contiguous()
            j["prefix"] = prefix.data_ptr()
            j["prefix_len"] = prefix.numel()
        j["out"] = np.uint64(heads.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(nbytes)
        j["out_cap"] = nbytes
        j["output_limit"] = (1 << 63) - 1
        d_jobs = to_device(j, dev)
        d_res = torch.empty(n * RES.itemsize, dtype=torch.uint8, device=dev)
        decompress_head_batch(d_jobs, d_res, n, stream=s)
        r = d_res.view(torch.int64).view(n, 2)
        lens = r[:, 0].clone()
        statuses = d_res.view(torch.int32).view(n, 4)[:, 2].clone()
    for t in (heads, d_jobs, d_res, lens, statuses):
        t.record_stream(s)
    return heads, lens, statuses


def xxh32_batch(d_ptrs, d_lens, d_out, n, stream=None):
    ffi.check(ffi.lib().lzf_xxh32_batch(d_ptrs.data_ptr(), d_lens.data_ptr(), d_out.data_ptr(), n, _stream_ptr(stream)))


XXH32_STATE = np.dtype([("v", "<u4", (4,)), ("buf", "u1", (16,)), ("fill", "<u4"), ("seed", "<u4"), ("total", "<u8")])     # lzf_xxh32_state
assert XXH32_STATE.itemsize == 48


def xxh32_update_batch(d_states, d_ptrs, d_lens, n, stream=None):
    """lzf_xxh32_update_batch: state i (48 bytes at d_states + 48 i, the host's lzf_xxh32_state) takes d_lens[i] bytes at the device
    address d_ptrs[i].  d_states: a uint8 CUDA tensor of 48 n bytes; d_ptrs, d_lens: uint64 / int64 CUDA tensors."""
    ffi.check(ffi.lib().lzf_xxh32_update_batch(d_states.data_ptr(), d_ptrs.data_ptr(), d_lens.data_ptr(), n, _stream_ptr(stream)))


def xxh32_digest_batch(d_states, d_out, n, stream=None):
    """lzf_xxh32_digest_batch: d_out[i] (uint32 as an int32 CUDA tensor) = the hash of everything state i has taken."""
    ffi.check(ffi.lib().lzf_xxh32_digest_batch(d_states.data_ptr(), d_out.data_ptr(), n, _stream_ptr(stream)))


def copy_ranges(d_src_ptrs, d_dst_ptrs, d_lens, n, max_len, stream=None):
    """Stored blocks moved on the device (lzf_copy_ranges); the three arrays are uint64 device tensors."""
    ffi.check(ffi.lib().lzf_copy_ranges(d_src_ptrs.data_ptr(), d_dst_ptrs.data_ptr(), d_lens.data_ptr(), n, max_len, _stream_ptr(stream)))


class BlockSet:
    """Equal-size independent blocks of one contiguous HBM buffer (the DP unit of
    src/framed/compress.rs:221-276 in independent-blocks mode): block i = data[i*bs : ...]."""

    def __init__(self, data, block_size):
        assert data.dtype == torch.uint8 and data.is_cuda and data.dim() == 1
        self.data = data
        self.block_size = block_size
        self.total = data.numel()
        self.n = (self.total + block_size - 1) // block_size
        self.lens = np.full(self.n, block_size, dtype=np.uint64)
        if self.total % block_size:
            self.lens[-1] = self.total % block_size
        self.offsets = np.arange(self.n, dtype=np.uint64) * np.uint64(block_size)

    def compress_jobs(self, out, out_stride):
        """One compress2 job per block, cursor 0, fresh U32Table, writer cap = block length
        (src/framed/compress.rs:242-243).  `out` = HBM slab of n * out_stride bytes."""
        j = np.zeros(self.n, dtype=CJOB)
        j["input"] = np.uint64(self.data.data_ptr()) + self.offsets
        j["input_len"] = self.lens
        j["out"] = np.uint64(out.data_ptr()) + np.arange(self.n, dtype=np.uint64) * np.uint64(out_stride)
        j["out_cap"] = self.lens
        j["table_kind"] = ffi.TABLE_U32
        return j


# ---- frames in device memory (include/lzfear_frame.h, "frames in device memory") -------------------------------------------

def _frame_args(frames):
    for t in frames:
        assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 1 and t.is_contiguous(), "frames: 1-D contiguous uint8 CUDA tensors"
    n = len(frames)
    return n, (C.c_void_p * n)(*[t.data_ptr() for t in frames]), (C.c_size_t * n)(*[t.numel() for t in frames])


def frame_decompress_bound(frames, stream=None):
    """lzf_frame_decompress_bound_device: per frame the most its blocks can decode to (0 for a frame whose header fails).
    Synchronous: the frames are scanned on the device and the bounds come back to the host."""
    n, ptrs, lens = _frame_args(frames)
    if n == 0:
        return []
    bound = (C.c_size_t * n)()
    ffi.check(ffi.lib().lzf_frame_decompress_bound_device(n, ptrs, lens, bound, _stream_ptr(stream)))
    return list(bound)


def frame_decompress_many(frames, outs, dictionary=None, stream=None):
    """lzf_frame_decompress_device_many: frames (1-D uint8 CUDA tensors) decoded into `outs` (1-D uint8 CUDA tensors, their
    lengths are the capacities).  Returns (status int32, out_len int64, consumed int64) as CUDA tensors, written in order on
    `stream`; nothing is synchronised beyond the call's own scan."""
    n, ptrs, lens = _frame_args(frames)
    assert len(outs) == n
    dev = frames[0].device if n else torch.device("cuda", torch.cuda.current_device())
    status = torch.empty(n, dtype=torch.int32, device=dev)         # (empty: no fill kernel on another stream; the call writes every entry)
    out_len = torch.empty(n, dtype=torch.int64, device=dev)
    consumed = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return status, out_len, consumed
    for t in outs:
        assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 1 and t.is_contiguous(), "outs: 1-D contiguous uint8 CUDA tensors"
    optr = (C.c_void_p * n)(*[t.data_ptr() for t in outs])
    caps = (C.c_size_t * n)(*[t.numel() for t in outs])
    dptr, dlen = None, 0
    if dictionary is not None and dictionary.numel():
        assert dictionary.dtype == torch.uint8 and dictionary.is_cuda and dictionary.is_contiguous()
        dptr, dlen = dictionary.data_ptr(), dictionary.numel()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    # (the results are written by kernels on `s`: keep torch's caching allocator from handing them out elsewhere meanwhile)
    for t in (status, out_len, consumed):
        t.record_stream(s)
    ffi.check(ffi.lib().lzf_frame_decompress_device_many(n, ptrs, lens, dptr, dlen, optr, caps, out_len.data_ptr(), consumed.data_ptr(),
                                                         status.data_ptr(), s.cuda_stream))
    return status, out_len, consumed


def frame_decompressed_size(frames, dictionary_len=0, stream=None):
    """lzf_frame_decompressed_size_device: per frame what frame_decompress_many would report with unlimited outputs and a
    dictionary of `dictionary_len` bytes, found without decoding.  Returns (status int32, out_len int64, consumed int64) as CUDA
    tensors, written in order on `stream`.  The content checksum is not verified (LZF_OK where the decode says FrameChecksumFail)."""
    n, ptrs, lens = _frame_args(frames)
    dev = frames[0].device if n else torch.device("cuda", torch.cuda.current_device())
    status = torch.empty(n, dtype=torch.int32, device=dev)         # (empty: the call writes every entry)
    out_len = torch.empty(n, dtype=torch.int64, device=dev)
    consumed = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return status, out_len, consumed
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    for t in (status, out_len, consumed):
        t.record_stream(s)
    ffi.check(ffi.lib().lzf_frame_decompressed_size_device(n, ptrs, lens, int(dictionary_len), out_len.data_ptr(), consumed.data_ptr(),
                                                           status.data_ptr(), s.cuda_stream))
    return status, out_len, consumed


def frame_verify(frames, expected, dictionary=None, stream=None):
    """lzf_frame_verify_device: does every frame (1-D uint8 CUDA tensors) deliver exactly the bytes of `expected` (1-D uint8 CUDA
    tensors, one per frame)?  Nothing is decoded, no output memory is taken.  Returns (status int32, at int64, consumed int64) as CUDA
    tensors, written in order on `stream`: LZF_OK with the length; ffi.MISMATCH with the first differing position, or the shorter
    length; FrameChecksumFail where the bytes are equal and the stored content checksum is not theirs; or the status and length
    frame_decompressed_size reports."""
    n, ptrs, lens = _frame_args(frames)
    assert len(expected) == n
    dev = frames[0].device if n else torch.device("cuda", torch.cuda.current_device())
    status = torch.empty(n, dtype=torch.int32, device=dev)         # (empty: the call writes every entry)
    at = torch.empty(n, dtype=torch.int64, device=dev)
    consumed = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return status, at, consumed
    _, eptrs, elens = _frame_args(expected)
    dptr, dlen = None, 0
    if dictionary is not None and dictionary.numel():
        assert dictionary.dtype == torch.uint8 and dictionary.is_cuda and dictionary.is_contiguous()
        dptr, dlen = dictionary.data_ptr(), dictionary.numel()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    for t in (status, at, consumed):
        t.record_stream(s)
    ffi.check(ffi.lib().lzf_frame_verify_device(n, ptrs, lens, dptr, dlen, eptrs, elens, at.data_ptr(), consumed.data_ptr(),
                                                status.data_ptr(), s.cuda_stream))
    return status, at, consumed


def frame_head_raw(in_ptrs, in_lens, out_ptrs, targets, d_out_len, d_status, dictionary=None, stream=None):
    """lzf_frame_head_device on plain addresses: frame f is in_lens[f] bytes at the device address in_ptrs[f], its first targets[f]
    decoded bytes go to the device address out_ptrs[f] (any alignment; 0 where the target is 0).  d_out_len (int64) and d_status
    (int32) are CUDA tensors of len(in_ptrs) entries, written in order on `stream`."""
    n = len(in_ptrs)
    assert len(in_lens) == n and len(out_ptrs) == n and len(targets) == n
    dptr, dlen = None, 0
    if dictionary is not None and dictionary.numel():
        assert dictionary.dtype == torch.uint8 and dictionary.is_cuda and dictionary.is_contiguous()
        dptr, dlen = dictionary.data_ptr(), dictionary.numel()
    ffi.check(ffi.lib().lzf_frame_head_device(n, (C.c_void_p * n)(*in_ptrs), (C.c_size_t * n)(*in_lens), dptr, dlen, (C.c_void_p * n)(*out_ptrs),
                                              (C.c_size_t * n)(*targets), d_out_len.data_ptr(), d_status.data_ptr(), _stream_ptr(stream)))


def frame_heads(frames, nbytes, dictionary=None, stream=None):
    """The first `nbytes` decoded bytes of every frame in `frames` (1-D uint8 CUDA tensors), `dictionary` (a 1-D uint8 CUDA tensor)
    being every frame's dictionary: (heads, lens, statuses) — heads a [n, nbytes] uint8 CUDA tensor (row f: the head of frame f,
    zeros behind lens[f] bytes where statuses[f] is 0), lens int64 and statuses int32 CUDA tensors, all written in order on `stream`.  One
    lzf_frame_head_device: a frame is decoded no further than the sequence that reaches nbytes, nothing comes back to the host.
    Block checksums and the content checksum are NOT verified (frame_decompressed_size and frame_verify do that): this is for
    reading a preamble.  The twin of block_heads."""
    n, _, in_lens = _frame_args(frames)
    dev = frames[0].device if n else torch.device("cuda", torch.cuda.current_device())
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        heads = torch.zeros((n, nbytes), dtype=torch.uint8, device=dev)
        lens = torch.zeros(n, dtype=torch.int64, device=dev)
        statuses = torch.zeros(n, dtype=torch.int32, device=dev)
        if n:
            base = heads.data_ptr()
            frame_head_raw([t.data_ptr() for t in frames], list(in_lens), [base + f * nbytes if nbytes else 0 for f in range(n)], [nbytes] * n,
                           lens, statuses, dictionary=dictionary, stream=s)
    for t in (heads, lens, statuses):
        t.record_stream(s)
    return heads, lens, statuses


def frame_cursor_bytes():
    """lzf_frame_cursor_bytes: device bytes per cursor of frame_resume."""
    return int(ffi.lib().lzf_frame_cursor_bytes())


def new_frame_cursors(n, device):
    """n zeroed cursors for frame_resume ([n, lzf_frame_cursor_bytes()] uint8): all zero = the start of a frame."""
    return torch.zeros((n, frame_cursor_bytes()), dtype=torch.uint8, device=device)


def frame_resume(frames, in_lens, cursors, outs, dictionary=None, stream=None):
    """lzf_frame_resume_device, the raw call: frame f is the first in_lens[f] bytes of frames[f] (None: all of them), decoded from
    where cursors[f] stands into outs[f] (1-D uint8 CUDA tensors, their lengths are the room of this call), as many whole blocks as
    fit.  `cursors`: what new_frame_cursors returned, the same rows on every call.  Returns (status int32, out_len int64, consumed
    int64, phase int32) as CUDA tensors, written in order on `stream`: the bytes of this call, the input offset the cursor now
    stands at, ffi.RESUME_MORE / RESUME_NEED_INPUT / RESUME_DONE."""
    n, ptrs, lens = _frame_args(frames)
    assert len(outs) == n and cursors.dtype == torch.uint8 and cursors.is_cuda and cursors.is_contiguous()
    assert cursors.numel() == n * frame_cursor_bytes(), "cursors: one row of frame_cursor_bytes() per frame"
    if in_lens is not None:
        assert len(in_lens) == n and all(0 <= int(l) <= t.numel() for l, t in zip(in_lens, frames))
        lens = (C.c_size_t * n)(*[int(l) for l in in_lens])
    dev = frames[0].device if n else torch.device("cuda", torch.cuda.current_device())
    status = torch.empty(n, dtype=torch.int32, device=dev)         # (empty: the call writes every entry)
    out_len = torch.empty(n, dtype=torch.int64, device=dev)
    consumed = torch.empty(n, dtype=torch.int64, device=dev)
    phase = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return status, out_len, consumed, phase
    for t in outs:
        assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 1 and t.is_contiguous(), "outs: 1-D contiguous uint8 CUDA tensors"
    optr = (C.c_void_p * n)(*[t.data_ptr() for t in outs])
    caps = (C.c_size_t * n)(*[t.numel() for t in outs])
    dptr, dlen = None, 0
    if dictionary is not None and dictionary.numel():
        assert dictionary.dtype == torch.uint8 and dictionary.is_cuda and dictionary.is_contiguous()
        dptr, dlen = dictionary.data_ptr(), dictionary.numel()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    for t in (status, out_len, consumed, phase):
        t.record_stream(s)
    ffi.check(ffi.lib().lzf_frame_resume_device(n, ptrs, lens, dptr, dlen, cursors.data_ptr(), optr, caps, out_len.data_ptr(), consumed.data_ptr(),
                                                status.data_ptr(), phase.data_ptr(), s.cuda_stream))
    return status, out_len, consumed, phase


def frame_write_cursor_bytes():
    """lzf_frame_wcursor_bytes: device bytes per write cursor of frame_append."""
    return int(ffi.lib().lzf_frame_wcursor_bytes())


def new_frame_write_cursors(n, device=None):
    """n zeroed write cursors for frame_append ([n, lzf_frame_wcursor_bytes()] uint8): all zero = nothing written yet."""
    device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    return torch.zeros((n, frame_write_cursor_bytes()), dtype=torch.uint8, device=device)


def frame_append(settings, offers, flags, cursors, outs, dictionary=None, stream=None, in_lens=None, caps=None):
    """lzf_frame_append_device, the raw call: offers[f] (1-D uint8 CUDA tensors; in_lens[f] bytes of them, default all) are the
    next bytes of stream f, flags[f] is 0 or ffi.APPEND_FINISH, and what the call takes of them is compressed behind cursors[f]
    into outs[f] (1-D uint8 CUDA tensors; caps[f], default their lengths, is the room of this call).  `cursors`: what
    new_frame_write_cursors returned, the same rows on every call, with the same `settings` (an ffi.Settings whose `dictionary`
    is NULL) and `dictionary` (a uint8 CUDA tensor).  Returns (status int32, out_len int64, taken int64, phase int32) as CUDA
    tensors, written in order on `stream`; nothing is synchronised and nothing comes back to the host."""
    n, ptrs, lens = _frame_args(offers)
    assert len(outs) == n and len(flags) == n and cursors.dtype == torch.uint8 and cursors.is_cuda and cursors.is_contiguous()
    assert cursors.numel() == n * frame_write_cursor_bytes(), "cursors: one row of frame_write_cursor_bytes() per frame"
    if in_lens is not None:
        assert len(in_lens) == n and all(0 <= int(l) <= t.numel() for l, t in zip(in_lens, offers))
        lens = (C.c_size_t * n)(*[int(l) for l in in_lens])
    dev = cursors.device
    status = torch.empty(n, dtype=torch.int32, device=dev)         # (empty: the call writes every entry)
    out_len = torch.empty(n, dtype=torch.int64, device=dev)
    taken = torch.empty(n, dtype=torch.int64, device=dev)
    phase = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return status, out_len, taken, phase
    for t in outs:
        assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 1 and t.is_contiguous(), "outs: 1-D contiguous uint8 CUDA tensors"
    optr = (C.c_void_p * n)(*[t.data_ptr() for t in outs])
    caps = (C.c_size_t * n)(*([t.numel() for t in outs] if caps is None else caps))
    dptr, dlen = None, 0
    if dictionary is not None and dictionary.numel():
        assert dictionary.dtype == torch.uint8 and dictionary.is_cuda and dictionary.is_contiguous()
        dptr, dlen = dictionary.data_ptr(), dictionary.numel()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    for t in (status, out_len, taken, phase):
        t.record_stream(s)
    ffi.check(ffi.lib().lzf_frame_append_device(C.byref(settings), n, ptrs, lens, (C.c_uint32 * n)(*[int(x) for x in flags]), dptr, dlen,
                                                cursors.data_ptr(), optr, caps, out_len.data_ptr(), taken.data_ptr(), status.data_ptr(),
                                                phase.data_ptr(), s.cuda_stream))
    return status, out_len, taken, phase


def frame_compress_many(settings, frames, outs, dictionary=None, stream=None, caps=None):
    """lzf_frame_compress_device_many: every input of `frames` (1-D uint8 CUDA tensors) compressed into an LZ4 frame in `outs`
    (1-D uint8 CUDA tensors, their lengths are the capacities) with `settings` (an ffi.Settings whose `dictionary` is NULL; the
    dictionary is the uint8 CUDA tensor `dictionary`).  Returns (status int32, out_len int64) as CUDA tensors, written in order on
    `stream`; nothing is synchronised.  `caps` (optional): the capacities the call is told, for outputs allocated with the exact
    lengths of frame_compressed_size — the call writes nothing outside [0, out_len) — default: the tensors' lengths."""
    n, ptrs, lens = _frame_args(frames)
    assert len(outs) == n
    dev = frames[0].device if n else torch.device("cuda", torch.cuda.current_device())
    status = torch.empty(n, dtype=torch.int32, device=dev)         # (empty: the call writes every entry)
    out_len = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return status, out_len
    for t in outs:
        assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 1 and t.is_contiguous(), "outs: 1-D contiguous uint8 CUDA tensors"
    optr = (C.c_void_p * n)(*[t.data_ptr() for t in outs])
    caps = (C.c_size_t * n)(*([t.numel() for t in outs] if caps is None else caps))
    dptr, dlen = None, 0
    if dictionary is not None and dictionary.numel():
        assert dictionary.dtype == torch.uint8 and dictionary.is_cuda and dictionary.is_contiguous()
        dptr, dlen = dictionary.data_ptr(), dictionary.numel()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    for t in (status, out_len):
        t.record_stream(s)
    ffi.check(ffi.lib().lzf_frame_compress_device_many(C.byref(settings), n, ptrs, lens, dptr, dlen, optr, caps, out_len.data_ptr(),
                                                       status.data_ptr(), s.cuda_stream))
    return status, out_len


# ---- the block index of a frame, and runs of its blocks (include/lzfear_frame.h) ------------------------------------------

def frame_block_count(frames, stream=None):
    """lzf_frame_block_count_device: per frame the blocks the walk finds (0 for a frame whose header fails).  Synchronous."""
    n, ptrs, lens = _frame_args(frames)
    if n == 0:
        return []
    found = (C.c_size_t * n)()
    ffi.check(ffi.lib().lzf_frame_block_count_device(n, ptrs, lens, found, _stream_ptr(stream)))
    return list(found)


def frame_block_index_raw(frames, dictionary_len=0, index=None, stream=None):
    """lzf_frame_block_index_device: frame_decompressed_size's results and, with `index` (one uint8 CUDA tensor per frame, room
    for numel() // 48 entries, 8-byte aligned), the blocks of every frame.  Returns (status int32, out_len int64, consumed int64,
    n_listed int64) as CUDA tensors, written in order on `stream`.  The content checksum is not verified."""
    n, ptrs, lens = _frame_args(frames)
    dev = frames[0].device if n else torch.device("cuda", torch.cuda.current_device())
    status = torch.empty(n, dtype=torch.int32, device=dev)         # (empty: the call writes every entry)
    out_len, consumed, n_listed = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
    if n == 0:
        return status, out_len, consumed, n_listed
    iptr = icap = None
    if index is not None:
        assert len(index) == n
        for t in index:
            assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 1 and t.is_contiguous() and (t.numel() < FBLOCK.itemsize or t.data_ptr() % 8 == 0), \
                "index: 1-D contiguous uint8 CUDA tensors at 8-byte aligned addresses"
        iptr = (C.c_void_p * n)(*[t.data_ptr() if t.numel() >= FBLOCK.itemsize else None for t in index])
        icap = (C.c_size_t * n)(*[t.numel() // FBLOCK.itemsize for t in index])
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    for t in (status, out_len, consumed, n_listed):
        t.record_stream(s)
    ffi.check(ffi.lib().lzf_frame_block_index_device(n, ptrs, lens, int(dictionary_len), iptr, icap, out_len.data_ptr(), consumed.data_ptr(),
                                                     status.data_ptr(), n_listed.data_ptr(), s.cuda_stream))
    return status, out_len, consumed, n_listed


def frame_block_index(frames, dictionary_len=0, stream=None):
    """The block index of every frame: counts the blocks (lzf_frame_block_count_device), allocates one entry tensor per frame and
    runs frame_block_index_raw.  Returns (status, out_len, consumed, n_listed, entries): CUDA tensors as above and a list of uint8
    CUDA tensors of 48 bytes per block found (view them as FBLOCK on the host)."""
    frames = list(frames)
    if not frames:
        return frame_block_index_raw([], dictionary_len=dictionary_len, stream=stream) + ([],)
    dev = frames[0].device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    found = frame_block_count(frames, stream=s)
    entries = [torch.empty(k * FBLOCK.itemsize, dtype=torch.uint8, device=dev) for k in found]
    for e in entries:
        e.record_stream(s)
    return frame_block_index_raw(frames, dictionary_len=dictionary_len, index=entries, stream=s) + (entries,)


def frame_decompress_blocks(frames, runs, outs, dictionary=None, stream=None):
    """lzf_frame_decompress_blocks_device: run r is `runs[r]`, a numpy FBLOCK array of consecutive entries of the block index of
    `frames[r]` (host copies), decoded into `outs[r]` (1-D uint8 CUDA tensors, their lengths are the capacities), every block
    straight to its place.  Returns (status int32, out_len int64) as CUDA tensors, written in order on `stream`; nothing is
    synchronised.  Raises ffi.LzfError(E_INVALID) for a run the call refuses; the content checksum is never verified."""
    n, ptrs, lens = _frame_args(frames)
    assert len(runs) == n and len(outs) == n
    dev = frames[0].device if n else torch.device("cuda", torch.cuda.current_device())
    status = torch.empty(n, dtype=torch.int32, device=dev)         # (empty: the call writes every entry)
    out_len = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return status, out_len
    for t in outs:
        assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 1 and t.is_contiguous(), "outs: 1-D contiguous uint8 CUDA tensors"
    keep = [np.ascontiguousarray(r, dtype=FBLOCK) for r in runs]
    rptr = (C.c_void_p * n)(*[r.ctypes.data if len(r) else None for r in keep])
    rcnt = (C.c_size_t * n)(*[len(r) for r in keep])
    optr = (C.c_void_p * n)(*[t.data_ptr() for t in outs])
    caps = (C.c_size_t * n)(*[t.numel() for t in outs])
    dptr, dlen = None, 0
    if dictionary is not None and dictionary.numel():
        assert dictionary.dtype == torch.uint8 and dictionary.is_cuda and dictionary.is_contiguous()
        dptr, dlen = dictionary.data_ptr(), dictionary.numel()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    for t in (status, out_len):
        t.record_stream(s)
    ffi.check(ffi.lib().lzf_frame_decompress_blocks_device(n, ptrs, lens, rptr, rcnt, dptr, dlen, optr, caps, out_len.data_ptr(),
                                                           status.data_ptr(), s.cuda_stream))
    return status, out_len


# ---- streams of back-to-back frames in device memory (include/lzfear_frame.h) ---------------------------------------------

def stream_decompress_bound(streams, stream=None):
    """lzf_frame_stream_bound_device: per stream the sum of its frames' bounds.  Synchronous."""
    n, ptrs, lens = _frame_args(streams)
    if n == 0:
        return []
    bound = (C.c_size_t * n)()
    ffi.check(ffi.lib().lzf_frame_stream_bound_device(n, ptrs, lens, bound, _stream_ptr(stream)))
    return list(bound)


def stream_decompress(streams, outs, dictionary=None, stream=None):
    """lzf_frame_decompress_stream_device: every stream of back-to-back frames (1-D uint8 CUDA tensors) decoded into its tensor
    of `outs` (their lengths are the capacities), frame behind frame.  Returns (status int32, out_len int64, consumed int64,
    n_frames int64) as CUDA tensors, written in order on `stream`; nothing is synchronised beyond the call's own scans."""
    n, ptrs, lens = _frame_args(streams)
    assert len(outs) == n
    dev = streams[0].device if n else torch.device("cuda", torch.cuda.current_device())
    status = torch.empty(n, dtype=torch.int32, device=dev)         # (empty: the call writes every entry)
    out_len = torch.empty(n, dtype=torch.int64, device=dev)
    consumed = torch.empty(n, dtype=torch.int64, device=dev)
    n_frames = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return status, out_len, consumed, n_frames
    for t in outs:
        assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 1 and t.is_contiguous(), "outs: 1-D contiguous uint8 CUDA tensors"
    optr = (C.c_void_p * n)(*[t.data_ptr() for t in outs])
    caps = (C.c_size_t * n)(*[t.numel() for t in outs])
    dptr, dlen = None, 0
    if dictionary is not None and dictionary.numel():
        assert dictionary.dtype == torch.uint8 and dictionary.is_cuda and dictionary.is_contiguous()
        dptr, dlen = dictionary.data_ptr(), dictionary.numel()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    for t in (status, out_len, consumed, n_frames):
        t.record_stream(s)
    ffi.check(ffi.lib().lzf_frame_decompress_stream_device(n, ptrs, lens, dptr, dlen, optr, caps, out_len.data_ptr(), consumed.data_ptr(),
                                                           status.data_ptr(), n_frames.data_ptr(), s.cuda_stream))
    return status, out_len, consumed, n_frames


def stream_count(streams, stream=None):
    """lzf_frame_stream_count_device: per stream the frames the walk finds (the failing last one included).  Synchronous."""
    n, ptrs, lens = _frame_args(streams)
    if n == 0:
        return []
    found = (C.c_size_t * n)()
    ffi.check(ffi.lib().lzf_frame_stream_count_device(n, ptrs, lens, found, _stream_ptr(stream)))
    return list(found)


def stream_decompressed_size(streams, dictionary_len=0, index=None, stream=None):
    """lzf_frame_stream_decompressed_size_device: per stream what stream_decompress would report with unlimited outputs and a
    dictionary of `dictionary_len` bytes, found without decoding, and, with `index` (one uint8 CUDA tensor per stream, room for
    numel() // 48 entries, 8-byte aligned), the frames of every stream.  Returns (status int32, out_len int64, consumed int64,
    n_frames int64, n_listed int64) as CUDA tensors, written in order on `stream`.  The content checksum is not verified."""
    n, ptrs, lens = _frame_args(streams)
    dev = streams[0].device if n else torch.device("cuda", torch.cuda.current_device())
    status = torch.empty(n, dtype=torch.int32, device=dev)         # (empty: the call writes every entry)
    out_len, consumed, n_frames, n_listed = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4))
    if n == 0:
        return status, out_len, consumed, n_frames, n_listed
    iptr = icap = None
    if index is not None:
        assert len(index) == n
        for t in index:
            assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 1 and t.is_contiguous() and t.data_ptr() % 8 == 0, \
                "index: 1-D contiguous uint8 CUDA tensors at 8-byte aligned addresses"
        iptr = (C.c_void_p * n)(*[t.data_ptr() for t in index])
        icap = (C.c_size_t * n)(*[t.numel() // SFRAME.itemsize for t in index])
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    for t in (status, out_len, consumed, n_frames, n_listed):
        t.record_stream(s)
    ffi.check(ffi.lib().lzf_frame_stream_decompressed_size_device(n, ptrs, lens, int(dictionary_len), iptr, icap, out_len.data_ptr(),
                                                                  consumed.data_ptr(), status.data_ptr(), n_frames.data_ptr(),
                                                                  n_listed.data_ptr(), s.cuda_stream))
    return status, out_len, consumed, n_frames, n_listed


def stream_index(streams, dictionary_len=0, stream=None):
    """The frame index of every stream: counts the frames (lzf_frame_stream_count_device), allocates one entry tensor per stream and
    runs stream_decompressed_size.  Returns (status, out_len, consumed, n_frames, n_listed, entries): CUDA tensors as above and
    a list of uint8 CUDA tensors of 48 bytes per frame found (view them as SFRAME on the host)."""
    streams = list(streams)
    if not streams:
        return stream_decompressed_size([], dictionary_len=dictionary_len, stream=stream) + ([],)
    dev = streams[0].device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    found = stream_count(streams, stream=s)
    entries = [torch.empty(k * SFRAME.itemsize, dtype=torch.uint8, device=dev) for k in found]
    for e in entries:
        e.record_stream(s)
    return stream_decompressed_size(streams, dictionary_len=dictionary_len, index=entries, stream=s) + (entries,)


def stream_compress(settings, frame_bytes, tensors, outs, dictionary=None, stream=None, caps=None):
    """lzf_frame_compress_stream_device: every input of `tensors` written as frames of `frame_bytes` input bytes each, back to
    back, into its tensor of `outs`.  Returns (status int32, out_len int64) as CUDA tensors, written in order on `stream`;
    nothing is synchronised.  `caps`: as for frame_compress_many."""
    n, ptrs, lens = _frame_args(tensors)
    assert len(outs) == n
    dev = tensors[0].device if n else torch.device("cuda", torch.cuda.current_device())
    status = torch.empty(n, dtype=torch.int32, device=dev)         # (empty: the call writes every entry)
    out_len = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return status, out_len
    for t in outs:
        assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 1 and t.is_contiguous(), "outs: 1-D contiguous uint8 CUDA tensors"
    optr = (C.c_void_p * n)(*[t.data_ptr() for t in outs])
    caps = (C.c_size_t * n)(*([t.numel() for t in outs] if caps is None else caps))
    dptr, dlen = None, 0
    if dictionary is not None and dictionary.numel():
        assert dictionary.dtype == torch.uint8 and dictionary.is_cuda and dictionary.is_contiguous()
        dptr, dlen = dictionary.data_ptr(), dictionary.numel()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    for t in (status, out_len):
        t.record_stream(s)
    ffi.check(ffi.lib().lzf_frame_compress_stream_device(C.byref(settings), int(frame_bytes), n, ptrs, lens, dptr, dlen, optr, caps,
                                                         out_len.data_ptr(), status.data_ptr(), s.cuda_stream))
    return status, out_len


# ---- compressed sizes without output (include/lzfear_frame.h) --------------------------------------------------------------

def _size_call(fn, head, tensors, dictionary, stream):
    n, ptrs, lens = _frame_args(tensors)
    dev = tensors[0].device if n else torch.device("cuda", torch.cuda.current_device())
    status = torch.empty(n, dtype=torch.int32, device=dev)         # (empty: the call writes every entry)
    out_len = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return status, out_len
    dptr, dlen = None, 0
    if dictionary is not None and dictionary.numel():
        assert dictionary.dtype == torch.uint8 and dictionary.is_cuda and dictionary.is_contiguous()
        dptr, dlen = dictionary.data_ptr(), dictionary.numel()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    for t in (status, out_len):
        t.record_stream(s)
    ffi.check(fn(*head, n, ptrs, lens, dptr, dlen, out_len.data_ptr(), status.data_ptr(), s.cuda_stream))
    return status, out_len


def frame_compressed_size(settings, frames, dictionary=None, stream=None):
    """lzf_frame_compressed_size_device: per input of `frames` the (status, out_len) frame_compress_many reports with outputs that
    hold the bound, found without writing a frame: no output memory, no checksum computed.  Returns (status int32, out_len int64)
    as CUDA tensors, written in order on `stream`; nothing is synchronised."""
    return _size_call(ffi.lib().lzf_frame_compressed_size_device, (C.byref(settings),), frames, dictionary, stream)


def stream_compressed_size(settings, frame_bytes, tensors, dictionary=None, stream=None):
    """lzf_frame_compress_stream_size_device: per input the (status, out_len) stream_compress reports with outputs that hold the
    bound — the sum over its pieces of `frame_bytes` — found without writing anything."""
    return _size_call(ffi.lib().lzf_frame_compress_stream_size_device, (C.byref(settings), int(frame_bytes)), tensors, dictionary, stream)
