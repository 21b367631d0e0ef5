"""Mirror of lz-fear's `framed` module on top of the C ABI (include/lzfear_frame.h):
`CompressionSettings` with the reference's builder methods (src/framed/compress.rs:56-157) and
`decompress_frame` (src/framed/decompress.rs:284-288).  Thin Python over the C++ frame layer —
every block is compressed / decompressed by the HIP kernels."""
import collections
import ctypes as C

from . import ffi

MAGIC = 0x184D2204          # src/framed/mod.rs:16
WINDOW_SIZE = 64 * 1024     # src/framed/mod.rs:20

FRAME_ERRORS = {
    1: "CodecError(UnexpectedEnd)", 2: "CodecError(MemoryLimitExceeded)", 3: "CodecError(ZeroDeduplicationOffset)",
    4: "CodecError(InvalidDeduplicationOffset)", 7: "OutCapacity", 8: "Mismatch",
    16: "InputError", 17: "WrongMagic", 18: "HeaderChecksumFail", 19: "BlockChecksumFail", 20: "FrameChecksumFail",
    21: "BlockLengthOverflow", 22: "BlockSizeOverflow", 23: "UnimplementedBlocksize", 24: "UnsupportedVersion",
    25: "ReservedFlagBitsSet", 26: "ReservedBdBitsSet", 27: "InvalidBlockSize", 28: "Panic",
}


class FrameError(Exception):
    def __init__(self, code, partial=b""):
        super().__init__(FRAME_ERRORS.get(code, str(code)))
        self.code = code
        self.partial = partial


class LZ4FrameWriter:
    """lzf_frame_writer_*: compress_internal's loop (src/framed/compress.rs:160-282) with the stream fed piece by piece."""
    _WRITE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t)

    def __init__(self, settings, sink, content_size=None, blocks_per_launch=0):
        self._exc = None

        def cb(ctx, p, n):
            try:
                sink(C.string_at(p, n))         # (one memcpy; a slice of the POINTER would build a list of n Python ints first)
                return 0
            except BaseException as e:          # the sink refuses: the writer stops (io::Error of the reference's writer);
                self._exc = e                   # KeyboardInterrupt and friends are re-raised by _done as well
                return 1
        self._cb = self._WRITE(cb)
        self._s = settings._struct(content_size)
        self._w = C.c_void_p()
        L = ffi.lib()
        L.lzf_frame_writer_new.argtypes = [C.c_void_p, self._WRITE, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.lzf_frame_writer_write.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        L.lzf_frame_writer_finish.argtypes = [C.c_void_p]
        L.lzf_frame_writer_free.argtypes = [C.c_void_p]
        rc = L.lzf_frame_writer_new(C.byref(self._s), self._cb, None, blocks_per_launch, C.byref(self._w))
        if rc != 0:
            ffi.check(rc)
            raise FrameError(rc)

    def _done(self, rc):
        if self._exc is not None:               # whatever the sink raised comes back to the caller, whatever status the C side made of it
            e, self._exc = self._exc, None
            raise e
        if rc != 0:
            ffi.check(rc)
            raise FrameError(rc)

    def write(self, data):
        data = bytes(data)
        self._done(ffi.lib().lzf_frame_writer_write(self._w, data, len(data)))

    def finish(self):
        self._done(ffi.lib().lzf_frame_writer_finish(self._w))

    def close(self):
        if self._w:
            ffi.lib().lzf_frame_writer_free(self._w)
            self._w = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CompressionSettings:
    """src/framed/compress.rs:36-55; the setters return self like the reference's builder."""

    def __init__(self):
        self._independent_blocks = True
        self._block_checksums = False
        self._content_checksum = True
        self._block_size = 4 * 1024 * 1024
        self._dictionary = None
        self._dictionary_id = None

    def independent_blocks(self, v):            # :63-66
        self._independent_blocks = bool(v); return self

    def block_checksums(self, v):               # :75-78
        self._block_checksums = bool(v); return self

    def content_checksum(self, v):              # :88-91
        self._content_checksum = bool(v); return self

    def block_size(self, v):                    # :97-100
        self._block_size = int(v); return self

    def dictionary(self, id, dict):             # :113-117
        self._dictionary_id = id; self._dictionary = bytes(dict); return self

    def dictionary_id_nonsense_override(self, id):   # :130-133
        self._dictionary_id = id; return self

    def _struct(self, content_size):
        s = ffi.Settings()
        ffi.lib().lzf_settings_default(C.byref(s))
        s.independent_blocks = int(self._independent_blocks)
        s.block_checksums = int(self._block_checksums)
        s.content_checksum = int(self._content_checksum)
        s.block_size = self._block_size
        keep = None
        if self._dictionary is not None:
            keep = C.create_string_buffer(self._dictionary, max(len(self._dictionary), 1))
            s.dictionary = C.addressof(keep)
            s.dictionary_len = len(self._dictionary)
        if self._dictionary_id is not None:
            s.has_dictionary_id = 1
            s.dictionary_id = self._dictionary_id
        if content_size is not None:
            s.has_content_size = 1
            s.content_size = content_size
        s._keep = keep
        return s

    def _run(self, data, content_size):
        data = bytes(data)
        s = self._struct(content_size)
        cap = ffi.lib().lzf_frame_compress_bound(C.byref(s), len(data))
        out = C.create_string_buffer(max(cap, 1))
        n = C.c_size_t(0)
        rc = ffi.lib().lzf_frame_compress(C.byref(s), data, len(data), out, cap, C.byref(n))
        ffi.check(rc)
        if rc != 0:
            raise FrameError(rc)
        return C.string_at(out, n.value)

    def compress(self, data):                    # :137-140
        return self._run(data, None)

    def writer(self, sink, content_size=None, blocks_per_launch=0):
        """Streaming form of compress / compress_with_size_unchecked (:138-146): feed the stream with .write(bytes) in any
        granularity, call .finish(); the frame's bytes go to `sink(bytes)` (raise to refuse) piece by piece, in the
        reference's order (lzf_frame_writer_* of lzfear_frame.h).  Byte-identical to compress() of the whole stream."""
        return LZ4FrameWriter(self, sink, content_size, blocks_per_launch)

    def compress_many(self, datas):
        """`compress` of every buffer in `datas`, all frames through the same launches (lzf_frame_compress_many): the
        way to keep the device busy when single frames have only a few blocks, and the only way for linked-block
        streams (block k of every stream goes into launch k).  Returns one frame per input, byte-identical to
        `compress(d)` of each."""
        datas = [bytes(d) for d in datas]
        n = len(datas)
        if n == 0:
            return []
        s = self._struct(None)
        L = ffi.lib()
        caps = [L.lzf_frame_compress_bound(C.byref(s), len(d)) for d in datas]
        outs = [C.create_string_buffer(max(c, 1)) for c in caps]
        ins = (C.c_char_p * n)(*datas)
        lens = (C.c_size_t * n)(*[len(d) for d in datas])
        outp = (C.c_void_p * n)(*[C.addressof(o) for o in outs])
        capa = (C.c_size_t * n)(*caps)
        olen = (C.c_size_t * n)()
        st = (C.c_int * n)()
        ffi.check(L.lzf_frame_compress_many(C.byref(s), n, ins, lens, outp, capa, olen, st))
        for f in range(n):
            if st[f] != 0:
                raise FrameError(st[f])
        return [C.string_at(outs[f], olen[f]) for f in range(n)]

    def _device_call(self, tensors, content_size):
        """What the device calls share: the settings without a host dictionary, the dictionary uploaded, the device."""
        import torch
        dev = tensors[0].device
        s = self._struct(content_size)
        s.dictionary = None                                 # (the device call takes the dictionary in device memory)
        s.dictionary_len = 0
        d_dict = None
        if self._dictionary:
            d_dict = torch.frombuffer(bytearray(self._dictionary), dtype=torch.uint8).to(dev)
        return dev, s, d_dict

    @staticmethod
    def _finish(st, status, out_len):
        st.synchronize()
        codes, lens = status.cpu().tolist(), out_len.cpu().tolist()
        for c in codes:
            if c != 0:
                raise FrameError(c)
        return lens

    def compressed_sizes_device(self, tensors, content_size=None, stream=None):
        """The length of every frame `compress_many_device` would return for `tensors`, found on the device without writing a
        frame (lzf_frame_compressed_size_device): no output memory is taken and no checksum is computed.  Returns a list of ints
        once `stream` (default: the current stream) has finished the call; raises FrameError like `compress_many_device`."""
        import torch
        from . import device
        tensors = list(tensors)
        if not tensors:
            return []
        dev, s, d_dict = self._device_call(tensors, content_size)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        if d_dict is not None:
            st.wait_stream(torch.cuda.current_stream(dev))   # (the upload ran on the current stream)
        with torch.cuda.stream(st):
            status, out_len = device.frame_compressed_size(s, tensors, dictionary=d_dict, stream=st)
        return self._finish(st, status, out_len)

    def compress_many_device(self, tensors, content_size=None, stream=None, exact=False, verify=False):
        """`compress_many` for inputs that live on the device (1-D uint8 CUDA tensors), compressed on the device into device
        memory (lzf_frame_compress_device_many); `content_size` goes into every header (compress_with_size_unchecked).
        Outputs are sized with lzf_frame_compress_bound; the dictionary is uploaded.  Returns one uint8 CUDA tensor per input,
        the frame's bytes, once `stream` (default: the current stream) has finished the call; raises FrameError like
        `compress_many`.
        exact=True: the outputs are allocated from the size call (lzf_frame_compressed_size_device) instead of from the bound, and
        every returned tensor owns exactly its frame's bytes.  (The compress call is still told the bound as the capacity: its
        contract is that nothing outside [0, out_len) is written, and out_len is what the size call reported.)
        verify=True: before the call returns the written frames are verified against the input tensors (lzf_frame_verify_device:
        no decode, no output memory) — for callers who free the input next.  The first frame that is not LZF_OK raises FrameError."""
        import torch
        from . import device
        tensors = list(tensors)
        if not tensors:
            return []
        dev, s, d_dict = self._device_call(tensors, content_size)
        L = ffi.lib()
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        if d_dict is not None:
            st.wait_stream(torch.cuda.current_stream(dev))   # (the upload ran on the current stream)
        bounds = [L.lzf_frame_compress_bound(C.byref(s), t.numel()) for t in tensors]
        caps = None
        if exact:
            with torch.cuda.stream(st):
                status, out_len = device.frame_compressed_size(s, tensors, dictionary=d_dict, stream=st)
            sizes, caps = self._finish(st, status, out_len), bounds
            outs = [torch.empty(n, dtype=torch.uint8, device=dev) for n in sizes]
        else:
            outs = [torch.empty(b, dtype=torch.uint8, device=dev) for b in bounds]
        with torch.cuda.stream(st):
            status, out_len = device.frame_compress_many(s, tensors, outs, dictionary=d_dict, stream=st, caps=caps)
        lens = self._finish(st, status, out_len)
        if exact:
            assert lens == sizes, "the size call and the compress call disagree"
        frames = outs if exact else [outs[f][:lens[f]] for f in range(len(tensors))]
        if verify:
            for code, _ in verify_frames_device(frames, tensors, dictionary=d_dict, stream=st):
                if code != 0:
                    raise FrameError(code)
        return frames

    def compress_pieces_device(self, pieces, content_size=None, stream=None):
        """ONE frame written piece by piece on the device (lzf_frame_append_device): `pieces` yields 1-D uint8 CUDA tensors, the
        stream's bytes one after another; every piece is offered to a FrameWriterDevice together with the tail the call before
        left untaken (less than one block), and the end of `pieces` finishes the frame.  Yields uint8 CUDA tensors, the frame's
        bytes in order: their concatenation is what `compress_many_device` returns for the concatenated input.  A piece may be
        reused by the caller once the next item has been yielded.  `content_size` goes into the header as it stands
        (compress_with_size_unchecked).  Raises FrameError."""
        import torch
        w, tail, L = None, None, ffi.lib()
        for piece in pieces:
            if w is None:
                w = FrameWriterDevice(self, content_size=content_size, device=piece.device)
            offer = piece if tail is None or not tail.numel() else torch.cat([tail, piece])
            out = torch.empty(L.lzf_frame_compress_bound(C.byref(w.settings), offer.numel()), dtype=torch.uint8, device=piece.device)
            view, taken, status, _ = w.write(offer, out, stream=stream)
            if status != 0:
                raise FrameError(status)
            tail = offer[taken:].clone()
            if view.numel():
                yield view
        if w is None:
            w = FrameWriterDevice(self, content_size=content_size)
        dev = w.cursor.device
        last = tail if tail is not None else torch.empty(0, dtype=torch.uint8, device=dev)
        out = torch.empty(L.lzf_frame_compress_bound(C.byref(w.settings), last.numel()), dtype=torch.uint8, device=dev)
        view, taken, status, phase = w.write(last, out, finish=True, stream=stream)
        if status != 0:
            raise FrameError(status)
        assert taken == last.numel() and phase == ffi.APPEND_DONE
        yield view

    def compress_streams_device(self, tensors, frame_bytes, with_size=False, stream=None, exact=False):
        """Every input of `tensors` (1-D uint8 CUDA tensors) written as a stream of back-to-back frames, one frame per
        `frame_bytes` input bytes (lzf_frame_compress_stream_device): the bytes of `compress_many_device` over the pieces,
        concatenated, packed on the device.  `with_size`: every frame's header carries its own piece's length.  Returns one
        uint8 CUDA tensor per input once `stream` (default: the current stream) has finished the call; raises FrameError.
        exact=True: as for `compress_many_device`, with lzf_frame_compress_stream_size_device as the size call."""
        import torch
        from . import device
        tensors = list(tensors)
        if not tensors:
            return []
        dev, s, d_dict = self._device_call(tensors, 0 if with_size else None)
        L = ffi.lib()
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        if d_dict is not None:
            st.wait_stream(torch.cuda.current_stream(dev))   # (the upload ran on the current stream)
        bounds = [L.lzf_frame_compress_stream_bound(C.byref(s), int(frame_bytes), t.numel()) for t in tensors]
        caps = None
        if exact:
            with torch.cuda.stream(st):
                status, out_len = device.stream_compressed_size(s, frame_bytes, tensors, dictionary=d_dict, stream=st)
            sizes, caps = self._finish(st, status, out_len), bounds
            outs = [torch.empty(n, dtype=torch.uint8, device=dev) for n in sizes]
        else:
            outs = [torch.empty(b, dtype=torch.uint8, device=dev) for b in bounds]
        with torch.cuda.stream(st):
            status, out_len = device.stream_compress(s, frame_bytes, tensors, outs, dictionary=d_dict, stream=st, caps=caps)
        lens = self._finish(st, status, out_len)
        if exact:
            assert lens == sizes, "the size call and the compress call disagree"
            return outs
        return [outs[f][:lens[f]] for f in range(len(tensors))]

    def compress_with_size(self, data):          # :147-157
        return self._run(data, len(data))

    def compress_with_size_unchecked(self, data, content_size):   # :142-145
        return self._run(data, content_size)


def read_header(frame):
    """LZ4FrameReader::new (src/framed/decompress.rs:102-161) -> ffi.FrameInfo."""
    frame = bytes(frame)
    info = ffi.FrameInfo()
    rc = ffi.lib().lzf_frame_read_header(frame, len(frame), C.byref(info))
    if rc != 0:
        raise FrameError(rc)
    return info


def decompress_frame(frame, dictionary=b"", cap=None):
    """decompress_frame (src/framed/decompress.rs:284-288); raises FrameError with the inner kind."""
    frame = bytes(frame)
    dictionary = bytes(dictionary)
    if cap is None:
        cap = min(max(1 << 20, len(frame) * 300 + (8 << 20)), 1 << 30)
    out = C.create_string_buffer(cap)
    n = C.c_size_t(0)
    used = C.c_size_t(0)
    rc = ffi.lib().lzf_frame_decompress(frame, len(frame), dictionary, len(dictionary), out, cap, C.byref(n), C.byref(used))
    ffi.check(rc)
    if rc != 0:
        raise FrameError(rc, ffi.buffer_bytes(out, n.value))
    return ffi.buffer_bytes(out, n.value)                 # (any length: a linked-block frame may decode to more than 2 GiB)


def decompress_frames(frames, dictionary=b"", caps=None, with_consumed=False):
    """`decompress_frame` of every frame through the same launches (lzf_frame_decompress_many).  Returns a list of
    (status, bytes): status 0 and the content, or the inner error kind and what the blocks before it produced —
    exactly what `decompress_frame` returns / raises for each frame alone."""
    frames = [bytes(f) for f in frames]
    dictionary = bytes(dictionary)
    n = len(frames)
    if n == 0:
        return []
    if caps is None:
        caps = [min(max(1 << 20, len(f) * 300 + (8 << 20)), 1 << 30) for f in frames]
    outs = [C.create_string_buffer(c) for c in caps]
    ins = (C.c_char_p * n)(*frames)
    lens = (C.c_size_t * n)(*[len(f) for f in frames])
    outp = (C.c_void_p * n)(*[C.addressof(o) for o in outs])
    capa = (C.c_size_t * n)(*caps)
    olen = (C.c_size_t * n)()
    used = (C.c_size_t * n)()
    st = (C.c_int * n)()
    ffi.check(ffi.lib().lzf_frame_decompress_many(n, ins, lens, dictionary, len(dictionary), outp, capa, olen, used, st))
    if with_consumed:
        return [(st[f], ffi.buffer_bytes(outs[f], olen[f]), used[f]) for f in range(n)]
    return [(st[f], ffi.buffer_bytes(outs[f], olen[f])) for f in range(n)]


def decompressed_sizes_device(frames, dictionary_len=0, stream=None):
    """Per frame (1-D uint8 CUDA tensors) what `decompress_frames_device` would report, without decoding and without output memory
    (lzf_frame_decompressed_size_device): [(status, size, consumed)] once `stream` has finished the call.  `dictionary_len`: the
    length of the dictionary the frames will be decoded with.  The content checksum is not verified: a frame that would fail it
    reports status 0."""
    import torch
    from . import device
    frames = list(frames)
    if not frames:
        return []
    s = stream if stream is not None else torch.cuda.current_stream(frames[0].device)
    with torch.cuda.stream(s):
        status, out_len, consumed = device.frame_decompressed_size(frames, dictionary_len=dictionary_len, stream=s)
    s.synchronize()
    return list(zip(status.cpu().tolist(), out_len.cpu().tolist(), consumed.cpu().tolist()))


def verify_frames_device(frames, expected, dictionary=None, stream=None):
    """Per frame (1-D uint8 CUDA tensors): does it deliver exactly the bytes of `expected[f]` (1-D uint8 CUDA tensors)?  Without
    decoding and without output memory (lzf_frame_verify_device): [(status, at)] once `stream` has finished the call — (0, length);
    (ffi.MISMATCH, the first differing position or the shorter length); (FrameChecksumFail, length) where the bytes are equal but the
    frame's content checksum is not theirs; or what `decompressed_sizes_device` reports for a frame that does not decode.
    `dictionary`: bytes or a uint8 CUDA tensor."""
    import torch
    from . import device
    frames, expected = list(frames), list(expected)
    if not frames:
        return []
    dev = frames[0].device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    if dictionary is not None and not isinstance(dictionary, torch.Tensor):
        dictionary = torch.frombuffer(bytearray(bytes(dictionary)), dtype=torch.uint8).to(dev) if len(dictionary) else None
        s.wait_stream(torch.cuda.current_stream(dev))   # (the upload ran on the current stream)
    with torch.cuda.stream(s):
        status, at, _ = device.frame_verify(frames, expected, dictionary=dictionary, stream=s)
    s.synchronize()
    return list(zip(status.cpu().tolist(), at.cpu().tolist()))


def frame_heads_device(frames, nbytes, dictionary=None, stream=None):
    """The first `nbytes` decoded bytes of every frame (1-D uint8 CUDA tensors), decoded on the device no further than that
    (lzf_frame_head_device): [(status, head)] once `stream` has finished the call — head a uint8 CUDA tensor of min(nbytes, the
    frame's length) bytes where the status is 0, the bytes of the blocks in front of the failing block otherwise.  A frame
    shorter than nbytes is status 0 with a shorter head.  Block checksums and the content checksum are NOT verified: a damaged
    frame may report status 0 here; `decompressed_sizes_device` and `verify_frames_device` verify.  `dictionary`: bytes or a uint8
    CUDA tensor."""
    import torch
    from . import device
    frames = list(frames)
    if not frames:
        return []
    dev = frames[0].device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    if dictionary is not None and not isinstance(dictionary, torch.Tensor):
        dictionary = torch.frombuffer(bytearray(bytes(dictionary)), dtype=torch.uint8).to(dev) if len(dictionary) else None
        s.wait_stream(torch.cuda.current_stream(dev))   # (the upload ran on the current stream)
    with torch.cuda.stream(s):
        heads, lens, statuses = device.frame_heads(frames, nbytes, dictionary=dictionary, stream=s)
    s.synchronize()
    st, ln = statuses.cpu().tolist(), lens.cpu().tolist()
    return [(st[f], heads[f, :ln[f]]) for f in range(len(frames))]


def stream_frame_heads_device(stream_tensor, index, nbytes, dictionary=None, stream=None):
    """The heads of the frames of one stream of back-to-back frames (a 1-D uint8 CUDA tensor) with `index`, its StreamIndex: one
    (status, head) per frame the index lists as reached — every entry without LZF_SFRAME_BEHIND_STOP, the frame that stopped the
    stream included — in the index's order.  A frame of a stream is a view of the stream tensor from the frame's in_off on, so this
    is `frame_heads_device` over those views: one lzf_frame_head_device."""
    reached = [e for e in index.frames if not int(e["flags"]) & ffi.SFRAME_BEHIND_STOP]
    return frame_heads_device([stream_tensor[int(e["in_off"]):] for e in reached], nbytes, dictionary=dictionary, stream=stream)


def decompress_frames_device(frames, dictionary=None, caps=None, stream=None, exact=False):
    """`decompress_frames` for frames that live on the device (1-D uint8 CUDA tensors), decoded on the device
    (lzf_frame_decompress_device_many).  Outputs are sized from lzf_frame_decompress_bound_device when `caps` is None — or, with
    `exact=True`, from lzf_frame_decompressed_size_device: each output is as long as its frame decodes to, not as long as its
    blocks could at worst.
    Returns [(status, out_tensor[:out_len], consumed)] once `stream` (default: the current stream) has finished the call."""
    import torch
    from . import device
    frames = list(frames)
    if not frames:
        return []
    dev = frames[0].device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    if caps is None and exact:
        dlen = dictionary.numel() if dictionary is not None else 0
        caps = [size for _, size, _ in decompressed_sizes_device(frames, dictionary_len=dlen, stream=s)]
    elif caps is None:
        caps = device.frame_decompress_bound(frames, stream=s)
    outs = [torch.empty(int(c), dtype=torch.uint8, device=dev) for c in caps]
    with torch.cuda.stream(s):
        status, out_len, consumed = device.frame_decompress_many(frames, outs, dictionary=dictionary, stream=s)
    s.synchronize()
    st, ol, co = status.cpu().tolist(), out_len.cpu().tolist(), consumed.cpu().tolist()
    return [(st[f], outs[f][:ol[f]], co[f]) for f in range(len(frames))]


def decompress_streams_device(streams, dictionary=None, caps=None, stream=None, exact=False):
    """Streams of back-to-back frames that live on the device (1-D uint8 CUDA tensors), every stream decoded on the device into
    one contiguous tensor (lzf_frame_decompress_stream_device).  Outputs are sized from lzf_frame_stream_bound_device when `caps`
    is None — or, with `exact=True`, from lzf_frame_stream_decompressed_size_device: each output is as long as its stream decodes
    to, not as long as its blocks could at worst.
    Returns [(status, out_tensor[:out_len], consumed, n_frames)] once `stream` (default: the current stream) has
    finished the call: the status that ended the stream (0: every byte was read), the bytes of its frames up to there, the
    input bytes read and the number of frames that ended at their EndMark."""
    import torch
    from . import device
    streams = list(streams)
    if not streams:
        return []
    dev = streams[0].device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    if caps is None and exact:
        dlen = dictionary.numel() if dictionary is not None else 0
        with torch.cuda.stream(s):
            sizes = device.stream_decompressed_size(streams, dictionary_len=dlen, stream=s)[1]
        s.synchronize()
        caps = sizes.cpu().tolist()
    elif caps is None:
        caps = device.stream_decompress_bound(streams, stream=s)
    outs = [torch.empty(int(c), dtype=torch.uint8, device=dev) for c in caps]
    with torch.cuda.stream(s):
        status, out_len, consumed, n_frames = device.stream_decompress(streams, outs, dictionary=dictionary, stream=s)
    s.synchronize()
    st, ol, co, nf = status.cpu().tolist(), out_len.cpu().tolist(), consumed.cpu().tolist(), n_frames.cpu().tolist()
    return [(st[f], outs[f][:ol[f]], co[f], nf[f]) for f in range(len(streams))]


StreamIndex = collections.namedtuple("StreamIndex", "status out_len consumed n_frames frames")
StreamIndex.__doc__ = """What lzf_frame_stream_decompressed_size_device says about one stream: `status`, `out_len`, `consumed` and
`n_frames` as decompress_streams_device would report them (the content checksums not verified), and `frames`, a numpy structured
array with the fields of lzf_stream_frame (in_off, consumed, out_off, out_len, content_size, status, flags), one entry per
frame the walk finds."""


def stream_index_device(streams, dictionary_len=0, stream=None):
    """Exact sizes and the frame index of streams of back-to-back frames that live on the device (1-D uint8 CUDA tensors), found
    without decoding and without output memory (lzf_frame_stream_count_device, lzf_frame_stream_decompressed_size_device).
    Returns [StreamIndex] once `stream` has finished the call.  `dictionary_len`: the length of the dictionary the streams
    will be decoded with."""
    import numpy as np
    import torch
    from . import device
    streams = list(streams)
    if not streams:
        return []
    s = stream if stream is not None else torch.cuda.current_stream(streams[0].device)
    with torch.cuda.stream(s):
        status, out_len, consumed, n_frames, _, entries = device.stream_index(streams, dictionary_len=dictionary_len, stream=s)
    s.synchronize()
    st, ol, co, nf = status.cpu().tolist(), out_len.cpu().tolist(), consumed.cpu().tolist(), n_frames.cpu().tolist()
    frames = [np.ascontiguousarray(e.cpu().numpy()).view(device.SFRAME) for e in entries]
    return [StreamIndex(st[k], ol[k], co[k], nf[k], frames[k]) for k in range(len(streams))]


def locate_frames(index, start, stop):
    """lzf_stream_index_locate: (first, count) of the frames of `index` (a StreamIndex or its `frames`) whose output meets the
    bytes [start, stop) of the stream's output; count 0 where none does.  Host only."""
    import numpy as np
    frames = np.ascontiguousarray(getattr(index, "frames", index))
    first, count = C.c_size_t(0), C.c_size_t(0)
    ffi.check(ffi.lib().lzf_stream_index_locate(frames.ctypes.data if len(frames) else None, len(frames), max(int(start), 0),
                                                max(int(stop), 0), C.byref(first), C.byref(count)))
    return first.value, count.value


def read_stream_range_device(stream_tensor, index, start, stop, dictionary=None, stream=None):
    """Bytes [start, min(stop, index.out_len)) of the output of one stream of back-to-back frames (a 1-D uint8 CUDA tensor) with
    `index`, its StreamIndex: only the frames that hold the range are decoded.  lzf_stream_index_locate finds them; a run of
    whole frames is itself a stream, so stream_tensor[in_off of the first : in_off + consumed of the last] goes through
    decompress_streams_device, with an output of exactly those frames' lengths.  Returns a view of that output.
    Raises FrameError when the decode of those frames does not end as the index says: with the decode's status where it is not 0
    (a damaged frame in the range: its error, also where the index lists it with that error; a content checksum, which the
    index never verifies), with InputError where the lengths differ (the index is not of these bytes).  A range read verifies the
    content checksums only of the frames it decodes: damage in the frames it skips goes unnoticed."""
    import torch
    frames = index.frames
    start, stop = max(int(start), 0), min(int(stop), int(index.out_len))
    first, count = locate_frames(frames, start, stop) if start < stop else (0, 0)
    if count == 0:
        return torch.empty(0, dtype=torch.uint8, device=stream_tensor.device)
    a, b = frames[first], frames[first + count - 1]
    lo, hi = int(a["in_off"]), int(b["in_off"]) + int(b["consumed"])
    base, total = int(a["out_off"]), int(b["out_off"]) + int(b["out_len"]) - int(a["out_off"])
    (st, out, used, _), = decompress_streams_device([stream_tensor[lo:hi]], dictionary=dictionary, caps=[total], stream=stream)
    if st != 0:
        raise FrameError(st)
    if out.numel() != total or used != hi - lo:
        raise FrameError(16)
    return out[start - base:stop - base]


FrameBlockIndex = collections.namedtuple("FrameBlockIndex", "status out_len consumed blocks")
FrameBlockIndex.__doc__ = """What lzf_frame_block_index_device says about one frame: `status`, `out_len` and `consumed` as
decompressed_sizes_device reports them (the content checksum not verified), and `blocks`, a numpy structured array with the fields
of lzf_frame_block (in_off, out_off, out_len, in_len, want_sum, block_maxsize, status, flags, reserved), one entry per block the
walk finds."""


def block_index_device(frames, dictionary_len=0, stream=None):
    """Exact sizes and the block index of frames that live on the device (1-D uint8 CUDA tensors), found without decoding and
    without output memory (lzf_frame_block_count_device, lzf_frame_block_index_device).  Returns [FrameBlockIndex] — per frame
    (status, out_len, consumed, entries as a numpy structured array) — once `stream` has finished the call.  `dictionary_len`: the
    length of the dictionary the frames will be decoded with."""
    import numpy as np
    import torch
    from . import device
    frames = list(frames)
    if not frames:
        return []
    s = stream if stream is not None else torch.cuda.current_stream(frames[0].device)
    with torch.cuda.stream(s):
        status, out_len, consumed, _, entries = device.frame_block_index(frames, dictionary_len=dictionary_len, stream=s)
    s.synchronize()
    st, ol, co = status.cpu().tolist(), out_len.cpu().tolist(), consumed.cpu().tolist()
    blocks = [np.ascontiguousarray(e.cpu().numpy()).view(device.FBLOCK) for e in entries]
    return [FrameBlockIndex(st[k], ol[k], co[k], blocks[k]) for k in range(len(frames))]


def locate_blocks(index, start, stop):
    """lzf_block_index_locate: (first, count) of the delivered blocks of `index` (a FrameBlockIndex or its `blocks`) whose output
    meets the bytes [start, stop) of the frame's output; count 0 where none does.  Host only."""
    import numpy as np
    blocks = np.ascontiguousarray(getattr(index, "blocks", index))
    first, count = C.c_size_t(0), C.c_size_t(0)
    ffi.check(ffi.lib().lzf_block_index_locate(blocks.ctypes.data if len(blocks) else None, len(blocks), max(int(start), 0),
                                               max(int(stop), 0), C.byref(first), C.byref(count)))
    return first.value, count.value


def read_frame_range_device(frame_tensor, index, start, stop, dictionary=None, stream=None):
    """Bytes [start, min(stop, index.out_len)) of the output of one frame of independent blocks (a 1-D uint8 CUDA tensor) with
    `index`, its FrameBlockIndex: only the blocks that hold the range are decoded (lzf_block_index_locate finds them,
    lzf_frame_decompress_blocks_device decodes the run into a tensor of exactly the run's length).  Returns a view of that output.
    Raises FrameError with the run's status where it is not 0 (a block damaged since the index was taken: BlockChecksumFail, a
    codec error, or 6, LZF_CONTRACT, where a block no longer decodes to the indexed length), ffi.LzfError for a linked-block frame (decode the
    frame).  A range read verifies neither the content checksum nor the blocks it skips."""
    import torch
    from . import device
    blocks = index.blocks
    start, stop = max(int(start), 0), min(int(stop), int(index.out_len))
    first, count = locate_blocks(blocks, start, stop) if start < stop else (0, 0)
    if count == 0:
        return torch.empty(0, dtype=torch.uint8, device=frame_tensor.device)
    run = blocks[first:first + count]
    base, total = int(run[0]["out_off"]), int(run["out_len"].sum())
    s = stream if stream is not None else torch.cuda.current_stream(frame_tensor.device)
    with torch.cuda.stream(s):
        out = torch.empty(total, dtype=torch.uint8, device=frame_tensor.device)
        status, out_len = device.frame_decompress_blocks([frame_tensor], [run], [out], dictionary=dictionary, stream=s)
    s.synchronize()
    st = int(status.item())
    if st != 0:
        raise FrameError(st)
    assert int(out_len.item()) == total
    return out[start - base:stop - base]


class FrameWriterDevice:
    """The incremental frame writer for bytes in device memory (lzf_frame_append_device): a write cursor the caller comes back
    to.  `settings`: a CompressionSettings (its dictionary is used unless `dictionary` — bytes or a uint8 CUDA tensor — is
    given) or an ffi.Settings without a host dictionary.  The stream's table, the last 64 KiB taken and the content hash are
    carried on the device; nothing of a call comes back to the host but its four result words."""

    def __init__(self, settings, dictionary=None, content_size=None, device=None):
        import torch
        from . import device as dev_mod
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        if isinstance(settings, CompressionSettings):
            if dictionary is None:
                dictionary = settings._dictionary or None
            settings = settings._struct(content_size)
            settings.dictionary = None                      # (the device call takes the dictionary in device memory)
            settings.dictionary_len = 0
        if dictionary is not None and not isinstance(dictionary, torch.Tensor):
            dictionary = torch.frombuffer(bytearray(bytes(dictionary)), dtype=torch.uint8).to(dev) if len(dictionary) else None
        self.settings, self.dictionary = settings, dictionary
        self.cursor = dev_mod.new_frame_write_cursors(1, dev)
        self.phase, self.status, self.taken = ffi.APPEND_MORE, 0, 0

    @property
    def finished(self):
        """The frame is over: the EndMark is written, or it stopped with `status`."""
        return self.phase == ffi.APPEND_DONE

    def write(self, tensor, out, finish=False, stream=None):
        """Offer `tensor` (1-D uint8 CUDA), the next bytes of the stream; `finish`: they are its last.  Whole blocks of it (under
        `finish` the shorter last one too) are taken as far as their frame bound fits `out` (1-D uint8 CUDA).  Returns
        (piece_view, taken, status, phase) once the stream has finished the call: out[:n], the next bytes of the frame; the
        bytes of `tensor` that were taken — offer tensor[taken:] again in front of what follows; the status (ffi.OUT_CAPACITY with
        phase APPEND_MORE: not even one block fits, pass more room); ffi.APPEND_MORE / APPEND_NEED_INPUT / APPEND_DONE."""
        import torch
        from . import device as dev_mod
        s = stream if stream is not None else torch.cuda.current_stream(self.cursor.device)
        with torch.cuda.stream(s):
            status, out_len, taken, phase = dev_mod.frame_append(self.settings, [tensor], [ffi.APPEND_FINISH if finish else 0], self.cursor, [out],
                                                                 dictionary=self.dictionary, stream=s)
        s.synchronize()
        self.status, self.phase = int(status.cpu()[0]), int(phase.cpu()[0])
        t = int(taken.cpu()[0])
        self.taken += t
        return out[:int(out_len.cpu()[0])], t, self.status, self.phase


class FrameCursorDevice:
    """LZ4FrameReader for a frame in device memory (a 1-D uint8 CUDA tensor), decoded on the device piece by piece
    (lzf_frame_resume_device): a cursor the caller comes back to.  `read_into(out)` decodes as many whole blocks as fit `out`
    and says where it stopped; the 64 KiB window of a linked-block frame and the content hash are carried on the device, the
    content checksum is verified at the EndMark.  The frame tensor may still be filling: pass the bytes that are there as
    `in_len`, and a frame that ends inside an item reports ffi.RESUME_NEED_INPUT — come back with more.  `dictionary`: bytes or a
    uint8 CUDA tensor, the same for every call."""

    def __init__(self, frame_tensor, dictionary=None):
        import torch
        from . import device
        self.frame = frame_tensor
        dev = frame_tensor.device
        if dictionary is not None and not isinstance(dictionary, torch.Tensor):
            dictionary = torch.frombuffer(bytearray(bytes(dictionary)), dtype=torch.uint8).to(dev) if len(dictionary) else None
        self.dictionary = dictionary
        self.cursor = device.new_frame_cursors(1, dev)
        self.phase, self.status, self.consumed = ffi.RESUME_MORE, 0, 0

    @property
    def finished(self):
        """The frame is over: the EndMark was read (and the content checksum verified), or it stopped with `status`."""
        return self.phase == ffi.RESUME_DONE

    def read_into(self, out_tensor, in_len=None, stream=None):
        """Decode the next whole blocks that fit `out_tensor` (1-D uint8 CUDA) from the first `in_len` bytes of the frame (None:
        all of them).  Returns (n_bytes, status, phase) once the stream has finished the call: out_tensor[:n_bytes] is the next
        piece of the content.  status ffi.OUT_CAPACITY with phase RESUME_MORE: not even the next block fits, pass more room."""
        import torch
        from . import device
        s = stream if stream is not None else torch.cuda.current_stream(self.frame.device)
        with torch.cuda.stream(s):
            status, out_len, consumed, phase = device.frame_resume([self.frame], None if in_len is None else [in_len], self.cursor, [out_tensor],
                                                                   dictionary=self.dictionary, stream=s)
        s.synchronize()
        self.status, self.phase, self.consumed = int(status.cpu()[0]), int(phase.cpu()[0]), int(consumed.cpu()[0])
        return int(out_len.cpu()[0]), self.status, self.phase


def iter_frame_pieces_device(frame_tensor, piece_bytes, dictionary=None):
    """The content of one frame in device memory, piece by piece through ONE buffer of `piece_bytes` bytes: yields views of that
    buffer (valid until the next step), each the next whole blocks that fit.  piece_bytes must hold the frame's largest block
    bound (block_maxsize always does).  Raises FrameError where the frame fails, the content checksum included, or ends early."""
    import torch
    cur = FrameCursorDevice(frame_tensor, dictionary=dictionary)
    buf = torch.empty(int(piece_bytes), dtype=torch.uint8, device=frame_tensor.device)
    while not cur.finished:
        n, status, phase = cur.read_into(buf)
        if status != 0:
            raise FrameError(status)
        if phase == ffi.RESUME_NEED_INPUT:
            raise FrameError(16)                # InputError: the frame ends inside an item, and no more input comes
        if n:
            yield buf[:n]


class FrameBlockReader:
    """The C ABI's block-by-block reader (lzf_frame_reader_*, include/lzfear_frame.h) over a frame in memory:
    `LZ4FrameReader::new` + `decode_block` (src/framed/decompress.rs:102-161,198-282), one call = one block."""

    def __init__(self, frame):
        self._frame = bytes(frame)                       # kept alive: the reader points into it
        self._h = C.c_void_p()
        rc = ffi.lib().lzf_frame_reader_new(self._frame, len(self._frame), C.byref(self._h))
        if rc != 0:
            raise FrameError(rc)
        self.info = ffi.FrameInfo()
        ffi.lib().lzf_frame_reader_info(self._h, C.byref(self.info))
        self._buf = C.create_string_buffer(int(self.info.block_maxsize) * 2 + 64)

    def decode_block(self, dictionary=b""):
        """One block (b"" once the frame is finished — or for a block that decodes to nothing); raises FrameError."""
        n = C.c_size_t(0)
        dictionary = bytes(dictionary)
        rc = ffi.lib().lzf_frame_reader_decode_block(self._h, dictionary, len(dictionary), self._buf, len(self._buf), C.byref(n))
        ffi.check(rc)
        if rc != 0:
            raise FrameError(rc)
        return C.string_at(self._buf, n.value)

    def finished(self):
        return bool(ffi.lib().lzf_frame_reader_finished(self._h))

    def consumed(self):
        return int(ffi.lib().lzf_frame_reader_consumed(self._h))

    def close(self):
        if self._h:
            ffi.lib().lzf_frame_reader_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LZ4FrameReader:
    """Block-by-block frame reader — `LZ4FrameReader` + `LZ4FrameIoReader` of the reference
    (src/framed/decompress.rs:46-77,82-280) over a file-like object: `read(n)`, `fill_buf()`,
    `consume(n)`, `block_size()`, `frame_size()`, `dictionary_id()`.

    The reference decodes one block per `fill_buf`; one GPU launch per block would waste the device,
    so independent-block frames are read ahead `readahead` blocks at a time and decoded as one batch
    (errors still surface at the block where the reference would report them).  Linked-block frames
    are sequential by construction and go block by block with the 64 KiB window as prefix."""

    def __init__(self, reader, dictionary=b"", readahead=16):
        self._r = reader
        self._dict = bytes(dictionary)
        self._readahead = max(1, int(readahead))
        hdr = self._read_exact(7)
        flg = hdr[4] if len(hdr) > 4 else 0
        extra = (8 if flg & 0x08 else 0) + (4 if flg & 0x01 else 0)
        if len(hdr) == 7 and extra:
            hdr += self._read_exact(extra, allow_short=True)
        self.info = ffi.FrameInfo()
        rc = ffi.lib().lzf_frame_read_header(hdr, len(hdr), C.byref(self.info))
        if rc != 0:
            raise FrameError(rc)
        self._linked = not (self.info.flags & 0x20)
        self._bsum = bool(self.info.flags & 0x10)
        self._csum = bool(self.info.flags & 0x04)
        self._hasher = ffi.Xxh32State()
        ffi.lib().lzf_xxh32_reset(C.byref(self._hasher), 0)
        self._window = b""                 # carryover_window (:90,:253-269)
        self._ready = []                   # decoded blocks waiting to be handed out
        self._pending_error = None
        self._buffer = b""
        self._taken = 0
        self._finished = False

    # ---- accessors (:167-175)
    def block_size(self):
        return int(self.info.block_maxsize)

    def frame_size(self):
        return int(self.info.content_size) if self.info.has_content_size else None

    def dictionary_id(self):
        return int(self.info.dictionary_id) if self.info.has_dictionary_id else None

    def _read_exact(self, n, allow_short=False):
        out = b""
        while len(out) < n:
            c = self._r.read(n - len(out))
            if not c:
                break
            out += c
        return out

    def _scan_block(self):
        """One block of the wire format (:205-235) -> ('end', checksum|None) | ('blk', data, compressed)."""
        w = self._read_exact(4)
        if len(w) < 4:
            raise FrameError(16)
        bl = int.from_bytes(w, "little")
        if bl == 0:
            want = None
            if self._csum:
                c = self._read_exact(4)
                if len(c) < 4:
                    raise FrameError(16)
                want = int.from_bytes(c, "little")
            return ("end", want)
        compressed = not (bl & 0x80000000)
        bl &= 0x7FFFFFFF
        if bl > self.block_size():
            raise FrameError(22)
        data = self._read_exact(bl)
        if len(data) < bl:
            raise FrameError(16)
        if self._bsum:
            c = self._read_exact(4)
            if len(c) < 4:
                raise FrameError(16)
            return ("blk", data, compressed, int.from_bytes(c, "little"))       # verified by _refill, on the device
        return ("blk", data, compressed, None)

    def _refill(self):
        """Scan up to `readahead` blocks and decode the compressed ones in one batch (one block at a time
        for linked frames).  Results, an EndMark or the first error are queued in stream order."""
        scanned, tail = [], None
        limit = 1 if self._linked else self._readahead
        while len(scanned) < limit:
            try:
                b = self._scan_block()
            except FrameError as e:
                tail = e                      # reported after the blocks before it have been delivered
                break
            if b[0] == "end":
                tail = b
                break
            scanned.append(b)
        if self._bsum and scanned:                                  # :228-235, all scanned blocks in one device launch
            got = ffi.xxh32_blocks_host([b[1] for b in scanned])
            for k, (b, h) in enumerate(zip(scanned, got)):
                if b[3] != h:
                    scanned, tail = scanned[:k], FrameError(19)     # reported after the blocks before it
                    break
        bmax = self.block_size()
        if self._linked and not self._window:
            self._window = self._dict                               # :239-241
        prefix = self._window if self._linked else self._dict       # :238-245
        items = [dict(input=d, prefix=prefix, limit=bmax, out_cap=bmax + len(d)) for (_, d, comp, _c) in scanned if comp]
        res = iter(ffi.decompress_blocks_host(items)) if items else iter(())
        for (_, d, comp, _c) in scanned:
            if comp:
                rc, out = next(res)
                if rc != 0:
                    self._ready.append(FrameError(rc))              # CodecError
                    return
            else:
                out = d                                             # :250
            if self._linked:                                        # window update :253-269
                self._window = (self._window + out)[-WINDOW_SIZE:] if len(out) < WINDOW_SIZE else out[-WINDOW_SIZE:]
            if len(out) > bmax:
                self._ready.append(FrameError(22))                  # :272-274
                return
            self._ready.append(out)
        if tail is not None:
            self._ready.append(tail)

    def fill_buf(self):
        """BufRead::fill_buf (:64-71): the current decoded block (b"" at the end of the frame)."""
        if self._taken == len(self._buffer) and not self._finished:
            self._buffer, self._taken = b"", 0
            if not self._ready:
                self._refill()
            item = self._ready[0]
            if isinstance(item, FrameError):
                raise item                                          # sticky
            if isinstance(item, tuple):                             # EndMark: verify the content checksum (:206-213)
                if item[1] is not None and item[1] != ffi.lib().lzf_xxh32_digest(C.byref(self._hasher)):
                    self._ready[0] = FrameError(20)
                    raise self._ready[0]
                self._ready.pop(0)
                self._finished = True
            else:
                self._ready.pop(0)
                if self._csum:
                    ffi.lib().lzf_xxh32_update(C.byref(self._hasher), item, len(item))    # :276-278
                self._buffer = item
        return self._buffer[self._taken:] if self._taken else self._buffer      # (no copy of a block nobody has consumed from)

    def consume(self, amt):
        self._taken += amt
        assert self._taken <= len(self._buffer), "You consumed more bytes than I even gave you!"   # :75

    def read(self, n=-1):
        """io::Read::read (:54-60) when n >= 0; read_to_end when n < 0 (a 0-byte block ends it, like the
        reference's read_to_end)."""
        if n is None or n < 0:
            out = b""
            while True:
                b = self.fill_buf()
                if not b:
                    return out
                out += b
                self.consume(len(b))
        b = self.fill_buf()
        take = min(len(b), n)
        self.consume(take)
        return b[:take]
