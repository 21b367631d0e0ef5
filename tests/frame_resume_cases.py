"""Cases and a pure-Python model of lzf_frame_resume_device (include/lzfear_frame.h, "resumable decode of frames in device memory")
— TEST INFRASTRUCTURE, no GPU.

The model restates the rule of one call over two things only: a plain walk of the frame's length words, and the oracle's frame
decode (tests/oracle_ffi.py) of the frame cut behind each block, which says what the reader delivers up to there and where it
stops.  tests/test_frame_resume_cases_cpu.py holds the model to the oracle's decode of the whole frame, holds the shared rules
header (rust-lz-fear_amd/csrc/lzf_frame_resume_rules.h, compiled with g++) to the model, and counts that every rule is reached;
tests/test_gpu_frame_resume.py holds the device to the model and to lzf_frame_decompress_device_many.

Frames of the flavour product are written by the oracle's frame compressor with block_size 64 KiB; the frames with chosen block
lengths (short linked blocks, stored blocks, an empty block, a block that decodes past block_maxsize) are assembled here from
blocks the oracle's compress2 wrote."""
import functools
import struct

import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import synth

BS = 65536                                  # block_maxsize of every frame here: the format's minimum
MORE, NEED_INPUT, DONE = 0, 1, 2            # LZF_RESUME_*
OK, OUT_CAPACITY, INPUT_ERROR, BLOCK_CHECKSUM_FAIL, FRAME_CHECKSUM_FAIL, BLOCK_SIZE_OVERFLOW = 0, 7, 16, 19, 20, 22
FL_INDEP, FL_BLOCKSUM, FL_CSIZE, FL_CSUM, FL_DICTID = 0x20, 0x10, 0x08, 0x04, 0x01
WINDOW = 65536
OUT_ROOM = 10 * BS                          # room for the content of any frame here, for the oracle's decode


def content(n, at=0):
    return synth.silesia_mix(at << 20, (at << 20) + n).tobytes()


@functools.lru_cache(maxsize=None)
def dictionary():
    return synth.text_zipf_64k().tobytes()[:40000]


# ---- frames ------------------------------------------------------------------------------------------------------------------

def oracle_frame(data, indep, dic, bsum, csum, csize):
    s = o.make_settings(independent_blocks=indep, block_checksums=bsum, content_checksum=csum, block_size=BS,
                        dictionary=dic if dic else None, content_size=len(data) if csize else None)
    rc, f = o.frame_compress(data, s)
    assert rc == 0
    return f


def assemble(blocks, linked, dic=b"", bsum=False, csum=True):
    """A frame of the given blocks: ("lz", data) compressed by the oracle's compress2 behind its history (a linked block: the last
    64 KiB of dictionary ++ content so far; an independent one: the dictionary), ("raw", data) stored, ("payload", bytes) a
    compressed block given as it stands.  Returns (frame, the content the blocks with data stand for)."""
    flg = 0x40 | (0 if linked else FL_INDEP) | (FL_BLOCKSUM if bsum else 0) | (FL_CSUM if csum else 0)
    hdr = bytes([flg, 0x40])
    out = struct.pack("<I", 0x184D2204) + hdr + bytes([(o.xxh32(hdr) >> 8) & 0xFF])
    whole = b""
    for kind, data in blocks:
        if kind == "lz":
            hist = ((dic + whole) if linked else dic)[-WINDOW:]
            rc, payload = o.compress2(hist + data, cursor=len(hist))
            assert rc == 0 and 0 < len(payload) <= BS
            word = len(payload)
            whole += data
        elif kind == "raw":
            payload, word = data, len(data) | 0x80000000
            whole += data
        else:
            payload, word = data, len(data)
        out += struct.pack("<I", word) + payload
        if bsum:
            out += struct.pack("<I", o.xxh32(payload))
    out += struct.pack("<I", 0)
    if csum:
        out += struct.pack("<I", o.xxh32(whole))
    return out, whole


def walk(frame):
    """The plain walk of length words over the whole frame: (flags, header_len, blocks [(word_off, len, compressed, end_off)],
    (endmark_off, end) or None).  Every frame here has a sound header."""
    flg = frame[4]
    r = 6 + (8 if flg & FL_CSIZE else 0) + (4 if flg & FL_DICTID else 0) + 1
    header_len, blocks, end = r, [], None
    while len(frame) - r >= 4:
        (w,) = struct.unpack_from("<I", frame, r)
        if w == 0:
            e = r + 4 + (4 if flg & FL_CSUM else 0)
            end = (r, e) if e <= len(frame) else None
            break
        n = w & 0x7FFFFFFF
        e = r + 4 + n + (4 if flg & FL_BLOCKSUM else 0)
        if n > BS or e > len(frame):
            break
        blocks.append((r, n, not (w & 0x80000000), e))
        r = e
    return flg, header_len, blocks, end


def damage(frame, at, xor=0x55):
    b = bytearray(frame)
    b[at] ^= xor
    return bytes(b)


@functools.lru_cache(maxsize=None)
def all_cases():
    """[dict(name, frame, dict, tags)]: the flavour product, the special frames, the damaged frames."""
    dic = dictionary()
    data = content(4 * BS + 20000)
    cases = []

    def add(name, frame, d=b"", **tags):
        cases.append(dict(name=name, frame=frame, dict=d, tags=tags))

    for indep in (True, False):
        for d in (b"", dic):
            for bsum in (False, True):
                for csum in (False, True):
                    for csize in (False, True):
                        add(f"{'indep' if indep else 'linked'}{'+dict' if d else ''}{'+bsum' if bsum else ''}{'+csum' if csum else ''}{'+csize' if csize else ''}",
                            oracle_frame(data, indep, d, bsum, csum, csize), d, flavour=True)
    add("empty frame", oracle_frame(b"", True, b"", False, True, False))
    add("one short block", oracle_frame(data[:1000], False, b"", True, True, True))
    noise = synth.gen_random(7, 3 * BS + 5).tobytes()
    add("stored blocks", oracle_frame(noise, False, b"", True, True, False))
    stored = walk(cases[-1]["frame"])[2]
    assert stored and not any(c for _, _, c, _ in stored)
    # linked blocks of chosen lengths: windows shorter than, equal to and longer than 64 KiB, a short piece behind a full window
    short = [("lz", data[0:1000]), ("lz", data[1000:31000]), ("lz", data[31000:65536]), ("lz", data[65536:65536 + 500]), ("raw", data[66036:70000]),
             ("lz", data[70000:70000 + BS]), ("lz", data[70000 + BS:70000 + BS + 300])]
    for d in (b"", dic):
        f, whole = assemble(short, True, d, bsum=True)
        add("linked short blocks" + ("+dict" if d else ""), f, d, whole=whole)
    mid = [("lz", data[:BS]), ("lz", data[BS:2 * BS]), ("payload", b"\x00"), ("lz", data[2 * BS:3 * BS])]
    for linked in (False, True):
        f, _ = assemble(mid, linked)
        add(("linked" if linked else "indep") + " empty block in the middle", f, stop="empty")
    # the stop rules, each at block 2 of 5: a damaged block checksum, a codec error, a block that decodes past block_maxsize
    for linked in (False, True):
        base = oracle_frame(data, not linked, b"", True, True, False)
        blk = walk(base)[2]
        add(("linked" if linked else "indep") + " block checksum damaged", damage(base, blk[2][3] - 1), stop="checksum")
        base = oracle_frame(data, not linked, b"", False, True, False)
        blk = walk(base)[2]
        bad = bytearray(base)
        bad[blk[2][0] + 4:blk[2][0] + 8] = b"\x0F\x00\x00\x00"          # a token with no literals and a match at offset 0
        add(("linked" if linked else "indep") + " codec error", bytes(bad), stop="codec")
        over = bytes(BS - 11) + bytes(range(1, 16))                     # a long match, then literals that carry it past block_maxsize
        f, _ = assemble([("lz", data[:BS]), ("lz", data[BS:2 * BS]), ("lz", over), ("lz", data[2 * BS:3 * BS]), ("lz", data[3 * BS:4 * BS])], linked)
        add(("linked" if linked else "indep") + " block past block_maxsize", f, stop="oversize")
    base = oracle_frame(data, False, dic, False, True, True)
    add("content checksum damaged", damage(base, len(base) - 2), dic, stop="content")
    base = oracle_frame(data, True, b"", False, True, False)
    blk = walk(base)[2]
    bad = bytearray(base)
    bad[blk[3][0]:blk[3][0] + 4] = struct.pack("<I", BS + 1)
    add("length word above block_maxsize", bytes(bad), stop="overflow")
    add("wrong magic", b"\x05" + base[1:], stop="header")
    # two blocks of very compressible content, both checksums: short enough to be cut at every byte
    add("two small blocks", oracle_frame(bytes(range(256)) * 400, False, b"", True, True, False), growth=True)
    return cases


# ---- the model ---------------------------------------------------------------------------------------------------------------

def parse_header(b):
    """LZ4FrameReader::new over b: ("cut",) | ("err", status, consumed) | ("ok", flags, header_len)."""
    if len(b) < 4:
        return ("cut",)
    if struct.unpack_from("<I", b)[0] != 0x184D2204:
        return ("err", 17, 4)
    if len(b) < 5:
        return ("cut",)
    flg = b[4]
    if flg >> 6 != 1:
        return ("err", 24, 5)
    if flg & 2:
        return ("err", 25, 5)
    if len(b) < 6:
        return ("cut",)
    if b[5] & 0x8F:
        return ("err", 26, 6)
    r = 6 + (8 if flg & FL_CSIZE else 0) + (4 if flg & FL_DICTID else 0) + 1
    if len(b) < r:
        return ("cut",)
    if b[r - 1] != (o.xxh32(b[4:r - 1]) >> 8) & 0xFF:
        return ("err", 18, r)
    if (b[5] >> 4) & 7 < 4:
        return ("err", 23, r)
    return ("ok", flg, r)


@functools.lru_cache(maxsize=None)
def _decoded(frame, dic):
    """(flags, header_len, blocks, cum, stop, content, end): the walk, and the oracle's decode of the frame cut behind block k — what the
    reader has delivered there (cum[k + 1] bytes of content) and whether it stopped (stop = (k, status, consumed))."""
    flags, header_len, blocks, end = walk(frame)
    cum, stop, content = [0], None, b""
    for k, (_, _, _, e) in enumerate(blocks):
        rc, out, used = o.frame_decompress(frame[:e], dic, cap=OUT_ROOM)
        if rc != INPUT_ERROR:
            stop = (k, rc, used)
            assert used == e and len(out) == cum[-1]
            break
        cum.append(len(out))
        content = out
    return flags, header_len, blocks, cum, stop, content, end


class Model:
    """One frame's cursor, restated: call(in_len, cap) -> (out bytes, status, consumed, phase, events)."""

    def __init__(self, case):
        self.frame, self.dict = case["frame"], case["dict"]
        self.phase, self.status, self.in_off, self.parsed, self.block, self.delivered = MORE, OK, 0, False, 0, 0
        self.window = min(len(self.dict), WINDOW)
        if parse_header(self.frame)[0] == "ok":
            self.flags, self.header_len, self.blocks, self.cum, self.stop, self.content, self.end = _decoded(self.frame, self.dict)

    def call(self, in_len, cap):
        ev = set()
        f = self.frame
        if self.phase == DONE:
            return b"", self.status, self.in_off, DONE, {"held"}
        if not self.parsed:
            h = parse_header(f[:in_len])
            if h[0] == "cut":
                return b"", OK, 0, NEED_INPUT, {"need input: header"}
            if h[0] == "err":
                self.phase, self.status, self.in_off = DONE, h[1], h[2]
                return b"", h[1], h[2], DONE, {"header error"}
        r = self.in_off if self.parsed else self.header_len
        room, k, first, end, status = cap, self.block, self.block, None, OK
        while end is None:
            if in_len - r < 4:
                end = NEED_INPUT; ev.add("need input: length word")
                if self.end and r == self.end[0]:
                    ev.add("need input: in front of the EndMark")
                break
            (w,) = struct.unpack_from("<I", f, r)
            if w == 0:
                if self.flags & FL_CSUM and in_len - (r + 4) < 4:
                    end = NEED_INPUT; ev |= {"need input: content checksum", "need input: in front of the EndMark"}
                    break
                end = DONE; r += 4 + (4 if self.flags & FL_CSUM else 0); ev.add("endmark")
                break
            n, compressed = w & 0x7FFFFFFF, not (w & 0x80000000)
            if n > BS:
                end, status = DONE, BLOCK_SIZE_OVERFLOW; r += 4; ev.add("length word overflow")
                break
            if in_len - (r + 4) < n:
                end = NEED_INPUT; ev.add("need input: payload")
                break
            e = r + 4 + n + (4 if self.flags & FL_BLOCKSUM else 0)
            if in_len < e:
                end = NEED_INPUT; ev.add("need input: block checksum")
                break
            bound = min(255 * n + 16, BS) if compressed else n
            if bound > room:
                ev.add("more at " + ("the first" if k == 0 else "the last" if k == len(self.blocks) - 1 else "a middle") + " block")
                if k == first:
                    return b"", OUT_CAPACITY, self.in_off, MORE, ev | {"no room"}
                end = MORE
                break
            room -= bound; k += 1; r = e
        self.parsed = True
        upto = k
        if self.stop is not None and first <= self.stop[0] < k:
            j, status, r = self.stop
            upto, end = j, DONE
            ev.add(f"stop {status}: " + ("alone" if k - first == 1 else "first of its piece" if j == first else "last of its piece" if j == k - 1 else "inside its piece"))
        out = self.content[self.cum[first]:self.cum[upto]] if upto > first else b""
        self.delivered += len(out)
        if end == DONE and status == OK and "endmark" in ev and self.flags & FL_CSUM and self.stop is None:
            if o.xxh32(self.content[:self.cum[upto]] if self.cum[upto] else b"") != struct.unpack_from("<I", f, r - 4)[0]:
                status = FRAME_CHECKSUM_FAIL; ev.add("content checksum fails")
        if out and end != DONE and not self.flags & FL_INDEP:
            total = self.window + len(out)
            ev.add("window " + ("shorter than" if total < WINDOW else "equal to" if total == WINDOW else "longer than") + " 64 KiB")
            if self.window == WINDOW and len(out) < WINDOW:
                ev.add("short piece behind a full window")
            self.window = min(total, WINDOW)
        self.block, self.in_off, self.phase, self.status = upto if end != DONE else k, r, end, status
        ev.add(("more", "need input", "done")[end])
        return out, status, r, end, ev


def bounds(case):
    _, _, blocks, _ = walk(case["frame"])
    return [min(255 * n + 16, BS) if c else n for _, n, c, _ in blocks]


CAP_SCHEDULES = ("one bound", "two bounds", "one bound + 1", "three bounds - 1", "everything")


def capacity(case, schedule):
    b = bounds(case)
    m = max(b + [1])
    return {"one bound": m, "two bounds": 2 * m, "one bound + 1": m + 1, "three bounds - 1": 3 * m - 1, "three bounds": 3 * m, "everything": max(sum(b), 1)}[schedule]


def run_model(case, cap, in_lens=None, limit=64):
    """The calls of one schedule: capacity `cap` per call, in_len from in_lens (then the full length) — until DONE, or until the
    full input rests in NEED_INPUT.  Returns [(out, status, consumed, phase, events)]."""
    m, calls = Model(case), []
    lens = list(in_lens or []) + [len(case["frame"])]
    for i in range(limit):
        n = lens[min(i, len(lens) - 1)]
        calls.append(m.call(n, cap))
        if calls[-1][3] == DONE or (calls[-1][3] == NEED_INPUT and n == len(case["frame"]) and i >= len(lens) - 1):
            break
        assert not (calls[-1][3] == MORE and calls[-1][1] == OUT_CAPACITY), "the schedule's capacity is below a block bound"
    else:
        raise AssertionError("the model did not end")
    return calls


# ---- the XXH32 state path: the splits the GPU test runs, pinned on the host by the CPU test ------------------------------------

def xxh_splits():
    """[(buffer, a, b)]: the buffer is hashed as [0, a), [a, b), [b, end).  Buffers of 0..100 bytes at every pair of split points —
    every fill 0..15 on both sides of a stripe boundary — and one of 70 000 bytes in three uneven pieces."""
    data = content(70000, at=3)
    rows = [(data[:n], a, b) for n in range(101) for a in range(n + 1) for b in range(a, n + 1)]
    rows.append((data, 1, 40007))
    return rows
