"""Frames for the tests of the block index and the block-run decode (include/lzfear_frame.h: lzf_frame_block_index_device,
lzf_block_index_locate, lzf_frame_decompress_blocks_device), and what those calls must say about them — TEST INFRASTRUCTURE.

Frames are put together here, block by block: the header of src/framed/header.rs, per block the length word, the payload and
the optional checksum word, the EndMark and the optional content checksum.  Every rule under test depends on the number of
blocks, not on their size, so the blocks are small pieces under a block_maxsize of 64 KiB: a piece's payload is block 0 of the
oracle's frame of that piece alone (with the dictionary, where there is one), stored where the oracle stores it.  The stops are
payloads written by hand.

Expected values come from the oracle decoding the frame block by block behind a host walk (ref_index), never from the library
under test; tests/test_block_index_cpu.py holds ref_index's frame results to the oracle's decompress_frame."""
import struct

import numpy as np
import xxhash

import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import synth

STORED, HAS_SUM, LINKED, DELIVERED, BEHIND_STOP = 1, 2, 4, 8, 16
BMAX = 64 << 10
FIELDS = ("in_off", "out_off", "out_len", "in_len", "want_sum", "block_maxsize", "status", "flags", "reserved")
COUNTS = (0, 1, 2, 63, 64, 65, 130)

# ---- payloads that stop the reader (src/raw/decompress.rs:58-138 under block_maxsize = 64 KiB, no dictionary) ------------------
ERR1 = b"\x50ab"                                                    # five literals announced, two there: UnexpectedEnd
ERR2 = b"\x1fa\x01\x00" + b"\xff" * 257 + b"\x00"                   # one literal, a match of 65 554: MemoryLimitExceeded
ERR3 = b"\x10a\x00\x00"                                             # a match at offset 0: ZeroDeduplicationOffset
ERR4 = b"\x10a\x09\x00"                                             # a match 9 back with one byte of output: InvalidDeduplicationOffset
PAST = b"\x1fa\x01\x00" + b"\xff" * 256 + bytes([236]) + b"\xa0" + b"0123456789"   # 1 + 65 535 = the limit, then ten literals: n > block_maxsize
EMPTY = b"\x00"                                                     # one token, nothing: the Read adapter stops here with LZF_OK
STOP_PAYLOADS = {"codec 1": ERR1, "codec 2": ERR2, "codec 3": ERR3, "codec 4": ERR4, "past block_maxsize": PAST, "empty block": EMPTY}


def header(block_checksums=False, content_checksum=False, independent=True, dictionary_id=None):
    flg = 0x40 | (0x20 if independent else 0) | (0x10 if block_checksums else 0) | (0x04 if content_checksum else 0) | (0x01 if dictionary_id is not None else 0)
    desc = bytes([flg, 0x40]) + (struct.pack("<I", dictionary_id) if dictionary_id is not None else b"")
    return struct.pack("<I", 0x184D2204) + desc + bytes([(xxhash.xxh32(desc).intdigest() >> 8) & 0xFF])


def piece_block(data, dictionary=None):
    """(payload, stored) of `data` as one independent block: block 0 of the oracle's frame of it."""
    rc, f = o.frame_compress(data, o.make_settings(block_size=BMAX, content_checksum=False, dictionary=dictionary,
                                                   dictionary_id=7 if dictionary else None))
    assert rc == 0 and 0 < len(data) <= BMAX
    at = 7 + (4 if dictionary else 0)
    word = struct.unpack_from("<I", f, at)[0]
    n = word & 0x7FFFFFFF
    assert len(f) == at + 4 + n + 4
    return f[at + 4:at + 4 + n], bool(word >> 31)


def assemble(blocks, plain=b"", **kw):
    """The frame of `blocks` [(payload, stored)]; `plain` feeds the content checksum."""
    out = [header(**kw)]
    for payload, stored in blocks:
        out.append(struct.pack("<I", len(payload) | (0x80000000 if stored else 0)) + payload)
        if kw.get("block_checksums"):
            out.append(struct.pack("<I", xxhash.xxh32(payload).intdigest()))
    out.append(b"\x00" * 4)
    if kw.get("content_checksum"):
        out.append(struct.pack("<I", xxhash.xxh32(plain).intdigest()))
    return b"".join(out)


_MIX = None


def pieces(n, seed=0):
    """n pieces of 150 .. 2 400 bytes; every seventh one, and the first, random bytes (stored raw)."""
    global _MIX
    if _MIX is None:
        _MIX = synth.silesia_mix(50 << 20, (50 << 20) + 600_000).tobytes()
    rng = np.random.default_rng(1000 + seed)
    out = []
    for k in range(n):
        size = int(rng.integers(150, 2400))
        if k % 7 == 0:
            out.append(rng.integers(0, 256, size, dtype=np.uint8).tobytes())
        else:
            at = int(rng.integers(0, len(_MIX) - size))
            out.append(_MIX[at:at + size])
    return out


_BLOCKS = {}


def good_blocks(n, seed=0, dictionary=None):
    """([(payload, stored)], [plain]) of pieces(n, seed), cached."""
    key = (n, seed, dictionary)
    if key not in _BLOCKS:
        data = pieces(n, seed)
        _BLOCKS[key] = ([piece_block(d, dictionary) for d in data], data)
    return _BLOCKS[key]


def good_frame(n, seed=0, dictionary=None, **kw):
    blocks, data = good_blocks(n, seed, dictionary)
    return assemble(blocks, b"".join(data), dictionary_id=7 if dictionary else None, **kw)


def linked_frame(n_bytes=200_000, dictionary=None, **kw):
    """A linked-block frame of the oracle's: 64 KiB blocks, every block behind the ones before it."""
    global _MIX
    pieces(1)
    rc, f = o.frame_compress(_MIX[:n_bytes], o.make_settings(block_size=BMAX, independent_blocks=False, dictionary=dictionary,
                                                             dictionary_id=7 if dictionary else None, **kw))
    assert rc == 0
    return f


def dictionary_bytes():
    return synth.gen_text_zipf(3, 70000).tobytes()


# ---- the host walk and the expected index -----------------------------------------------------------------------------------

def walk(frame):
    """Header and block walk (decompress.rs:102-235) restated: dict(status, consumed, flg, header_len, blocks) with blocks
    [(in_off, in_len, stored, want_sum, end_off)]; status != 0 with no blocks for a header that fails."""
    d, n = frame, len(frame)
    fail = lambda st, used: dict(status=st, consumed=used, flg=0, header_len=0, blocks=[], header_ok=False)
    if n < 4:
        return fail(16, n)
    if struct.unpack_from("<I", d, 0)[0] != 0x184D2204:
        return fail(17, 4)
    if n < 6:
        return fail(16, n)
    flg = d[4]
    hl = 6 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    if n < hl + 1:
        return fail(16, n)
    assert flg >> 6 == 1 and not flg & 2 and d[5] == 0x40 and d[hl] == (xxhash.xxh32(d[4:hl]).intdigest() >> 8) & 0xFF, "test frames have sound headers"
    r, blocks = hl + 1, []
    while True:
        if n - r < 4:
            return dict(status=16, consumed=n, flg=flg, header_len=hl + 1, blocks=blocks, header_ok=True)
        bl = struct.unpack_from("<I", d, r)[0]; r += 4
        if bl == 0:
            if flg & 4:
                if n - r < 4:
                    return dict(status=16, consumed=n, flg=flg, header_len=hl + 1, blocks=blocks, header_ok=True)
                r += 4
            return dict(status=0, consumed=r, flg=flg, header_len=hl + 1, blocks=blocks, header_ok=True)
        stored, bl = bool(bl >> 31), bl & 0x7FFFFFFF
        if bl > BMAX:
            return dict(status=22, consumed=r, flg=flg, header_len=hl + 1, blocks=blocks, header_ok=True)
        if n - r < bl:
            return dict(status=16, consumed=n, flg=flg, header_len=hl + 1, blocks=blocks, header_ok=True)
        off = r; r += bl
        want = 0
        if flg & 0x10:
            if n - r < 4:
                return dict(status=16, consumed=n, flg=flg, header_len=hl + 1, blocks=blocks, header_ok=True)
            want = struct.unpack_from("<I", d, r)[0]; r += 4
        blocks.append((off, bl, stored, want, r))


def ref_index(frame, dictionary=b""):
    """(entries [dict of FIELDS + plain], (status, out_len, consumed)) by the rules of lzfear_frame.h, every block decoded by the
    oracle's decompress_raw.  `plain` is the block's output (None where it has none to deliver)."""
    w = walk(frame)
    linked, bsum = not w["flg"] & 0x20, bool(w["flg"] & 0x10)
    entries, run, stop, history = [], 0, None, b""
    for k, (off, ln, stored, want, end) in enumerate(w["blocks"]):
        payload = frame[off:off + ln]
        code, n, plain = 0, 0, None
        if bsum and xxhash.xxh32(payload).intdigest() != want:
            code = 19
        elif stored:
            n, plain = ln, payload
        else:
            rc, out = o.decompress_raw(payload, prefix=dictionary, existing=history if linked else b"", limit=len(history if linked else b"") + BMAX)
            if rc:
                code = rc
            else:
                plain = out[len(history):] if linked else out
                n = len(plain)
        if not code and n > BMAX:
            code = 22
        stops = stop is None and (code != 0 or n == 0)
        flags = (STORED if stored else 0) | (HAS_SUM if bsum else 0) | (LINKED if linked else 0)
        if stop is None and not stops:
            flags |= DELIVERED
        if stop is not None:
            flags |= BEHIND_STOP
        entries.append(dict(in_off=off, out_off=run, out_len=n, in_len=ln, want_sum=want if bsum else 0, block_maxsize=BMAX, status=code,
                            flags=flags, reserved=0, plain=plain, end_off=end))
        if stops:
            stop = k
        if stop is None:
            run += n
            if linked:
                history += plain
    if stop is None:
        return entries, (w["status"], run, w["consumed"])
    return entries, (entries[stop]["status"], run, entries[stop]["end_off"])


def comparable(e):
    """The fields of an expected entry that the header specifies: out_len is unspecified where the block's status is a codec
    error or a failed checksum, and behind a stop in a linked-block frame."""
    skip_len = e["status"] in (1, 2, 3, 4, 19) or (e["flags"] & LINKED and e["flags"] & BEHIND_STOP)
    return [f for f in FIELDS if not (f == "out_len" and skip_len) and not (f == "status" and e["flags"] & LINKED and e["flags"] & BEHIND_STOP)]


# ---- the frames with stops ---------------------------------------------------------------------------------------------------

def stop_frame(kind, at, n=130, seed=0):
    """A frame of n blocks, block `at` replaced so that it stops the reader in the way `kind`; block checksums on for
    'block checksum' (one payload byte flipped under a sound word)."""
    blocks, data = good_blocks(n, seed)
    blocks = list(blocks)
    if kind == "block checksum":
        f = bytearray(assemble(blocks, block_checksums=True))
        off, ln = walk(bytes(f))["blocks"][at][:2]
        f[off + ln // 2] ^= 0x10
        return bytes(f)
    if kind == "truncated":
        f = assemble(blocks)
        off, ln = walk(f)["blocks"][at][:2]
        return f[:off + ln // 2]
    blocks[at] = (STOP_PAYLOADS[kind], False)
    return assemble(blocks)


STOP_KINDS = ("block checksum",) + tuple(STOP_PAYLOADS) + ("truncated",)
STOP_PLACES = (0, 63, 64, 129)


def census():
    """What the built frames reach: every flag, every stop kind (by the status or rule it shows as), blocks on both sides of the
    64-block round."""
    flags, stops, counts = 0, set(), set()
    frames = [(good_frame(n, block_checksums=bool(n % 2)), b"") for n in COUNTS]
    frames += [(stop_frame(kind, at), b"") for kind in STOP_KINDS for at in STOP_PLACES]
    frames.append((linked_frame(), b""))
    for f, dct in frames:
        entries, (st, _, _) = ref_index(f, dct)
        counts.add(len(entries))
        for e in entries:
            flags |= e["flags"]
        first = next((e for e in entries if not e["flags"] & DELIVERED), None)
        if first is not None:
            stops.add("empty" if first["status"] == 0 else first["status"])
        elif st:
            stops.add("walk %d" % st)
    return flags, stops, counts
