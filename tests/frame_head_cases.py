"""Cases of the frame head tests (test_frame_head_cases_cpu.py, test_gpu_frame_head.py): frames put together with
block_index_cases.py's builders, each with a dictionary and a TARGET, and what lzf_frame_head_device must say about them — TEST
INFRASTRUCTURE.

Every expectation comes from model(): block_index_cases.walk (the reader's walk restated in Python) and, per block entered in front
of the target, the ORACLE's decompress_raw with head_cases.ref_walk naming the failing sequence of a block that does not decode —
never from the code under test.  Frames whose header fails state their status by hand (the CPU test holds it to the oracle's).
An expectation is (status, out_len, bytes or None, room): `bytes` the first out_len bytes where the status is LZF_OK, None where
the bytes below the target are unspecified; `room` the bytes of output memory the call may write (never more than the target)."""
import struct

import xxhash

import block_index_cases as B
import head_cases as H
import oracle_ffi as o
from head_cases import seq
from verify_cases import _rand

BMAX = B.BMAX
CONTRACT, MAX_LEN = 6, 0x7FFFFF00
FAR = MAX_LEN - 1           # the largest target the call takes: far past every frame's end
INPUT_ERROR, WRONG_MAGIC, HEADER_CHECKSUM_FAIL, BLOCK_CHECKSUM_FAIL, BLOCK_SIZE_OVERFLOW = 16, 17, 18, 19, 22
UNIMPLEMENTED_BLOCKSIZE, UNSUPPORTED_VERSION, RESERVED_FLAG_BITS, RESERVED_BD_BITS = 23, 24, 25, 26
END = seq(b"tail!", None, 0)

_raw = {}


def _decode(payload, prefix, existing, limit):
    key = (payload, prefix, existing, limit)
    if key not in _raw:
        _raw[key] = o.decompress_raw(payload, prefix=prefix, existing=existing, limit=limit, cap=len(existing) + limit + len(payload) + 64)
        assert _raw[key][0] != o.OUT_CAPACITY
    return _raw[key]


def model(frame, dictionary, target):
    """(status, out_len, bytes or None, room) of a frame whose header is sound (or cut, or of the wrong magic)."""
    if target >= MAX_LEN:
        return CONTRACT, 0, None, 0
    w = B.walk(frame)
    if not w["header_ok"]:
        return w["status"], 0, None, 0
    linked = not w["flg"] & 0x20
    out, pos = b"", 0
    for off, ln, stored, _want, _end in w["blocks"]:
        if pos >= target:
            return 0, target, out[:target], target
        payload = frame[off:off + ln]
        if stored:
            n = ln
            out += payload
        else:
            existing = out if linked else b""
            limit = len(existing) + BMAX
            rc, dec = _decode(payload, dictionary, existing, limit)
            st, p, tp, _ = H.ref_walk(payload, len(dictionary), len(existing), limit)
            assert st == rc and (rc != 0 or p == len(dec)), "ref_walk does not reproduce the oracle"
            if rc != 0:
                fp = p if linked else pos + p                  # where the failing sequence starts in the frame's output
                if target > fp:
                    return rc, pos, None, fp
                rc2, dec2 = _decode(payload[:tp], dictionary, existing, limit)
                assert rc2 == 0 and len(dec2) == p
                return 0, target, (out + dec2[len(existing):])[:target], target
            n = len(dec) - len(existing)
            out += dec[len(existing):]
        if pos + n >= target:                                  # the block reaches the target: nothing more is asked of it
            return 0, target, out[:target], target
        if n > BMAX:
            return BLOCK_SIZE_OVERFLOW, pos, None, pos + n
        if n == 0:
            return 0, pos, out[:pos], pos
        pos += n
    if pos >= target:
        return 0, target, out[:target], target
    return w["status"], pos, (out[:pos] if w["status"] == 0 else None), pos      # the EndMark, or the walk's error


# ---- builders on top of block_index_cases ---------------------------------------------------------------------------------------

def header(content_size=None, bd=0x40, flg_xor=0, hc_xor=0, **kw):
    """block_index_cases.header with a content size, and with the damage the header cases need."""
    plain = B.header(**kw)
    flg = plain[4] | (0x08 if content_size is not None else 0)
    desc = bytes([flg ^ flg_xor, bd]) + (struct.pack("<Q", content_size) if content_size is not None else b"") + plain[6:-1]
    return plain[:4] + desc + bytes([((xxhash.xxh32(desc).intdigest() >> 8) & 0xFF) ^ hc_xor])


def with_header(frame, old_kw, **new_kw):
    return header(**new_kw) + frame[len(B.header(**old_kw)):]


def case(name, cls, frame, target, dictionary=b"", expect=None, sub=""):
    return dict(name=f"{cls}/{name}, target {target}", cls=cls, sub=sub, frame=bytes(frame), dict=bytes(dictionary), target=target, expect=expect)


def block_starts(frame, dictionary):
    """Output position of every block's first byte, and the frame's length, by the oracle's whole decode."""
    w = B.walk(frame)
    linked = not w["flg"] & 0x20
    pos, starts, out = 0, [], b""
    for off, ln, stored, _w, _e in w["blocks"]:
        starts.append(pos)
        if stored:
            out += frame[off:off + ln]; pos += ln
        else:
            ex = out if linked else b""
            rc, dec = _decode(frame[off:off + ln], dictionary, ex, len(ex) + BMAX)
            if rc:
                break
            out += dec[len(ex):]; pos = pos + len(dec) - len(ex)
    return starts, pos


def clean_targets(frame, dictionary):
    starts, total = block_starts(frame, dictionary)
    ts = {0, 1, 64, total - 1, total, total + 1, FAR}
    for b in starts[1:4]:                                      # the ends of the first three blocks
        ts |= {b - 1, b, b + 1}
    if len(starts) > 2:
        ts.add((starts[2] + (starts[3] if len(starts) > 3 else total)) // 2)      # inside block 2
    return sorted(t for t in ts if t >= 0)


DICT = None


def dictionary_bytes():
    global DICT
    if DICT is None:
        DICT = B.dictionary_bytes()
    return DICT


def clean_frames():
    """[(name, frame, dictionary)]: independent and linked, with and without a dictionary, every header length."""
    d = dictionary_bytes()
    out = []
    for tag, dic in (("no dictionary", b""), ("a dictionary", d)):
        dkw = dict(dictionary_id=7) if dic else {}
        blocks, data = B.good_blocks(4, 0, dic or None)
        plain = b"".join(data)
        for indep in (True, False):
            kind = "independent" if indep else "linked"
            out.append((f"{kind}, {tag}", B.assemble(blocks, plain, independent=indep, **dkw), dic))
            out.append((f"{kind}, {tag}, block checksums", B.assemble(blocks, plain, independent=indep, block_checksums=True, **dkw), dic))
            out.append((f"{kind}, {tag}, content checksum", B.assemble(blocks, plain, independent=indep, content_checksum=True, **dkw), dic))
            f = B.assemble(blocks, plain, independent=indep, block_checksums=True, content_checksum=True, **dkw)
            out.append((f"{kind}, {tag}, both checksums and a content size",
                        with_header(f, dict(independent=indep, block_checksums=True, content_checksum=True, **dkw),
                                    content_size=len(plain), independent=indep, block_checksums=True, content_checksum=True, **dkw), dic))
    assert {len(B.walk(f)["blocks"]) for _, f, _ in out} == {4}
    assert {B.walk(f)["header_len"] for _, f, _ in out} == {7, 11, 15, 19}
    return out


def clean_cases():
    out = []
    for name, f, dic in clean_frames():
        out += [case(name, "clean", f, t, dic, sub="linked" if "linked" in name else "independent") for t in clean_targets(f, dic)]
    big = B.linked_frame()                                     # 200 000 bytes, 64 KiB blocks, every block behind the ones before it
    starts, total = block_starts(big, b"")
    assert total == 200_000 and starts == [0, 65536, 131072, 196608]
    out += [case("the oracle's linked frame of 200 000 bytes", "clean", big, t, sub="linked oracle")
            for t in (64, 65535, 65536, 65537, 65536 + 300, 131072 + 1, 199_999, 200_000, 200_001, FAR)]
    big_d = B.linked_frame(dictionary=dictionary_bytes())
    out += [case("the oracle's linked frame of 200 000 bytes behind a dictionary", "clean", big_d, t, dictionary_bytes(), sub="linked oracle")
            for t in (64, 4096, 65537, FAR)]
    return out


def stored_cases():
    """Stored first, stored then compressed, compressed then stored: the target inside the stored block and on its end."""
    blocks, _ = B.good_blocks(4, 0)
    assert blocks[0][1] and not blocks[1][1] and not blocks[2][1]
    out = []
    for name, bl in (("stored first", [blocks[0]]), ("stored then compressed", [blocks[0], blocks[1]]),
                     ("compressed then stored", [blocks[1], blocks[0], blocks[2]]), ("two stored blocks", [blocks[0], blocks[0]])):
        for indep in (True, False):
            f = B.assemble(bl, independent=indep)
            starts, total = block_starts(f, b"")
            k = [s for _, s in bl].index(True)
            a, e = starts[k], (starts[k + 1] if k + 1 < len(starts) else total)
            out += [case(f"{name}, {'independent' if indep else 'linked'}", "stored", f, t, sub=name)
                    for t in sorted({a + 1, a + 15, a + 16, a + 17, (a + e) // 2, e - 1, e, e + 1, total, FAR})]
    out += [case("an empty stored block behind a block", "stored", B.assemble([blocks[1], (b"", True), blocks[2]]), t, sub="empty stored")
            for t in (10, FAR)]
    return out


def history_cases():
    """Hand-built payloads: a linked frame whose block 1 opens with a match into block 0's output; a block 0 that opens with a match
    into the dictionary, linked and independent, with the dictionary and without it."""
    out = []
    b0 = seq(_rand(51, 100), None, 0)
    b1 = seq(b"", 30, 20) + seq(b"xy", 110, 40) + END              # 20 bytes from block 0's tail, 40 from its front
    f = B.assemble([(b0, False), (b1, False)], independent=False)
    out += [case("block 1 opens with a match into block 0", "history", f, t, sub="into block 0") for t in (99, 100, 101, 110, 120, 121, 130, 167, 168, FAR)]
    d = dictionary_bytes()
    p0 = seq(b"", 50, 30) + seq(b"ab", 32 + 400, 70) + END        # 30 bytes from the dictionary's tail, 70 from further back
    for indep in (False, True):
        kind = "independent" if indep else "linked"
        f = B.assemble([(p0, False), (b1, False)] if not indep else [(p0, False)], independent=indep, dictionary_id=7)
        out += [case(f"block 0 opens with a match into the dictionary, {kind}", "history", f, t, d, sub=f"into the dictionary, {kind}")
                for t in (1, 29, 30, 31, 64, 102, 107, 108, FAR)]
        out += [case(f"the same payload without the dictionary, {kind}", "history", f, t, b"", sub=f"no dictionary, {kind}") for t in (0, 1, 64, FAR)]
    return out


HEADER_ERRORS = None


def header_error_frames():
    """[(name, frame, status)]: every way lzf_frame_scan.h's read_header fails."""
    good = B.good_frame(2)
    long_h = header(content_size=5, dictionary_id=7) + good[7:]
    out = [("an empty input", b"", INPUT_ERROR), ("three bytes", good[:3], INPUT_ERROR), ("the magic alone", good[:4], INPUT_ERROR),
           ("cut behind FLG", good[:5], INPUT_ERROR), ("cut in front of HC", good[:6], INPUT_ERROR),
           ("cut inside the content size", long_h[:10], INPUT_ERROR), ("cut inside the dictionary id", long_h[:16], INPUT_ERROR),
           ("cut in front of HC behind both", long_h[:18], INPUT_ERROR),
           ("the wrong magic", b"\x05" + good[1:], WRONG_MAGIC),
           ("version 0", header(flg_xor=0x40) + good[7:], UNSUPPORTED_VERSION), ("version 3", header(flg_xor=0x80) + good[7:], UNSUPPORTED_VERSION),
           ("the reserved FLG bit", header(flg_xor=0x02) + good[7:], RESERVED_FLAG_BITS),
           ("a reserved BD bit", header(bd=0x41) + good[7:], RESERVED_BD_BITS), ("the top BD bit", header(bd=0xC0) + good[7:], RESERVED_BD_BITS),
           ("a wrong HC", header(hc_xor=0x01) + good[7:], HEADER_CHECKSUM_FAIL),
           ("block size 3", header(bd=0x30) + good[7:], UNIMPLEMENTED_BLOCKSIZE), ("block size 0", header(bd=0x00) + good[7:], UNIMPLEMENTED_BLOCKSIZE)]
    return out


def header_cases():
    out = []
    for name, f, st in header_error_frames():
        out += [case(name, "header", f, t, expect=(st, 0, None, 0), sub=str(st)) for t in (0, 64)]
    return out


def cut_frame():
    """The three-block frame of the cut cases: block checksums and a content checksum, the shortest of twenty seeds."""
    best = None
    for seed in range(20):
        blocks, data = B.good_blocks(3, seed)
        f = B.assemble(blocks, b"".join(data), block_checksums=True, content_checksum=True)
        if best is None or len(f) < len(best):
            best = f
    return best


def cut_cases():
    f = cut_frame()
    return [case(f"a three-block frame cut to {n} bytes", "cut", f[:n], t, sub="cut") for n in range(len(f)) for t in (64, FAR)]


def stop_cases():
    """Every STOP_PAYLOADS kind at block 0, 1 and 2: the target in front of the block (not seen), inside it, behind it."""
    out = []
    for kind in B.STOP_PAYLOADS:
        for at in (0, 1, 2):
            f = B.stop_frame(kind, at, n=4)
            start = block_starts(f, b"")[0][at]
            span = 65546 if kind == "past block_maxsize" else 0
            ts = sorted({start, start + 1, start + 2, start + 70_000, FAR} | ({start + span - 1, start + span, start + span + 1} if span else set()))
            out += [case(f"{kind} at block {at}", "stop", f, t, sub=kind) for t in ts if t >= 0]
    return out


def length_word_cases():
    blocks, _ = B.good_blocks(4, 0)
    tail = struct.pack("<I", BMAX + 1) + b"\x00" * 64
    stored_tail = struct.pack("<I", (BMAX + 1) | 0x80000000) + b"\x00" * 64
    f0 = B.header() + tail
    f1 = B.assemble(blocks[:2])[:-4] + stored_tail
    starts, total = block_starts(B.assemble(blocks[:2]), b"")
    out = [case("a length word above block_maxsize at block 0", "length word", f0, t, sub="at 0") for t in (0, 1, FAR)]
    out += [case("a stored length word above block_maxsize at block 2", "length word", f1, t, sub="at 2") for t in (total - 1, total, total + 1, FAR)]
    return out


def endmark_cases():
    blocks, data = B.good_blocks(3, 1)
    f = B.assemble(blocks, b"".join(data), content_checksum=True)
    total = len(b"".join(data))
    out = []
    for drop in (1, 3, 4):
        out += [case(f"the EndMark's content checksum word short of {drop} bytes", "endmark", f[:-drop], t, sub="word cut") for t in (total - 1, total, total + 1, FAR)]
    bad = f[:-1] + bytes([f[-1] ^ 0x55])
    out += [case("a content checksum that is not the content's", "endmark", bad, t, sub="wrong word") for t in (total, FAR)]
    return out


def contract_cases():
    good = B.good_frame(2)
    return [case("a sound frame", "contract", good, t, expect=(CONTRACT, 0, None, 0), sub="sound") for t in (MAX_LEN, MAX_LEN + 1, 1 << 40, (1 << 64) - 1)] + \
           [case("a frame of the wrong magic", "contract", b"\x05" + good[1:], MAX_LEN, expect=(CONTRACT, 0, None, 0), sub="bad header"),
            case("the largest target", "contract", good, MAX_LEN - 1, sub="largest")]


def flipped_frame():
    """Block checksums on, and a literal byte of block 0 (a compressed block) flipped under its sound word."""
    blocks, _ = B.good_blocks(4, 0)
    f = bytearray(B.assemble([blocks[1], blocks[2]], block_checksums=True))
    off, ln = B.walk(bytes(f))["blocks"][0][:2]
    tp, _pos, L, _M, _off = next(s for s in H.ref_walk(bytes(f[off:off + ln]), 0, 0, BMAX)[3] if s[2] > 0)
    lit_at = tp + 1 + ((L - 15) // 255 + 1 if L >= 15 else 0)
    f[off + lit_at] ^= 0x20
    return bytes(f), lit_at


def checksum_cases():
    f, _ = flipped_frame()
    return [case("a flipped literal byte under a sound block checksum", "checksum", f, t, sub="flipped") for t in (64, FAR)]


_ALL = None


def all_cases():
    """[(case, (status, out_len, bytes or None, room))]"""
    global _ALL
    if _ALL is None:
        cs = (clean_cases() + stored_cases() + history_cases() + header_cases() + cut_cases() + stop_cases() + length_word_cases()
              + endmark_cases() + contract_cases() + checksum_cases())
        assert len({c["name"] for c in cs}) == len(cs)
        _ALL = [(c, c["expect"] if c["expect"] is not None else model(c["frame"], c["dict"], c["target"])) for c in cs]
    return _ALL


CLASSES = ("clean", "stored", "history", "header", "cut", "stop", "length word", "endmark", "contract", "checksum")


def assert_covers(rows):
    """The census: every class is there with the kinds and the verdicts it is about, and the targets meet all three sides of a block
    boundary.  What keeps the suite from quietly losing a class."""
    by = lambda k: [(c, e) for c, e in rows if c["cls"] == k]      # noqa: E731
    for k in CLASSES:
        assert by(k), k
    clean = by("clean")
    assert all(e[0] == 0 and e[1] == min(c["target"], e[1]) for c, e in clean)
    assert {c["sub"] for c, _ in clean} == {"independent", "linked", "linked oracle"}
    assert {bool(c["dict"]) for c, _ in clean} == {False, True}
    assert {B.walk(c["frame"])["header_len"] for c, _ in clean} == {7, 11, 15, 19}
    assert {B.walk(c["frame"])["flg"] & 0x14 for c, _ in clean} == {0x00, 0x04, 0x10, 0x14}
    for name, f, dic in clean_frames():                            # all three sides of the first three block boundaries, 0, 1, 64, the end, FAR
        ts = {c["target"] for c, _ in clean if c["frame"] == f and c["dict"] == dic}
        starts, total = block_starts(f, dic)
        for b in starts[1:4]:
            assert {b - 1, b, b + 1} <= ts, name
        assert {0, 1, 64, total - 1, total, total + 1, FAR} <= ts and any(starts[2] + 1 < t < starts[3] - 1 for t in ts), name
    assert {c["sub"] for c, _ in by("stored")} == {"stored first", "stored then compressed", "compressed then stored", "two stored blocks", "empty stored"}
    hist = by("history")
    assert {c["sub"] for c, _ in hist} == {"into block 0"} | {f"{a}, {b}" for a in ("into the dictionary", "no dictionary") for b in ("linked", "independent")}
    assert all(e[0] == 0 for c, e in hist if not c["sub"].startswith("no dictionary"))
    assert {e[0] for c, e in hist if c["sub"].startswith("no dictionary") and c["target"] > 0} == {4}
    assert {e[0] for _, e in by("header")} == {INPUT_ERROR, WRONG_MAGIC, HEADER_CHECKSUM_FAIL, UNIMPLEMENTED_BLOCKSIZE, UNSUPPORTED_VERSION,
                                                RESERVED_FLAG_BITS, RESERVED_BD_BITS}
    assert {c["target"] for c, _ in by("header")} == {0, 64} and all(e[1] == 0 for _, e in by("header"))
    cut = by("cut")
    assert len(cut) == 2 * len(cut_frame()) and {e[0] for _, e in cut} == {0, INPUT_ERROR} and {c["target"] for c, _ in cut} == {64, FAR}
    stops = by("stop")
    assert {c["sub"] for c, _ in stops} == set(B.STOP_PAYLOADS)
    for kind, want in (("codec 1", 1), ("codec 2", 2), ("codec 3", 3), ("codec 4", 4), ("past block_maxsize", BLOCK_SIZE_OVERFLOW)):
        got = {e[0] for c, e in stops if c["sub"] == kind}
        assert got == {0, want}, (kind, got)                       # not seen in front of the block, seen behind it
    assert {e[0] for c, e in stops if c["sub"] == "empty block"} == {0}
    assert any(c["sub"] == "empty block" and e[1] < c["target"] for c, e in stops)
    assert {e[0] for _, e in by("length word")} == {0, BLOCK_SIZE_OVERFLOW}
    assert {e[0] for _, e in by("endmark")} == {0, INPUT_ERROR}
    assert {e[0] for _, e in by("contract")} == {0, CONTRACT}
    assert all(e[0] == 0 for _, e in by("checksum"))
