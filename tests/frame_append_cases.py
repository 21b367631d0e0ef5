"""Cases, schedules and a pure-Python model of lzf_frame_append_device (include/lzfear_frame.h, "streaming frame writer in device
memory") — TEST INFRASTRUCTURE, no GPU.

The model restates the rule of one call the way the reference's compress_internal runs (src/framed/compress.rs:221-276): it
keeps the in_buffer window as bytes and the stream's table as the oracle's U32Table, compresses every taken block with the
oracle's compress2 behind that window and applies table.offset(forget) right behind the block.  What is taken is found by a plain
loop over the offer's blocks.  tests/test_frame_append_cases_cpu.py holds the model to the oracle's frame_compress of the whole
input on every case and schedule, holds the shared rules header (rust-lz-fear_amd/csrc/lzf_frame_append_rules.h, compiled with
g++) to the model call by call, and counts that every rule is reached; tests/test_gpu_frame_append.py holds the device to the
model and to lzf_frame_compress_device_many.

Every case uses block_size 64 KiB, the smallest legal size: a case is a few hundred KiB at most."""
import ctypes as C
import functools
import struct

import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import synth

BS = 65536
WINDOW = 65536
MORE, NEED_INPUT, DONE = 0, 1, 2            # LZF_APPEND_*
FINISH = 1                                  # LZF_APPEND_FINISH
OK, OUT_CAPACITY, INVALID_BLOCK_SIZE, PANIC = 0, 7, 27, 28
LENGTHS = (0, 1, 65535, 65536, 65537, 3 * 65536, 3 * 65536 + 5)


def bound(t, bs=BS):
    """lzf_frame_compress_bound(s, t): header, EndMark and checksum words always counted."""
    return 19 + t + (t // bs + 1) * 8 + 8


def content(n, at=0):
    return synth.silesia_mix(at << 20, (at << 20) + n).tobytes()


@functools.lru_cache(maxsize=None)
def dictionaries():
    text = synth.text_zipf_64k().tobytes()
    big = (text + content(8192, at=5))[:70000]
    assert len(big) == 70000
    return {"none": b"", "7": text[:7], "100": text[100:200], "70000": big}


@functools.lru_cache(maxsize=None)
def all_cases():
    """[dict(name, data, dict, indep, bsum, csum, csize, tags)].  Every (linked?, dictionary) pair at every length, its checksum
    flavour going round with the pair; the full flavour product at the longest length behind the 100-byte dictionary; a frame
    with an incompressible block; the window-carry input."""
    cases = []

    def add(name, data, dic, indep, bsum, csum, csize, **tags):
        cases.append(dict(name=name, data=data, dict=dic, indep=indep, bsum=bsum, csum=csum, csize=csize, tags=tags))

    flavours = [(False, True, False), (True, False, False), (True, True, True), (False, False, True)]
    data = content(LENGTHS[-1])
    pair = 0
    for indep in (True, False):
        for dname, dic in dictionaries().items():
            bsum, csum, csize = flavours[pair % 4]
            pair += 1
            for n in LENGTHS:
                add(f"{'indep' if indep else 'linked'} dict {dname} len {n}", data[:n], dic, indep, bsum, csum, csize, pair=True)
    for combo in range(16):
        indep, bsum, csum, csize = bool(combo & 1), bool(combo & 2), bool(combo & 4), bool(combo & 8)
        add(f"flavour {combo:04b}", data, dictionaries()["100"], indep, bsum, csum, csize, flavour=True)
    noise = synth.gen_random(11, 3 * BS).tobytes()
    for indep in (True, False):
        add(("indep" if indep else "linked") + " stored block in the middle", data[:BS] + noise[:BS] + data[BS:2 * BS + 77], b"", indep, True, True, False, stored=True)
    # window carry: block 0 repeats the dictionary's last 60 000 bytes, block k + 1 the last 60 000 of block k, 60 000 bytes back
    # (a match reaches 65 535 bytes back at most); everything else is noise, so a block compresses only through its history
    dic = synth.gen_random(12, 70000).tobytes()
    blocks, prev = [], dic
    for k in range(3):
        blocks.append(prev[-60000:] + noise[k * 5536:(k + 1) * 5536])
        prev = blocks[-1]
    assert all(len(b) == BS for b in blocks)
    add("window carry", b"".join(blocks) + noise[-5:], dic, False, True, True, False, carry=True)
    return cases


def oracle_settings(c, block_size=BS):
    return o.make_settings(independent_blocks=c["indep"], block_checksums=c["bsum"], content_checksum=c["csum"], block_size=block_size,
                           dictionary=c["dict"] if c["dict"] else None, content_size=len(c["data"]) if c["csize"] else None)


@functools.lru_cache(maxsize=None)
def _oracle_frame(name):
    c = next(c for c in all_cases() if c["name"] == name)
    rc, f = o.frame_compress(c["data"], oracle_settings(c))
    assert rc == 0
    return f


def oracle_frame(c):
    return _oracle_frame(c["name"])


def header_bytes(c, bd=0x40):
    """compress.rs:163-200 for block_size 64 KiB: magic, FLG, BD, [content size], HC."""
    flg = 0x40 | (0x20 if c["indep"] else 0) | (0x10 if c["bsum"] else 0) | (0x08 if c["csize"] else 0) | (0x04 if c["csum"] else 0)
    h = bytes([flg, bd]) + (struct.pack("<Q", len(c["data"])) if c["csize"] else b"")
    return struct.pack("<I", 0x184D2204) + h + bytes([(o.xxh32(h) >> 8) & 0xFF])


_rep = None


def template_table(dic):
    """compress.rs:202-211: for window in dict.windows(8).step_by(3) { template_table.replace(dict, offset) }"""
    global _rep
    if _rep is None:
        _rep = o.lib().lzfo_u32_replace
        _rep.restype = C.c_size_t
        _rep.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_int)]
    t, contract = o.new_table(), C.c_int(0)
    for off in range(0, len(dic) - 7, 3):
        _rep(C.addressof(t), dic, len(dic), off, C.byref(contract))
    return t


def clone_table(t):
    c = o.new_table()
    C.memmove(C.addressof(c), C.addressof(t), C.sizeof(t))
    return c


def block_bytes(c, history, block, table):
    """One block as it goes into the frame (:240-263): the length word (stored when the writer refuses), payload, block checksum."""
    rc, payload = o.compress2(history + block, cursor=len(history), table=table, cap=len(block))
    word = len(payload)
    if rc != 0:
        payload, word = block, len(block) | 0x80000000
    return struct.pack("<I", word) + payload + (struct.pack("<I", o.xxh32(payload)) if c["bsum"] else b""), rc != 0


def bad_block_size_status(block_size):
    """BlockDescriptor::new (header.rs:53-62) for a block size that is not one of the format's."""
    tz = (block_size & -block_size).bit_length() - 1 if block_size else 64
    b = ((((tz - 8) if tz > 8 else 0) // 2) & 0xFF) << 4 & 0xFF
    if b & 0x8F:
        return PANIC
    size = (b >> 4) & 7
    if size < 4 or (1 << (size * 2 + 8)) != block_size:
        return INVALID_BLOCK_SIZE
    return OK


class Model:
    """One frame's write cursor, restated: call(offer, finish, cap) -> (out bytes, taken, status, phase, events)."""

    def __init__(self, case, block_size=BS):
        self.c, self.bs = case, block_size
        self.phase, self.status, self.taken, self.header_out = MORE, OK, 0, False
        self.window = case["dict"]                              # linked: in_buffer in front of the next block
        self.template = template_table(case["dict"])
        self.table = clone_table(self.template)                 # linked: the stream's
        self.all = b""

    def call(self, offer, finish, cap):
        c, bs = self.c, self.bs
        if self.phase == DONE:
            return b"", 0, self.status, DONE, {"held"}
        bad = bad_block_size_status(bs)
        if bad != OK:
            self.phase, self.status = DONE, bad
            return b"", 0, bad, DONE, {"bad block size"}
        # what is taken: the reference's cut of the offer, then block after block while the frame bound of the run fits
        cuts = [offer[i:i + bs] for i in range(0, len(offer), bs)]
        if cuts and len(cuts[-1]) < bs and not finish:
            cuts.pop()
        k, t = 0, 0
        while k < len(cuts) and bound(t + len(cuts[k]), bs) <= cap:
            t += len(cuts[k])
            k += 1
        ev = set()
        if cuts and k == 0:
            return b"", 0, OUT_CAPACITY, MORE, {"no room"}
        if not cuts:
            if not finish:
                return b"", 0, OK, NEED_INPUT, {"need input: untouched", "need input: nothing offered" if not offer else "need input: part-block alone"}
            if cap < bound(0, bs):
                return b"", 0, OUT_CAPACITY, MORE, {"no room", "no room for the end alone"}
            ev.add("finish alone")
        out = b""
        if not self.header_out:
            out += header_bytes(c)
            ev.add("header")
            if k and not c["indep"]:
                ev.add("fresh cursor with dictionary" if c["dict"] else "fresh cursor without dictionary")
        elif k and not c["indep"]:
            ev.add("window carried")
            if self.table.offset:
                ev.add("table offset carried")
        for b in cuts[:k]:
            if c["indep"]:
                piece, stored = block_bytes(c, c["dict"], b, clone_table(self.template))
            else:
                piece, stored = block_bytes(c, self.window, b, self.table)
                self.window += b
                if len(self.window) > WINDOW:                   # :271-275
                    forget = len(self.window) - WINDOW
                    self.window = self.window[forget:]
                    self.table.offset += forget
            out += piece
            ev.add("stored block" if stored else "compressed block")
            if len(b) < bs:
                ev.add("short last block")
        self.header_out = True
        self.taken += t
        self.all += offer[:t]
        if finish and k == len(cuts):
            out += struct.pack("<I", 0) + (struct.pack("<I", o.xxh32(self.all)) if c["csum"] else b"")
            self.phase = DONE
            ev.add("done")
        elif k < len(cuts):
            self.phase = MORE
            ev.add("more")
        else:
            self.phase = NEED_INPUT
            ev.add("need input: part-block left" if len(offer) > t else "need input: nothing left")
        assert len(out) <= cap
        return out, t, OK, self.phase, ev


# ---- schedules: how an input is cut into offers and which room each call gets ------------------------------------------------

SCHEDULES = ("everything", "one block per call", "one and a half blocks", "small offers", "finish alone", "room for one block",
             "one byte short, then cured")


class Schedule:
    """The offers of one frame under a named schedule: step() -> (a, b, finish, cap) offers data[a:b]; feed(taken, status, phase)
    moves on.  Untaken tails are offered again.  Once the frame is DONE it goes on offering its first block with FINISH: a DONE
    cursor called again."""

    def __init__(self, name, n, bs=BS):
        self.name, self.n, self.bs, self.pos, self.calls, self.grow, self.done = name, n, bs, 0, 0, 0, False

    def step(self):
        n, bs, pos, left = self.n, self.bs, self.pos, self.n - self.pos
        if self.done:
            return 0, min(n, bs), True, bound(bs, bs)
        s = self.name
        if s == "everything":
            return pos, n, True, bound(left, bs)
        if s == "one block per call":
            return pos, min(n, pos + bs), left <= bs, bound(bs, bs)
        if s == "one and a half blocks":
            return pos, min(n, pos + bs + bs // 2), left <= bs + bs // 2, bound(2 * bs, bs)
        if s == "small offers":                                 # offers that grow by a third of a block until a block is taken
            b = min(n, pos + (self.grow + 1) * (bs // 3))
            return pos, b, b == n and self.grow >= 1, bound(2 * bs, bs)
        if s == "finish alone":                                 # everything without FINISH, then the tail (or nothing) with it
            return pos, n, self.calls > 0, bound(left, bs)
        if s == "room for one block":
            return pos, n, True, bound(bs, bs)
        if s == "one byte short, then cured":
            return pos, n, True, bound(min(left, bs), bs) - 1 if self.calls == 0 else bound(left, bs)
        raise KeyError(s)

    def feed(self, taken, status, phase):
        self.calls += 1
        self.pos += taken
        self.grow = 0 if taken else self.grow + 1
        if phase == DONE:
            self.done = True


def run_model(case, schedule, limit=40, block_size=BS):
    """The calls of one schedule until DONE, and one call more: [(out, taken, status, phase, events)]."""
    m, s, calls = Model(case, block_size), Schedule(schedule, len(case["data"])), []
    for _ in range(limit):
        was_done = s.done
        a, b, finish, cap = s.step()
        calls.append(m.call(case["data"][a:b], finish, cap))
        s.feed(*calls[-1][1:4])
        if was_done:
            return calls
    raise AssertionError("the model did not end")
