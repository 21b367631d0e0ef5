"""CPU tests of the streaming frame writer's rules (no GPU): the Python model of tests/frame_append_cases.py against the oracle's
frame_compress of the whole input on every case and schedule; a census that every rule and phase is reached; the shared rules
header (rust-lz-fear_amd/csrc/lzf_frame_append_rules.h) compiled with g++ (tests/emu/emu_frame_append.cpp) against the model, call
by call; and the ABI-facing pieces that need no device."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import frame_append_cases as A
import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import build, ffi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def cases():
    return A.all_cases()


def test_model_equals_the_oracle_on_every_case_and_schedule(cases):
    for c in cases:
        want = A.oracle_frame(c)
        for sch in A.SCHEDULES:
            calls = A.run_model(c, sch)
            assert b"".join(x[0] for x in calls) == want, (c["name"], sch)
            assert sum(x[1] for x in calls) == len(c["data"]), (c["name"], sch)
            assert calls[-2][3] == A.DONE and calls[-2][2] == A.OK and calls[-1][:4] == (b"", 0, A.OK, A.DONE), (c["name"], sch)
            for x in calls[:-2]:
                assert x[3] != A.DONE and x[2] in (A.OK, A.OUT_CAPACITY), (c["name"], sch)
                assert (x[2] == A.OUT_CAPACITY) == ("no room" in x[4]) and (x[2] == A.OK or (x[0], x[1], x[3]) == (b"", 0, A.MORE))


def test_bad_block_size_ends_the_frame_at_once(cases):
    c = cases[3]
    for size, want in ((65537, A.INVALID_BLOCK_SIZE), (1000, A.INVALID_BLOCK_SIZE), (0, A.PANIC), (1 << 24, A.PANIC)):
        assert A.bad_block_size_status(size) == want
        calls = A.run_model(c, "everything", block_size=size)
        assert [x[:4] for x in calls] == [(b"", 0, want, A.DONE)] * 2 and calls[0][4] == {"bad block size"} and calls[1][4] == {"held"}
    rc, _ = o.frame_compress(c["data"], A.oracle_settings(c, block_size=65537))
    assert rc == A.INVALID_BLOCK_SIZE
    assert all(A.bad_block_size_status(1 << k) == A.OK for k in (16, 18, 20, 22))


def test_census_every_rule_is_reached(cases):
    seen = set()
    for c in cases:
        for sch in A.SCHEDULES:
            for x in A.run_model(c, sch):
                seen |= x[4]
    seen |= A.run_model(cases[0], "everything", block_size=1000)[0][4]
    want = {"held", "bad block size", "no room", "no room for the end alone", "need input: untouched", "need input: nothing offered",
            "need input: part-block alone", "need input: part-block left", "need input: nothing left", "more", "done", "finish alone", "header",
            "fresh cursor with dictionary", "fresh cursor without dictionary", "window carried", "table offset carried",
            "stored block", "compressed block", "short last block"}
    assert want <= seen, sorted(want - seen)
    # rule 7 (a block status that is neither LZF_OK nor LZF_OUTPUT_FULL) is not reachable from data: the compressor refuses a
    # block only for room.  test_rules_header_block_failure drives it through the rules header.


def test_window_carry_case_depends_on_what_crosses_the_call_boundary(cases):
    """The oracle's frame of the window-carry input differs when the dictionary is withheld (block 0), when the blocks are
    independent (the window: blocks 1 and 2), and block 1 compressed behind its window with a FRESH table differs from the
    frame's block 1 (the table)."""
    c = next(c for c in cases if "carry" in c["tags"])
    frame = A.oracle_frame(c)
    hl = len(A.header_bytes(c))
    words, r = [], hl
    for _ in range(3):
        (w,) = struct.unpack_from("<I", frame, r)
        words.append((r, w))
        r += 4 + (w & 0x7FFFFFFF) + 4
    assert all(not w & 0x80000000 and w < 12000 for _, w in words), words          # every whole block compresses through its history
    data = c["data"]
    for k in range(3):                      # no block compresses without its history: the dictionary (block 0), the window (blocks 1, 2)
        rc, _ = o.compress2(data[k * A.BS:(k + 1) * A.BS], cap=A.BS)
        assert rc != 0, k
    other = dict(c, dict=b"")
    rc, f = o.frame_compress(data, A.oracle_settings(other))
    assert rc == 0 and struct.unpack_from("<I", f, hl)[0] == A.BS | 0x80000000        # the dictionary withheld: block 0 is stored
    rc, fresh = o.compress2(data[A.BS - A.WINDOW:2 * A.BS], cursor=A.WINDOW, cap=A.BS)
    at, w = words[1]
    assert rc != 0 or fresh != frame[at + 4:at + 4 + w]
    # and across a call boundary the model reproduces the frame only by carrying all three
    calls = A.run_model(c, "one block per call")
    assert "window carried" in calls[1][4] and "table offset carried" in calls[1][4] and "fresh cursor with dictionary" in calls[0][4]


# ---- the shared rules header against the model ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("frame_append") / "libemu_frame_append.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(HERE, "emu", "emu_frame_append.cpp")])
    L = C.CDLL(so)
    for f in (L.lzf_emu_append_head_bytes, L.lzf_emu_append_cursor_bytes, L.lzf_emu_append_hash_offset, L.lzf_emu_append_bound):
        f.restype = C.c_uint64
    L.lzf_emu_append_bound.argtypes = [C.c_uint64, C.c_uint64]
    L.lzf_emu_append_hash_reset.argtypes = [C.c_void_p]
    L.lzf_emu_append_hash_reset.restype = None
    L.lzf_emu_append_cut.argtypes = [C.c_int32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p]
    L.lzf_emu_append_cut.restype = None
    L.lzf_emu_append_first_window.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    L.lzf_emu_append_first_window.restype = None
    L.lzf_emu_append_settle.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    L.lzf_emu_append_settle.restype = None
    return L


END_FINISH = 5


class EmuCursor:
    """One frame's cursor driven through the rules header: what is taken, block 0's history, the table offsets and the
    transitions are the header's; the blocks are compressed by the oracle behind exactly the history and table the header
    names; the window is kept as the device keeps it (the last 64 KiB taken)."""

    def __init__(self, L, case, block_size=A.BS):
        self.L, self.c, self.bs = L, case, block_size
        self.head = C.create_string_buffer(int(L.lzf_emu_append_head_bytes()))
        self.window, self.all = b"", b""
        self.template = A.template_table(case["dict"])
        self.table = None

    def call(self, offer, finish, cap, block_status=0):
        L, c, bs = self.L, self.c, self.bs
        bd = A.bad_block_size_status(bs)
        off = (C.c_uint64 * 4)()
        L.lzf_emu_append_cut(bd, bs if bd == A.OK else 1, len(offer), A.FINISH if finish else 0, cap, off)
        t, nb, end = int(off[0]), int(off[1]), int(off[2])
        phase, header_out = struct.unpack_from("<II", self.head.raw, 0)
        linked = not c["indep"]
        body, blocks = b"", [offer[i:min(i + bs, t)] for i in range(0, t, bs)]
        assert len(blocks) == nb
        if end >= 3 and phase != A.DONE and nb:
            if linked:
                w = (C.c_uint64 * 3)()
                L.lzf_emu_append_first_window(self.head, len(c["dict"]), len(blocks[0]), w)
                hist = int(w[0])
                source = self.window if header_out else c["dict"]
                assert hist <= len(source)
                history = source[len(source) - hist:]
                if not header_out:
                    self.table = A.clone_table(self.template)
                for k, b in enumerate(blocks):
                    self.table.offset += int(w[1]) if k == 0 else int(w[2]) if k == 1 else bs
                    piece, _ = A.block_bytes(c, history if k == 0 else offer[k * bs - A.WINDOW:k * bs], b, self.table)
                    body += piece
            else:
                for b in blocks:
                    body += A.block_bytes(c, c["dict"], b, A.clone_table(self.template))[0]
        header = A.header_bytes(c)
        rep = (C.c_uint64 * 6)()
        L.lzf_emu_append_settle(self.head, off, block_status, len(body), len(header), 4 + (4 if c["csum"] else 0), int(linked), len(c["dict"]), bs,
                                len(blocks[-1]) if blocks else 0, rep)
        out_len, taken, status, ph, writes, hdr = int(rep[0]), int(rep[1]), C.c_int32(rep[2] & 0xFFFFFFFF).value, int(rep[3]), int(rep[4]), int(rep[5])
        out = b""
        if writes:
            self.all += offer[:t]
            if linked and t >= A.WINDOW:
                self.window = offer[t - A.WINDOW:t]
            out = (header if hdr else b"") + body
            if end == END_FINISH:
                out += struct.pack("<I", 0) + (struct.pack("<I", o.xxh32(self.all)) if c["csum"] else b"")
        assert len(out) == out_len
        return out, taken, status, ph


def test_rules_header_equals_the_model_on_every_case(emu, cases):
    assert emu.lzf_emu_append_cursor_bytes() % 256 == 0
    for t in (0, 1, A.BS - 1, A.BS, A.BS + 1, 7 * A.BS + 3):
        assert emu.lzf_emu_append_bound(A.BS, t) == A.bound(t)
    for c in cases:
        for sch in A.SCHEDULES:
            want = A.run_model(c, sch)
            e, s = EmuCursor(emu, c), A.Schedule(sch, len(c["data"]))
            for i, x in enumerate(want):
                a, b, finish, cap = s.step()
                before = e.head.raw
                got = e.call(c["data"][a:b], finish, cap)
                assert got == x[:4], (c["name"], sch, i, got[1:], x[1:4])
                if "held" in x[4] or "no room" in x[4] or "need input: untouched" in x[4]:
                    assert e.head.raw == before, (c["name"], sch, i, "the cursor was touched")
                s.feed(*got[1:])


def test_rules_header_bad_block_size_and_block_failure(emu, cases):
    c = cases[3]
    for size, want in ((65537, A.INVALID_BLOCK_SIZE), (1 << 24, A.PANIC)):
        e = EmuCursor(emu, c, block_size=size)
        assert e.call(c["data"], True, A.bound(len(c["data"]))) == (b"", 0, want, A.DONE)
        assert e.call(c["data"], True, A.bound(len(c["data"]))) == (b"", 0, want, A.DONE)
    # rule 7: the first bad block status ends the frame, nothing of the call is written or taken, and it sticks
    c = next(c for c in cases if c["name"] == "linked dict 100 len 196613")
    e = EmuCursor(emu, c)
    assert e.call(c["data"][:A.BS], False, A.bound(A.BS))[1:] == (A.BS, A.OK, A.NEED_INPUT)
    assert e.call(c["data"][A.BS:], True, A.bound(3 * A.BS), block_status=3) == (b"", 0, 3, A.DONE)
    assert e.call(c["data"][A.BS:], True, A.bound(3 * A.BS)) == (b"", 0, 3, A.DONE)


def test_rules_header_fresh_hash_is_the_hosts_reset(emu):
    lib = ffi.lib()
    state, fresh = ffi.Xxh32State(), ffi.Xxh32State()
    lib.lzf_xxh32_reset(C.byref(fresh), 0)
    emu.lzf_emu_append_hash_reset(C.byref(state))
    assert bytes(state)[:16] == bytes(fresh)[:16] and (state.fill, state.seed, state.total) == (0, 0, 0)
    assert emu.lzf_emu_append_hash_offset() % 8 == 0 and emu.lzf_emu_append_hash_offset() + 48 <= emu.lzf_emu_append_head_bytes() <= 256


# ---- the ABI-facing pieces that need no device -----------------------------------------------------------------------------------

def test_append_entry_points_are_exported_and_sized(emu):
    build.build_library()
    lib = ffi.lib()
    for name in ("lzf_frame_wcursor_bytes", "lzf_frame_append_device"):
        assert hasattr(lib, name), name
        assert name in ffi.FRAME_EXPORTS
    assert lib.lzf_frame_wcursor_bytes() == emu.lzf_emu_append_cursor_bytes() and lib.lzf_frame_wcursor_bytes() % 256 == 0
    assert lib.lzf_frame_wcursor_bytes() >= 256 + A.WINDOW + C.sizeof(ffi.U32Table)
    assert (ffi.APPEND_MORE, ffi.APPEND_NEED_INPUT, ffi.APPEND_DONE, ffi.APPEND_FINISH) == (A.MORE, A.NEED_INPUT, A.DONE, A.FINISH)
    hdr = open(os.path.join(ROOT, "include", "lzfear_frame.h")).read()
    for name, v in (("LZF_APPEND_MORE", 0), ("LZF_APPEND_NEED_INPUT", 1), ("LZF_APPEND_DONE", 2), ("LZF_APPEND_FINISH", 1)):
        assert f"#define {name}" in hdr and hdr.split(f"#define {name}")[1].split()[0] == f"{v}u"
    s = ffi.Settings()
    lib.lzf_settings_default(C.byref(s))
    s.block_size = A.BS
    so = o.make_settings(block_size=A.BS)
    for t in (0, 1, A.BS - 1, A.BS, A.BS + 1, 3 * A.BS + 5):
        assert lib.lzf_frame_compress_bound(C.byref(s), t) == A.bound(t) == o.lib().lzfo_frame_compress_bound(C.byref(so), t)


def test_append_rejects_bad_arguments_without_a_device():
    lib = ffi.lib()
    s = ffi.Settings()
    lib.lzf_settings_default(C.byref(s))
    assert lib.lzf_frame_append_device(None, 0, None, None, None, None, 0, None, None, None, None, None, None, None, None) == ffi.E_INVALID
    assert lib.lzf_frame_append_device(C.byref(s), 1, None, None, None, None, 0, None, None, None, None, None, None, None, None) == ffi.E_INVALID
    keep = C.create_string_buffer(8)
    s.dictionary, s.dictionary_len = C.cast(keep, C.c_void_p), 8
    assert lib.lzf_frame_append_device(C.byref(s), 0, None, None, None, None, 0, None, None, None, None, None, None, None, None) == ffi.E_INVALID
