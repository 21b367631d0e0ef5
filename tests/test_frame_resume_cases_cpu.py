"""CPU tests of the resumable frame decode's rules (no GPU): the Python model of tests/frame_resume_cases.py against the oracle's
decode of the whole frame on every case and schedule; a census that every rule is reached by some case; the shared rules header
(rust-lz-fear_amd/csrc/lzf_frame_resume_rules.h) compiled with g++ (tests/emu/emu_frame_resume.cpp) against the model, call by
call; the XXH32 state path on the host for every split the GPU test uses; and the ABI-facing pieces that need no device."""
import ctypes as C
import os
import subprocess

import pytest

import frame_resume_cases as R
import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import build, ffi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def cases():
    return R.all_cases()


_whole = {}


def whole(c):
    """The oracle's decode of the whole frame."""
    if c["name"] not in _whole:
        _whole[c["name"]] = o.frame_decompress(c["frame"], c["dict"], cap=R.OUT_ROOM)
    return _whole[c["name"]]


def _growth(case):
    """in_len at every byte of the frame (the model is then given the full length)."""
    return range(len(case["frame"]))


def census_runs(cases):
    """Every (case, capacity, in_lens, label) the tests run: the capacity schedules of every case, three bounds per call for the
    frames that stop, every cut of the small two-block frame, a capacity below the first bound, a DONE cursor called again."""
    for c in cases:
        for sch in R.CAP_SCHEDULES:
            yield c, R.capacity(c, sch), None, sch
        if "stop" in c["tags"]:
            yield c, R.capacity(c, "three bounds"), None, "three bounds"
        if "growth" in c["tags"]:
            for cut in _growth(c):
                yield c, R.capacity(c, "everything"), [cut], f"cut at {cut}"
                if cut % 37 == 0:
                    yield c, R.capacity(c, "one bound"), [cut], f"cut at {cut}"
            yield c, R.capacity(c, "everything"), [20, 300, len(c["frame"]) - 9], "three cuts"


def test_model_equals_the_oracle_on_every_case_and_schedule(cases):
    for c, cap, in_lens, label in census_runs(cases):
        rc, out, used = whole(c)
        calls = R.run_model(c, cap, in_lens)
        got = b"".join(x[0] for x in calls)
        assert (calls[-1][1], calls[-1][2]) == (rc, used) and got == out, (c["name"], label, calls[-1][1:4], (rc, used), len(got), len(out))
        assert calls[-1][3] == R.DONE
        for x in calls[:-1]:
            assert x[1] == R.OK and x[3] != R.DONE, (c["name"], label)     # nothing is sticky before the end


def test_truncated_input_rests_in_need_input_with_the_cut_frames_output(cases):
    """THE ONE DIFFERENCE: in_len never reaches the end.  The frame rests in NEED_INPUT with LZF_OK; what was delivered is the
    whole decode's output for the cut input, whose status is InputError; consumed is the start of the incomplete item."""
    c = next(c for c in cases if "growth" in c["tags"])
    for cut in range(len(c["frame"])):
        m = R.Model(c)
        out, status, consumed, phase, _ = m.call(cut, R.capacity(c, "everything"))
        rc, want, used = o.frame_decompress(c["frame"][:cut], cap=R.OUT_ROOM)
        assert (rc, used) == (R.INPUT_ERROR, cut) and (status, phase) == (R.OK, R.NEED_INPUT) and out == want and consumed <= cut, cut
        again = m.call(cut, R.capacity(c, "everything"))
        assert again[:4] == (b"", R.OK, consumed, R.NEED_INPUT)


def test_census_every_rule_is_reached(cases):
    seen = set()
    for c, cap, in_lens, _ in census_runs(cases):
        for x in R.run_model(c, cap, in_lens):
            seen |= x[4]
    c = cases[0]
    m = R.Model(c)
    first = m.call(len(c["frame"]), R.capacity(c, "one bound") - 1)
    assert first[:4] == (b"", R.OUT_CAPACITY, 0, R.MORE)
    seen |= first[4]
    assert m.call(len(c["frame"]), R.capacity(c, "one bound"))[1] == R.OK           # more room cures it
    while m.phase != R.DONE:
        m.call(len(c["frame"]), R.capacity(c, "two bounds"))
    seen |= m.call(len(c["frame"]), R.capacity(c, "two bounds"))[4]
    want = {"more", "need input", "done", "held", "no room", "header error", "endmark", "length word overflow", "content checksum fails",
            "more at the first block", "more at a middle block", "more at the last block",
            "need input: header", "need input: length word", "need input: payload", "need input: block checksum",
            "need input: in front of the EndMark", "need input: content checksum",
            "window shorter than 64 KiB", "window equal to 64 KiB", "window longer than 64 KiB", "short piece behind a full window"}
    for status in (0, 3, R.BLOCK_CHECKSUM_FAIL, R.BLOCK_SIZE_OVERFLOW):             # the empty block, a codec error, a damaged block checksum, past block_maxsize
        want |= {f"stop {status}: {where}" for where in ("first of its piece", "last of its piece", "inside its piece", "alone")}
    assert want <= seen, sorted(want - seen)


# ---- the shared rules header against the model ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("frame_resume") / "libemu_frame_resume.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(HERE, "emu", "emu_frame_resume.cpp")])
    L = C.CDLL(so)
    for f in (L.lzf_emu_resume_head_bytes, L.lzf_emu_resume_cursor_bytes, L.lzf_emu_resume_hash_offset, L.lzf_emu_resume_walk):
        f.restype = C.c_uint64
    L.lzf_emu_resume_walk.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
    L.lzf_emu_resume_settle.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
    L.lzf_emu_resume_settle.restype = None
    L.lzf_emu_resume_window.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p]
    L.lzf_emu_resume_window.restype = None
    L.lzf_emu_resume_dict_window.argtypes = [C.c_uint64]
    L.lzf_emu_resume_dict_window.restype = C.c_uint32
    L.lzf_emu_resume_hash_reset.argtypes = [C.c_void_p]
    L.lzf_emu_resume_hash_reset.restype = None
    L.lzf_emu_resume_delivers.argtypes = [C.c_void_p]
    return L


class EmuCursor:
    """One frame's cursor driven through the rules header: the walk and the transitions are the header's; the blocks' decode comes
    from the oracle (the model's table), the hash from the host's lzf_xxh32_update; the window is kept as bytes."""

    def __init__(self, L, case):
        self.L, self.case = L, case
        self.head = C.create_string_buffer(int(L.lzf_emu_resume_head_bytes()))
        self.m = R.Model(case)                          # for the oracle's table only: cum / stop / content
        self.block, self.window, self.had = 0, case["dict"][-R.WINDOW:] if case["dict"] else b"", False
        self.hash_at = int(L.lzf_emu_resume_hash_offset())

    def call(self, in_len, cap):
        L, lib = self.L, ffi.lib()
        f = self.case["frame"]
        piece = C.create_string_buffer(64)
        blocks = (C.c_uint64 * (5 * 64))()
        nb = int(L.lzf_emu_resume_walk(f[:in_len], in_len, self.head, cap, piece, blocks, 64))       # (only in[0, in_len) is handed in)
        stopped, st, consumed, w, upto = 0, 0, 0, 0, self.block + nb
        delivers = bool(L.lzf_emu_resume_delivers(piece))
        if delivers and getattr(self.m, "stop", None) is not None and self.block <= self.m.stop[0] < upto:
            upto, (_, st, consumed), stopped = self.m.stop[0], self.m.stop, 1
        out = self.m.content[self.m.cum[self.block]:self.m.cum[upto]] if delivers else b""
        # the hash: a fresh cursor's is lzf_xxh32_reset; the delivered bytes go through the host's update
        state = ffi.Xxh32State.from_buffer_copy(self.head.raw[self.hash_at:self.hash_at + 48])
        parsed = int.from_bytes(self.head.raw[4:8], "little")
        if not parsed:
            fresh = ffi.Xxh32State()
            lib.lzf_xxh32_reset(C.byref(fresh), 0)
            L.lzf_emu_resume_hash_reset(C.byref(state))
            assert bytes(state)[:16] == bytes(fresh)[:16] and (state.fill, state.seed, state.total) == (0, 0, 0)
        flags = C.c_uint32.from_buffer_copy(piece.raw[8:12]).value
        if out and flags & R.FL_CSUM:
            lib.lzf_xxh32_update(C.byref(state), out, len(out))
        report = (C.c_uint64 * 4)()
        L.lzf_emu_resume_settle(self.head, piece, stopped, st, consumed, len(out), C.byref(state), lib.lzf_xxh32_digest(C.byref(state)), report)
        n, used, status, phase = int(report[0]), int(report[1]), C.c_int32(report[2] & 0xFFFFFFFF).value, int(report[3])
        if delivers and not stopped:
            self.block = upto
        if n and phase != R.DONE and not flags & R.FL_INDEP:
            plan = (C.c_uint32 * 3)()
            L.lzf_emu_resume_window(len(self.window), n, plan)
            keep, take, new_len = plan
            self.window = (self.window[len(self.window) - keep:] + out[len(out) - take:])
            assert len(self.window) == new_len
        assert n == len(out)
        return out, status, used, phase


def test_rules_header_equals_the_model_on_every_case(emu, cases):
    assert emu.lzf_emu_resume_cursor_bytes() % 256 == 0 and emu.lzf_emu_resume_dict_window(40000) == 40000 and emu.lzf_emu_resume_dict_window(1 << 20) == R.WINDOW
    for c, cap, in_lens, label in census_runs(cases):
        if "growth" in c["tags"] and label.startswith("cut at") and int(label[7:]) % 7 and int(label[7:]) > 40:
            continue                                    # (every cut of the header and its surroundings, every seventh behind them)
        want = R.run_model(c, cap, in_lens)
        e = EmuCursor(emu, c)
        lens = list(in_lens or []) + [len(c["frame"])]
        delivered = b""
        for i, x in enumerate(want):
            got = e.call(lens[min(i, len(lens) - 1)], cap)
            assert got == x[:4], (c["name"], label, i, got[1:], x[1:4])
            delivered += got[0]
            if got[0] and got[3] != R.DONE and not c["frame"][4] & R.FL_INDEP:
                assert e.window == (c["dict"] + delivered)[-R.WINDOW:], (c["name"], label, i, "the window")
        held = e.call(len(c["frame"]), cap)
        assert held == (b"", want[-1][1], want[-1][2], R.DONE), (c["name"], label, "a DONE cursor called again")


def test_rules_header_no_room_leaves_the_cursor_untouched(emu, cases):
    c = cases[0]
    e = EmuCursor(emu, c)
    assert e.call(len(c["frame"]), R.capacity(c, "one bound") - 1) == (b"", R.OUT_CAPACITY, 0, R.MORE)
    assert e.head.raw == bytes(len(e.head.raw))
    assert e.call(len(c["frame"]), R.capacity(c, "one bound"))[1:] == (R.OK, R.Model(c).call(len(c["frame"]), R.capacity(c, "one bound"))[2], R.MORE)
    before = e.head.raw
    assert e.call(len(c["frame"]), 10)[1:] == (R.OUT_CAPACITY, R.Model(c).call(len(c["frame"]), R.capacity(c, "one bound"))[2], R.MORE)
    assert e.head.raw == before


# ---- the XXH32 state path on the host ---------------------------------------------------------------------------------------------

def test_host_xxh32_update_in_pieces_is_the_hash_of_the_whole():
    """The model of "update in pieces" is the host's own lzf_xxh32_update: for every split tests/test_gpu_xxh32_state.py runs on
    the device it gives lzf_xxh32 of the concatenation (and the oracle's XXH32)."""
    lib = ffi.lib()
    rows = R.xxh_splits()
    assert {len(buf[:a]) % 16 for buf, a, b in rows} == set(range(16)) and {(b - a) % 16 for _, a, b in rows} == set(range(16))
    whole = {}
    for buf, a, b in rows:
        st = ffi.Xxh32State()
        lib.lzf_xxh32_reset(C.byref(st), 0)
        for piece in (buf[:a], buf[a:b], buf[b:]):
            lib.lzf_xxh32_update(C.byref(st), piece, len(piece))
        if len(buf) not in whole:
            whole[len(buf)] = lib.lzf_xxh32(buf, len(buf), 0)
            assert whole[len(buf)] == o.xxh32(buf)
        assert lib.lzf_xxh32_digest(C.byref(st)) == whole[len(buf)], (len(buf), a, b)


# ---- the ABI-facing pieces that need no device -----------------------------------------------------------------------------------

def test_resume_entry_points_are_exported_and_sized(emu):
    build.build_library()
    lib = ffi.lib()
    for name in ("lzf_frame_cursor_bytes", "lzf_frame_resume_device", "lzf_xxh32_update_batch", "lzf_xxh32_digest_batch"):
        assert hasattr(lib, name), name
        assert name in ffi.EXPORTS + ffi.FRAME_EXPORTS
    assert lib.lzf_frame_cursor_bytes() == emu.lzf_emu_resume_cursor_bytes() and lib.lzf_frame_cursor_bytes() % 256 == 0
    assert C.sizeof(ffi.Xxh32State) == 48
    from rust_lz_fear_amd import device
    assert device.XXH32_STATE.itemsize == 48
    assert [device.XXH32_STATE.fields[n][1] for n in ("v", "buf", "fill", "seed", "total")] == \
        [getattr(ffi.Xxh32State, n).offset for n in ("v", "buf", "fill", "seed", "total")]
    assert (ffi.RESUME_MORE, ffi.RESUME_NEED_INPUT, ffi.RESUME_DONE) == (R.MORE, R.NEED_INPUT, R.DONE)
    hdr = open(os.path.join(ROOT, "include", "lzfear_frame.h")).read()
    for name, v in (("LZF_RESUME_MORE", 0), ("LZF_RESUME_NEED_INPUT", 1), ("LZF_RESUME_DONE", 2)):
        assert f"#define {name}" in hdr and hdr.split(f"#define {name}")[1].split()[0] == f"{v}u"
