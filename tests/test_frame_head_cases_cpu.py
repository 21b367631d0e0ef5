"""CPU tests (no GPU) of the frame head call (lzf_frame_head_device): the rule the kernel runs
(rust-lz-fear_amd/csrc/lzf_frame_head_rules.h), compiled here with g++ as its serial reference function head_frame, gives on every
case of frame_head_cases.py what the model over the oracle's block decodes expects — status, length and bytes — without touching
an output byte at or beyond the target; on every small clean frame at every target it gives the oracle's whole decode cut there;
and at a target far past the end its status and length are the oracle's frame decode's."""
import ctypes as C
import os
import subprocess

import pytest

import frame_head_cases as cases
import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ZONE = 64
POISON = 0xA5


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("frame_head") / "libemu_frame_head.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(HERE, "emu", "emu_frame_head.cpp")])
    L = C.CDLL(so)
    L.lzf_emu_frame_head.restype = C.c_int
    L.lzf_emu_frame_head.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64,
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]

    def run(frame, dictionary, target, room, what=""):
        """(status, out_len, the `room` bytes of output memory) — no access at or beyond min(room, target), the zone behind untouched."""
        mem = C.create_string_buffer(bytes([POISON]) * (room + ZONE), room + ZONE)
        n, outside = C.c_uint64(0), C.c_uint64(0)
        rc = L.lzf_emu_frame_head(frame, len(frame), dictionary, len(dictionary), C.addressof(mem), room, target, C.byref(n), C.byref(outside))
        assert outside.value == 0, (what, target, "an output byte at or beyond the target (or the room) was read or written")
        raw = mem.raw
        assert raw[room:] == bytes([POISON]) * ZONE, (what, target, "written behind the room")
        return rc, n.value, raw[:room]
    run.lib = L
    return run


@pytest.fixture(scope="module")
def rows():
    r = cases.all_cases()
    cases.assert_covers(r)
    return r


def test_head_frame_meets_every_expectation(emu, rows):
    """Fails on a tree without the feature (there is no lzf_frame_head_rules.h to compile)."""
    for c, (st, ln, data, room) in rows:
        rc, n, raw = emu(c["frame"], c["dict"], c["target"], room, c["name"])
        assert (rc, n) == (st, ln), c["name"]
        if data is not None:
            assert raw[:ln] == data and raw[ln:] == bytes([POISON]) * (room - ln), c["name"]


def test_head_frame_at_every_target_of_the_small_clean_frames(emu):
    """Every clean frame of small blocks at every target from 0 to one past its length: the oracle's whole decode, cut there."""
    frames = cases.clean_frames()
    assert len(frames) == 16
    for name, f, dic in frames:
        rc, whole, _ = o.frame_decompress(f, dic, cap=1 << 18)
        assert rc == 0 and 600 <= len(whole) <= 4 * 2400, name
        for t in range(len(whole) + 2):
            want = min(t, len(whole))
            assert emu(f, dic, t, want, name) == (0, want, whole[:want]), (name, t)


def test_far_targets_report_what_the_oracle_reports(emu, rows):
    """Every case at the far target whose blocks pass their checksums: status and length are the oracle's frame decode's, but for a
    content checksum that fails, which this call never compares."""
    n = 0
    for c, (st, ln, _, room) in rows:
        if c["target"] != cases.FAR or c["cls"] == "checksum":
            continue
        rc, out, _ = o.frame_decompress(c["frame"], c["dict"], cap=1 << 19)
        want = 0 if rc == 20 else rc
        assert (st, ln) == (want, len(out)), (c["name"], "the model", (st, ln), (rc, len(out)))
        got = emu(c["frame"], c["dict"], cases.FAR, room, c["name"])
        assert got[:2] == (want, len(out)), c["name"]
        if rc == 0:
            assert got[2] == out, c["name"]
        n += 1
    assert n >= 100, n
    f, _ = cases.flipped_frame()
    assert o.frame_decompress(f, b"", cap=1 << 18)[0] == cases.BLOCK_CHECKSUM_FAIL        # (what the flipped frame is about: the reader refuses it)


def test_header_statuses_are_the_oracles():
    for name, f, st in cases.header_error_frames():
        rc, out, _ = o.frame_decompress(f, b"", cap=1 << 18)
        assert (rc, len(out)) == (st, 0), name


def test_contract_targets_read_nothing(emu):
    """A target of 2 GiB - 256 and more is LZF_CONTRACT before a byte of the frame is looked at: the frame handed in is a NULL."""
    n, outside = C.c_uint64(7), C.c_uint64(0)
    for t in (cases.MAX_LEN, cases.MAX_LEN + 1, 1 << 40, (1 << 64) - 1):
        assert emu.lib.lzf_emu_frame_head(None, 1 << 20, None, 0, None, 0, t, C.byref(n), C.byref(outside)) == cases.CONTRACT
        assert (n.value, outside.value) == (0, 0)
