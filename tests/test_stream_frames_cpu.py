"""CPU tests (no GPU) of the streams of back-to-back frames (include/lzfear_frame.h, "streams of back-to-back frames in device
memory"): the four entry points are declared and exported and fail loudly without a device; the frame-to-frame walk the device
runs (rust-lz-fear_amd/csrc/lzf_stream_walk.h), compiled here with g++, finds the frames, the stop status and the `consumed`
of the loop a caller writes over the reference's decompress_frame (the oracle); the stream bound of the compress side is the
sum of the per-frame bounds over the pieces."""
import ctypes as C
import json
import os
import subprocess

import pytest

import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import build, ffi
from test_abi import declared_functions
from test_device_frames_cpu import SCAN_KINDS, py_scan_blocks
from test_oracle import fuzz_corpus

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
NAMES = ("lzf_frame_stream_bound_device", "lzf_frame_decompress_stream_device", "lzf_frame_compress_stream_bound",
         "lzf_frame_compress_stream_device")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return ffi.lib()


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("walk") / "libemu_stream_walk.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so,
                           os.path.join(HERE, "emu", "emu_stream_walk.cpp")])
    L = C.CDLL(so)
    L.lzf_emu_stream_walk.restype = C.c_int
    L.lzf_emu_stream_walk.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint64]

    def run(data):
        cap = len(data) // 4 + 8
        out = (C.c_uint64 * (4 + cap))()
        L.lzf_emu_stream_walk(data, len(data), out, cap)
        assert out[2] <= cap
        return dict(status=out[0], consumed=out[1], starts=list(out[4:4 + out[2]]), complete=out[3])
    return run


def lz4f_frames():
    J = json.load(open(os.path.join(GOLD, "lz4f_frames.json")))
    blob = open(os.path.join(GOLD, "lz4f_frames.bin"), "rb").read()
    return [blob[e["offset"]: e["offset"] + e["length"]] for e in J["frames"]]


def ended_at_endmark(frame, used):
    """The frame's reader stopped behind the EndMark (and the content checksum word): the walk of its length words ends there."""
    flags, bd = frame[4], frame[5]
    header_len = 7 + (8 if flags & 0x08 else 0) + (4 if flags & 0x01 else 0)
    _, (err, cons) = py_scan_blocks(frame, header_len, flags, 1 << (((bd >> 4) & 7) * 2 + 8))
    return err == 0 and cons == used


def reference_loop(data):
    """The loop of the issue over the oracle's decompress_frame: (frame starts, status, consumed, frames that ended well); status
    None where the stream ends with LZF_OK in mid-frame (the Read adapter's stop at an empty block)."""
    pos, starts, good = 0, [], 0
    while pos < len(data):
        starts.append(pos)
        rc, _, used = o.frame_decompress(data[pos:], cap=8 << 20)
        frame = data[pos:]
        pos += used
        if rc != 0:
            return starts, rc, pos, good
        if not ended_at_endmark(frame, used):
            return starts, None, pos, good
        good += 1
    return starts, 0, pos, good


def hold_to_reference(walk, data, name=""):
    """What the walk must share with the reference loop.  The walk sees structure only: where the reference stops for what
    only a decode finds (codec error, checksum, an empty block, a block that decodes beyond block_maxsize), the walk has found
    the same frames up to there and goes on; everywhere else frames, status and consumed are the reference's."""
    got = walk(data)
    starts, rc, pos, good = reference_loop(data)
    structural = rc == 0 or (rc in SCAN_KINDS and not (rc == 22 and got["status"] != 22))
    assert got["starts"][:len(starts)] == starts, name
    if structural:
        assert (got["starts"], got["status"], got["consumed"], got["complete"]) == (starts, rc, pos, good), name
    return structural


def test_entry_points_declared_exported_and_loud_without_a_device(lib):
    names = declared_functions("lzfear_frame.h")
    for n in NAMES:
        assert n in names and n in ffi.FRAME_EXPORTS
        assert hasattr(lib, n), n
    assert lib.lzf_abi_version() == 2
    if lib.lzf_device_count() > 0:
        return                                    # (the loud-failure half is for GPU-less hosts)
    ptr = (C.c_void_p * 1)(C.cast(C.create_string_buffer(16), C.c_void_p).value)
    ln = (C.c_size_t * 1)(16)
    bound = (C.c_size_t * 1)()
    res = (C.c_uint64 * 4)()
    s = ffi.Settings()
    lib.lzf_settings_default(C.byref(s))
    assert lib.lzf_frame_stream_bound_device(1, ptr, ln, bound, None) == ffi.E_NO_DEVICE
    assert lib.lzf_frame_decompress_stream_device(1, ptr, ln, None, 0, ptr, ln, res, res, res, res, None) == ffi.E_NO_DEVICE
    assert lib.lzf_frame_compress_stream_device(C.byref(s), 1 << 20, 1, ptr, ln, None, 0, ptr, ln, res, res, None) == ffi.E_NO_DEVICE


def test_compress_stream_arguments(lib):
    """frame_bytes == 0 and a host dictionary in the settings are LZF_E_INVALID, with or without a device."""
    ptr = (C.c_void_p * 1)(C.cast(C.create_string_buffer(16), C.c_void_p).value)
    ln = (C.c_size_t * 1)(16)
    res = (C.c_uint64 * 4)()
    s = ffi.Settings()
    lib.lzf_settings_default(C.byref(s))
    assert lib.lzf_frame_compress_stream_device(C.byref(s), 0, 1, ptr, ln, None, 0, ptr, ln, res, res, None) == ffi.E_INVALID
    keep = C.create_string_buffer(b"dictionary")
    s.dictionary = C.addressof(keep)
    s.dictionary_len = 10
    assert lib.lzf_frame_compress_stream_device(C.byref(s), 1 << 20, 1, ptr, ln, None, 0, ptr, ln, res, res, None) == ffi.E_INVALID


def test_compress_stream_bound_is_the_sum_over_the_pieces(lib):
    bs_all = (64 << 10, 256 << 10, 1 << 20, 4 << 20)
    checked = 0
    for bs in bs_all:
        for size in (False, True):
            s = ffi.Settings()
            lib.lzf_settings_default(C.byref(s))
            s.block_size = bs
            s.has_content_size = int(size)
            for fb in (1, 1000, bs - 1, bs, bs + 1, 3 * bs, 3 * bs + 12345, (5 * bs) // 2):
                for n in (0, 1, fb - 1, fb, fb + 1, 2 * fb, 7 * fb, 7 * fb + 1, 7 * fb - 1, 1000003):
                    if n < 0 or (fb < 1000 and n > 4096):
                        continue
                    pieces = [min(fb, n - k) for k in range(0, n, fb)] or [0]
                    assert len(pieces) == max(1, -(-n // fb))
                    want = sum(lib.lzf_frame_compress_bound(C.byref(s), p) for p in pieces)
                    assert lib.lzf_frame_compress_stream_bound(C.byref(s), fb, n) == want, (bs, fb, n)
                    checked += 1
    assert checked > 400
    assert lib.lzf_frame_compress_stream_bound(C.byref(s), 0, 100) == 0


def test_walk_empty_and_trailing_bytes(walk):
    assert walk(b"") == dict(status=0, consumed=0, starts=[], complete=0)
    fr = lz4f_frames()
    two = fr[6] + fr[0]
    for tail, st, cons in ((b"\x04", 16, len(two) + 1), (b"\x04\x22\x4d", 16, len(two) + 3), (b"\x00\x00\x00\x00", 17, len(two) + 4),
                           (b"\x04\x22\x4d\x18\x64\x40\xa7"[1:] + b"\x00", 17, len(two) + 4),
                           (b"\x50\x2a\x4d\x18\x00\x00\x00", 17, len(two) + 4),          # a skippable frame's magic: not understood
                           (b"\x02\x21\x4c\x18\x00\x00\x00", 17, len(two) + 4)):         # the legacy magic: not understood
        got = walk(two + tail)
        assert got == dict(status=st, consumed=cons, starts=[0, len(fr[6]), len(two)], complete=2), tail
        assert hold_to_reference(walk, two + tail)


def test_walk_golden_frames_in_several_orders(walk):
    fr = lz4f_frames()
    assert len(fr) == 8
    orders = [list(range(8)), list(range(7, -1, -1)), [3, 1, 4, 1, 5, 2, 6, 5, 3, 5], [6] * 40, [0, 7], [7, 0]]
    for order in orders:
        data = b"".join(fr[i] for i in order)
        got = walk(data)
        starts = [sum(len(fr[i]) for i in order[:k]) for k in range(len(order))]
        assert got == dict(status=0, consumed=len(data), starts=starts, complete=len(order)), order
        assert hold_to_reference(walk, data, str(order))


def test_walk_uncomp_data_repeated(walk):
    one = open(os.path.join(GOLD, "uncomp.data.lz4"), "rb").read()
    assert hold_to_reference(walk, one)
    for k in (2, 5):
        got = walk(one * k)
        assert got == dict(status=0, consumed=k * len(one), starts=[i * len(one) for i in range(k)], complete=k)
    assert hold_to_reference(walk, one * 3)
    cut = (one * 2)[:len(one) + len(one) // 2]                   # a truncated last frame
    got = walk(cut)
    assert (got["status"], got["consumed"], got["starts"], got["complete"]) == (16, len(cut), [0, len(one)], 1)
    assert hold_to_reference(walk, cut)


def test_walk_every_decode_corpus_file_behind_a_valid_frame(walk):
    """All 830 packed decode-corpus files, valid or malformed, second behind a valid frame: the walk's frames, stop status and
    `consumed` are the reference loop's wherever the reference stops for a structural reason or reads the whole stream."""
    head = lz4f_frames()[6]
    files = fuzz_corpus("decode")
    assert len(files) == 830
    structural = 0
    for name, data in files:
        structural += bool(hold_to_reference(walk, head + data, name))
    assert structural > 400, structural
