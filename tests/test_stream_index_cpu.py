"""CPU tests (no GPU) of the exact sizes and the frame index of streams of back-to-back frames (include/lzfear_frame.h:
lzf_frame_stream_count_device / lzf_frame_stream_decompressed_size_device / lzf_stream_index_locate).

The rules the index kernel runs (rust-lz-fear_amd/csrc/lzf_stream_index.h: the ending-frame predicate, the entry fill, locate),
compiled here with g++ and applied frame by frame by a serial driver (tests/emu/emu_stream_index.cpp), are held to a Python
restatement of the stream rule of lzfear_frame.h over the oracle's decompress_frame of every frame; locate, in the emulator and
in the product library (host code: no device needed), to brute force."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
import xxhash

import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import build, device, ffi, synth
from test_abi import declared_functions
from test_device_frames_cpu import py_scan_blocks
from test_gpu_stream_frames import FLAVOURS
from test_stream_frames_cpu import lz4f_frames

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("lzf_frame_stream_count_device", "lzf_frame_stream_decompressed_size_device", "lzf_stream_index_locate")
COMPLETE, BEHIND = ffi.SFRAME_COMPLETE, ffi.SFRAME_BEHIND_STOP
NO_SIZE = ffi.STREAM_NO_CONTENT_SIZE


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return ffi.lib()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sindex") / "libemu_stream_index.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(HERE, "..", "include"),
                           "-o", so, os.path.join(HERE, "emu", "emu_stream_index.cpp")])
    L = C.CDLL(so)
    L.lzf_emu_index_walk.restype = C.c_uint64
    L.lzf_emu_index_walk.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64]
    L.lzf_emu_stream_index.restype = None
    L.lzf_emu_stream_index.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    L.lzf_emu_stream_locate.restype = None
    L.lzf_emu_stream_locate.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return L


def mk(data, **kw):
    rc, f = o.frame_compress(data, o.make_settings(**kw))
    assert rc == 0
    return f


# ---- the restatement: structure from the bytes, every frame's results from the oracle, the stream rule of lzfear_frame.h ------

def py_header(d):
    """LZ4FrameReader::new (decompress.rs:102-161), restated: (status, header_len, FLG)."""
    if len(d) < 4:
        return 16, 0, 0
    if struct.unpack_from("<I", d, 0)[0] != 0x184D2204:
        return 17, 0, 0
    if len(d) < 5:
        return 16, 0, 0
    flg = d[4]
    if flg >> 6 != 1:
        return 24, 0, 0
    if flg & 2:
        return 25, 0, 0
    if len(d) < 6:
        return 16, 0, 0
    if d[5] & 0x8F:
        return 26, 0, 0
    n = 6 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    if len(d) < n + 1:
        return 16, 0, 0
    if d[n] != (xxhash.xxh32(d[4:n]).intdigest() >> 8) & 0xFF:
        return 18, 0, 0
    if (d[5] >> 4) & 7 < 4:
        return 23, 0, 0
    return 0, n + 1, flg


def ref_index(data, dictionary=b""):
    """[entry dicts] of every frame the structural walk finds, and the stream's (status, out_len, consumed, n_frames)."""
    entries, pos = [], 0
    while pos < len(data):
        rest = data[pos:]
        rc, out, used = o.frame_decompress(rest, dictionary=dictionary, cap=1 << 20)
        hst, hlen, flg = py_header(rest)
        werr, wcons = (hst, 0) if hst else py_scan_blocks(rest, hlen, flg, 1 << (((rest[5] >> 4) & 7) * 2 + 8))[1]
        size = struct.unpack_from("<Q", rest, 6)[0] if hst == 0 and flg & 8 else NO_SIZE
        entries.append(dict(in_off=pos, status=rc, out_len=len(out), consumed=used, content_size=size,
                            complete=rc == 0 and werr == 0 and used == wcons))
        if werr:
            break
        pos += wcons
    run = cons = good = status = 0
    stopped = False
    for e in entries:
        e["flags"] = (COMPLETE if e["complete"] else 0) | (BEHIND if stopped else 0)
        e["out_off"] = run
        if stopped:
            continue
        run += e["out_len"]; cons += e["consumed"]
        if e["complete"]:
            good += 1
        else:
            status, stopped = e["status"], True
    return entries, (status, run, cons, good)


def ref_stream(data, dictionary=b""):
    """The loop of lzfear_frame.h with unlimited room, over the oracle: (status, out_len, consumed, frames)."""
    pos = out = good = status = 0
    while pos < len(data):
        rest = data[pos:]
        rc, b, used = o.frame_decompress(rest, dictionary=dictionary, cap=1 << 20)
        out += len(b); pos += used
        if rc != 0:
            status = rc
            break
        hst, hlen, flg = py_header(rest)
        if py_scan_blocks(rest, hlen, flg, 1 << (((rest[5] >> 4) & 7) * 2 + 8))[1] != (0, used):
            break
        good += 1
    return status, out, pos, good


def emu_index(emu, data, dictionary=b"", cap=None):
    """The emulator's walk, the oracle's results for every frame it lists, the serial driver: (entries as SFRAME array, results)."""
    room = len(data) // 4 + 8
    w = np.zeros(3 * room, dtype=np.uint64)
    n = emu.lzf_emu_index_walk(data, len(data), w.ctypes.data, room)
    assert n <= room
    fr = np.zeros((n, 6), dtype=np.uint64)
    for k in range(n):
        at = int(w[3 * k])
        rc, out, used = o.frame_decompress(data[at:], dictionary=dictionary, cap=1 << 20)
        fr[k] = (at, rc, len(out), used, w[3 * k + 1], w[3 * k + 2])
    cap = n if cap is None else cap
    out = np.zeros(max(cap, 1) + 1, dtype=device.SFRAME)
    out["flags"] = 0xDEAD
    res = np.zeros(4, dtype=np.uint64)
    emu.lzf_emu_stream_index(data, fr.ctypes.data, n, out.ctypes.data, cap, res.ctypes.data)
    assert (out["flags"][min(cap, n):] == 0xDEAD).all()              # nothing behind min(cap, n) entries
    return out[:min(cap, n)], tuple(int(x) for x in res), n


def hold(emu, data, dictionary=b"", name=""):
    want, want_res = ref_index(data, dictionary)
    got, res, n = emu_index(emu, data, dictionary)
    assert n == len(want) == len(got), name
    assert res == want_res == ref_stream(data, dictionary), name
    run = 0
    for k, (g, e) in enumerate(zip(got, want)):
        for f in ("in_off", "status", "out_len", "consumed", "content_size", "flags", "out_off"):
            assert int(g[f]) == e[f], (name, k, f)
        behind = bool(e["flags"] & BEHIND)
        assert int(g["out_off"]) == (res[1] if behind else run), (name, k)     # the prefix sum; frozen behind the stop
        if not behind:
            run += e["out_len"]
    stops = [k for k, e in enumerate(want) if not e["complete"]]
    assert all(bool(e["flags"] & BEHIND) == bool(stops and k > stops[0]) for k, e in enumerate(want)), name
    return want, want_res


def inputs():
    mix = synth.silesia_mix(30 << 20, (30 << 20) + 140_000).tobytes()
    return [mix[:5000], b"", mix[5000:5017], mix[10_000:10_000 + 70_001], mix[100_000:100_001]]


def good_frames():
    out = []
    for k, kw in enumerate(FLAVOURS):
        for d in inputs():
            out.append(mk(d, content_size=len(d) if k == 4 else None, **kw))
    return out


def damaged_frames():
    """(a codec error in block 0, a bad block checksum), as tests/test_gpu_stream_frames.py makes them."""
    mix = synth.silesia_mix(41 << 20, (41 << 20) + 100_000).tobytes()
    plain = mk(mix, block_size=64 << 10, content_checksum=False)
    sums = mk(mix, block_size=64 << 10, block_checksums=True)
    assert plain[7 + 3] == 0 and plain[7 + 4] >= 0x10               # (block 0 is compressed and opens with literals)
    codec = bytearray(plain); codec[7 + 4: 7 + 7] = b"\x00\x00\x00"  # block 0 opens with a match at offset 0
    bsum = bytearray(sums); bsum[len(sums) // 2] ^= 0x40
    return bytes(codec), bytes(bsum)


def test_entry_points_declared_exported_and_loud_without_a_device(lib):
    names = declared_functions("lzfear_frame.h")
    for n in NAMES:
        assert n in names and n in ffi.FRAME_EXPORTS
        assert hasattr(lib, n), n
    assert lib.lzf_abi_version() == 2
    assert C.sizeof(ffi.StreamFrame) == 48 == device.SFRAME.itemsize
    assert [device.SFRAME.fields[n][1] for n, _ in ffi.StreamFrame._fields_] == [getattr(ffi.StreamFrame, n).offset for n, _ in ffi.StreamFrame._fields_]
    ptr = (C.c_void_p * 1)(C.cast(C.create_string_buffer(16), C.c_void_p).value)
    ln = (C.c_size_t * 1)(16)
    found = (C.c_size_t * 1)()
    res = (C.c_uint64 * 4)()
    a = C.addressof(res)
    # bad arguments, with or without a device
    assert lib.lzf_frame_stream_count_device(1, ptr, ln, None, None) == ffi.E_INVALID
    assert lib.lzf_frame_stream_decompressed_size_device(1, ptr, ln, 0, None, None, None, a, a, None, None, None) == ffi.E_INVALID
    assert lib.lzf_frame_stream_decompressed_size_device(1, ptr, ln, 0, ptr, None, a, a, a, None, None, None) == ffi.E_INVALID
    if lib.lzf_device_count() > 0:
        return                                    # (the loud-failure half is for GPU-less hosts)
    assert lib.lzf_frame_stream_count_device(1, ptr, ln, found, None) == ffi.E_NO_DEVICE
    assert lib.lzf_frame_stream_decompressed_size_device(1, ptr, ln, 0, None, None, a, a, a, a, a, None) == ffi.E_NO_DEVICE


def test_streams_of_oracle_frames_in_every_flavour(emu):
    p = good_frames()
    rng = np.random.default_rng(5)
    streams = [p[0], p[9] + p[2], b"".join(p[int(i)] for i in rng.integers(0, len(p), 30)), b"".join(p), mk(b""), mk(b"") * 3,
               b"".join(lz4f_frames())]
    for i, s in enumerate(streams):
        want, res = hold(emu, s, name=f"stream {i}")
        assert res[0] == 0 and res[2] == len(s) and res[3] == len(want)
        assert all(e["flags"] == COMPLETE for e in want)
    got, res, n = emu_index(emu, b"")
    assert len(got) == 0 and res == (0, 0, 0, 0) and n == 0
    sized = [e["content_size"] for e in hold(emu, b"".join(p))[0]]
    assert sized[20:25] == [len(d) for d in inputs()] and set(sized[:20] + sized[25:]) == {NO_SIZE}


def test_dictionary_stream(emu):
    dct = synth.gen_text_zipf(3, 70000).tobytes()
    frames = [mk(d, block_size=64 << 10, dictionary=dct, dictionary_id=9, independent_blocks=bool(i % 2)) for i, d in enumerate(inputs())]
    want, res = hold(emu, b"".join(frames), dictionary=dct)
    assert res == (0, sum(len(d) for d in inputs()), sum(len(f) for f in frames), len(frames))


def test_an_ending_frame_first_in_the_middle_and_last(emu):
    """A damaged block and a bad block checksum end the stream where they are; the structural walk goes on, so the frames behind
    are listed, behind the stop."""
    p = good_frames()
    good = [p[0], p[8], p[13], p[21], p[1]]
    kinds = set()
    for bad in damaged_frames():
        for at in (0, 2, 4):
            fr = list(good)
            fr[at] = bad
            want, res = hold(emu, b"".join(fr), name=f"bad at {at}")
            kinds.add(res[0])
            assert len(want) == 5 and res[0] != 0 and res[3] == at
            assert [bool(e["flags"] & BEHIND) for e in want] == [k > at for k in range(5)]
            assert [bool(e["flags"] & COMPLETE) for e in want] == [k != at for k in range(5)]
            assert all(e["out_off"] == res[1] for e in want[at + 1:])
    assert 19 in kinds and kinds & {1, 2, 3, 4}, kinds


def test_truncated_last_frame_and_trailing_bytes(emu):
    p = good_frames()
    two = p[3] + p[12]
    last = p[18]
    for cut in (1, 5, 7, len(last) // 2, len(last) - 4, len(last) - 1):
        want, res = hold(emu, two + last[:cut], name=f"cut {cut}")
        assert res[0] == 16 and res[2] == len(two) + cut and res[3] == 2 and len(want) == 3 and want[2]["flags"] == 0
    for tail in (b"\x04", b"\x04\x22", b"\x04\x22\x4d"):
        want, res = hold(emu, two + tail, name=str(tail))
        assert (res[0], res[2], res[3]) == (16, len(two) + len(tail), 2) and len(want) == 3
        assert (want[2]["status"], want[2]["out_len"], want[2]["consumed"], want[2]["content_size"]) == (16, 0, len(tail), NO_SIZE)
    for tail in (b"\x00\x00\x00\x00", b"\x00" * 7, b"\x50\x2a\x4d\x18\x04\x00\x00\x00abcd", b"\x02\x21\x4c\x18" + b"\x00" * 9):
        want, res = hold(emu, two + tail, name=str(tail))
        assert (res[0], res[2], res[3]) == (17, len(two) + 4, 2) and len(want) == 3          # listed as a frame
        assert (want[2]["status"], want[2]["consumed"], want[2]["flags"]) == (17, 4, 0)
    for tail in (b"\x01", b"\x00" * 5):                     # ... and in front of everything: the ending frame is the first
        want, res = hold(emu, tail + two)
        assert len(want) == 1 and res[3] == 0 and res[1] == 0


def test_capacity_in_the_serial_driver(emu):
    s = b"".join(good_frames()[:7])
    full, res, n = emu_index(emu, s)
    assert n == 7
    for cap in (0, 1, 6, 7, 12):
        got, r, found = emu_index(emu, s, cap=cap)
        assert (r, found) == (res, 7) and len(got) == min(cap, 7) and (got == full[:len(got)]).all()


# ---- locate ---------------------------------------------------------------------------------------------------------------

def make_index(lens, stop=None):
    """An index of frames of `lens` output bytes; `stop`: the frame that ends the stream."""
    ix = np.zeros(len(lens), dtype=device.SFRAME)
    run = 0
    for k, n in enumerate(lens):
        behind = stop is not None and k > stop
        ix[k] = (100 * k, 100, run, n, NO_SIZE, 19 if k == stop else 0, (0 if k == stop else COMPLETE) | (BEHIND if behind else 0))
        if not behind:
            run += n
    return ix


def rows(ix):
    return [(int(e["out_off"]), int(e["out_len"]), int(e["flags"])) for e in ix]


def brute(rws, a, b):
    hit = [k for k, (off, n, fl) in enumerate(rws) if not fl & BEHIND and n and off < b and off + n > a]
    return (hit[0], hit[-1] - hit[0] + 1) if hit and a < b else (0, 0)


INDEXES = [make_index([]), make_index([10]), make_index([0]), make_index([0, 0, 0]), make_index([5, 0, 0, 7, 1, 0, 300, 0]),
           make_index([0, 4, 4, 0]), make_index([3, 9, 2, 6, 8], stop=2), make_index([3, 9, 0, 6, 8], stop=2), make_index([7, 1], stop=0),
           make_index(list(range(1, 41)), stop=39), make_index([2, 0] * 33)]


def ranges(ix):
    edges = sorted({0} | {int(e["out_off"]) for e in ix} | {int(e["out_off"] + e["out_len"]) for e in ix})
    pts = sorted({max(0, e + d) for e in edges for d in (-1, 0, 1)} | {edges[-1] + 1000})
    return [(a, b) for a in pts for b in pts]


def test_locate_in_the_emulator_against_brute_force(emu):
    checked = 0
    for ix in INDEXES:
        rws = rows(ix)
        for a, b in ranges(ix):
            first, count = C.c_uint64(7), C.c_uint64(7)
            emu.lzf_emu_stream_locate(ix.ctypes.data if len(ix) else None, len(ix), a, b, C.byref(first), C.byref(count))
            assert (first.value, count.value) == brute(rws, a, b), (ix["out_len"].tolist(), a, b)
            checked += 1
    assert checked > 5000


def test_locate_in_the_product_library(lib):
    """Host code: no device needed.  The same cases, with a >= b, n = 0 and a range wholly behind the output among them."""
    for ix in INDEXES:
        rws = rows(ix)
        total = max((off + n for off, n, _ in rws), default=0)
        for a, b in ranges(ix) + [(total, total + 5), (total + 5, total + 9), (3, 3), (4, 2), (0, 1 << 63), (0, (1 << 64) - 1)]:
            first, count = C.c_size_t(7), C.c_size_t(7)
            assert lib.lzf_stream_index_locate(ix.ctypes.data if len(ix) else None, len(ix), a, b, C.byref(first), C.byref(count)) == 0
            assert (first.value, count.value) == brute(rws, a, b), (ix["out_len"].tolist(), a, b)
            if a >= b or a >= total or len(ix) == 0:
                assert count.value == 0
    first = C.c_size_t()
    assert lib.lzf_stream_index_locate(None, 0, 0, 1, None, C.byref(first)) == ffi.E_INVALID
    assert lib.lzf_stream_index_locate(None, 3, 0, 1, C.byref(first), C.byref(first)) == ffi.E_INVALID
