"""CPU tests (no GPU) of the device frame layer (include/lzfear_frame.h, "frames in device memory"): the two entry points are
declared and exported, fail loudly without a device, and the scan they run on the device (rust-lz-fear_amd/csrc/lzf_frame_scan.h),
compiled here with g++, walks every file of the decode corpus like the host driver's scan_blocks and reports the reference's
header / walk errors with the reference's `consumed`."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import build, ffi
from test_abi import declared_functions
from test_oracle import fuzz_corpus

HERE = os.path.dirname(os.path.abspath(__file__))
SCAN_H = os.path.join(os.path.dirname(HERE), "rust-lz-fear_amd", "csrc", "lzf_frame_scan.h")
NAMES = ("lzf_frame_decompress_bound_device", "lzf_frame_decompress_device_many")
# the statuses a header parse or the block walk decides (decompress.rs:18-35, header.rs:19-28)
SCAN_KINDS = {16, 17, 18, 22, 23, 24, 25, 26}


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return ffi.lib()


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("scan") / "libemu_frame_scan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so,
                           os.path.join(HERE, "emu", "emu_frame_scan.cpp")])
    L = C.CDLL(so)
    L.lzf_emu_frame_scan.restype = C.c_int
    L.lzf_emu_frame_scan.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint64]

    def run(data):
        cap = len(data) // 4 + 8
        out = (C.c_uint64 * (7 + 5 * cap))()
        L.lzf_emu_frame_scan(data, len(data), out, cap)
        nb = out[6]
        assert nb <= cap
        blocks = [tuple(out[7 + 5 * k: 12 + 5 * k]) for k in range(nb)]
        return dict(hdr=(out[0], out[1]), walk=(out[2], out[3], bool(out[4]), out[5]), blocks=blocks)
    return run


def test_entry_points_declared_and_exported(lib):
    names = declared_functions("lzfear_frame.h")
    for n in NAMES:
        assert n in names and n in ffi.FRAME_EXPORTS
        assert hasattr(lib, n), n
    assert lib.lzf_abi_version() == 2


def test_no_device_no_fallback(lib):
    """Without a HIP device both calls fail with LZF_E_NO_DEVICE: there is no CPU path."""
    if lib.lzf_device_count() > 0:
        pytest.skip("a GPU is present; the loud-failure path is for GPU-less hosts")
    ptr = (C.c_void_p * 1)(C.cast(C.create_string_buffer(16), C.c_void_p).value)
    ln = (C.c_size_t * 1)(16)
    bound = (C.c_size_t * 1)()
    assert lib.lzf_frame_decompress_bound_device(1, ptr, ln, bound, None) == ffi.E_NO_DEVICE
    res = (C.c_uint64 * 3)()
    assert lib.lzf_frame_decompress_device_many(1, ptr, ln, None, 0, ptr, ln, res, res, res, None) == ffi.E_NO_DEVICE


def py_scan_blocks(data, header_len, flags, bmax):
    """frame.cpp's scan_blocks (decompress.rs:205-235), restated: [(off, len, compressed, want_sum, end_off)], (err, consumed)."""
    r, n, out = header_len, len(data), []
    u32 = lambda p: struct.unpack_from("<I", data, p)[0]
    while True:
        if n - r < 4:
            return out, (16, n)
        bl = u32(r); r += 4
        if bl == 0:
            if flags & 0x04:
                if n - r < 4:
                    return out, (16, n)
                r += 4
            return out, (0, r)
        comp = 0 if bl & 0x80000000 else 1
        bl &= 0x7FFFFFFF
        if bl > bmax:
            return out, (22, r)
        if n - r < bl:
            return out, (16, n)
        off = r; r += bl
        want = 0
        if flags & 0x10:
            if n - r < 4:
                return out, (16, n)
            want = u32(r); r += 4
        out.append((off, bl, comp, want, r))


def test_scan_header_walks_the_decode_corpus_like_the_host(scan):
    """All 830 packed decode-corpus files: the g++-compiled device scan finds the blocks the host's scan_blocks finds, and where
    the reference stops in the header parse or the block walk, with its status and its `consumed`."""
    files = fuzz_corpus("decode")
    assert len(files) == 830
    checked = walked = 0
    for name, data in files:
        got = scan(data)
        hst, hcons = got["hdr"]
        erc, _, eused = o.frame_decompress(data, cap=8 << 20)
        if hst == 0:
            flags, bd = data[4], data[5]
            header_len = 7 + (8 if flags & 0x08 else 0) + (4 if flags & 0x01 else 0)
            bmax = 1 << (((bd >> 4) & 7) * 2 + 8)
            blocks, (werr, wcons) = py_scan_blocks(data, header_len, flags, bmax)
            assert got["blocks"] == blocks, name
            assert got["walk"][:2] == (werr, wcons), name
            walked += 1
        if erc in SCAN_KINDS:
            if hst != 0:
                assert (hst, hcons) == (erc, eused), name
            elif erc != 22 or got["walk"][0] == 22:           # (22 also comes from a block that decodes beyond block_maxsize)
                assert got["walk"][:2] == (erc, eused), name
            checked += 1
    assert checked > 400 and walked > 100, (checked, walked)
