"""CPU tests (no GPU) of the device frame layer (include/lzfear_frame.h, "frames in device memory"): the two entry points are
declared and exported, fail loudly without a device, and the frame layer's one walk (rust-lz-fear_amd/csrc/lzf_frame_scan.h: the
device scan kernels and the host driver both run it), compiled here with g++, walks every file of the decode corpus like the
restatement of the block walk below and reports the reference's header / walk errors with the reference's `consumed`; the built
library's lzf_frame_read_header, a wrapper of that header parse, agrees with it and with a parse of the bytes written here."""
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
    """The block walk of decode_block (decompress.rs:205-235), restated independently of lzf_frame_scan.h:
    [(off, len, compressed, want_sum, end_off)], (err, consumed)."""
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
    """All 830 packed decode-corpus files: the g++-compiled walk finds the blocks the restated walk finds, and where the
    reference stops in the header parse or the block walk, with its status and its `consumed`."""
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


def py_header(data):
    """The fields of a header that parses, read from the bytes (decompress.rs:102-161; FLG, BD, [content size], [dictionary id], HC)."""
    flags, bd, p = data[4], data[5], 6
    size = did = 0
    if flags & 0x08:
        size = struct.unpack_from("<Q", data, p)[0]; p += 8
    if flags & 0x01:
        did = struct.unpack_from("<I", data, p)[0]; p += 4
    return dict(flags=flags, bd=bd, block_maxsize=1 << (((bd >> 4) & 7) * 2 + 8), header_len=p + 1,
                has_content_size=int(bool(flags & 0x08)), content_size=size, has_dictionary_id=int(bool(flags & 0x01)), dictionary_id=did)


def lib_header(lib, data):
    info = ffi.FrameInfo()
    rc = lib.lzf_frame_read_header(data, len(data), C.byref(info))
    return rc, {k: getattr(info, k) for k in ("flags", "bd", "block_maxsize", "header_len", "has_content_size", "content_size",
                                              "has_dictionary_id", "dictionary_id")}


def test_read_header_is_the_walk_headers_parse(lib, scan):
    """lzf_frame_read_header of the built library (it loads without a device) over all 830 decode-corpus files: its status is
    the g++-compiled lzf_scan::read_header's; where the reference stops in the header, that status and that `consumed` are the
    reference's; where the header parses, every field of lzf_frame_info equals the parse of the bytes above."""
    files = fuzz_corpus("decode")
    assert len(files) == 830
    parsed = failed = with_size = with_id = 0
    for name, data in files:
        hst, hcons = scan(data)["hdr"]
        rc, info = lib_header(lib, data)
        assert rc == hst, name
        if hst != 0:
            erc, _, eused = o.frame_decompress(data, cap=8 << 20)
            if erc in SCAN_KINDS:                             # (a header error is the first thing the reference can report)
                assert (rc, hcons) == (erc, eused), name
                failed += 1
            continue
        want = py_header(data)
        assert info == want, name
        parsed += 1; with_size += want["has_content_size"]; with_id += want["has_dictionary_id"]
    assert parsed > 100 and failed > 50 and with_size and with_id, (parsed, failed, with_size, with_id)


def test_read_header_every_optional_field_and_every_cut(lib, scan):
    """The four combinations of content size and dictionary id, written by the reference's compressor: fields from the bytes, and
    the walk header's status for every truncation of the header and for every single-byte change of it."""
    for size, did in ((None, None), (0x1122334455, None), (None, 0xA1B2C3D4), (0x0102030405060708, 7)):
        st = o.make_settings(block_size=64 << 10, content_size=size, dictionary_id=did, dictionary_id_override=did is not None)
        erc, frame = o.frame_compress(b"header fields " * 10, st)
        assert erc == 0
        rc, info = lib_header(lib, frame)
        want = py_header(frame)
        assert rc == 0 and info == want
        assert (want["has_content_size"], want["has_dictionary_id"]) == (int(size is not None), int(did is not None))
        assert want["content_size"] == (size or 0) and want["dictionary_id"] == (did or 0)
        hl = want["header_len"]
        for cut in range(hl + 1):
            rc, _ = lib_header(lib, frame[:cut])
            assert rc == scan(frame[:cut])["hdr"][0] == (16 if cut < hl else 0), cut
        for at in range(hl):
            for flip in (0x01, 0x40, 0x80):
                bad = bytearray(frame); bad[at] ^= flip; bad = bytes(bad)
                rc, info = lib_header(lib, bad)
                assert rc == scan(bad)["hdr"][0], (at, flip)
                if rc == 0:
                    assert info == py_header(bad), (at, flip)
