"""CPU tests (no GPU) of lzf_frame_compress_device_many (include/lzfear_frame.h, "frames in device memory"): the entry point is
declared and exported, refuses bad arguments before it looks for a device, fails loudly without one, and the frame layout rule its
assembly kernel runs (rust-lz-fear_amd/csrc/lzf_frame_layout.h), compiled here with g++, builds lzf_frame_assemble's bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import build, ffi
from test_abi import declared_functions

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "lzf_frame_compress_device_many"
OUTPUT_FULL, CONTRACT = 5, 6


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return ffi.lib()


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("layout") / "libemu_frame_layout.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-o", so,
                           os.path.join(HERE, "emu", "emu_frame_layout.cpp")])
    L = C.CDLL(so)
    L.lzf_emu_frame_layout.restype = C.c_int
    L.lzf_emu_frame_layout.argtypes = [C.POINTER(ffi.Settings), C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32),
                                       C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return L


def settings(lib, combo, block_size):
    s = ffi.Settings()
    lib.lzf_settings_default(C.byref(s))
    s.independent_blocks, s.block_checksums, s.content_checksum = combo & 1, (combo >> 1) & 1, (combo >> 2) & 1
    s.has_dictionary_id, s.dictionary_id = (combo >> 3) & 1, 0xC0FFEE11
    s.has_content_size, s.content_size = (combo >> 4) & 1, 0x123456789A
    s.block_size = block_size
    return s


def args(n, ptrs=True):
    buf = C.create_string_buffer(64)
    p = (C.c_void_p * n)(*[C.addressof(buf)] * n)
    ln = (C.c_size_t * n)(*[16] * n)
    res = (C.c_uint64 * n)()
    return buf, p, ln, res


def test_entry_point_declared_and_exported(lib):
    assert NAME in declared_functions("lzfear_frame.h")
    assert NAME in ffi.FRAME_EXPORTS
    assert hasattr(lib, NAME)
    assert lib.lzf_abi_version() == 2


def test_invalid_arguments_before_the_device(lib):
    """NULL arrays with n_frames > 0 and a host dictionary in the settings are refused on any host, GPU or not."""
    s = settings(lib, 7, 64 << 10)
    keep, p, ln, res = args(2)
    call = lib.lzf_frame_compress_device_many
    assert call(None, 2, p, ln, None, 0, p, ln, res, res, None) == ffi.E_INVALID
    assert call(C.byref(s), 2, None, ln, None, 0, p, ln, res, res, None) == ffi.E_INVALID
    assert call(C.byref(s), 2, p, None, None, 0, p, ln, res, res, None) == ffi.E_INVALID
    assert call(C.byref(s), 2, p, ln, None, 0, None, ln, res, res, None) == ffi.E_INVALID
    assert call(C.byref(s), 2, p, ln, None, 0, p, None, res, res, None) == ffi.E_INVALID
    assert call(C.byref(s), 2, p, ln, None, 0, p, ln, None, res, None) == ffi.E_INVALID
    assert call(C.byref(s), 2, p, ln, None, 0, p, ln, res, None, None) == ffi.E_INVALID
    d = C.create_string_buffer(b"dictionary bytes")
    s.dictionary, s.dictionary_len = C.addressof(d), 16
    assert call(C.byref(s), 2, p, ln, None, 0, p, ln, res, res, None) == ffi.E_INVALID
    assert call(C.byref(s), 0, None, None, None, 0, None, None, None, None, None) == ffi.E_INVALID


def test_no_device_no_fallback(lib):
    """Without a HIP device the call fails with LZF_E_NO_DEVICE: there is no CPU path."""
    if lib.lzf_device_count() > 0:
        pytest.skip("a GPU is present; the loud-failure path is for GPU-less hosts")
    s = settings(lib, 7, 64 << 10)
    keep, p, ln, res = args(1)
    assert lib.lzf_frame_compress_device_many(C.byref(s), 1, p, ln, None, 0, p, ln, res, res, None) == ffi.E_NO_DEVICE
    assert lib.lzf_frame_compress_device_many(C.byref(s), 0, None, None, None, 0, None, None, None, None, None) == ffi.E_NO_DEVICE


def assemble(lib, s, payloads, comp_len, raw_len, content):
    n = len(payloads)
    cap = 64 + sum(len(p) + 8 for p in payloads)
    out = C.create_string_buffer(cap)
    olen = C.c_size_t(0)
    pp = (C.c_void_p * max(n, 1))(*[C.cast(p, C.c_void_p).value for p in payloads])
    rc = lib.lzf_frame_assemble(C.byref(s), n, pp, (C.c_uint32 * max(n, 1))(*comp_len), (C.c_uint32 * max(n, 1))(*raw_len),
                                content, out, cap, C.byref(olen))
    assert rc == 0
    return out.raw[:olen.value]


def test_layout_rule_builds_lzf_frame_assemble_bytes(lib, layout):
    """All 32 combinations of independent blocks, block checksums, content checksum, dictionary id and content size, random
    block results (compressed lengths, stored blocks, empty frames) and the four block sizes: the layout header places header,
    length words, payloads, checksum words and EndMark where lzf_frame_assemble does, byte for byte; a block whose status is
    neither LZF_OK nor LZF_OUTPUT_FULL fails the frame with the first such status."""
    rng = np.random.default_rng(2024)
    checked = failed = 0
    for combo in range(32):
        for trial in range(12):
            bs = [64 << 10, 256 << 10, 1 << 20, 4 << 20][trial % 4]
            s = settings(lib, combo, bs)
            nb = int(rng.integers(0, 7)) if trial else 0
            raw_len = [int(rng.integers(1, 3000)) for _ in range(nb)]
            raws = [C.create_string_buffer(rng.integers(0, 256, r, dtype=np.uint8).tobytes(), r) for r in raw_len]
            stored = [bool(rng.integers(0, 3) == 0) for _ in range(nb)]
            out_len = [0 if st else int(rng.integers(0, r + 1)) for st, r in zip(stored, raw_len)]
            comps = [C.create_string_buffer(rng.integers(0, 256, max(o, 1), dtype=np.uint8).tobytes(), max(o, 1)) for o in out_len]
            status = [OUTPUT_FULL if st else 0 for st in stored]
            bad = nb and trial % 5 == 4
            if bad:
                for i in sorted(rng.choice(nb, size=min(nb, 2), replace=False).tolist()):
                    status[i] = CONTRACT if status[i] == 0 else 1 + i % 4
            payloads = [raws[i] if stored[i] else comps[i] for i in range(nb)]
            lens = [raw_len[i] if stored[i] else out_len[i] for i in range(nb)]
            sums = [lib.lzf_xxh32(C.string_at(payloads[i], lens[i]), lens[i], 0) for i in range(nb)]
            content = int(rng.integers(0, 1 << 32))
            out = C.create_string_buffer(64 + sum(lens) + 8 * nb)
            flen = C.c_uint64(0)
            pos = (C.c_uint64 * max(nb, 1))()
            arr = lambda T, v: (T * max(nb, 1))(*v)
            st = layout.lzf_emu_frame_layout(C.byref(s), nb, arr(C.c_int32, status), arr(C.c_uint64, out_len), arr(C.c_uint32, raw_len),
                                             arr(C.c_void_p, [C.addressof(c) for c in comps]), arr(C.c_void_p, [C.addressof(r) for r in raws]),
                                             arr(C.c_uint32, sums), content, out, C.byref(flen), pos)
            first_bad = next((x for x in status if x not in (0, OUTPUT_FULL)), 0)
            assert st == first_bad, (combo, trial)
            if st:
                assert flen.value == 0
                failed += 1
                continue
            want = assemble(lib, s, payloads, [0xFFFFFFFF if stored[i] else out_len[i] for i in range(nb)], raw_len, content)
            assert out.raw[:flen.value] == want, (combo, trial)
            hdr = 7 + 8 * s.has_content_size + 4 * s.has_dictionary_id
            expect, w = [], hdr
            for i in range(nb):
                expect.append(w)
                w += 4 + lens[i] + 4 * s.block_checksums
            assert list(pos)[:nb] == expect
            checked += 1
    assert checked > 250 and failed > 20, (checked, failed)
