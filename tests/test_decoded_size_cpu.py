"""CPU tests (no GPU) of the decoded-size query (lzf_decompressed_size_batch, lzf_decompressed_size_batch_host,
lzf_frame_decompressed_size_device): the entry points are declared and exported, check their arguments and fail loudly without
a device; and the arithmetic the size kernel runs per token (rust-lz-fear_amd/csrc/lzf_size_rules.h), compiled here with g++
into a serial driver, gives the oracle's decompress_raw status and output.len() on blocks of every DecodeError kind."""
import ctypes as C
import os
import subprocess

import pytest

import decoded_size_cases as cases
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import build, ffi
from test_abi import declared_functions

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK_NAMES = ("lzf_decompressed_size_batch", "lzf_decompressed_size_batch_host")
FRAME_NAME = "lzf_frame_decompressed_size_device"


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return ffi.lib()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dsize") / "libemu_decoded_size.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so,
                           os.path.join(HERE, "emu", "emu_decoded_size.cpp")])
    L = C.CDLL(so)
    L.lzf_emu_decoded_size.restype = C.c_int
    L.lzf_emu_decoded_size.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]

    def run(case):
        n = C.c_uint64(0)
        rc = L.lzf_emu_decoded_size(case["input"], len(case["input"]), case["prefix_len"], case["existing_len"], case["limit"], C.byref(n))
        return rc, (n.value if rc == 0 else None)
    return run


def test_entry_points_declared_and_exported(lib):
    """Fails on a tree without the feature."""
    hip, frame = declared_functions("lzfear_hip.h"), declared_functions("lzfear_frame.h")
    for n in BLOCK_NAMES:
        assert n in hip and n in ffi.EXPORTS
        assert hasattr(lib, n), n
    assert FRAME_NAME in frame and FRAME_NAME in ffi.FRAME_EXPORTS
    assert hasattr(lib, FRAME_NAME)
    assert lib.lzf_abi_version() == 2


def test_argument_checks(lib):
    """NULL arrays with work to do are refused, an empty call is LZF_OK — with or without a device."""
    assert lib.lzf_decompressed_size_batch(None, None, 1, 0, None) == ffi.E_INVALID
    assert lib.lzf_decompressed_size_batch_host(None, None, 1) == ffi.E_INVALID
    assert lib.lzf_frame_decompressed_size_device(1, None, None, 0, None, None, None, None) == ffi.E_INVALID
    assert lib.lzf_decompressed_size_batch(None, None, 0, 0, None) == ffi.OK
    assert lib.lzf_decompressed_size_batch_host(None, None, 0) == ffi.OK
    assert lib.lzf_frame_decompressed_size_device(0, None, None, 0, None, None, None, None) == ffi.OK


def test_no_device_no_fallback(lib):
    """Without a HIP device the three calls fail with LZF_E_NO_DEVICE: there is no CPU path."""
    if lib.lzf_device_count() > 0:
        pytest.skip("a GPU is present; the loud-failure path is for GPU-less hosts")
    buf = C.create_string_buffer(16)
    addr = C.cast(buf, C.c_void_p).value
    jobs = (ffi.DecompressJob * 1)()
    jobs[0].input = addr; jobs[0].input_len = 16; jobs[0].output_limit = 1 << 20
    res = (ffi.JobResult * 1)()
    assert lib.lzf_decompressed_size_batch(C.addressof(jobs), C.addressof(res), 1, 16, None) == ffi.E_NO_DEVICE
    assert lib.lzf_decompressed_size_batch_host(jobs, res, 1) == ffi.E_NO_DEVICE
    ptr = (C.c_void_p * 1)(addr)
    ln = (C.c_size_t * 1)(16)
    out = (C.c_uint64 * 3)()
    assert lib.lzf_frame_decompressed_size_device(1, ptr, ln, 0, out, out, out, None) == ffi.E_NO_DEVICE


def test_size_rules_match_the_oracle(emu):
    """lzf_size_rules.h, token by token on the CPU: decompress_raw's status, and output.len() when Ok, for the liblz4 HC
    fixtures, valid blocks, the mutated-block recipe (seed 12345, both limits) and the prefix / existing-output sweep."""
    blocks = cases.block_cases()
    cases.assert_all_kinds(blocks)
    assert len(blocks) > 200
    for name, case, exp in blocks:
        assert emu(case) == exp, name


def test_size_rules_lengths_beyond_32_bits(emu):
    """A match length of more than 2^32 (0xFF bytes cost nothing to count) keeps its 64-bit value; the limit check sees it."""
    n_ff = 17_000_000
    blk = bytes([0x1F]) + b"a" + (1).to_bytes(2, "little") + b"\xff" * n_ff + bytes([7])
    want = 1 + 4 + 15 + 255 * n_ff + 7
    assert want > 1 << 32
    big = dict(input=blk, prefix_len=0, existing_len=0, limit=(1 << 63) - 1)
    assert emu(big) == (0, want)
    assert emu(dict(big, limit=want)) == (0, want)
    assert emu(dict(big, limit=want - 1)) == (2, None)
