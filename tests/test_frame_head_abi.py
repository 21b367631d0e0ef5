"""The frame head call's ABI (no GPU): lzf_frame_head_device is declared by include/lzfear_frame.h, exported by the product and the
analysis library, bound by ffi.py and the Rust sys crate, its sources and headers are in build.py's lists, it checks its arguments
and fails loudly without a device.  Fails on a tree without the feature."""
import ctypes as C
import os

import pytest

import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import build, device, ffi, framed
from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lzf_frame_head_device"


@pytest.fixture(scope="module")
def libs():
    build.build_library()
    return ffi.lib(), C.CDLL(build.build_analysis_library())


def _args(n, in_ptr, in_len, out_ptr, target):
    return ((C.c_void_p * n)(*[in_ptr] * n), (C.c_size_t * n)(*[in_len] * n), (C.c_void_p * n)(*[out_ptr] * n), (C.c_size_t * n)(*[target] * n))


def test_entry_point_declared_exported_and_bound(libs):
    assert NAME in declared_functions("lzfear_frame.h") and NAME in ffi.FRAME_EXPORTS
    for L in libs:
        assert hasattr(L, NAME)
    assert libs[0].lzf_abi_version() == 2
    assert libs[0].lzf_frame_head_device.argtypes is not None and len(libs[0].lzf_frame_head_device.argtypes) == 10
    for n in ("frame_head_raw", "frame_heads"):
        assert callable(getattr(device, n))
    for n in ("frame_heads_device", "stream_frame_heads_device"):
        assert callable(getattr(framed, n))
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "lz-fear-hip-sys", "src", "lib.rs")).read()
    assert f"pub fn {NAME}(" in sys_rs
    assert "frame_device_head.hip" in build.PRODUCT_HIP
    for h in ("lzf_frame_head_rules.h", "lz4_decode_head_walk.inc", "lz4_decode_head_copies.inc"):
        assert h in build.HEADERS and os.path.exists(os.path.join(build.CSRC, h)), h


def test_one_walk_for_both_head_kernels():
    """The raw head kernel and the frame head kernel include the same walk and the same copies: neither source holds a copy."""
    for src in ("lz4_decode_head.hip", "frame_device_head.hip"):
        text = open(os.path.join(build.CSRC, src)).read()
        assert '#include "lz4_decode_head_walk.inc"' in text and '#include "lz4_decode_head_copies.inc"' in text, src
        assert "wave_scan_add64" not in text and "__device__ __forceinline__ void wave_match" not in text, src


def test_argument_checks(libs):
    """NULL arrays with work to do are refused, as is a NULL output with a target; an empty call is LZF_OK — with or without a device."""
    lib = libs[0]
    buf = C.create_string_buffer(64)
    addr = C.cast(buf, C.c_void_p).value
    ins, lens, outs, tgs = _args(1, addr, 16, addr, 8)
    assert lib.lzf_frame_head_device(0, None, None, None, 0, None, None, None, None, None) == ffi.OK
    assert lib.lzf_frame_head_device(1, None, None, None, 0, None, None, None, None, None) == ffi.E_INVALID
    for hole in range(6):
        a = [ins, lens, outs, tgs, addr, addr]
        a[hole] = None
        assert lib.lzf_frame_head_device(1, a[0], a[1], None, 0, a[2], a[3], a[4], a[5], None) == ffi.E_INVALID, hole
    null_out = _args(1, addr, 16, None, 8)
    assert lib.lzf_frame_head_device(1, null_out[0], null_out[1], None, 0, null_out[2], null_out[3], addr, addr, None) == ffi.E_INVALID
    null_in = _args(1, None, 16, addr, 8)
    assert lib.lzf_frame_head_device(1, null_in[0], null_in[1], None, 0, null_in[2], null_in[3], addr, addr, None) == ffi.E_INVALID


def test_no_device_no_fallback(libs):
    """Without a HIP device the call fails with LZF_E_NO_DEVICE: there is no CPU path."""
    lib = libs[0]
    if lib.lzf_device_count() > 0:
        pytest.skip("a GPU is present; the loud-failure path is for GPU-less hosts")
    buf = C.create_string_buffer(64)
    addr = C.cast(buf, C.c_void_p).value
    ins, lens, outs, tgs = _args(1, addr, 16, addr + 32, 8)
    assert lib.lzf_frame_head_device(1, ins, lens, None, 0, outs, tgs, addr, addr, None) == ffi.E_NO_DEVICE
    zero = _args(1, addr, 16, None, 0)                       # (a NULL output is fine where nothing is asked for)
    assert lib.lzf_frame_head_device(1, zero[0], zero[1], None, 0, zero[2], zero[3], addr, addr, None) == ffi.E_NO_DEVICE
