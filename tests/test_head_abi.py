"""The head call's ABI (no GPU): lzf_decompress_head_batch and lzf_decompress_head_batch_host are declared by include/lzfear_hip.h,
exported by the product and the analysis library, bound by ffi.py and the Rust sys crate, check their arguments and fail loudly
without a device.  Fails on a tree without the feature."""
import ctypes as C
import os

import pytest

import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import build, device, ffi
from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lzf_decompress_head_batch", "lzf_decompress_head_batch_host")


@pytest.fixture(scope="module")
def libs():
    build.build_library()
    return ffi.lib(), C.CDLL(build.build_analysis_library())


def test_entry_points_declared_exported_and_bound(libs):
    hip = declared_functions("lzfear_hip.h")
    for n in NAMES:
        assert n in hip and n in ffi.EXPORTS
        for L in libs:
            assert hasattr(L, n), n
    assert libs[0].lzf_abi_version() == 2
    for n in ("decompress_head_batch", "decompress_head_batch_long_history", "block_heads"):
        assert callable(getattr(device, n))
    assert callable(ffi.block_heads_host)
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "lz-fear-hip-sys", "src", "lib.rs")).read()
    safe_rs = open(os.path.join(ROOT, "bindings", "rust", "lz-fear-hip", "src", "lib.rs")).read()
    for n in NAMES:
        assert f"pub fn {n}(" in sys_rs, n
    assert "lzf_decompress_head_batch_host" in safe_rs
    assert "lz4_decode_head.hip" in build.PRODUCT_HIP and "capi_head.hip" in build.PRODUCT_HIP and "lzf_head_rules.h" in build.HEADERS


def test_argument_checks(libs):
    """NULL arrays with work to do are refused, an empty call is LZF_OK — with or without a device."""
    lib = libs[0]
    assert lib.lzf_decompress_head_batch(None, None, 1, None) == ffi.E_INVALID
    assert lib.lzf_decompress_head_batch_host(None, None, 1) == ffi.E_INVALID
    assert lib.lzf_decompress_head_batch(None, None, 0, None) == ffi.OK
    assert lib.lzf_decompress_head_batch_host(None, None, 0) == ffi.OK
    assert ffi.block_heads_host([]) == []


def test_no_device_no_fallback(libs):
    """Without a HIP device the calls fail with LZF_E_NO_DEVICE: there is no CPU path."""
    lib = libs[0]
    if lib.lzf_device_count() > 0:
        pytest.skip("a GPU is present; the loud-failure path is for GPU-less hosts")
    buf = C.create_string_buffer(16)
    addr = C.cast(buf, C.c_void_p).value
    jobs = (ffi.DecompressJob * 1)()
    jobs[0].input = addr; jobs[0].input_len = 16; jobs[0].out = addr; jobs[0].out_cap = 16; jobs[0].output_limit = 1 << 20
    res = (ffi.JobResult * 1)()
    assert lib.lzf_decompress_head_batch(C.addressof(jobs), C.addressof(res), 1, None) == ffi.E_NO_DEVICE
    assert lib.lzf_decompress_head_batch_host(jobs, res, 1) == ffi.E_NO_DEVICE
