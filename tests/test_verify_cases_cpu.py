"""CPU tests (no GPU) of the verify call (lzf_decompress_verify_batch, lzf_decompress_verify_batch_host): the entry points are
declared and exported, check their arguments and fail loudly without a device; and the rule the kernel runs
(rust-lz-fear_amd/csrc/lzf_verify_rules.h), compiled here with g++ as its serial reference function, gives on every case of
verify_cases.py what decode-then-compare by the oracle gives, without reading a byte outside the job's three buffers."""
import ctypes as C
import os
import subprocess

import pytest

import verify_cases as cases
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import build, ffi, framed
from test_abi import declared_functions

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("lzf_decompress_verify_batch", "lzf_decompress_verify_batch_host", "lzf_last_verify_launch")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return ffi.lib()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("verify") / "libemu_verify.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so, os.path.join(HERE, "emu", "emu_verify.cpp")])
    L = C.CDLL(so)
    L.lzf_emu_verify.restype = C.c_int
    L.lzf_emu_verify.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]

    def run(c, origin=0):
        n, outside = C.c_uint64(0), C.c_uint64(0)
        rc = L.lzf_emu_verify(c["input"], len(c["input"]), c["prefix"], c["prefix_len"], c["mem"], origin, c["existing_len"] + origin,
                              c["out_cap"] + origin, c["limit"] + origin, C.byref(n), C.byref(outside))
        assert outside.value == 0, (c["name"], "a byte outside input, prefix or out[0, out_cap) was read")
        return rc, (n.value - origin if rc in (0, cases.MISMATCH) else None)
    return run


@pytest.fixture(scope="module")
def rows():
    r = cases.block_cases()
    cases.assert_covers(r)
    return r


def test_entry_points_declared_and_exported(lib):
    """Fails on a tree without the feature."""
    hip = declared_functions("lzfear_hip.h")
    for n in NAMES:
        assert n in hip and n in ffi.EXPORTS
        assert hasattr(lib, n), n
    assert lib.lzf_abi_version() == 2
    assert ffi.MISMATCH == cases.MISMATCH == 8 and framed.FRAME_ERRORS[8] == "Mismatch"
    assert "#define LZF_MISMATCH 8" in open(os.path.join(HERE, "..", "include", "lzfear_hip.h")).read()


def test_argument_checks(lib):
    """NULL arrays with work to do are refused, an empty call is LZF_OK — with or without a device."""
    assert lib.lzf_decompress_verify_batch(None, None, 1, 0, None) == ffi.E_INVALID
    assert lib.lzf_decompress_verify_batch_host(None, None, 1) == ffi.E_INVALID
    assert lib.lzf_decompress_verify_batch(None, None, 0, 0, None) == ffi.OK
    assert lib.lzf_decompress_verify_batch_host(None, None, 0) == ffi.OK


def test_no_device_no_fallback(lib):
    """Without a HIP device the calls fail with LZF_E_NO_DEVICE: there is no CPU path."""
    if lib.lzf_device_count() > 0:
        pytest.skip("a GPU is present; the loud-failure path is for GPU-less hosts")
    buf = C.create_string_buffer(16)
    addr = C.cast(buf, C.c_void_p).value
    jobs = (ffi.DecompressJob * 1)()
    jobs[0].input = addr; jobs[0].input_len = 16; jobs[0].out = addr; jobs[0].out_cap = 16; jobs[0].output_limit = 1 << 20
    res = (ffi.JobResult * 1)()
    assert lib.lzf_decompress_verify_batch(C.addressof(jobs), C.addressof(res), 1, 16, None) == ffi.E_NO_DEVICE
    assert lib.lzf_decompress_verify_batch_host(jobs, res, 1) == ffi.E_NO_DEVICE


def test_verify_rules_match_decode_then_compare(emu, rows):
    """lzf_verify_rules.h's serial reference function on every case: the size call's status first, else LZF_MISMATCH with the first
    differing position (or the shorter length), else LZF_OK — the oracle's decode compared by numpy."""
    for c, exp in rows:
        if exp[0] == cases.CONTRACT:
            continue                                   # (a length without a buffer: below)
        assert emu(c) == exp, c["name"]


def test_verify_rules_contract(emu):
    """Lengths of 2 GiB - 256 and more are LZF_CONTRACT, whatever the bytes, and nothing is read."""
    c = dict(name="contract", input=b"\x50hello", prefix=b"", prefix_len=0, existing_len=0, mem=b"hellx", out_cap=5, limit=100)
    assert emu(c) == (cases.MISMATCH, 4)
    assert emu(dict(c, prefix_len=0x7FFFFF00)) == (cases.CONTRACT, None)
    assert emu(dict(c, existing_len=0x7FFFFF00, out_cap=0x7FFFFF05)) == (cases.CONTRACT, None)


def test_verify_rules_behind_a_gib_of_history(emu, rows):
    """Positions beyond 2^30: the cases without a prefix, restated with their origin 1 GiB + 5 bytes further on — the way a trimmed
    job (lzf_history_trim.h) sees a long history, and 64-bit positions all the way.  Only memory from the origin on exists."""
    origin = (1 << 30) + 5
    some = [(c, e) for c, e in rows if c["prefix_len"] == 0 and e[0] in (0, cases.MISMATCH) and c["existing_len"] >= 65535][:6]
    some += [(c, e) for c, e in rows if c["name"].startswith("match/source in the existing output")]
    assert len(some) >= 12
    for c, exp in some:
        # an offset never reaches further back than 65 535 bytes; these cases' matches stay within their own history
        assert emu(c, origin=origin) == exp, c["name"]


def test_frame_entry_point_and_frame_cases(lib):
    """lzf_frame_verify_device is declared and exported and checks its arguments; the frame cases of the GPU test cover every
    verdict (their expectations are the oracle's frame decode compared by numpy)."""
    assert "lzf_frame_verify_device" in declared_functions("lzfear_frame.h") and "lzf_frame_verify_device" in ffi.FRAME_EXPORTS
    assert lib.lzf_frame_verify_device(1, None, None, None, 0, None, None, None, None, None, None) == ffi.E_INVALID
    assert lib.lzf_frame_verify_device(0, None, None, None, 0, None, None, None, None, None, None) == ffi.OK
    cases.assert_frames_cover(cases.frame_cases())


ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def plan_emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vplan") / "libemu_verify_dispatch.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(HERE, "emu", "emu_verify_dispatch.cpp")])
    L = C.CDLL(so)
    L.lzf_emu_verify_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_char_p)]
    L.lzf_emu_verify_layout.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]

    def plan(cu, n, max_in, mode=0, lds=160 << 10):
        out, strs = (C.c_uint32 * 3)(), (C.c_char_p * 2)()
        L.lzf_emu_verify_plan(cu, lds, mode, n, max_in, out, strs)
        return bool(out[0]), out[1], strs[0].decode(), strs[1].decode()

    def layout(n, max_in):
        out = (C.c_uint64 * 6)()
        L.lzf_emu_verify_layout(n, max_in, out)
        return list(out)
    return plan, layout


def _design_table():
    """The verify call's class table of DESIGN.md: {name: number}."""
    import re
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("#### The verify call's classes"):]
    sec = sec[:sec.index("\n\n", sec.index("|---"))]
    rows = {}
    for line in sec.splitlines():
        m = re.match(r"\| `(\w+)` \| ([\d ]+) \|", line)
        if m:
            rows[m.group(1)] = int(m.group(2).replace(" ", ""))
    return rows


def test_verify_plan_and_layout_follow_the_design_table(plan_emu):
    """verify_plan takes the class by the table's three numbers — jobs per CU, the input bound, the scratch cap — and by the analysis
    knob; verify_layout is the size layout plus 8 bytes per tile and 8 per job, each area 256-aligned."""
    plan, layout = plan_emu
    T = _design_table()
    assert T == dict(jobs_per_cu=16, min_input_bound=65536, max_scratch=3 << 30, bytes_per_tile=8, bytes_per_job=8), T
    ANY = (1 << 64) - 1
    for cu in (256, 304, 8):
        edge = T["jobs_per_cu"] * cu
        for n in (1, 49, edge - 1, edge, edge + 1, 5 * edge):
            for max_in in (0, T["min_input_bound"] - 1, T["min_input_bound"], 1 << 20, 4 << 20, ANY):
                size_total, o_base, o_min, total, maxtile, size_again = layout(n, max_in)
                up = lambda v: (v + 255) // 256 * 256      # noqa: E731
                assert size_total == size_again and o_base == size_total and o_min == o_base + up(T["bytes_per_tile"] * n * maxtile)
                assert total == o_min + up(T["bytes_per_job"] * n)
                fits = total <= T["max_scratch"] and n <= 65535
                want = n <= edge and max_in >= T["min_input_bound"] and fits
                got = plan(cu, n, max_in)
                assert got[0] == want and got[1] == T["min_input_bound"], (cu, n, max_in, got)
                assert plan(cu, n, max_in, mode=2)[0] is False
                assert plan(cu, n, max_in, mode=1)[0] == (max_in >= T["min_input_bound"] and fits)
    p = plan(256, 49, ANY)
    assert p[2].startswith("latency: ") and "lzf_verify_tile_kernel" in p[2] and p[2].endswith(p[3]) and p[3] == "lzf_verify_kernel<48,768>"


def test_class_cases_preconditions():
    """The class cases build (the builder asserts input_len >= 65536 and LZF_OK in the oracle for every case but the error job) and
    hold every verdict the class must give or leave."""
    rows = cases.class_cases()
    kinds = {e[0] for _, e in rows}
    assert {0, cases.MISMATCH, 3} <= kinds and len(rows) >= 25
    for c, e in rows:
        if "tile's output" in c["name"] or "tile before" in c["name"]:
            assert e[0] == cases.MISMATCH
