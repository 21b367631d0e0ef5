"""The history trim on the CPU: rust-lz-fear_amd/csrc/lzf_history_trim.h compiled with g++ (tests/emu/emu_history_trim.cpp) and held to
its rule at the lengths where the decode kernels' 31-bit positions and 32-bit arithmetic could bite, and the rule itself — restated in
tests/history_trim_cases.py with the threshold as a parameter — held to the oracle: decompress_raw of the trimmed job plus restore
equals decompress_raw of the original job, on histories small enough to decode here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_ffi as o
import history_trim_cases as H
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import ffi, synth

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "rust-lz-fear_amd", "csrc")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    assert os.path.exists(os.path.join(CSRC, "lzf_history_trim.h")), "the rule's header is missing"
    so = str(tmp_path_factory.mktemp("trim") / "libemu_history_trim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so, os.path.join(HERE, "emu", "emu_history_trim.cpp")])
    L = C.CDLL(so)
    L.lzf_emu_trim_shift.restype = C.c_uint64
    L.lzf_emu_trim_shift.argtypes = [C.c_uint64, C.c_uint64]
    L.lzf_emu_trim.restype = None
    L.lzf_emu_trim.argtypes = [C.POINTER(ffi.DecompressJob), C.POINTER(ffi.DecompressJob), C.POINTER(C.c_uint64)]
    L.lzf_emu_restore.restype = None
    L.lzf_emu_restore.argtypes = [C.POINTER(ffi.JobResult), C.c_uint64]
    return L


LENGTHS = ((1 << 30) - 1, 1 << 30, (1 << 30) + 15, 0x7FFFFF00 - 1, 0x7FFFFF00, 0x7FFFFF00 + 1, 1 << 31, (1 << 32) - 1, (1 << 32) + 12345, 1 << 40)
FIELDS = ("input", "input_len", "prefix", "prefix_len", "out", "out_existing_len", "out_cap", "output_limit")


def _emu_trim(emu, **kw):
    j, t, s = ffi.DecompressJob(), ffi.DecompressJob(), C.c_uint64(0xDEAD)
    for k, v in kw.items():
        setattr(j, k, v)
    emu.lzf_emu_trim(C.byref(j), C.byref(t), C.byref(s))
    return {f: getattr(t, f) or 0 for f in FIELDS}, s.value


def test_the_header_at_every_length_where_positions_could_wrap(emu):
    out = 0x7F00_0000_0123                      # (any address: & 15 = 3)
    for E in LENGTHS:
        cap = E + (4 << 20) + 70000
        want = 0 if E < (1 << 30) else (E - 65536) & ~15
        assert emu.lzf_emu_trim_shift(E, cap) == want == H.shift_of(E, cap), hex(E)
        if want:
            assert want % 16 == 0 and 65536 <= E - want <= 65551, hex(E)
        # limits below, at and above the shift (the decoder's limit counts from position 0, as out_existing_len does)
        for limit in (0, 1, max(want, 1) - 1, want, want + 1, E, E + (4 << 20), (1 << 63) - 1):
            job = dict(input=0x1000, input_len=777, prefix=0x2000, prefix_len=99, out=out, out_existing_len=E, out_cap=cap, output_limit=limit)
            got, s = _emu_trim(emu, **job)
            model, ms = H.trim(job)
            assert s == ms == want and got == model, (hex(E), limit)
            assert got["out"] == out + want and got["out"] & 15 == out & 15
            assert (got["out_existing_len"], got["out_cap"]) == (E - want, cap - want)
            assert got["output_limit"] == (limit - want if limit > want else 0)
            assert [got[f] for f in FIELDS[:4]] == [0x1000, 777, 0x2000, 99]
        # more existing output than room: the decoder's LZF_CONTRACT, left for it to say
        job = dict(input=0x1000, input_len=5, prefix=0, prefix_len=0, out=out, out_existing_len=E, out_cap=E - 1, output_limit=E + 9)
        got, s = _emu_trim(emu, **job)
        assert s == 0 and got == job, hex(E)
        # no output (the size calls): NULL stays NULL
        got, s = _emu_trim(emu, out=None, out_existing_len=E, out_cap=cap, output_limit=E + 5)
        assert s == want and got["out"] == 0


def test_restore_adds_the_shift_to_ok_results_only(emu):
    for status in range(0, 8):
        r = ffi.JobResult(out_len=70000, status=status, reserved=0xABCD)
        emu.lzf_emu_restore(C.byref(r), (1 << 33) + 16)
        assert (r.out_len, r.status, r.reserved) == (70000 + ((1 << 33) + 16 if status == 0 else 0), status, 0xABCD)
        assert H.restore(status, 70000, 16) == (status, 70016 if status == 0 else 70000)


# ---- the rule against the oracle, with a threshold that histories of a few hundred KiB pass -------------------------------------
T = 65536


def _history(n, seed):
    return synth.silesia_mix(seed << 16, (seed << 16) + n).tobytes()


def _both(block, existing, limit, prefix=b""):
    """(original, trimmed + restored) as (status, out_len, bytes from the shift on)."""
    E = len(existing)
    cap = E + 400000
    job = dict(out=0, out_existing_len=E, out_cap=cap, output_limit=limit)
    t, s = H.trim(job, threshold=T)
    assert s == ((E - 65536) & ~15 if E >= T else 0)
    rc0, out0 = o.decompress_raw(block, prefix, existing, limit, cap)
    rc1, out1 = o.decompress_raw(block, prefix, existing[s:], t["output_limit"], t["out_cap"])
    assert len(existing[s:]) == t["out_existing_len"]
    st, n = H.restore(rc1, len(out1), s)
    return (rc0, len(out0), out0[s:]), (st, n if st == 0 else len(out1) + s, out1), s


EXISTING = (65536, 65537, 65551, 65552, 70001, 131072 + 5, 300000)


@pytest.mark.parametrize("E", EXISTING)
def test_trimmed_job_plus_restore_is_the_original_job(E):
    existing = _history(E, 7)
    prefix = _history(1000, 99)
    lit = bytes(range(40, 60))
    s = H.shift_of(E, threshold=T)
    blocks = {
        "offset 1": H.seq(lit, 1, 300) + H.seq(b"tail!"),
        "offset 65535 at the first position": H.seq(b"", 65535, 70000) + H.seq(b"tail!"),
        "offset 65535 behind literals": H.seq(lit, 65535, 4) + H.seq(b"tail!"),
        "offset as deep as the trimmed history allows": H.seq(b"", min(E - s, 65535), 5000) + H.seq(b"tail!"),
        "a match that straddles the end of the history": H.seq(b"", 10, 100) + H.seq(b"ab", 50, 200) + H.seq(b"tail!"),
        "zero offset": H.seq(lit, 0, 8) + H.seq(b"tail!"),
        "truncated inside the literals": (H.seq(lit, 65535, 40) + H.seq(b"0123456789"))[:-4],
        "truncated inside a length": H.seq(lit, 3, 4000)[:-1],
    }
    for name, b in blocks.items():
        for pre in (b"", prefix):
            a, t, _ = _both(b, existing, (1 << 63) - 1, pre)
            assert a == t, (name, E, len(pre))
        # the prefix is out of reach on both sides: the same answer without it
        assert _both(b, existing, (1 << 63) - 1, prefix)[0] == _both(b, existing, (1 << 63) - 1)[0], name
    assert _both(blocks["zero offset"], existing, (1 << 63) - 1)[0][0] == o.ZERO_DEDUP_OFFSET
    assert _both(blocks["truncated inside a length"], existing, (1 << 63) - 1)[0][0] == o.UNEXPECTED_END
    assert _both(blocks["offset 65535 at the first position"], existing, (1 << 63) - 1)[0][:2] == (o.OK, E + 70005)


@pytest.mark.parametrize("E", EXISTING)
def test_memory_limit_on_either_side_of_the_shift(E):
    existing = _history(E, 11)
    s = H.shift_of(E, threshold=T)
    b = H.seq(b"abc", 1000, 500) + H.seq(b"xyz", 7, 64) + H.seq(b"tail!")
    first, second = E + 3 + 500, E + 3 + 500 + 3 + 64          # the two match ends: MemoryLimitExceeded where one is beyond the limit
    seen = set()
    for limit in (0, max(s, 1) - 1, s, s + 1, s + 7, E, first - 1, first, second - 1, second, second + 5):
        a, t, _ = _both(b, existing, limit)
        assert a == t, (E, limit)
        assert a[0] == (o.MEMORY_LIMIT_EXCEEDED if limit < second else o.OK), (E, limit)
        seen.add((limit < s, limit == first, limit == second))
    assert (True, False, False) in seen or s == 0
    assert a[1] == second + 5


def test_below_the_threshold_nothing_changes():
    for E in (0, 1, 65535):
        existing = _history(E, 3)
        a, t, s = _both(H.seq(b"literals", 3, 40) + H.seq(b"tail!"), existing, (1 << 63) - 1, _history(70000, 5))
        assert s == 0 and a == t and a[0] == o.OK
    job = dict(out=4096, out_existing_len=H.THRESHOLD - 1, out_cap=1 << 40, output_limit=5)
    assert H.trim(job) == (job, 0)
