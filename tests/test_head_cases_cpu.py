"""CPU tests (no GPU) of the head call (lzf_decompress_head_batch, lzf_decompress_head_batch_host): the rule the kernel runs
(rust-lz-fear_amd/csrc/lzf_head_rules.h), compiled here with g++ as its serial reference function, gives on every case of
head_cases.py what the oracle's decode cut at the target gives — status, length and bytes — without touching a byte outside the
job's buffers; on every small clean case at every target; over more than a GiB of history, directly and through the trim."""
import ctypes as C
import os
import subprocess

import pytest

import head_cases as cases
import rust_lz_fear_amd  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ZONE = 64
POISON = 0xA5


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("head") / "libemu_head.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(HERE, "emu", "emu_head.cpp")])
    L = C.CDLL(so)
    L.lzf_emu_head.restype = C.c_int
    L.lzf_emu_head.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int,
                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]

    def run(c, target=None, trim=False, shift_out=None):
        """(status, out_len or None, bytes or None) of the case (at `target` instead of its own), lengths relative to the origin; the
        memory behind the room and the existing output must come back untouched."""
        t = c["target"] if target is None else target
        ex, origin = len(c["existing"]), c["origin"]
        rm = cases.room(dict(c, target=t))
        mem = C.create_string_buffer(c["existing"] + bytes([POISON]) * (rm + ZONE), ex + rm + ZONE)
        n, outside, shift = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = L.lzf_emu_head(c["input"], len(c["input"]), c["prefix"], c["prefix_len"], C.addressof(mem), origin, origin + ex, origin + t,
                            origin + c["limit"], int(trim), C.byref(n), C.byref(outside), C.byref(shift))
        assert outside.value == 0, (c["name"], t, "a byte outside input, prefix, out[0, out_cap) was read or one outside out[existing, out_cap) written")
        raw = mem.raw
        assert raw[:ex] == c["existing"] and raw[ex + rm:] == bytes([POISON]) * ZONE, (c["name"], t, "written outside the room")
        if shift_out is not None:
            shift_out.append(shift.value)
        if rc != 0:
            return rc, None, None
        ln = n.value - origin
        assert raw[max(ln, ex):ex + rm] == bytes([POISON]) * (ex + rm - max(ln, ex)), (c["name"], t, "written at or beyond out_len")
        return 0, ln, raw[ex:ln]
    return run


@pytest.fixture(scope="module")
def rows():
    r = cases.all_cases()
    cases.assert_covers(r)
    return r


def test_constants_are_the_kernels():
    """The case file builds its blocks from what the sources say: one parse covers 64 x 48 bytes and lists 768 tokens, a round is 64
    tokens, a lane moves runs of up to 64 bytes by itself, the wave 1 KiB a step."""
    assert cases.header_constants() == dict(CHUNK=3072, TOKCAP=768, ROUND=64, OWN=64, STEP=1024)
    assert cases.N_FF > cases.CHUNK


def test_head_rules_meet_every_expectation(emu, rows):
    """Fails on a tree without the feature (there is no lzf_head_rules.h to compile)."""
    for c, exp in rows:
        assert emu(c) == exp, c["name"]


def test_head_rules_at_every_target_of_the_small_clean_cases(emu, rows):
    """Every clean block that decodes to at most 2 KiB, at every target from out_existing_len to one past its end: D[:t]."""
    seen, n = set(), 0
    for c, _ in rows:
        key = (c["input"], c["prefix"], c["existing"], c["limit"], c["origin"])
        if key in seen or c["cls"] == "i":                       # (a length in contract: nothing is decoded)
            continue
        seen.add(key)
        ex = len(c["existing"])
        rc, dec = cases._oracle(c["input"], c["prefix"], c["existing"], c["limit"])
        if rc != 0 or len(dec) - ex > cases.SWEEP_MAX:
            continue
        for t in range(ex, len(dec) + 2):
            assert emu(c, target=t) == (0, min(t, len(dec)), dec[ex:t]), (c["name"], t)
        n += 1
    assert n >= 40, n


def test_head_rules_behind_a_gib_of_history_and_through_the_trim(emu, rows):
    """Class (j): jobs with more than 1 GiB of existing output, stated over their last bytes — directly (64-bit positions all the
    way) and trimmed and restored by lzf_history_trim.h's rule, which moves the target with the origin."""
    some = [(c, e) for c, e in rows if c["cls"] == "j"]
    assert len(some) >= 15
    for c, exp in some:
        assert emu(c) == exp, c["name"]
        shifts = []
        assert emu(c, trim=True, shift_out=shifts) == exp, c["name"]
        assert shifts[0] > 0 and shifts[0] % 16 == 0 and 65536 <= c["origin"] + len(c["existing"]) - shifts[0] <= 65551, c["name"]
    # a short history is not trimmed, and a target below the existing output holds the trim back
    c = next(c for c, _ in rows if c["cls"] == "b" and c["sub"] == "existing")
    shifts = []
    emu(c, trim=True, shift_out=shifts)
    assert shifts == [0]


def test_contract_lengths(emu, rows):
    """Lengths of 2 GiB - 256 and more are LZF_CONTRACT whatever the target, and nothing is read or written."""
    for c, exp in rows:
        if c["cls"] == "i":
            assert exp == (cases.CONTRACT, None, None) and emu(c) == exp, c["name"]
    c = dict(next(c for c, _ in rows if c["cls"] == "i" and c["sub"] == "prefix"), target=0)
    assert emu(c) == (cases.CONTRACT, None, None)
