"""CPU tests (no GPU) of the block index of a frame and of the block-run decode's host side (include/lzfear_frame.h:
lzf_frame_block_count_device / lzf_frame_block_index_device / lzf_block_index_locate / lzf_frame_decompress_blocks_device).

The rules the index kernel and the host run (rust-lz-fear_amd/csrc/lzf_block_index.h: the placement around the stop, the entry
fill, the run validation, locate), compiled here with g++ and driven serially in rounds of 64 (tests/emu/emu_block_index.cpp), are
held to tests/block_index_cases.py's expected index — the oracle decoding every block behind a host walk — which is itself held
to the oracle's decompress_frame; locate, in the emulator and in the product library (host code: no device needed), to a linear
scan; the stream locate, which now shares its search with the block locate, to the cases of tests/test_stream_index_cpu.py.
The stop rules are not emulated here: they are device code (frame_deliver_body.inc), the serial driver is told which block stops
the reader, and the body's index-mode control flow is covered by tests/test_gpu_block_index.py alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import block_index_cases as bc
import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import build, device, ffi
from test_abi import declared_functions
import test_stream_index_cpu as sic

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("lzf_frame_block_count_device", "lzf_frame_block_index_device", "lzf_block_index_locate", "lzf_frame_decompress_blocks_device")
STORED, HAS_SUM, LINKED, DELIVERED, BEHIND = bc.STORED, bc.HAS_SUM, bc.LINKED, bc.DELIVERED, bc.BEHIND_STOP


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return ffi.lib()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bindex") / "libemu_block_index.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(HERE, "..", "include"),
                           "-o", so, os.path.join(HERE, "emu", "emu_block_index.cpp")])
    L = C.CDLL(so)
    L.lzf_emu_block_index.restype = None
    L.lzf_emu_block_index.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    L.lzf_emu_check_run.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    L.lzf_emu_run_total.restype = C.c_uint64
    L.lzf_emu_run_total.argtypes = [C.c_void_p, C.c_uint64]
    for f in (L.lzf_emu_block_locate, L.lzf_emu_stream_locate2):
        f.restype = None
        f.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return L


def case_frames():
    """(name, frame, dictionary) of every frame the GPU tests index."""
    dct = bc.dictionary_bytes()
    out = [(f"{n} blocks, checksums {bool(n % 2)}", bc.good_frame(n, block_checksums=bool(n % 2), content_checksum=bool(n % 3)), b"") for n in bc.COUNTS]
    out += [(f"{n} blocks behind a dictionary", bc.good_frame(n, seed=1, dictionary=dct, block_checksums=True), dct) for n in (2, 65)]
    out += [(f"{kind} at {at}", bc.stop_frame(kind, at), b"") for kind in bc.STOP_KINDS for at in bc.STOP_PLACES]
    out += [("linked", bc.linked_frame(), b""), ("linked, dictionary, checksums", bc.linked_frame(150_000, dictionary=dct, block_checksums=True), dct)]
    return out


def emu_index(emu, frame, dictionary=b"", cap=None):
    """The expected per-block facts (walk, status, length, whether the delivery stops there) through the serial driver."""
    want, _ = bc.ref_index(frame, dictionary)
    n = len(want)
    blk = np.zeros((max(n, 1), 8), dtype=np.uint64)
    stopped = False
    for k, e in enumerate(want):
        stops = not stopped and (e["status"] != 0 or e["out_len"] == 0)
        blk[k] = (e["in_off"], e["in_len"], bool(e["flags"] & STORED), bool(e["flags"] & HAS_SUM), e["want_sum"], e["status"] & 0xFFFFFFFFFFFFFFFF,
                  e["out_len"], stops)
        stopped = stopped or stops
    cap = n if cap is None else cap
    out = np.zeros(max(cap, n) + 2, dtype=device.FBLOCK)
    out["reserved"] = 0xDEAD
    res = np.zeros(2, dtype=np.uint64)
    linked = bool(want and want[0]["flags"] & LINKED)
    emu.lzf_emu_block_index(blk.ctypes.data, n, bc.BMAX, int(linked), out.ctypes.data, cap, res.ctypes.data)
    assert (out["reserved"][min(cap, n):] == 0xDEAD).all()              # nothing behind min(cap, n) entries
    return out[:min(cap, n)], (int(res[0]), int(res[1])), want


# ---- the ABI ---------------------------------------------------------------------------------------------------------------

def test_entry_points_declared_exported_and_loud_without_a_device(lib):
    names = declared_functions("lzfear_frame.h")
    for n in NAMES:
        assert n in names and n in ffi.FRAME_EXPORTS
        assert hasattr(lib, n), n
    assert lib.lzf_abi_version() == 2
    assert C.sizeof(ffi.FrameBlock) == 48 == device.FBLOCK.itemsize
    assert [device.FBLOCK.fields[n][1] for n, _ in ffi.FrameBlock._fields_] == [getattr(ffi.FrameBlock, n).offset for n, _ in ffi.FrameBlock._fields_]
    assert tuple(n for n, _ in ffi.FrameBlock._fields_) == bc.FIELDS == device.FBLOCK.names
    assert (ffi.FBLOCK_STORED, ffi.FBLOCK_HAS_SUM, ffi.FBLOCK_LINKED, ffi.FBLOCK_DELIVERED, ffi.FBLOCK_BEHIND_STOP) == (1, 2, 4, 8, 16)
    ptr = (C.c_void_p * 1)(C.cast(C.create_string_buffer(64), C.c_void_p).value)
    ln = (C.c_size_t * 1)(16)
    found = (C.c_size_t * 1)()
    res = (C.c_uint64 * 4)()
    a = C.addressof(res)
    assert lib.lzf_frame_block_count_device(1, ptr, ln, None, None) == ffi.E_INVALID
    assert lib.lzf_frame_block_index_device(1, ptr, ln, 0, None, None, None, a, a, None, None) == ffi.E_INVALID
    assert lib.lzf_frame_block_index_device(1, ptr, ln, 0, ptr, None, a, a, a, None, None) == ffi.E_INVALID      # d_index without index_cap
    odd = (C.c_void_p * 1)(ptr[0] + 4)
    assert lib.lzf_frame_block_index_device(1, ptr, ln, 0, odd, ln, a, a, a, None, None) == ffi.E_INVALID        # an entry address off its 8 bytes
    assert lib.lzf_frame_decompress_blocks_device(1, ptr, ln, None, ln, None, 0, ptr, ln, a, a, None) == ffi.E_INVALID
    if lib.lzf_device_count() > 0:
        return                                    # (the loud-failure half is for GPU-less hosts)
    assert lib.lzf_frame_block_count_device(1, ptr, ln, found, None) == ffi.E_NO_DEVICE
    assert lib.lzf_frame_block_index_device(1, ptr, ln, 0, None, None, a, a, a, a, None) == ffi.E_NO_DEVICE
    zero = (C.c_size_t * 1)(0)
    assert lib.lzf_frame_decompress_blocks_device(1, ptr, ln, ptr, zero, None, 0, ptr, ln, a, a, None) == ffi.E_NO_DEVICE


# ---- the cases -------------------------------------------------------------------------------------------------------------

def test_census_every_flag_every_stop_kind_and_the_round_boundary():
    flags, stops, counts = bc.census()
    assert flags == STORED | HAS_SUM | LINKED | DELIVERED | BEHIND
    assert stops == {19, 1, 2, 3, 4, 22, "empty", "walk 16"}
    assert set(bc.COUNTS) <= counts and {63, 64, 65, 130} <= counts     # both sides of a round of 64, and a third round
    for kind in bc.STOP_KINDS:
        for at in bc.STOP_PLACES:
            entries, (st, n, used) = bc.ref_index(bc.stop_frame(kind, at))
            if kind == "truncated":
                assert len(entries) == at and st == 16 and all(e["flags"] & DELIVERED for e in entries)
                continue
            assert len(entries) == 130
            assert [bool(e["flags"] & DELIVERED) for e in entries] == [k < at for k in range(130)], (kind, at)
            assert [bool(e["flags"] & BEHIND) for e in entries] == [k > at for k in range(130)], (kind, at)
            assert all(e["out_off"] == n for e in entries[at:]) and n == sum(e["out_len"] for e in entries[:at])
    good = bc.ref_index(bc.good_frame(130))[0]
    assert sum(bool(e["flags"] & STORED) for e in good) >= 19 and not all(e["flags"] & STORED for e in good)


def test_the_expected_index_is_the_oracles_frame_decode():
    """ref_index's frame results and delivered bytes against decompress_frame of the oracle, on every case frame."""
    for name, f, dct in case_frames():
        entries, res = bc.ref_index(f, dct)
        rc, out, used = o.frame_decompress(f, dictionary=dct, cap=16 << 20)
        if rc == 20:                                                   # (none of the cases: content checksums are sound)
            rc = 0
        assert res == (rc, len(out), used), name
        assert b"".join(e["plain"] for e in entries if e["flags"] & DELIVERED) == out, name
        assert len(entries) == len(bc.walk(f)["blocks"])


# ---- entries ---------------------------------------------------------------------------------------------------------------

def test_entries_and_behind_stop_placement_in_the_serial_driver(emu):
    for name, f, dct in case_frames():
        got, (w, stop_at), want = emu_index(emu, f, dct)
        _, (st, out_len, _) = bc.ref_index(f, dct)
        assert len(got) == len(want) and w == out_len, name
        stops = [k for k, e in enumerate(want) if not e["flags"] & DELIVERED]
        assert stop_at == (stops[0] if stops else len(want)), name
        for k, (g, e) in enumerate(zip(got, want)):
            for fld in bc.FIELDS:
                assert int(g[fld]) == e[fld], (name, k, fld)
        if stops:
            assert int(got[stops[0]]["status"]) == st, name             # the stopping block carries the frame's status


def test_capacity_in_the_serial_driver(emu):
    f = bc.stop_frame("codec 3", 64)
    full, res, want = emu_index(emu, f)
    assert len(full) == 130
    for cap in (0, 1, 63, 64, 65, 129, 130, 135):
        got, r, _ = emu_index(emu, f, cap=cap)
        assert r == res and len(got) == min(cap, 130) and (got == full[:len(got)]).all()


# ---- run validation --------------------------------------------------------------------------------------------------------

def py_check_run(run, frame_len):
    for k, e in enumerate(run):
        fl = int(e["flags"])
        if not fl & DELIVERED:
            return 1
        if fl & LINKED:
            return 2
        if int(e["in_off"]) + int(e["in_len"]) + (4 if fl & HAS_SUM else 0) > frame_len:
            return 3
        if int(e["in_len"]) > int(e["block_maxsize"]):
            return 4
        if int(e["out_len"]) > int(e["block_maxsize"]):
            return 5
        if fl & STORED and int(e["out_len"]) != int(e["in_len"]):
            return 6
        if k + 1 < len(run) and (int(run[k + 1]["out_off"]) - int(e["out_off"])) % (1 << 64) != int(e["out_len"]):
            return 7
    return 0


def as_array(entries):
    a = np.zeros(len(entries), dtype=device.FBLOCK)
    for k, e in enumerate(entries):
        a[k] = tuple(e[f] for f in bc.FIELDS)
    return a


def bad_runs():
    """(reason, run, frame_len): a sound run of 70 blocks with checksums, and one change each that the call must refuse."""
    f = bc.good_frame(130, block_checksums=True)
    ix = as_array(bc.ref_index(f)[0])
    run = ix[30:100].copy()
    out = [(0, run.copy(), len(f)), (0, ix[:0].copy(), len(f)), (0, ix[129:130].copy(), len(f))]

    def change(reason, k, frame_len=len(f), **kw):
        r = run.copy()
        for fld, v in kw.items():
            r[k][fld] = v
        out.append((reason, r, frame_len))
    change(1, 0, flags=int(run[0]["flags"]) & ~DELIVERED)
    change(1, 69, flags=HAS_SUM | BEHIND)
    change(2, 33, flags=int(run[33]["flags"]) | LINKED)
    change(3, 69, frame_len=int(run[69]["in_off"]) + int(run[69]["in_len"]) + 3)          # the checksum word would lie beyond the frame
    change(0, 69, frame_len=int(run[69]["in_off"]) + int(run[69]["in_len"]) + 4)
    change(3, 5, in_off=(1 << 64) - 8)
    change(3, 5, in_off=len(f) + 1)
    change(4, 7, in_len=bc.BMAX + 1, frame_len=1 << 40)
    change(5, 7, out_len=bc.BMAX + 1)
    stored = next(k for k in range(70) if run[k]["flags"] & STORED)
    change(6, stored, out_len=int(run[stored]["out_len"]) - 1)
    change(7, 20, out_off=int(run[20]["out_off"]) + 1)
    packed = next(k for k in range(40, 69) if not run[k]["flags"] & STORED)
    change(7, packed, out_len=int(run[packed]["out_len"]) - 1)
    change(7, 69, out_off=0)
    return out


def test_run_validation_every_reason_against_the_model(emu, lib):
    seen = set()
    for reason, run, frame_len in bad_runs():
        assert py_check_run(run, frame_len) == reason
        assert emu.lzf_emu_check_run(run.ctypes.data if len(run) else None, len(run), frame_len) == reason, reason
        seen.add(reason)
        if reason == 0:
            assert emu.lzf_emu_run_total(run.ctypes.data if len(run) else None, len(run)) == int(run["out_len"].sum())
            continue
        # the product refuses the call before it looks for a device, and enqueues nothing
        buf = C.create_string_buffer(64)
        ptr = (C.c_void_p * 1)(C.cast(buf, C.c_void_p).value)
        ln, cnt, cap = (C.c_size_t * 1)(frame_len), (C.c_size_t * 1)(len(run)), (C.c_size_t * 1)(1 << 40)
        rp = (C.c_void_p * 1)(run.ctypes.data)
        res = (C.c_uint64 * 2)()
        assert lib.lzf_frame_decompress_blocks_device(1, ptr, ln, rp, cnt, None, 0, ptr, cap, C.addressof(res), C.addressof(res), None) == ffi.E_INVALID
    assert seen == set(range(8))
    linked = as_array(bc.ref_index(bc.linked_frame())[0])
    assert len(linked) >= 3 and emu.lzf_emu_check_run(linked.ctypes.data, len(linked), 1 << 30) == 2


# ---- locate ----------------------------------------------------------------------------------------------------------------

def make_index(lens, stop=None):
    """An index of blocks of `lens` output bytes; `stop`: the block that stops the frame (not delivered; its own length does
    not count)."""
    ix = np.zeros(len(lens), dtype=device.FBLOCK)
    run = 0
    for k, n in enumerate(lens):
        place = DELIVERED if stop is None or k < stop else 0 if k == stop else BEHIND
        ix[k] = (100 * k, run, n, 90, 0, 65536, 3 if k == stop else 0, place, 0)
        if place == DELIVERED:
            run += n
    return ix


def rows(ix):
    return [(int(e["out_off"]), int(e["out_len"]), int(e["flags"])) for e in ix]


def linear(rws, a, b):
    hit = [k for k, (off, n, fl) in enumerate(rws) if fl & DELIVERED and n and off < b and off + n > a]
    return (hit[0], hit[-1] - hit[0] + 1) if hit and a < b else (0, 0)


INDEXES = [make_index([]), make_index([10]), make_index([0]), make_index([0, 0, 0]), make_index([5, 0, 0, 7, 1, 0, 300, 0]),
           make_index([0, 4, 4, 0]), make_index([3, 9, 2, 6, 8], stop=2), make_index([3, 9, 0, 6, 8], stop=2), make_index([7, 1], stop=0),
           make_index([4, 0, 0, 5, 9], stop=3), make_index(list(range(1, 41)), stop=39), make_index([2, 0] * 70), make_index([1] * 130, stop=64)]


def ranges(ix):
    edges = sorted({0} | {int(e["out_off"]) for e in ix} | {int(e["out_off"] + e["out_len"]) for e in ix})
    if len(edges) > 40:
        edges = edges[:12] + edges[60:70] + edges[-12:]
    pts = sorted({max(0, e + d) for e in edges for d in (-1, 0, 1)} | {edges[-1] + 1000})
    return [(a, b) for a in pts for b in pts]


def test_block_locate_in_the_emulator_and_the_product_against_a_linear_scan(emu, lib):
    checked = 0
    for ix in INDEXES:
        rws = rows(ix)
        total = max((off + n for off, n, fl in rws if fl & DELIVERED), default=0)
        p = ix.ctypes.data if len(ix) else None
        for a, b in ranges(ix) + [(total, total + 5), (total + 5, total + 9), (3, 3), (4, 2), (0, 1 << 63), (0, (1 << 64) - 1)]:
            want = linear(rws, a, b)
            first, count = C.c_uint64(7), C.c_uint64(7)
            emu.lzf_emu_block_locate(p, len(ix), a, b, C.byref(first), C.byref(count))
            assert (first.value, count.value) == want, (ix["out_len"].tolist(), a, b)
            f2, c2 = C.c_size_t(7), C.c_size_t(7)
            assert lib.lzf_block_index_locate(p, len(ix), a, b, C.byref(f2), C.byref(c2)) == 0
            assert (f2.value, c2.value) == want, (ix["out_len"].tolist(), a, b)
            if a >= b or a >= total or len(ix) == 0:
                assert count.value == 0
            elif count.value:                                           # blocks of zero length are never at an edge
                assert rws[first.value][1] and rws[first.value + count.value - 1][1]
            checked += 1
    assert checked > 5000
    first = C.c_size_t()
    assert lib.lzf_block_index_locate(None, 0, 0, 1, None, C.byref(first)) == ffi.E_INVALID
    assert lib.lzf_block_index_locate(None, 3, 0, 1, C.byref(first), C.byref(first)) == ffi.E_INVALID


def test_block_locate_on_built_frames(emu):
    for name, f, dct in case_frames()[:9] + [("stop", bc.stop_frame("codec 1", 64), b"")]:
        ix = as_array(bc.ref_index(f, dct)[0])
        rws = rows(ix)
        for a, b in ranges(ix)[::7]:
            first, count = C.c_uint64(7), C.c_uint64(7)
            emu.lzf_emu_block_locate(ix.ctypes.data if len(ix) else None, len(ix), a, b, C.byref(first), C.byref(count))
            assert (first.value, count.value) == linear(rws, a, b), (name, a, b)


def test_the_stream_locate_is_unchanged(emu, lib):
    """The cases of tests/test_stream_index_cpu.py through the search the two locates now share."""
    checked = 0
    for ix in sic.INDEXES:
        rws = sic.rows(ix)
        p = ix.ctypes.data if len(ix) else None
        for a, b in sic.ranges(ix) + [(3, 3), (4, 2), (0, 1 << 63), (0, (1 << 64) - 1)]:
            first, count = C.c_uint64(7), C.c_uint64(7)
            emu.lzf_emu_stream_locate2(p, len(ix), a, b, C.byref(first), C.byref(count))
            assert (first.value, count.value) == sic.brute(rws, a, b), (ix["out_len"].tolist(), a, b)
            f2, c2 = C.c_size_t(7), C.c_size_t(7)
            assert lib.lzf_stream_index_locate(p, len(ix), a, b, C.byref(f2), C.byref(c2)) == 0
            assert (f2.value, c2.value) == (first.value, count.value)
            checked += 1
    assert checked > 5000
