"""CPU test (no GPU) of the dispatch rules of lzf_decompress_batch / lzf_compress_batch (rust-lz-fear_amd/csrc/lzf_dispatch.h),
compiled here with g++.  Held to a Python restatement written from DESIGN.md's class table ("Decompress: three classes by batch
size") and from what tests/fake_cu_check.py expects of a device of another size — not from the header: which path a call of n
jobs tries on a device of `cu` compute units with `lds` bytes of LDS each, the groups of the segmented pipeline, the areas of the
two scratch allocations, the compress classes, and every lzf_last_*_launch string byte for byte."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

ANY = 0xFFFFFFFFFFFFFFFF                     # lzf_decompress_batch: the caller gives no bound of its inputs
GEOMETRIES = [(256, 163840), (64, 163840), (512, 163840), (256, 65536), (1, 163840)]
BY_RULE, FORCED, OFF = 0, 1, 2
KEEP = 0xFFFFFFFF

# the launch strings, as lzf_last_decompress_launch / lzf_last_compress_launch have given them so far
S_SEG = {r: "segmented: lzf_seg_resolve_pair_kernel<%d> + lzf_decompress_paired_kernel<4096,48,640>" % r for r in (131072, 65536, 32768)}
S_FED = "bitmap-fed: lzf_seg_parse_kernel + lzf_decompress_fed_kernel<4096,32,352> + lzf_decompress_paired_kernel<4096,24,384>"
S_LAST = {48: "lzf_decompress_paired_kernel<4096,48,640>", 24: "lzf_decompress_paired_kernel<4096,24,384>", 16: "lzf_decompress_batched_kernel<4096,16,256,staged>"}
S_VARIANT = "analysis variant (LZF_DECOMPRESS_KERNEL)"
S_U16 = "lzf_compress_wave_kernel<U16>"
S_GENERAL = "lzf_compress_wave_kernel (analysis: general)"
S_TEAM = "lzf_compress_team_kernel"
S_TEAM_ALL = "lzf_compress_team_kernel + lzf_compress_team_carry_kernel + lzf_compress_wave_kernel"
S_COMPACT = "lzf_compress_compact_kernel"
S_COMPACT_ALL = "lzf_compress_compact_kernel + lzf_compress_wave_kernel"
LAST_OF = {0: 48, 1: 24, 2: 16}


def knobs(seg=KEEP, fed=KEEP, fed_min_in=KEEP, fed_open=0, groups=(), d_order=KEEP, c_order=KEEP, c_kernel=KEEP, team_max=None):
    pct = list(groups) + [0] * (4 - len(groups))
    return (C.c_uint32 * 13)(seg, fed, fed_min_in, fed_open, len(groups), *pct, d_order, c_order, c_kernel, 0 if team_max is None else team_max + 1)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dispatch") / "libemu_dispatch.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(HERE, "emu", "emu_dispatch.cpp")])
    L = C.CDLL(so)
    L.lzf_emu_decompress_plan.restype = None
    L.lzf_emu_decompress_plan.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_char_p)]
    L.lzf_emu_compress_plan.restype = C.c_char_p
    L.lzf_emu_compress_plan.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.lzf_emu_seg_layout.restype = None
    L.lzf_emu_seg_layout.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
    L.lzf_emu_fed_layout.restype = None
    L.lzf_emu_fed_layout.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
    L.lzf_emu_launch_variant.restype = C.c_char_p

    class Emu:
        @staticmethod
        def decompress(cu, lds, n, max_in=ANY, kn=None):
            out = (C.c_uint32 * 12)(); strs = (C.c_char_p * 3)()
            L.lzf_emu_decompress_plan(cu, lds, kn, n, max_in, out, strs)
            return dict(want_order=bool(out[0]), try_seg=bool(out[1]), seg_min_in=out[2], ring=out[3], groups=list(out[5:5 + out[4]]), try_fed=bool(out[9]), seg_class=bool(out[11]),
                        last=LAST_OF[out[10]], s_seg=strs[0].decode(), s_fed=strs[1].decode(), s_last=strs[2].decode())

        @staticmethod
        def compress(cu, lds, n, kinds, kn=None):
            out = (C.c_uint32 * 6)()
            s = L.lzf_emu_compress_plan(cu, lds, kn, n, kinds, out)
            return dict(kinds=out[0], compact=bool(out[1]), team=bool(out[2]), fresh_only=bool(out[3]), want_order=bool(out[4]), general_skip=out[5], launch=s.decode())

        @staticmethod
        def seg_layout(n, max_in):
            out = (C.c_uint64 * 16)(); L.lzf_emu_seg_layout(n, max_in, out)
            return dict(max_in=out[0], maxch=out[1], maxtile=out[2], rec_cap=out[3], offs=list(out[4:15]), total=out[15])

        @staticmethod
        def fed_layout(n, max_in):
            out = (C.c_uint64 * 9)(); L.lzf_emu_fed_layout(n, max_in, out)
            return dict(max_in=out[0], maxch=out[1], maxtile=out[2], offs=list(out[3:8]), total=out[8])

        variant = L.lzf_emu_launch_variant().decode()
    return Emu


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def per_cu(lds, bytes_each):
    """workgroups of that much LDS a CU holds; a kernel that fits at all runs one"""
    return max(1, lds // bytes_each)


def py_dims(max_in):
    """the pipeline parses inputs of 16 KiB .. 4 MiB + 32 KiB: chunks of 16 KiB that overlap by 2 KiB, tiles of 2 KiB"""
    m = min(max(max_in, 16384), 4 * 1024 * 1024 + 32 * 1024)
    nch = 1 if m <= 16384 else 1 + -(-(m - 16384) // 14336)
    return m, nch, -(-m // 2048)


def py_seg_sizes(n, max_in):
    m, nch, tiles = py_dims(max_in)
    rec_cap = n * min(m // 3 + 192, 448 * 1024)
    # state, arena top, xexit, vfrom, tile tokens, tile bytes, bit maps (512 words per chunk), records of 16 bytes, order, by_len, est
    return [48 * n, 8, 4 * n * nch, 4 * n * nch, 4 * n * tiles, 4 * n * tiles, 4 * n * nch * 512, 16 * rec_cap, 4 * n, 4 * n, 4 * n], rec_cap


def py_fed_sizes(n, max_in):
    m, nch, tiles = py_dims(max_in)
    # state, arena top, bit maps, 32 ticket counters a 128-byte line apart, the decoder state a job's pieces hand on
    return [48 * n, 8, 4 * n * nch * 512, 32 * 128, 16 * n]


def aligned_total(sizes):
    return sum(-(-s // 256) * 256 for s in sizes)


def py_decompress(cu, lds, n, max_in, seg=BY_RULE, fed=BY_RULE, fed_min_in=65536, fed_open=False):
    seg_max = min(per_cu(lds, 32768 + 8192) * cu, 1024)                    # a block per 32 KiB ring (+ 8 KiB); the rank kernels take 1 024 jobs
    r48, r24 = per_cu(lds, 20 * 1024) * cu, per_cu(lds, 12800) * cu        # MI355X: 8 and 12 per CU
    ring = 32768
    for r in (65536, 131072):                                              # the largest ring with which every block of the call is resident
        if lds >= r + 8192 and n <= per_cu(lds, r + 8192) * cu:
            ring = r
    seg_on = seg == FORCED or (seg == BY_RULE and n <= seg_max)
    fed_on = fed == FORCED or (fed == BY_RULE and n > r24)
    return dict(want_order=n > r48,
                seg_class=seg_on,                                          # the sampled order runs in front of this class, taken or not
                try_seg=seg_on and max_in >= 65536,
                ring=ring,
                try_fed=fed_on and n <= 65535 and max_in > fed_min_in and max_in > (0 if fed_open else 262144) and aligned_total(py_fed_sizes(n, max_in)) <= 24 << 30,
                last=48 if n <= r48 else 24 if n <= 8 * r48 else 16)


def py_groups(cu, n, seg_max):
    if n > seg_max or n < (cu + 7) // 8 or n < 8:
        return [n]
    q = n * 25 // 100
    return [q, q, q, n - 3 * q]


def check_decompress(emu, cu, lds, n, max_in, **kn):
    got = emu.decompress(cu, lds, n, max_in, knobs(seg=kn.get("seg", KEEP), fed=kn.get("fed", KEEP), fed_min_in=kn.get("fed_min_in", KEEP), fed_open=int(kn.get("fed_open", False))) if kn else None)
    want = py_decompress(cu, lds, n, max_in, **kn)
    for key, v in want.items():
        assert got[key] == v, (cu, lds, n, max_in, kn, key, got)
    assert got["s_seg"] == S_SEG[want["ring"]] and got["s_fed"] == S_FED and got["s_last"] == S_LAST[want["last"]]
    assert got["seg_min_in"] == 65536
    return got


# ---- decompress ------------------------------------------------------------------------------------------------------------------
def test_mi355x_classes_by_number(emu):
    """DESIGN.md's table, in its own numbers: <= 1 024 pipeline (rings by 256 / 512), <= 2 048 paired48, <= 3 072 paired24, beyond the
    fed path unless the caller bounds the inputs at <= 256 KiB, then paired24 up to 16 384 and staged16."""
    cu, lds = 256, 163840
    for n, ring in ((1, 131072), (256, 131072), (257, 65536), (512, 65536), (513, 32768), (1024, 32768)):
        p = emu.decompress(cu, lds, n)
        assert p["try_seg"] and p["ring"] == ring and p["s_seg"] == S_SEG[ring] and not p["try_fed"] and p["last"] == 48 and not p["want_order"], (n, p)
    for n, last, order in ((1025, 48, False), (2048, 48, False), (2049, 24, True), (3072, 24, True)):
        p = emu.decompress(cu, lds, n)
        assert not p["try_seg"] and not p["try_fed"] and p["last"] == last and p["s_last"] == S_LAST[last] and p["want_order"] == order, (n, p)
    for n in (3073, 16384, 16385, 65535):
        p = emu.decompress(cu, lds, n, 1 << 20)                  # (65 535 jobs of unbounded inputs would not fit the scratch: test_fed_scratch_limit)
        assert p["try_fed"] and p["s_fed"] == S_FED and p["want_order"] and not p["try_seg"], (n, p)
        assert not emu.decompress(cu, lds, n, 262144)["try_fed"] and emu.decompress(cu, lds, n, 262145)["try_fed"]
    assert not emu.decompress(cu, lds, 65536, 1 << 20)["try_fed"]
    assert [emu.decompress(cu, lds, n, 262144)["last"] for n in (3073, 16384, 16385)] == [24, 24, 16]
    # inputs below the pipeline's 64 KiB window: not tried (the call is still of the pipeline's class)
    assert not emu.decompress(cu, lds, 100, 65535)["try_seg"] and emu.decompress(cu, lds, 100, 65536)["try_seg"]
    assert emu.decompress(cu, lds, 100, 65535)["seg_class"] and not emu.decompress(cu, lds, 1025, 65535)["seg_class"]
    assert emu.variant == S_VARIANT


def test_fake_cu_expectations(emu):
    """what tests/fake_cu_check.py sees on a device: LZF_FAKE_CU=64 crosses every class, 512 CUs meet the rank kernels' 1 024 jobs"""
    cu, lds = 64, 163840
    want = {cu - 4: ("seg", 131072), cu + 4: ("seg", 65536), 2 * cu + 4: ("seg", 32768), 4 * cu - 4: ("seg", 32768),
            4 * cu + 8: (48, None), 8 * cu + 8: (24, None), 13 * cu + 8: ("fed", None), 64 * cu + 16: ("fed", None)}
    for n, (cls, ring) in want.items():
        p = emu.decompress(cu, lds, n)
        if cls == "seg":
            assert p["try_seg"] and p["ring"] == ring, (n, p)
        else:
            assert not p["try_seg"] and p["try_fed"] == (cls == "fed"), (n, p)
            assert cls == "fed" or p["last"] == cls, (n, p)
    assert emu.decompress(512, lds, 1000)["try_seg"]
    p = emu.decompress(512, lds, 1500)
    assert not p["try_seg"] and not p["try_fed"] and p["last"] == 48


@pytest.mark.parametrize("cu,lds", GEOMETRIES)
def test_decompress_boundaries(emu, cu, lds):
    """every class boundary of every geometry, at n and n + 1 (and the job before), for inputs on both sides of the two windows"""
    one = per_cu(lds, 20480)
    bounds = {min(4 * cu, 1024) if lds == 163840 else cu, cu, 2 * cu, 4 * cu, 1024, one * cu, per_cu(lds, 12800) * cu, 8 * one * cu, 65535}
    if lds == 163840:
        assert one == 8 and per_cu(lds, 12800) == 12
        bounds |= {8 * cu, 12 * cu, 64 * cu}
    checked = 0
    for b in sorted(bounds):
        for n in (b - 1, b, b + 1):
            if n < 1:
                continue
            for max_in in (65535, 65536, 262144, 262145, 4 * 1024 * 1024, ANY):
                check_decompress(emu, cu, lds, n, max_in)
                checked += 1
    assert checked >= 100
    if lds == 65536:                         # one block per CU and the 32 KiB ring only
        assert all(emu.decompress(cu, lds, n)["ring"] == 32768 for n in (1, cu))
        assert emu.decompress(cu, lds, cu)["try_seg"] and not emu.decompress(cu, lds, cu + 1)["try_seg"]
    # a launch order is wanted from one residency of 48-byte pairs + 1 on
    assert not emu.decompress(cu, lds, one * cu)["want_order"] and emu.decompress(cu, lds, one * cu + 1)["want_order"]


def test_groups(emu):
    """cu = 256: one group below 32 jobs, quarters from 32 on — three of n * 25 / 100, the last takes the rest"""
    for n in range(1, 1025):
        g = emu.decompress(256, 163840, n)["groups"]
        assert g == py_groups(256, n, 1024), (n, g)
        assert sum(g) == n and len(g) == (1 if n < 32 else 4)
        if n >= 32:
            assert g[0] == g[1] == g[2] == n * 25 // 100 and g[3] == n - 3 * g[0]
    for cu, lds in GEOMETRIES:
        seg_max = min(per_cu(lds, 40960) * cu, 1024)
        for n in (1, 7, 8, 9, (cu + 7) // 8, (cu + 7) // 8 + 1, cu, seg_max, seg_max + 1, 2000):
            assert emu.decompress(cu, lds, n)["groups"] == py_groups(cu, n, seg_max), (cu, lds, n)


# ---- scratch layouts ----------------------------------------------------------------------------------------------------------------
def check_layout(offs, sizes, total):
    at = 0
    for o, s in zip(offs, sizes):
        assert o % 256 == 0 and o == at, (offs, sizes)      # aligned, in order, nothing between or over one another
        at = o + -(-s // 256) * 256
    assert total == at == aligned_total(sizes)


@pytest.mark.parametrize("n", [1, 33, 1024])
@pytest.mark.parametrize("max_in", [1, 16384, 16385, 262145, 4 * 1024 * 1024 + 32 * 1024, ANY])
def test_layouts(emu, n, max_in):
    m, nch, tiles = py_dims(max_in)
    s = emu.seg_layout(n, max_in)
    sizes, rec_cap = py_seg_sizes(n, max_in)
    assert (s["max_in"], s["maxch"], s["maxtile"], s["rec_cap"]) == (m, nch, tiles, rec_cap)
    check_layout(s["offs"], sizes, s["total"])
    f = emu.fed_layout(n, max_in)
    assert (f["max_in"], f["maxch"], f["maxtile"]) == (m, nch, tiles)
    check_layout(f["offs"], py_fed_sizes(n, max_in), f["total"])


def test_chunk_counts():
    assert [py_dims(x)[1] for x in (1, 16384, 16385, 16384 + 14336, 16384 + 14337)] == [1, 1, 2, 2, 3]
    assert py_dims(ANY) == (4227072, 295, 2064)


def test_fed_scratch_limit(emu):
    """the bit maps of 65 535 jobs of the largest input exceed 24 GiB: declined; 12 240 jobs are taken"""
    assert emu.fed_layout(65535, ANY)["total"] > 24 << 30
    assert emu.fed_layout(12240, ANY)["total"] <= 24 << 30
    assert not emu.decompress(256, 163840, 65535, ANY)["try_fed"] and emu.decompress(256, 163840, 12240, ANY)["try_fed"]
    check_decompress(emu, 256, 163840, 65535, ANY)
    check_decompress(emu, 256, 163840, 65535, 300000)


# ---- compress ------------------------------------------------------------------------------------------------------------------------
U32, U16, FRESH = 1, 2, 4


@pytest.mark.parametrize("cu,lds", GEOMETRIES)
def test_compress_classes(emu, cu, lds):
    team_ok = lds >= 163840
    for n in (1, cu, cu + 1):
        for kinds, s_team, s_compact in ((U32 | FRESH, S_TEAM, S_COMPACT), (U32, S_TEAM_ALL, S_COMPACT_ALL), (0, S_TEAM_ALL, S_COMPACT_ALL), (U32 | U16, S_TEAM_ALL, S_COMPACT_ALL)):
            p = emu.compress(cu, lds, n, kinds)
            team = team_ok and n <= cu
            assert p["compact"] and p["team"] == team and p["launch"] == (s_team if team else s_compact), (n, kinds, p)
            assert p["fresh_only"] == bool(kinds & FRESH) and p["general_skip"] == (2 if team else 1)
            assert p["kinds"] & 3 == (kinds & 3 or 3)
        p = emu.compress(cu, lds, n, U16)
        assert p["launch"] == S_U16 and not p["want_order"]
    # the probe order: beyond one residency of the compact kernel (8 960 bytes of LDS: 18 per CU on MI355X), or beyond four jobs per CU when the call vouches for fresh tables
    res = per_cu(lds, (2048 + 128 + 64) * 4) * cu
    assert lds != 163840 or res == 18 * cu
    for n in (4 * cu, 4 * cu + 1, res, res + 1):
        assert emu.compress(cu, lds, n, U32)["want_order"] == (n > res), (n,)
        assert emu.compress(cu, lds, n, U32 | FRESH)["want_order"] == (n > 4 * cu), (n,)
        assert not emu.compress(cu, lds, n, U16)["want_order"]


# ---- knobs ------------------------------------------------------------------------------------------------------------------------
def test_knobs_move_what_they_name(emu):
    cu, lds = 256, 163840
    # defaults = no knobs at all
    for n in (100, 3000, 4000):
        assert emu.decompress(cu, lds, n, ANY, knobs()) == emu.decompress(cu, lds, n)
    # seg off / forced
    assert emu.decompress(cu, lds, 100)["try_seg"] and not emu.decompress(cu, lds, 100, ANY, knobs(seg=OFF))["try_seg"]
    assert not emu.decompress(cu, lds, 3000)["try_seg"] and emu.decompress(cu, lds, 3000, ANY, knobs(seg=FORCED))["try_seg"]
    check_decompress(emu, cu, lds, 100, ANY, seg=OFF)
    # fed forced / off
    assert not emu.decompress(cu, lds, 64, 300000)["try_fed"] and emu.decompress(cu, lds, 64, 300000, knobs(fed=FORCED))["try_fed"]
    assert emu.decompress(cu, lds, 4000)["try_fed"] and not emu.decompress(cu, lds, 4000, ANY, knobs(fed=OFF))["try_fed"]
    check_decompress(emu, cu, lds, 64, 300000, fed=FORCED)
    # the caller's bound keeps a forced call off the path too, until fed_min_in = 0 opens the hint
    assert not emu.decompress(cu, lds, 64, 200000, knobs(fed=FORCED))["try_fed"]
    assert emu.decompress(cu, lds, 64, 200000, knobs(fed=FORCED, fed_min_in=0, fed_open=1))["try_fed"]
    assert emu.decompress(cu, lds, 64, 1, knobs(fed=FORCED, fed_min_in=0, fed_open=1))["try_fed"]
    check_decompress(emu, cu, lds, 64, 200000, fed=FORCED, fed_min_in=0, fed_open=True)
    # groups "100": one group
    assert len(emu.decompress(cu, lds, 196)["groups"]) == 4 and emu.decompress(cu, lds, 196, ANY, knobs(groups=(100,)))["groups"] == [196]
    assert emu.decompress(cu, lds, 196, ANY, knobs(groups=(50, 50)))["groups"] == [98, 98]
    # orders: natural / always
    assert not emu.decompress(cu, lds, 4000, ANY, knobs(d_order=0))["want_order"] and emu.decompress(cu, lds, 10, ANY, knobs(d_order=2))["want_order"]
    assert not emu.compress(cu, lds, 9000, U32, knobs(c_order=0))["want_order"] and emu.compress(cu, lds, 10, U32, knobs(c_order=2))["want_order"]
    # compress kernel / team max
    p = emu.compress(cu, lds, 10, U32, knobs(c_kernel=1))
    assert not p["compact"] and not p["team"] and p["launch"] == S_GENERAL and p["general_skip"] == 0
    assert not emu.compress(cu, lds, 10, U32, knobs(c_kernel=3))["team"]
    assert not emu.compress(cu, lds, 10, U32, knobs(team_max=9))["team"] and emu.compress(cu, lds, 300, U32, knobs(team_max=300))["team"]
