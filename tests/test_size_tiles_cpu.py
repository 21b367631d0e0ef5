"""CPU tests (no GPU) of the size call's latency class: a block summed up tile by tile.

The rule (rust-lz-fear_amd/csrc/lzf_size_rules.h: TileSum, summarise, fold), compiled with g++ into a serial driver
(tests/emu/emu_size_tiles.cpp), is held to the oracle: the fold says "clean" with the oracle's length iff the oracle says Ok and no
length is beyond the clamp, and "not clean" otherwise — at tiles of 64 bytes, 2 048 bytes and one tile for the whole block, because
the answer must not depend on where a block is cut.  The dispatch (lzf_dispatch.h: size_plan, size_layout; emu_size_dispatch.cpp)
is held to a Python restatement written from DESIGN.md's class table ("Decoded sizes: two classes"), not from the header."""
import ctypes as C
import os
import subprocess

import pytest

import decoded_size_cases as D
import seg_stage_cases as S
import size_latency_cases as Z

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TILES = (64, 2048, 0)                       # 0: one tile for the whole block
ANY = 0xFFFFFFFFFFFFFFFF
KEEP = 0xFFFFFFFF
BY_RULE, FORCED, OFF = 0, 1, 2
S_CLASS = "latency: lzf_seg_parse_kernel + lzf_size_tile_kernel + lzf_size_finish_kernel + lzf_decoded_size_kernel<48,768>"
S_WAVE = "lzf_decoded_size_kernel<48,768>"


def _gxx(tmp, name, *inc):
    so = str(tmp / f"lib{name}.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", *inc, "-o", so, os.path.join(HERE, "emu", name + ".cpp")])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def tiles(tmp_path_factory):
    L = _gxx(tmp_path_factory.mktemp("size_tiles"), "emu_size_tiles")
    L.lzf_emu_size_tiles.restype = C.c_int
    L.lzf_emu_size_tiles.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32)]
    L.lzf_emu_tile_len_clamp.restype = C.c_uint32
    assert L.lzf_emu_tile_len_clamp() == S.LEN_CLAMP

    def run(case, tile, want_sums=False):
        n = C.c_uint64(0); nt = C.c_uint32(0)
        data = case["input"]
        sums = (C.c_uint32 * (4 * (len(data) // max(tile, 1) + 2)))() if want_sums else None
        clean = L.lzf_emu_size_tiles(data, len(data), tile, case["prefix_len"], case["existing_len"], case["limit"], C.byref(n), sums, C.byref(nt))
        r = (bool(clean), n.value if clean else None)
        return r + ([tuple(sums[4 * t:4 * t + 4]) for t in range(nt.value)],) if want_sums else r
    return run


def _want(case, exp):
    return (True, exp[1]) if Z.finishes(case, exp) else (False, None)


def _check(tiles, pairs):
    for case, exp in pairs:
        for tile in TILES:
            assert tiles(case, tile) == _want(case, exp), (case["name"], tile, exp)


def test_block_cases_every_kind(tiles):
    """decoded_size_cases.block_cases(): fixtures, valid, mutated, prefix / existing — all five oracle statuses present."""
    blocks = D.block_cases()
    D.assert_all_kinds(blocks)
    _check(tiles, [(dict(c, name=name), exp) for name, c, exp in blocks])


def test_stage_cases(tiles):
    """The seam, tile and damaged cases of the segmented pipeline's corpus (one tile up to 67 chunks), as size jobs."""
    pairs = [(c, D.expect(c)) for c in Z.stage_cases()]
    assert {e[0] for _, e in pairs} == {0, 1, 2, 3, 4}
    _check(tiles, pairs)


def test_mutated_blocks(tiles):
    """200 mutated blocks from a fixed seed; both answers occur."""
    pairs = [(c, D.expect(c)) for c in Z.mutated_cases()]
    assert len(pairs) == 200
    kinds = {e[0] for _, e in pairs}
    assert 0 in kinds and len(kinds) >= 4, kinds
    _check(tiles, pairs)


def test_boundaries_at_a_tile_seam(tiles):
    """The sequence under test as a tile's last and as the next tile's first token, prefix and existing output each none and some: the
    limit met exactly and passed by one byte, an offset that reaches the first byte there is and one beyond, offset zero, and a late
    violation behind an early one.  The oracle decides what each case is; here it must be what the case was built for."""
    cases = Z.boundary_cases()
    assert len(cases) == 2 * 4 * 6
    want_status = {"limit exact": 0, "limit one past": 2, "offset to the first byte": 0, "offset one beyond the first byte": 4, "offset zero": 3,
                   "late violation behind an early one": 4}
    pairs = []
    for c in cases:
        exp = D.expect(c)
        assert exp[0] == want_status[c["name"].split(":")[0]], (c["name"], exp)
        pairs.append((c, exp))
    _check(tiles, pairs)
    # the sequence under test really is where the case says: the tile it starts in holds a match that ends the tile's sum
    c = next(c for c in cases if c["name"].startswith("limit exact: last of a tile"))
    _, _, sums = tiles(c, 2048, want_sums=True)
    assert len(sums) == 2 and sums[0][0] == sums[0][1] and sums[1] == (5, 0, 0, 0), sums
    c = next(c for c in cases if c["name"].startswith("limit exact: first of the next"))
    _, _, sums = tiles(c, 2048, want_sums=True)
    assert len(sums) == 2 and sums[1][:2] == (Z.M_TEST + 5, Z.M_TEST), sums


def test_input_edges_and_long_lengths(tiles):
    """Input lengths at the tile's and the chunk's edges, an empty input, one token, one stray byte behind the last literals — all clean;
    a match length beyond the clamp is Ok to the oracle and not this rule's to answer."""
    pairs = [(c, D.expect(c)) for c in Z.size_edge_cases()]
    assert all(e[0] == 0 for _, e in pairs), [(c["name"], e) for c, e in pairs if e[0]]
    _check(tiles, pairs)
    big = Z.long_run_case()
    exp = D.expect(big)
    assert exp[0] == 0 and exp[1] > 76_000_000
    for tile in TILES:
        assert tiles(big, tile) == (False, None)


# ---------------------------------------------------------------------------------------------------------------------- the dispatch
CHUNK, STRIDE, TILE, MAX_IN, MIN_IN = 16384, 14336, 2048, 4 * 1024 * 1024 + 32 * 1024, 64 * 1024
MAX_SCRATCH = 3 << 30


def py_layout(n, max_in):
    """DESIGN.md, "Decoded sizes": the class's scratch, 256-aligned areas in this order."""
    m = min(max(max_in, CHUNK), MAX_IN)
    maxch = 1 if m <= CHUNK else 1 + (m - CHUNK + STRIDE - 1) // STRIDE
    maxtile = (m + TILE - 1) // TILE
    offs, off = [], 0
    for size in (48 * n, 4 * n * maxch, 4 * n * maxch, 16 * n * maxtile, 4 * n * maxch * (CHUNK // 32), 4 * n):
        offs.append(off); off = (off + size + 255) // 256 * 256
    return dict(max_in=m, maxch=maxch, maxtile=maxtile, offs=offs, total=off, sizes=(48 * n, 4 * n * maxch, 4 * n * maxch, 16 * n * maxtile, 4 * n * maxch * (CHUNK // 32), 4 * n))


def py_class_max(cu):
    """16 jobs per CU: where the one-wave kernel begins to fill the chip."""
    return 16 * cu


def py_rank_max(cu, lds):
    """The segmented pipeline's batch, which its one-workgroup rank kernel orders: four blocks per CU — one per 32 KiB ring + 8 KiB the
    LDS holds — and no more than 1 024."""
    return min(max(lds // (32768 + 8192), 1) * cu, 1024)


def py_plan(cu, lds, n, max_in, mode=BY_RULE, min_in=MIN_IN, force=0):
    in_class = mode == FORCED or (mode == BY_RULE and n <= py_class_max(cu))
    tried = in_class and n <= 65535 and max_in >= min_in and py_layout(n, max_in)["total"] <= MAX_SCRATCH
    return dict(try_seg=tried, min_in=min_in, by_len=(cu + 7) // 8 <= n <= py_rank_max(cu, lds), last=force != 2)


@pytest.fixture(scope="module")
def dispatch(tmp_path_factory):
    L = _gxx(tmp_path_factory.mktemp("size_dispatch"), "emu_size_dispatch", "-I", os.path.join(ROOT, "include"))
    L.lzf_emu_size_plan.restype = None
    L.lzf_emu_size_plan.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_char_p)]
    L.lzf_emu_size_layout.restype = None
    L.lzf_emu_size_layout.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
    L.lzf_emu_size_max_scratch.restype = C.c_uint64
    assert L.lzf_emu_size_max_scratch() == MAX_SCRATCH

    class Emu:
        @staticmethod
        def plan(cu, lds, n, max_in=ANY, mode=KEEP, min_in=KEEP, force=0):
            out = (C.c_uint32 * 4)(); strs = (C.c_char_p * 2)()
            L.lzf_emu_size_plan(cu, lds, (C.c_uint32 * 3)(mode, min_in, force), n, max_in, out, strs)
            assert (strs[0].decode(), strs[1].decode()) == (S_CLASS, S_WAVE)
            return dict(try_seg=bool(out[0]), min_in=out[1], by_len=bool(out[2]), last=bool(out[3]))

        @staticmethod
        def layout(n, max_in):
            out = (C.c_uint64 * 10)(); L.lzf_emu_size_layout(n, max_in, out)
            return dict(max_in=out[0], maxch=out[1], maxtile=out[2], offs=list(out[3:9]), total=out[9])
    return Emu


@pytest.mark.parametrize("cu", [256, 64, 512])
def test_size_plan_boundaries(dispatch, cu):
    lds = 163840
    top, rank = py_class_max(cu), py_rank_max(cu, lds)
    assert (top, rank) == {256: (4096, 1024), 64: (1024, 256), 512: (8192, 1024)}[cu]
    for n in (1, (cu + 7) // 8 - 1, (cu + 7) // 8, rank, rank + 1, top - 1, top, top + 1, 5000, 65535, 65536):
        if n < 1:
            continue
        for max_in in (ANY, 1 << 20, MIN_IN, MIN_IN - 1, 0):
            got, want = dispatch.plan(cu, lds, n, max_in), py_plan(cu, lds, n, max_in)
            assert got == want, (cu, n, max_in)
    assert dispatch.plan(cu, lds, top, 1 << 20)["try_seg"] and not dispatch.plan(cu, lds, top + 1, 1 << 20)["try_seg"]
    assert dispatch.plan(cu, lds, top, MIN_IN)["try_seg"] and not dispatch.plan(cu, lds, top, MIN_IN - 1)["try_seg"]


def test_size_plan_knobs_and_scratch_cap(dispatch):
    cu, lds = 256, 163840
    # forced: whatever the count, while the rows of the grid and the scratch cap allow; off: never
    for n, max_in in ((5000, 1 << 20), (5000, ANY), (4096, ANY), (5100, ANY), (65535, 16384), (65536, 16384)):
        for min_in in (0, MIN_IN):
            assert dispatch.plan(cu, lds, n, max_in, FORCED, min_in) == py_plan(cu, lds, n, max_in, FORCED, min_in), (n, max_in, min_in)
    assert dispatch.plan(cu, lds, 5000, 1 << 18, FORCED, 0)["try_seg"]
    assert not dispatch.plan(cu, lds, 5100, ANY, FORCED, 0)["try_seg"]             # 3.04 GiB, bit maps mostly: over the cap
    assert not dispatch.plan(cu, lds, 65536, 16384, FORCED, 0)["try_seg"]
    assert not dispatch.plan(cu, lds, 100, ANY, OFF)["try_seg"]
    # the cap holds the whole class at the largest input, and not twice that
    assert py_layout(4096, ANY)["total"] <= MAX_SCRATCH < py_layout(5100, ANY)["total"]
    assert dispatch.plan(cu, lds, 4096, ANY)["try_seg"]
    assert not dispatch.plan(512, lds, 8192, ANY)["try_seg"] and dispatch.plan(512, lds, 8192, 2 << 20)["try_seg"]      # a larger device's class needs the caller's bound
    # size_force: 1 = the scratch refused where the pool would refuse it, in the driver — the plan still tries; 2 = nothing behind the class
    for force in (0, 1, 2):
        got = dispatch.plan(cu, lds, 100, ANY, force=force)
        assert got == py_plan(cu, lds, 100, ANY, force=force)
        assert got["try_seg"] and got["last"] == (force != 2)


@pytest.mark.parametrize("n,max_in", [(1, ANY), (1, 0), (49, ANY), (1024, ANY), (1024, 70000), (7, 16385), (300, 1 << 20), (5000, 1 << 18)])
def test_size_layout_areas(dispatch, n, max_in):
    got, want = dispatch.layout(n, max_in), py_layout(n, max_in)
    assert {k: got[k] for k in got} == {k: want[k] for k in got}, (n, max_in)
    # no two areas overlap, every one is 256-aligned, all lie inside the allocation
    ends = [o + s for o, s in zip(want["offs"], want["sizes"])]
    for i, o in enumerate(got["offs"]):
        assert o % 256 == 0 and ends[i] <= (got["offs"][i + 1] if i + 1 < len(ends) else got["total"])
    assert got["total"] >= sum(want["sizes"])
