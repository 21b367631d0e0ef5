"""The built cases of aux_kernel_cases.py without a GPU: every named edge of the small kernels (XXH32 in both forms, the chain step, the
table helpers, lzf_copy_ranges over several launches) is reached by a case, and every expectation the GPU test compares with is
pinned to the oracle — the hashes to its XXH32 and to the library's host hash, the chain model to its frame reader over linked-block
frames, the numpy restatement of the template table to its replace loop, the offsets to the library's host twin."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_ffi as o
import aux_kernel_cases as K
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import build, ffi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return ffi.lib()


# ------------------------------------------------------------------------------------------------------------------- XXH32
def test_wave_case_has_every_length_class_at_every_residue_class():
    c = K.xxh_wave_case()
    have = {(n, off & 15) for n, off in zip(c["lens"], c["offs"])}
    assert have == {(n, r) for n in K.XXH_LONG for r in range(16)} | {(n, r) for n in K.XXH_SHORT for r in K.XXH_SHORT_RESIDUES}
    assert min(K.XXH_LONG) == 1024 and max(K.XXH_SHORT) < 1024 and set(range(49)) <= set(K.XXH_SHORT)
    assert len(c["lens"]) <= K.XXH32_WAVE_KERNEL_MAX_N                     # one call of the wave kernel
    shapes = {K.xxh_shape(n) for n in c["lens"]}
    assert {s[0] for s in shapes} == {0, 1, 2, 3, "many"}                  # nothing, one and both of the first two loads, the prefetch on and off
    for chunks in (1, 2, 3, "many"):
        assert {0, 1} <= {s[1] for s in shapes if s[0] == chunks}, chunks   # no stripe and one stripe behind the last chunk
    assert {63} <= {s[1] for s in shapes if s[0] == 0} & {s[1] for s in shapes if s[0] == 1} & {s[1] for s in shapes if s[0] == 2}
    assert {s[2] for s in shapes if s[0] != 0} == set(range(16)) == {s[2] for s in shapes if s[0] == 0}
    assert 65536 + 1024 + 17 in c["lens"]
    for (a, n), (b, _) in zip(sorted(zip(c["offs"], c["lens"])), sorted(zip(c["offs"], c["lens"]))[1:]):
        assert a + n < b                                                   # no two buffers touch


def test_lane_lists_switch_the_kernel_and_mix_stripe_counts_inside_a_wavefront():
    same, more, longer = K.xxh_lane_cases()
    assert len(same["lens"]) == K.XXH32_WAVE_KERNEL_MAX_N and len(more["lens"]) == K.XXH32_WAVE_KERNEL_MAX_N + 1
    assert more["lens"][:-1] == same["lens"] and more["offs"][:-1] == same["offs"] and more["arena"] is same["arena"]
    for c in (more, longer):
        lens, n = c["lens"], len(c["lens"])
        assert n > K.XXH32_WAVE_KERNEL_MAX_N and n % 16 != 0               # the lane kernel, and its last wavefront has idle groups
        assert max(lens[n - n % 16:]) >= 16                                # ... beside groups that have stripes to hash
        assert sorted(x for x in lens if x > 257) == sorted(K.LANE_HANDFUL) and sum(lens) < 4 << 20
        assert {off & 15 for off, x in zip(c["offs"], lens) if x >= 16} == set(range(16))
        assert all(off + x <= len(c["arena"]) for off, x in zip(c["offs"], lens))
        waves = [[x >> 4 for x in lens[w:w + 16]] for w in range(0, n - 15, 16)]
        assert any(len(set(w)) == 16 for w in waves)                       # 16 pairwise different stripe counts
        for j in range(15):                                                # every group ends before, with and after its neighbour
            assert {(w[j] > w[j + 1]) - (w[j] < w[j + 1]) for w in waves} == {-1, 0, 1}, j
            assert {(w[j] // 4 > w[j + 1] // 4) - (w[j] // 4 < w[j + 1] // 4) for w in waves} == {-1, 0, 1}, j      # ... in the loop of four stripes too
        assert {w[j] % 4 for w in waves for j in range(16)} == {0, 1, 2, 3}
        big = [g for g, x in enumerate(lens) if x >= 1024]
        assert all(0 < g % 16 < 15 and lens[g - 1] < 272 and lens[g + 1] < 272 for g in big)
        first = lens[:16]
        assert any(first[i] == 0 and 0 < first[i + 1] < 16 and first[i + 2] == 16 for i in range(14))
        assert any(first[i] == 16 and first[i + 1] == 0 for i in range(15)) and any(0 < first[i] < 16 and first[i + 1] == 0 for i in range(15))
    assert len(longer["lens"]) % 16 > 1


def test_the_switch_count_is_the_literal_in_capi_hip():
    src = open(os.path.join(ROOT, "rust-lz-fear_amd", "csrc", "capi.hip")).read()
    m = re.search(r"if \(n <= (\d+)u\) LAUNCH\(lzf::lzf_xxh32_wave_kernel", src)
    assert m and int(m.group(1)) == K.XXH32_WAVE_KERNEL_MAX_N
    assert "test_xxh32_lane_kernel_on_both_sides_of_the_switch" in src[m.start() - 400:m.start()]


def test_every_hash_expectation_is_the_oracles_and_the_host_hashes(lib):
    same, more, longer = K.xxh_lane_cases()
    for c in (K.xxh_wave_case(), more, longer):
        for k, b in enumerate(K.xxh_buffers(c)):
            assert lib.lzf_xxh32(b, len(b), 0) == o.xxh32(b), (c["name"], k, len(b))


# ------------------------------------------------------------------------------------------------------------ the chain step
def _by_name(c):
    state, jobs, out = K.chain_expect(c, 0x00)
    rows = {}
    for i, name in enumerate(c["names"]):
        k = c["steps"]["job"][i]
        rows[name] = dict(i=i, length=int(state["length"][i]), dead=int(state["dead"][i]),
                          job=None if k == K.NONE else tuple(int(jobs[f][k]) for f in ("input_len", "out_existing_len", "out_cap", "output_limit")))
    return rows, state, jobs, out


def test_chain_case_names_every_edge_and_the_model_gives_each_its_outcome():
    c = K.chain_case()
    rows, state, jobs, out = _by_name(c)
    assert len(set(c["names"])) == len(c["names"]) and 55 <= len(c["names"]) <= 90
    r = rows["prev none, job"]
    assert (r["length"], r["dead"], r["job"]) == (1000, 0, (777, 1000, 1000 + K.BM + 777, 1000 + K.BM))
    r = rows["prev ok, job"]
    assert (r["length"], r["dead"], r["job"]) == (5321, 0, (999, 5321, 5321 + K.BM + 999, 5321 + K.BM))
    for s in range(1, 8):
        r = rows[f"prev status {s}, job emptied"]
        assert (r["length"], r["dead"], r["job"]) == (1000, 1, (0, 0, 0, 0)), s
    r = rows["prev ok, grown by block_maxsize: alive"]
    assert (r["length"], r["dead"], r["job"][1]) == (1000 + K.BM, 0, 1000 + K.BM)
    r = rows["prev ok, grown by block_maxsize + 1: dead, length updated"]
    assert (r["length"], r["dead"], r["job"]) == (1001 + K.BM, 1, (0, 0, 0, 0))
    assert rows["prev ok, 4 MiB blocks, grown by block_maxsize: alive"]["dead"] == 0
    assert rows["prev ok, 4 MiB blocks, grown by block_maxsize + 1: dead"]["dead"] == 1
    r = rows["dead on entry, job emptied, prev ignored"]
    assert (r["length"], r["dead"], r["job"]) == (1000, 1, (0, 0, 0, 0))
    r = rows["dead on entry, stored block not copied"]
    assert (r["length"], r["dead"]) == (1000, 1)
    assert (rows["job none, stored_len 0"]["length"], rows["job none, stored_len 0"]["dead"]) == (4242, 0)
    assert rows["prev ok, job none, stored_len 0: the chain's last step"]["length"] == 1017
    assert rows["prev ok, stored block behind the new length"]["length"] == 1333 + 500
    r = rows["length above 4 GiB, job"]
    assert r["job"] == ((1 << 20) + 3, (5 << 32) + 77, (5 << 32) + 77 + K.BM + (1 << 20) + 3, (5 << 32) + 77 + K.BM)
    assert rows["length across 4 GiB, prev ok grown by block_maxsize: alive"]["job"][3] == (1 << 32) - 5 + 2 * K.BM
    assert rows["length above 4 GiB, prev ok grown by block_maxsize + 1: dead"]["dead"] == 1
    # stored blocks: every size at every pair of residues, copied to the end of the history, inside red zones of both kinds
    src0, out0 = K.chain_arenas(c, 0x00)
    src1, out1 = K.chain_arenas(c, 0xFF)
    seen = set()
    for i, s in enumerate(c["streams"]):
        if not s["name"].startswith("stored "):
            continue
        st = c["steps"][i]
        a, b, n = int(st["stored_src"]), int(st["out"]) + s["length"], s["stored"]
        seen.add((n, a & 15, b & 15))
        assert (a & 15, b & 15) == (s["sr"], s["dr"])
        for arena, poison, p in ((src0, 0x00, a), (src1, 0xFF, a)):
            assert (arena[p - K.ZONE:p] == poison).all() and (arena[p + n:p + n + K.ZONE] == poison).all()
        assert (out0[b:b + n + K.ZONE] == K.OUT_POISON).all() and (out0[int(st["out"]) - K.ZONE:int(st["out"])] == K.OUT_POISON).all()
        assert (out[b:b + n] == src0[a:a + n]).all() and (out[b + n:b + n + K.ZONE] == K.OUT_POISON).all()
        assert int(state["length"][i]) == s["length"] + n
    assert seen == {(n, a, b) for n in K.STORED_SIZES for a in K.STORED_RESIDUES for b in K.STORED_RESIDUES}
    assert K.STORED_SIZES == (1, 255, 256, 257, 4097, 65539) and K.STORED_RESIDUES == (0, 1, 15)
    assert (K.OUT_POISON, K.IN_POISONS) == (0xA5, (0x00, 0xFF))            # tests/redzone.py: OUT_POISON and check_decompress's two runs
    # the streams that copy nothing leave their outputs alone; jobs of no stream stay as they are
    for name in ("dead on entry, stored block not copied", "prev status 4, stored block not copied",
                 "prev ok, grown by block_maxsize + 1, stored block not copied"):
        assert rows[name]["dead"] == 1
    changed = np.nonzero(out != out0)[0]
    copied = sum(s["stored"] for s in c["streams"] if s["name"].startswith("stored ")) + 500
    assert 0 < len(changed) <= copied
    used = {int(k) for k in c["steps"]["job"] if k != K.NONE}
    idle = [k for k in range(len(jobs)) if k not in used]
    assert len(idle) >= 7 + sum(k != K.NONE for k in c["steps"]["prev_job"]) and (jobs[idle] == c["jobs"][idle]).all()
    for f in ("input", "prefix", "prefix_len", "out"):                      # fields the step never writes
        assert (jobs[f] == c["jobs"][f]).all()
    assert (state["reserved"] == c["state"]["reserved"]).all() and len(set(c["state"]["reserved"].tolist())) > 50
    assert sorted({int(x) for x in c["steps"]["job"]} | {int(x) for x in c["steps"]["prev_job"]})[:-1] != list(range(len(used)))   # not in order


def _chain_frames():
    BS = 64 << 10
    text = synth.gen_text_zipf(21, 5 * BS).tobytes()
    noise = bytes(np.random.default_rng(3302).integers(0, 256, BS, dtype=np.uint8))
    data = text[:2 * BS] + noise + text[2 * BS:4 * BS] + text[:BS // 2]
    dct = synth.gen_text_zipf(3, 40000).tobytes()
    plain = o.frame_compress(data, o.make_settings(block_size=BS, independent_blocks=False))[1]
    withd = o.frame_compress(data, o.make_settings(block_size=BS, independent_blocks=False, dictionary=dct, dictionary_id=7))[1]
    kinds = [st for st, _ in K.frame_walk(plain)[2]]
    assert len(kinds) >= 5 and True in kinds[1:-1] and kinds[0] is False and kinds[-1] is False      # a stored block between compressed ones
    first_after = kinds.index(True) + 1

    def damaged(frame, k):         # a sequence of no literals and offset 0 at the start of block k
        blk = K.frame_walk(frame)[2][k][1]
        return K.frame_with_block(frame, k, b"\x00\x00\x00" + blk[3:])
    return [("linked", plain, b""), ("linked, dictionary", withd, dct), ("first block damaged", damaged(plain, 0), b""),
            ("block behind the stored one damaged", damaged(plain, first_after), b""), ("dictionary, second block damaged", damaged(withd, 1), dct),
            ("second block's last literals pass block_maxsize", K.frame_with_block(plain, 1, K.overflowing_block(BS)), b""),
            ("first block's last literals pass block_maxsize", K.frame_with_block(withd, 0, K.overflowing_block(BS)), dct)]


def test_the_chain_model_is_the_frame_reader_over_linked_blocks():
    def dec(blk, prefix, existing, limit, cap):
        return o.decompress_raw(blk, prefix=prefix, existing=existing, limit=limit, cap=cap)
    statuses = {}
    for name, frame, dct in _chain_frames():
        erc, eout, _ = o.frame_decompress(frame, dictionary=dct)
        r = K.run_chain(frame, dct, dec)
        assert r["status"] == erc, (name, r["status"], erc)
        assert r["out"] == eout, (name, len(r["out"]), len(eout))                # the bytes, and so the block where the stream dies
        assert (r["trace"][-1][1] == 1) == (erc != 0)
        # the count-only rule walks the same lengths
        assert K.run_chain_count_only(frame, r["results"]) == r["trace"], name
        statuses[name] = erc
    assert statuses["linked"] == statuses["linked, dictionary"] == 0
    assert statuses["first block damaged"] == statuses["block behind the stored one damaged"] == o.ZERO_DEDUP_OFFSET
    assert statuses["second block's last literals pass block_maxsize"] == statuses["first block's last literals pass block_maxsize"] \
        == o.F_BLOCK_SIZE_OVERFLOW == K.F_BLOCK_SIZE_OVERFLOW == 22


# ----------------------------------------------------------------------------------------------------------- table helpers
def test_offset_expectations_are_the_host_twins(lib):
    lib.lzf_table_offset_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
    assert K.OFFSET_ADDS == (0, 1, 65536, (1 << 32) + 5, 1 << 63) and K.OFFSET_BATCH_N == (1, 255, 256, 257, 1000)
    assert C.sizeof(ffi.U32Table) == C.sizeof(ffi.U16Table) == K.TABLE_BYTES
    tables = K.offset_tables()[:12]
    for kind, T in ((ffi.TABLE_U32, ffi.U32Table), (ffi.TABLE_U16, ffi.U16Table)):
        host = [T.from_buffer_copy(t.tobytes()) for t in tables]
        exp = tables
        for rnd in range(2):                                                # two calls accumulate
            adds = K.offset_adds(len(tables), rnd)
            for t, a in zip(host, adds):
                assert lib.lzf_table_offset_host(C.addressof(t), kind, int(a)) == 0
            exp = K.offset_expect(exp, adds)
            assert b"".join(bytes(t) for t in host) == exp.tobytes()
            assert [t.offset for t in host] == [(int(x) + sum(int(K.offset_adds(len(tables), r)[i]) for r in range(rnd + 1))) & K.M64
                                                for i, x in enumerate(tables[:, 16384:].copy().view("<u8")[:, 0])]
    assert {int(a) for a in K.offset_adds(5, 0)} == set(K.OFFSET_ADDS) == {int(a) for a in K.offset_adds(5, 1)}
    few = K.offset_expect(tables, K.offset_adds(3, 0))
    assert (few[3:] == tables[3:]).all() and (few[:, :16384] == tables[:, :16384]).all()


def _replace_loop(dic):
    rep = o.lib().lzfo_u32_replace
    rep.restype = C.c_size_t
    rep.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_int)]
    t, contract = o.new_table(), C.c_int(0)
    for off in range(0, len(dic) - 7, 3):
        rep(C.addressof(t), dic, len(dic), off, C.byref(contract))
    assert not contract.value
    return bytes(t)


def test_the_numpy_template_table_is_the_oracles_replace_loop():
    dic = synth.gen_text_zipf(3, 70000).tobytes()
    assert K.seed_expect(dic) == _replace_loop(dic)
    cases = K.seed_cases()
    for name, d, _ in cases:
        if len(d) <= 5000:
            assert K.seed_expect(d) == _replace_loop(d), name
    name, d, _ = [c for c in cases if c[0].endswith("third pass of one window, (dict_len - 8) % 3 = 2")][0]
    assert K.seed_expect(d) == _replace_loop(d), name


def test_seed_cases_reach_every_edge():
    cases = K.seed_cases()
    by = {name: (d, r) for name, d, r in cases}
    assert len(by) == len(cases)
    assert [len(by[f"dict_len {n}"][0]) for n in range(41)] == list(range(41))
    assert {r for name, (d, r) in by.items() if name.startswith("dict_len 1000")} == set(range(8))
    assert K.seed_windows(len(by["one full pass of the grid"][0])) == K.SEED_GRID_ITEMS == 1024 * 256
    loops = [(name, len(d)) for name, (d, r) in by.items() if name.startswith("grid-stride loop")]
    assert len(loops) == 6
    for name, n in loops:
        count = K.seed_windows(n)
        assert count > 1024 * 256 and count % (1024 * 256) == 1, name       # the loop runs, and its last pass is a partial one
    assert {(K.seed_windows(n) // (1024 * 256), (n - 8) % 3) for _, n in loops} == {(p, k) for p in (1, 2) for k in range(3)}
    assert {n for _, n in loops} == {786432 + 8 + k for k in range(3)} | {2 * 786432 + 8 + k for k in range(3)}
    t = np.frombuffer(K.seed_expect(by["all zero"][0]), dtype="<u4")[:4096]
    assert np.count_nonzero(t) == 1 and t[0] == 90 == 3 * ((100 - 8) // 3)   # one slot: the last window wins
    d = by["window 0 alone in its slot"][0]
    h = K.seed_hashes(d)
    t = np.frombuffer(K.seed_expect(d), dtype="<u4")[:4096]
    assert h[0] not in h[1:] and t[h[0]] == 0 and np.count_nonzero(t) == len(set(h[1:].tolist()))      # as good as empty, as in the reference
    d = by["four symbols"][0]
    assert set(d) == {0, 1, 2, 3} and len(set(K.seed_hashes(d).tolist())) < K.seed_windows(len(d)) // 2     # heavy collisions
    assert all(len(d) + r <= 2 * 786432 + 8 + 2 + 16 for d, r in by.values())


# ----------------------------------------------------------------------------------------------------------- lzf_copy_ranges
def test_copy_case_crosses_two_relaunches():
    c = K.copy_case()
    lens, so, do = c["lens"], c["so"], c["do"]
    assert len(lens) == K.COPY_N == 65535 + 65535 + 3 and K.COPY_LAUNCH == 65535
    big = {0: 65535, 65534: 65536, 65535: 65537, 65536: 65535, len(lens) - 1: 65537}
    assert {i: int(lens[i]) for i in big} == big and {65535, 65536, 65537} == set(big.values())
    small = np.array([i not in big for i in range(len(lens))])
    assert (lens[small] == np.array(K.COPY_SMALL)[np.arange(len(lens)) % 6][small]).all() and K.COPY_SMALL == (0, 1, 15, 16, 17, 33)
    assert int(lens.max()) == K.COPY_MAX_LEN == 65537 and (K.COPY_MAX_LEN + 65535) // 65536 == 2          # two pieces per range
    for at in (0, 65535, 2 * 65535):                                        # every launch: each length at every source and destination residue
        sl = slice(at, min(at + 65535, len(lens)))
        got = {(int(n), int(a) & 15, int(b) & 15) for n, a, b in zip(lens[sl], so[sl], do[sl])}
        if at < 2 * 65535:
            assert {(n, a) for n, a, _ in got} >= {(n, a) for n in K.COPY_SMALL for a in range(16)}
            assert {(n, b) for n, _, b in got} >= {(n, b) for n in K.COPY_SMALL for b in range(16)}
            assert len({(a, b) for _, a, b in got}) == 256                  # the two residues turn independently
        else:
            assert len(got) == 3
    assert (so[1:] > (so + lens)[:-1]).all() and (do[1:] > (do + lens)[:-1]).all() and int((do + lens)[-1]) < c["total"]
    exp = K.copy_expect(c)
    assert int(lens.sum()) < 2_200_000 and np.count_nonzero(exp != K.OUT_POISON) > 0.99 * int(lens.sum())
    k = 65535
    assert (exp[do[k]:do[k] + lens[k]] == c["src"][so[k]:so[k] + lens[k]]).all() and exp[do[k] - 1] == exp[do[k] + lens[k]] == K.OUT_POISON
