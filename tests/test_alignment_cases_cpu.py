"""The shapes of the buffer-alignment sweep (tests/alignment_cases.py), checked without a GPU: every claimed residue matrix is
complete, every expectation has the intended status, every structural claim holds — and a byte-wise model of ring_flush's
(head, vector, tail) split shows that the tiny shapes reach each of its branches at every rb.  The model is held against the rule
the kernels compile (lzf_ring_split of rust-lz-fear_amd/csrc/lzf_out_ring.h, through tests/emu/emu_ring_split.cpp and g++), not
against the kernels; tests/test_gpu_alignment.py compares the kernels' bytes with the oracle's.  (The model itself,
ring_flush_split, is in tests/alignment_cases.py beside the builders; ring_fill splits a range the same way.)"""
import ctypes as C
import os
import subprocess

import alignment_cases as ac
import oracle_ffi as o

HERE = os.path.dirname(os.path.abspath(__file__))


def _pairs(s, idx=None):
    idx = range(len(s.items)) if idx is None else idx
    return {(s.in_low[i] & 15, s.out_low[i] & 15) for i in idx}


ALL_PAIRS = {(a, b) for a in range(16) for b in range(16)}


def _common(s, decompress=True):
    n = len(s.items)
    assert n and all(len(f) == n for f in s)
    assert all(0 <= v <= 255 for f in (s.in_low, s.out_low, s.prefix_low) for v in f)
    if decompress:
        for it, (st, b), m in zip(s.items, s.expect, s.meta):
            if "decoded" in m:
                assert st == o.OK and b == m["decoded"]
                if m.get("exact"):
                    assert it["out_cap"] == len(b)                       # not one byte of slack behind the block
                else:
                    assert it["out_cap"] == len(b) + len(it["input"]) + 64


def test_ring_flush_model_is_a_partition():
    for rb in range(16):
        for a in range(40):
            for b in range(a, a + 70):
                nh, nv, nt, clamped = ac.ring_flush_split(a, b, rb)
                assert nh + 16 * nv + nt == b - a and 0 <= nh < 16 and 0 <= nt < 16
                assert nv == 0 or (a + nh + rb) % 16 == 0                # vector stores at 16-byte addresses only
                assert clamped == (b - a < (-(a + rb)) % 16)


def test_ring_flush_model_is_the_kernels_split_rule():
    """ring_flush_split(a, b, rb) against lzf_ring_split, the one function OutRing::fill and OutRing::flush take their split from,
    for every rb 0..15, a 0..31 and b - a 0..80: the clamped head, no vector store, one and several, and every tail 0..15."""
    src = os.path.join(HERE, "emu", "emu_ring_split.cpp")
    hdr = os.path.join(os.path.dirname(HERE), "rust-lz-fear_amd", "csrc", "lzf_out_ring.h")
    so = os.path.join(HERE, "emu", "libemu_ring_split.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so, src])
    L = C.CDLL(so)
    L.lzf_emu_ring_split_sweep.restype = None
    L.lzf_emu_ring_split_sweep.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    n_a, n_len = 32, 81
    parts = (C.c_uint32 * (16 * n_a * n_len * 3))()
    L.lzf_emu_ring_split_sweep(n_a, n_len, parts)
    seen_tails, clamped_heads, vecs = set(), 0, set()
    for rb in range(16):
        for a in range(n_a):
            for n in range(n_len):
                k = ((rb * n_a + a) * n_len + n) * 3
                nh, nv, nt, clamped = ac.ring_flush_split(a, a + n, rb)
                assert (nh, nv, nt) == tuple(parts[k:k + 3]), (rb, a, n)
                seen_tails.add(nt); vecs.add(nv); clamped_heads += clamped
    assert seen_tails == set(range(16)) and {0, 1, 2} <= vecs and clamped_heads > 0


def test_tiny_shape():
    s = ac.tiny()
    _common(s)
    assert _pairs(s) == ALL_PAIRS
    for rb in range(16):
        for kind in ("literals", "match"):
            for exact in (True, False):
                ns = sorted(m["n"] for m, ol in zip(s.meta, s.out_low) if ol & 15 == rb and m["kind"] == kind and m["exact"] == exact)
                assert ns == list(range(0 if kind == "literals" else 5, ac.TINY_MAX + 1)), (rb, kind, exact)
    for it, m in zip(s.items, s.meta):
        if m["kind"] == "match":                                         # the block ends in its match, as the KAT 11 61 01 00 does
            assert it["input"][0] >> 4 == 1 and it["input"][2:4] == b"\x01\x00" and len(set(m["decoded"])) == 1
            assert len(it["input"]) == (4 if m["n"] - 1 < 19 else 5)
    assert o.decompress_raw(bytes([0x11, 0x61, 1, 0]))[1] == b"aaaaaa"
    # every branch of the flush of [0, n) at every rb.  (The head is empty where (a + rb) & 15 == 0, so it cannot be clamped there:
    # at rb == 0 the shape must hold a flush with no head instead.)
    for rb in range(16):
        splits = [ac.ring_flush_split(0, m["n"], rb) for m, ol in zip(s.meta, s.out_low) if ol & 15 == rb]
        if rb:
            assert any(c for _, _, _, c in splits), rb                   # nh > b - a
            assert any(nh == 16 - rb and not c and nv for nh, nv, _, c in splits), rb      # a whole head in front of vector stores
        else:
            assert all(nh == 0 for nh, _, _, _ in splits)
        assert any(nv == 0 and nh + nt > 0 for nh, nv, nt, _ in splits), rb                 # no vector part
        assert any(nv > 0 and nt == 0 for _, nv, nt, _ in splits), rb                       # no tail
        assert any(nv > 0 and nt > 0 for _, nv, nt, _ in splits), rb
        assert any(nv >= 2 for _, nv, _, _ in splits), rb


def test_existing_and_prefix_shape():
    s = ac.existing_prefix()
    _common(s)
    assert _pairs(s) == ALL_PAIRS
    ex = [i for i, m in enumerate(s.meta) if m["kind"] == "existing"]
    sh = [i for i, m in enumerate(s.meta) if m["kind"] == "existing short"]
    px = [i for i, m in enumerate(s.meta) if m["kind"] == "prefix"]
    hm = [i for i, m in enumerate(s.meta) if m["kind"] == "existing short, match into it"]
    assert len(ex) + len(sh) + len(hm) + len(px) == len(s.items)
    # handcrafted: the first sequence copies the whole history of e bytes (and on, overlapping), so every byte the fill loaded is read
    assert {(s.meta[i]["e"], s.out_low[i] & 15) for i in hm} == {(e, rb) for e in range(1, 18) for rb in range(16)}
    for i in hm:
        it, (st, b), e = s.items[i], s.expect[i], s.meta[i]["e"]
        assert st == o.OK and len(b) == it["out_cap"] and len(it["existing"]) == e
        assert it["input"][0] >> 4 == 0 and int.from_bytes(it["input"][1:3], "little") == e          # no literals, offset e
        assert b[:e] == it["existing"] and b[e:2 * e] == it["existing"]
    # the decode starts at out + existing_len: every residue of (o + rb) & 15 under every rb, behind a short and a long history
    for idx, base in ((sh, 0), (ex, 20000)):
        assert {(len(s.items[i]["existing"]) % 16, s.out_low[i] & 15) for i in idx} == ALL_PAIRS
        assert {s.meta[i]["e"] for i in idx} == set(range(18))
        assert all(len(s.items[i]["existing"]) == base + s.meta[i]["e"] for i in idx)
        assert all({len(s.items[i]["existing"]) for i in idx if s.out_low[i] & 15 == rb} == set(range(base, base + 18)) for rb in range(16))
    assert {len(s.items[i]["existing"]) for i in sh} == set(range(18))
    # the history of the short ones is loaded by ring_fill(0, e), split like a flush: at every rb its head is clamped for some e
    # (where a head of two bytes or more exists: rb in 1..14) and it has no vector part, head and tail only, for some e
    for rb in range(16):
        fills = [ac.ring_flush_split(0, len(s.items[i]["existing"]), rb) for i in sh if s.out_low[i] & 15 == rb and s.items[i]["existing"]]
        assert len(fills) == 17
        assert rb in (0, 15) or any(c for _, _, _, c in fills), rb       # (rb 15: a head of one byte, which no non-empty range clamps)
        assert rb == 0 or any(nh == e for e, (nh, _, _, _) in enumerate(fills, 1)), rb     # the whole fill is head bytes
        assert any(nv == 0 for _, nv, _, _ in fills), rb
        assert any(nt > 0 and nv == 0 for _, nv, nt, _ in fills), rb
    # ... of the long ones by ring_fill(o - 4096, o): never clamped, always with a vector part
    assert all(not ac.ring_flush_split(len(s.items[i]["existing"]) - 4096, len(s.items[i]["existing"]), s.out_low[i] & 15)[3] for i in ex)
    assert {(s.prefix_low[i] & 15, s.out_low[i] & 15) for i in px} == ALL_PAIRS
    for i in ex + sh + px:
        it, (st, b) = s.items[i], s.expect[i]
        assert st == o.OK and b == s.meta[i]["full"]
        assert len(b) == it["out_cap"]                                   # existing + decoded ends exactly at out_cap
        assert len(it["input"]) < 65536
    assert all(len(s.items[i]["prefix"]) == 20000 for i in px)


def test_handcrafted_shape():
    s = ac.handcrafted()
    _common(s)
    assert _pairs(s) == ALL_PAIRS
    profs = [p for _, _, p in ac.H_STREAMS]
    assert profs == ["classes", "rle", "long", "dense"]
    for p in profs:
        idx = [i for i, m in enumerate(s.meta) if m["kind"] == p]
        assert {s.out_low[i] & 15 for i in idx} == set(range(16)) and len({s.in_low[i] & 15 for i in idx}) >= 4
        blk = s.items[idx[0]]["input"]
        assert 4096 < len(blk) < 65536
        assert {m["exact"] for m in (s.meta[i] for i in idx)} == {True, False}
    first = {m["kind"]: it["input"] for it, m in zip(reversed(s.items), reversed(s.meta))}
    assert ac.max_offset(first["rle"]) <= 9                              # overlapping run-length matches
    assert ac.max_offset(first["classes"]) > 4096 and ac.max_offset(first["long"]) > 4096
    assert len(first["dense"]) >= 3 * 3900                               # 3-byte tokens


def test_segmented_shape():
    s = ac.segmented()
    _common(s)
    good = [i for i, m in enumerate(s.meta) if "decoded" in m]
    rest = [i for i in range(len(s.items)) if i not in set(good)]
    assert all(len(s.items[i]["input"]) >= 65536 for i in good)          # the pipeline's window
    text = [i for i in good if s.meta[i]["kind"] == "text 1 MiB"]
    assert _pairs(s, [i for i in text if s.meta[i]["exact"]]) == ALL_PAIRS
    assert len(s.meta[text[0]]["decoded"]) == 1 << 20
    kinds = ["text 1 MiB", "classes", "rle", "long", "zeros + text + zeros", "300 KB literal run"]
    assert sorted({s.meta[i]["kind"] for i in good}) == sorted(kinds)
    for k in kinds:
        for exact in (True, False):
            idx = [i for i in good if s.meta[i]["kind"] == k and s.meta[i]["exact"] == exact]
            assert {s.out_low[i] & 15 for i in idx} == set(range(16)), (k, exact)
        assert len({s.in_low[i] & 15 for i in good if s.meta[i]["kind"] == k}) >= 8, k
    lit = s.items[[i for i in good if s.meta[i]["kind"] == "300 KB literal run"][0]]["input"]
    assert _longest_literal_run(lit) >= 290000
    z = s.meta[[i for i in good if s.meta[i]["kind"] == "zeros + text + zeros"][0]]["decoded"]
    assert z[:2 << 20] == bytes(2 << 20) and z[-(1 << 20):] == bytes(1 << 20)
    # a tenth of the jobs go to the pair kernel behind the pipeline: not Ok, or one byte short of capacity
    assert len(rest) == len(good) // 10
    short = [i for i in rest if s.meta[i]["kind"] == "short"]
    assert short and all(s.expect[i][0] == o.OUT_CAPACITY for i in short)
    dam = [i for i in rest if s.meta[i]["kind"] == "damaged"]
    assert len({s.expect[i][0] for i in dam}) >= 2 and any(s.expect[i][0] != o.OK for i in dam)
    assert all(len(s.items[i]["input"]) >= 65536 // 3 for i in dam)
    # (a truncated block may fall below the pipeline's window; enough non-Ok jobs stay inside it to be handed over by the pipeline)
    assert sum(s.expect[i][0] != o.OK and len(s.items[i]["input"]) >= 65536 for i in rest) >= len(rest) // 2


def _longest_literal_run(blk):
    p, n, best = 0, len(blk), 0
    while p < n:
        t = blk[p]; p += 1; L = t >> 4
        if L == 15:
            while True:
                b = blk[p]; p += 1; L += b
                if b != 255:
                    break
        best = max(best, L); p += L
        if n - p < 2:
            break
        p += 2
        if (t & 15) == 15:
            while blk[p] == 255:
                p += 1
            p += 1
    return best


def test_fed_shape():
    blocks = ac.fed_blocks()
    assert 8 <= len(blocks) <= 16 and len({c for _, c in blocks}) == len(blocks)
    for d, c in blocks:
        assert 200000 <= len(d) <= 400000 and len(c) >= 65536
        assert ac.max_offset(c) > 4096                                   # sources further back than the 4 KiB ring: re-read from `out`
        assert o.decompress_raw(c, limit=len(d), cap=len(d)) == (0, d)
    assert any(len(c) > 262144 for _, c in blocks)
    n = 700
    s = ac.fed(n, blocks=blocks)
    _common(s)
    assert len(s.items) == n and _pairs(s) == ALL_PAIRS and _pairs(s, range(256, 512)) == ALL_PAIRS
    assert all(it["out_cap"] == it["limit"] == len(blocks[m["block"]][0]) for it, m in zip(s.items, s.meta))
    bad = [i for i, m in enumerate(s.meta) if m["kind"] == "damaged"]
    assert len(bad) == n // 10 and any(s.expect[i][0] != o.OK for i in bad)
    # inputs are shared: one object per (block, kind)
    assert len({id(it["input"]) for it in s.items}) <= 2 * len(blocks)
    assert {m["block"] for m in s.meta} == set(range(len(blocks)))


def test_compress_shape():
    s = ac.compress()
    _common(s, decompress=False)
    u32 = [i for i, m in enumerate(s.meta) if m["kind"] == "u32"]
    u16 = [i for i, m in enumerate(s.meta) if m["kind"] == "u16"]
    cur = [i for i, m in enumerate(s.meta) if m["kind"] == "cursor"]
    assert len(u32) + len(u16) + len(cur) == len(s.items)
    assert _pairs(s, u32) == ALL_PAIRS
    assert {s.in_low[i] & 15 for i in u16} == set(range(16)) == {s.in_low[i] & 15 for i in cur}
    assert {s.out_low[i] & 15 for i in u16} == set(range(16)) == {s.out_low[i] & 15 for i in cur}
    lens = {s.meta[i]["n"] for i in u32}
    assert set(range(41)) | {63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, 200000, 1 << 20} <= lens
    assert all(s.meta[i]["n"] <= 65535 and s.items[i]["kind"] == o.TABLE_U16 for i in u16) and 65535 in {s.meta[i]["n"] for i in u16}
    assert {s.items[i]["cursor"] for i in cur} == set(ac.C_CURSORS)
    assert any(s.items[i]["cursor"] > s.meta[i]["n"] for i in cur)
    for n in range(41):                                                   # the ragged last 16 bytes at every out residue
        assert {s.out_low[i] & 15 for i in u32 if s.meta[i]["n"] == n and s.items[i]["out_cap"] == s.meta[i]["C"]} == set(range(16)), n
    for i, (it, (st, b), m) in enumerate(zip(s.items, s.expect, s.meta)):
        assert m["status_full"] == o.OK
        cap, C = it["out_cap"], m["C"]
        assert cap in (max(C - 1, 0), C, m["n"])
        if cap >= C:
            assert st == o.OK and len(b) == C
        else:
            assert st == o.OUTPUT_FULL                                   # a cap of C - 1 is refused
    for kind in (u32, u16, cur):
        assert {o.OK, o.OUTPUT_FULL} <= {s.expect[i][0] for i in kind}
        assert any(s.items[i]["out_cap"] == s.meta[i]["C"] for i in kind)


def test_chunks_leave_nothing_out():
    s = ac.tiny()
    for lo, hi in ((0, 256), (1024, 2048), (2048, 3072), (16384, 1 << 20)):
        cs = ac.chunks(s, lo, hi)
        assert all(lo < len(c.items) <= hi for c in cs)
        seen = {id(it) for c in cs for it in c.items}
        assert seen == {id(it) for it in s.items}
