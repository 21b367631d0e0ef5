"""Job lists for the buffer-alignment sweep (CPU-side; tests/test_alignment_cases_cpu.py checks the shapes, tests/test_gpu_alignment.py
and tests/alignment_check.py run them through tests/redzone.py with explicit placement).

Every decompress kernel flushes its LDS ring to `out` as a byte-wise head up to the next 16-byte address, 16-byte vector stores and
a byte-wise tail, all computed from rb = out & 15 (lz4_decompress_paired.hip ring_flush, lz4_decompress_fed.hip,
lz4_seg_resolve.hip flush_range / fill_to, lz4_decompress_batched.hip); the compress kernels read and write with unaligned
8 / 16-byte accesses.  Each builder below returns a Shape: `items` (as ffi.decompress_blocks_host / compress_blocks_host), `expect`
((status, bytes) from the oracle), the low address bits `in_low` / `out_low` / `prefix_low` of every job, and `meta` (what the job is
there for, for the structural checks).

    T  decoded length 0..48 at every rb: literal-only and "1 literal + run-length match" blocks, exact and slack capacity
    E  a 50 KB text block behind existing output of e and of 20000 + e bytes (e in 0..17) and behind a prefix at every pointer residue
    H  handcrafted streams below 64 KiB of input (two-ended copies, overlapping run-length matches, multi-KiB matches, 3-byte tokens)
    S  the segmented pipeline's window (input >= 64 KiB): a 1 MiB text block at all 256 (input & 15, out & 15) pairs and five
       other blocks at every rb; a tenth damaged or one byte short of capacity
    F  the bitmap-fed kernel's window: 12 blocks of 200..400 KB with far matches, inputs shared, every job its own exact-fit output
    C  compress: the lengths around every size rule, caps C - 1 / C / N, U32 / U16 tables, cursor > 0 behind a prefix
"""
from collections import namedtuple

import numpy as np

import oracle_ffi as o
import vectors
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import synth

Shape = namedtuple("Shape", "items expect in_low out_low prefix_low meta")

TINY_MAX = 48


def _shape():
    return Shape([], [], [], [], [], [])


def _add(s, item, expect, in_low, out_low, prefix_low=0, **meta):
    s.items.append(item); s.expect.append(expect)
    s.in_low.append(in_low & 255); s.out_low.append(out_low & 255); s.prefix_low.append(prefix_low & 255)
    s.meta.append(meta)


def concat(*shapes):
    r = _shape()
    for s in shapes:
        for f, g in zip(r, s):
            f.extend(g)
    return r


def take(s, idx):
    return Shape(*[[f[i] for i in idx] for f in s])


def chunks(s, lo, hi):
    """The jobs of `s` in calls of lo < n <= hi jobs each, none left out; a call that would be too small is filled up with jobs
    from the front of `s` (run twice rather than dropped)."""
    n = len(s.items)
    assert 0 <= lo < hi
    k = max(1, -(-n // hi))
    out = []
    for c in range(k):
        idx = list(range(c * n // k, (c + 1) * n // k))
        j = 0
        while len(idx) <= lo:
            idx.append(j % n); j += 1
        assert lo < len(idx) <= hi
        out.append(take(s, idx))
    return out


def residues(in_ptrs, out_ptrs):
    """16 x 16 histogram of (input & 15, out & 15) from device addresses."""
    h = np.zeros((16, 16), dtype=np.int64)
    np.add.at(h, (np.asarray(in_ptrs, dtype=np.uint64) & np.uint64(15), np.asarray(out_ptrs, dtype=np.uint64) & np.uint64(15)), 1)
    return h


def ring_flush_split(a, b, rb):
    """Byte-wise model of ring_flush(a, b) of a kernel whose out & 15 is rb: (head bytes, 16-byte vector stores, tail bytes, whether
    the head was clamped to the range)."""
    nh = (16 - ((a + rb) & 15)) & 15
    clamped = nh > b - a
    nh = min(nh, b - a)
    a += nh
    nv = (b - a) >> 4
    a += nv << 4
    return nh, nv, b - a, clamped


def max_offset(blk):
    """The largest match offset of a valid block."""
    p, n, best = 0, len(blk), 0
    while p < n:
        t = blk[p]; p += 1; L = t >> 4
        if L == 15:
            while True:
                b = blk[p]; p += 1; L += b
                if b != 255:
                    break
        p += L
        if n - p < 2:
            break
        best = max(best, blk[p] | (blk[p + 1] << 8)); p += 2
        if (t & 15) == 15:
            while blk[p] == 255:
                p += 1
            p += 1
    return best


# ------------------------------------------------------------------------------------------------------------------------------ T
def tiny():
    """16 rb x decoded lengths 0..48 x {literal-only, 1 literal + run-length match (n >= 5: a match has four bytes at least)} x
    {out_cap == n, out_cap == n + input_len + 64}; the input residue cycles with the job number, so every (input & 15, out & 15)
    pair occurs."""
    from test_gpu_fed_decode_once import _seq
    s = _shape()
    k = 0
    for rb in range(16):
        for n in range(TINY_MAX + 1):
            lit = vectors.rng_bytes(5000 + n, n)
            blocks = [("literals", _seq(lit, None, 0), lit)]
            if n >= 5:
                c = bytes([0x41 + n])
                blocks.append(("match", _seq(c, 1, n - 1), c * n))
            for kind, blk, dec in blocks:
                for slack in (0, len(blk) + 64):
                    cap = n + slack
                    _add(s, dict(input=blk, limit=n, out_cap=cap), o.decompress_raw(blk, limit=n, cap=cap),
                         (k % 16) | ((k // 16 % 16) << 4), rb | ((k % 13) << 4), kind=kind, n=n, decoded=dec, exact=slack == 0)
                    k += 1
    return s


# ------------------------------------------------------------------------------------------------------------------------------ E
def existing_prefix():
    """The 50 KB text block of test_decompress_prefix_and_existing_output, compressed behind its first bytes: as existing output of
    e bytes (e in 0..17: the history is shorter than any ring, ring_fill(0, e)) and of 20000 + e bytes (a ring's worth of history,
    ring_fill(o - RING, o)) — the decode starts at out + existing_len, every residue of o + rb — at every rb, and behind a prefix at
    every prefix-pointer residue and every rb.  out_cap is exactly what the job fills."""
    s = _shape()
    d = synth.gen_text_zipf(31, 50000).tobytes()
    k = 0
    for e in range(18):
        cut = 20000 + e
        comp = o.compress2(d, cursor=cut)[1]
        for rb in range(16):
            it = dict(input=comp, existing=d[:cut], limit=len(d), out_cap=len(d))
            _add(s, it, o.decompress_raw(comp, existing=d[:cut], limit=len(d), cap=len(d)), (k + k // 16) % 16, rb | ((k % 7) << 4), kind="existing", e=e, full=d)
            k += 1
    # existing output shorter than any ring: the history is loaded by ring_fill(0, e) — a clamped head, no vector part
    for e in range(18):
        comp = o.compress2(d, cursor=e)[1]
        for rb in range(16):
            it = dict(input=comp, existing=d[:e], limit=len(d), out_cap=len(d))
            _add(s, it, o.decompress_raw(comp, existing=d[:e], limit=len(d), cap=len(d)), (k + k // 16) % 16, rb | ((k % 7) << 4), kind="existing short", e=e, full=d)
            k += 1
    # ... and a block whose first sequence is a match over all e bytes of that history (an encoder's first match rarely reaches
    # back to the first bytes; this one reads every byte ring_fill(0, e) loaded), then one into what that match wrote
    from test_gpu_fed_decode_once import _seq
    for e in range(1, 18):
        hist = vectors.rng_bytes(7000 + e, e)
        blk = _seq(b"", e, e + 21) + _seq(b"xy", e + 3, 40) + _seq(b"tail.", None, 0)
        for rb in range(16):
            cap = e + e + 21 + 2 + 40 + 5
            it = dict(input=blk, existing=hist, limit=cap, out_cap=cap)
            _add(s, it, o.decompress_raw(blk, existing=hist, limit=cap, cap=cap), (k + k // 16) % 16, rb | ((k % 7) << 4), kind="existing short, match into it", e=e)
            k += 1
    dic, payload = d[:20000], d[20000:]
    comp = o.compress2(d, cursor=len(dic))[1]
    for pl in range(16):
        for rb in range(16):
            it = dict(input=comp, prefix=dic, limit=len(payload), out_cap=len(payload))
            _add(s, it, o.decompress_raw(comp, prefix=dic, limit=len(payload), cap=len(payload)), (k + k // 16) % 16, rb | ((k % 5) << 4),
                 pl | ((k % 3) << 4), kind="prefix", full=payload)
            k += 1
    return s


# ------------------------------------------------------------------------------------------------------------------------------ H
H_STREAMS = [(31, 3000, "classes"), (32, 1500, "rle"), (33, 36, "long"), (34, 4000, "dense")]


def handcrafted():
    """vectors.synth_stream blocks below 64 KiB of input, each at every rb and four input residues; over the four profiles every
    (input & 15, out & 15) pair occurs.  Exact and slack capacity alternate."""
    s = _shape()
    for pi, (seed, nseq, prof) in enumerate(H_STREAMS):
        blk, dec = vectors.synth_stream(seed, nseq, prof)
        for rb in range(16):
            for q in range(4):
                cap = len(dec) + ((len(blk) + 64) if (rb + q) % 2 else 0)
                _add(s, dict(input=blk, limit=len(dec), out_cap=cap), (0, dec), ((4 * q + pi + rb) % 16) | (q << 4), rb | (pi << 4),
                     kind=prof, decoded=dec, exact=cap == len(dec))
    return s


# ------------------------------------------------------------------------------------------------------------------------------ S
def _seg_blocks():
    mib = 1 << 20
    out = []
    for seed, nseq, prof in [(41, 8000, "classes"), (42, 13000, "rle"), (43, 120, "long")]:
        blk, dec = vectors.synth_stream(seed, nseq, prof)
        out.append((prof, blk, dec))
    d = bytes(2 * mib) + synth.gen_text_zipf(7, 300000).tobytes() + bytes(mib)          # (the block of _seg_mixed_items)
    out.append(("zeros + text + zeros", o.compress2(d)[1], d))
    d = synth.gen_text_zipf(8, 200000).tobytes() + synth.gen_random(9, 300000).tobytes() + synth.gen_text_zipf(8, 400000).tobytes()
    out.append(("300 KB literal run", o.compress2(d)[1], d))
    return out


def segmented(seed=811):
    """Blocks of 64 KiB and more of input: a 1 MiB text block at all 256 (input & 15, out & 15) pairs with exact capacity and at
    every rb with slack, five other blocks at every rb with both capacities (the input residue cycles) — and a tenth as many jobs
    that the pipeline hands to the pair kernel: damaged blocks and blocks one byte short of capacity."""
    from test_gpu_hardening import _damage
    rng = np.random.default_rng(seed)
    s = _shape()
    d = synth.gen_text_zipf(100, 1 << 20).tobytes()
    c = o.compress2(d)[1]
    for il in range(16):
        for rb in range(16):
            _add(s, dict(input=c, limit=len(d), out_cap=len(d)), (0, d), il | (rb << 4), rb | (il << 4), kind="text 1 MiB", decoded=d, exact=True)
    k = 0
    for name, blk, dec in [("text 1 MiB", c, d)] + _seg_blocks():
        for rb in range(16):
            for slack in ((len(blk) + 64,) if name == "text 1 MiB" else (0, len(blk) + 64)):
                _add(s, dict(input=blk, limit=len(dec), out_cap=len(dec) + slack), (0, dec), (k * 5 + 3) % 16 | ((k % 11) << 4), rb | ((k % 9) << 4),
                     kind=name, decoded=dec, exact=slack == 0)
                k += 1
    good = list(range(len(s.items)))
    for t in range(len(good) // 10):
        i = good[(t * 37 + 5) % len(good)]
        blk, dec = s.items[i]["input"], s.meta[i]["decoded"]
        if t % 3 == 2:
            it = dict(input=blk, limit=len(dec), out_cap=len(dec) - 1)
            why = "short"
        else:
            m = _damage(rng, blk, t % 4)
            it = dict(input=m, limit=len(dec), out_cap=len(dec) + len(m) + 64)
            why = "damaged"
        _add(s, it, o.decompress_raw(it["input"], limit=it["limit"], cap=it["out_cap"]), (t * 3 + 1) % 16, (t * 7 + 3) % 16 | ((t % 5) << 4), kind=why)
    return s


# ------------------------------------------------------------------------------------------------------------------------------ F
def fed_blocks():
    """12 distinct blocks of 200..400 KB whose compressed length is >= 65536 (one > 262144), each with matches further back than the
    fed kernel's 4 KiB ring: (raw, compressed)."""
    raws = [synth.silesia_mix(k << 20, (k << 20) + ln).tobytes() for k, ln in ((0, 200000), (12, 206000), (40, 212000), (70, 390000), (100, 224000), (130, 230000),
                                                                                (150, 236000), (170, 242000), (180, 248000), (160, 254000))]
    t = synth.gen_text_zipf(77, 150000).tobytes()
    raws.append(t[:50000] + synth.gen_random(5, 270000).tobytes() + t[70000:])          # (compressed > 262144)
    raws.append(synth.gen_markup(6, 120000).tobytes() + synth.gen_random(7, 60000).tobytes() + synth.gen_markup(6, 180000).tobytes()[100000:] + synth.gen_log(8, 100000).tobytes())
    return [(d, o.compress2(d)[1]) for d in raws]


def fed(n_jobs, seed=523, blocks=None):
    """n_jobs jobs over fed_blocks(): job i reads block i % 12 at input residue i & 15 and writes at rb (i >> 4) & 15, so every 256
    consecutive jobs hold every residue pair; jobs that read the same block at the same residue share the input object (pass
    alias_inputs to the harness).  Every output has exactly the decoded size.  Every tenth job reads a damaged block."""
    from test_gpu_hardening import _damage
    rng = np.random.default_rng(seed)
    blocks = blocks if blocks is not None else fed_blocks()
    bad = []
    for k, (d, c) in enumerate(blocks):
        m = _damage(rng, c, k % 4)
        bad.append((m, o.decompress_raw(m, limit=len(d), cap=len(d))))
    s = _shape()
    for i in range(n_jobs):
        k = i % len(blocks)
        d, c = blocks[k]
        lows = ((i & 15) | ((k % 16) << 4), ((i >> 4) & 15) | ((i % 11) << 4))
        if i % 10 == 3:
            _add(s, dict(input=bad[k][0], limit=len(d), out_cap=len(d)), bad[k][1], *lows, kind="damaged", block=k)
        else:
            _add(s, dict(input=c, limit=len(d), out_cap=len(d)), (0, d), *lows, kind="good", block=k, decoded=d, exact=True)
    return s


# ------------------------------------------------------------------------------------------------------------------------------ C
C_CURSORS = (1, 7, 15, 16, 17, 100, 65537)


def _compress_inputs():
    ins = [("len%d" % n, synth.gen_text_zipf(900 + n, max(n, 1)).tobytes()[:n]) for n in list(range(41)) + [63, 64, 65, 4095, 4096, 4097]]
    ins += [("len%d" % n, synth.silesia_mix(3 << 20, (3 << 20) + n).tobytes()) for n in (65535, 65536, 65537)]
    ins += [("text 200 KB", synth.gen_text_zipf(12, 200000).tobytes()), ("mix 1 MiB", synth.silesia_mix(9 << 20, 10 << 20).tobytes()),
            ("noise", vectors.rng_bytes(21, 70001)), ("zeros", bytes(100003)), ("repeat256", synth.repeat256(65535).tobytes())]
    return ins


def compress():
    """Compress jobs: meta kind "u32" (fresh U32 table, cursor 0), "u16" (inputs of up to 65535 bytes), "cursor" (cursor > 0 behind a
    prefix, and cursor = 65537 beyond most inputs).  Caps C - 1, C and N for every input; the inputs of up to 40 bytes also at every
    out residue.  The residue pair advances with the job number, so the u32 jobs alone hold all 256 pairs."""
    s = _shape()
    ins = _compress_inputs()
    p = [0]

    def add(d, kind, why, cursor=0, caps=None, out_res=None):
        full = o.compress2(d, cursor=cursor, kind=kind)
        C = len(full[1])
        for cap in (caps if caps is not None else sorted({max(C - 1, 0), C, len(d)})):
            it = dict(input=d, out_cap=cap, kind=kind, cursor=cursor)
            ol = out_res if out_res is not None else p[0] // 16 % 16 if why == "u32" else (p[0] * 7 + p[0] // 16) % 16
            _add(s, it, o.compress2(d, cursor=cursor, kind=kind, cap=cap), (p[0] % 16) | ((p[0] % 7) << 4), ol | ((p[0] % 5) << 4),
                 kind=why, C=C, status_full=full[0], n=len(d))
            p[0] += 1

    for name, d in ins:
        add(d, o.TABLE_U32, "u32")
    while p[0] < 256:                                  # (the short ones again, until the advancing residue pair has been everywhere)
        for name, d in ins[:41]:
            add(d, o.TABLE_U32, "u32")
    for name, d in ins[:41]:                           # every out residue for the ragged last 16 bytes of a short block
        full = o.compress2(d)
        for r in range(16):
            add(d, o.TABLE_U32, "u32", caps=[len(full[1])], out_res=r)
    for name, d in ins:
        if len(d) <= 65535:
            add(d, o.TABLE_U16, "u16")
    for name, d in ins:
        if len(d) >= 200:
            for cur in C_CURSORS:
                add(d, o.TABLE_U32, "cursor", cursor=cur)
    return s
