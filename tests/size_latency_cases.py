"""Cases of the size call's latency class (lz4_decoded_size_seg.hip; the rule: lzf_size_rules.h TileSum / summarise / clean), shared by
tests/test_size_tiles_cpu.py and tests/test_gpu_size_latency.py.  Plain Python and numpy + the oracle for the expectations.

A case is decoded_size_cases' dict (input, prefix_len, existing_len, limit, prefix, existing) with a name; its expectation is the
oracle's (status, output.len() or None).  The class answers a job — "finishes" it — iff the oracle says Ok and no literal or match
length is beyond the clamp; every other job it must leave alone."""
import numpy as np

import decoded_size_cases as D
import seg_stage_cases as S

TILE, CHUNK = S.TILE, S.CHUNK
NO_LIMIT = 1 << 24                                     # far beyond every case's output (the oracle allocates what a limit allows)
PRE_EX = ((0, 0), (37, 0), (0, 53), (37, 53))          # prefix and existing output: each none and some


def named(name, data, limit, prefix=b"", existing=b""):
    c = D.make_case(data, limit, prefix, existing)
    c["name"] = name
    return c


def exceeds_clamp(c):
    """A literal or match length beyond kLenClamp: the tile decoder gives such a job up (a run of 263 173 0xFF bytes at the least)."""
    if b"\xff" * (S.LEN_CLAMP // 255 - 10) not in c:
        return False
    toks, _ = S.Parse(c).chain(0)
    return any(t[1] > S.LEN_CLAMP or t[2] > S.LEN_CLAMP + 4 for t in toks)


def finishes(case, exp):
    return exp[0] == 0 and not exceeds_clamp(case["input"])


def _bytes(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def _front(seed, start):
    """A block whose next token starts at compressed position `start`."""
    b = S.Blk(seed)
    b.near(20, 5).small_until(start - 300).to_c(start)
    assert b.cpos == start
    return b


def _patch_offset(b, at, off):
    c = bytearray(b.c); c[at + 1:at + 3] = int(off).to_bytes(2, "little"); b.c = c


M_TEST = 9


def boundary_cases():
    """The sequence under test (no literals, a match of 9) is the last token of tile 0 (it starts three bytes in front of the tile's end)
    and then the first of tile 1; behind it only the last literals, which no rule checks.  mo = the output position of its match."""
    out = []
    rng = np.random.default_rng(2026)
    for place, start in (("last of a tile", TILE - 3), ("first of the next tile", TILE)):
        for plen, elen in PRE_EX:
            prefix, existing = _bytes(rng, plen), _bytes(rng, elen)
            tag = f"{place}, prefix {plen}, existing {elen}"

            def build(off=None):
                b = _front(71, start)
                at, mo = b.cpos, b.opos
                b.seq(0, 7, M_TEST)
                if off is not None:
                    _patch_offset(b, at, off)
                return b, at, mo
            b, at, mo = build()
            assert at == start and seq_tile(at) == (0 if start < TILE else 1)
            c, _ = b.end(5)
            # a match that ends exactly at output_limit, and one byte past it (the last literals are not limit-checked)
            out.append(named(f"limit exact: {tag}", c, elen + mo + M_TEST, prefix, existing))
            out.append(named(f"limit one past: {tag}", c, elen + mo + M_TEST - 1, prefix, existing))
            # an offset that reaches exactly the first byte of prefix + existing + output, and one beyond
            reach = plen + elen + mo
            assert reach + 1 <= 0xFFFF
            for name, off in (("offset to the first byte", reach), ("offset one beyond the first byte", reach + 1), ("offset zero", 0)):
                b, at, mo = build(off)
                c, _ = b.end(5)
                out.append(named(f"{name}: {tag}", c, NO_LIMIT, prefix, existing))
            # a late violation (offset zero, two tiles on) behind an early one (the offset one beyond, at the place under test)
            b, at, mo = build(reach + 1)
            b.small_until(b.cpos + 2 * TILE)
            late = b.cpos
            b.seq(0, 5, M_TEST); _patch_offset(b, late, 0)
            b.small_until(b.cpos + 500)
            c, _ = b.end(5)
            out.append(named(f"late violation behind an early one: {tag}", c, NO_LIMIT, prefix, existing))
    return out


def seq_tile(pos):
    return pos // TILE


def stage_cases():
    """The seam, tile and damaged cases of seg_stage_cases.py as size jobs (out_cap is not a size job's business)."""
    return [named("stage/" + c["name"], c["input"], c["limit"]) for c in S.seam_cases() + S.tile_cases() + S.damaged_cases()]


def _valid_of_length(seed, n):
    """A valid block of exactly n compressed bytes (n >= 40)."""
    b = S.Blk(seed)
    b.near(20, 5)
    if n > 600:
        b.small_until(n - 300)
    b.to_c(n - 6)
    c, o = b.end(5)
    assert len(c) == n, (len(c), n)
    return c, o


def size_edge_cases():
    """Input lengths at the tile's and the chunk's edges, 65 tiles (the finish kernel's second round), an empty and a one-token input, and
    "one byte left after the literals" (read_u16 fails, decompress.rs:70: the block ends Ok) on a tile's and a chunk's last byte."""
    out = []
    for n in (TILE, TILE + 1, CHUNK, CHUNK + 1, 64 * TILE + 100):
        c, o = _valid_of_length(200 + n % 97, n)
        out.append(named(f"edge/input of {n} bytes", c, len(o)))
    assert S.seg_ntile(64 * TILE + 100) == 65
    out.append(named("edge/empty input", b"", 100))
    out.append(named("edge/one token", b"\x00", 100))
    out.append(named("edge/one token, three literals", b"\x30abc", 100))
    # a clean match length of 2^24 or more (25.5 million: 100 000 0xFF bytes), ordinary sequences around it in its round: the tile kernel's
    # scan in 16-bit halves, and tiles without a token behind it
    b = S.Blk(402)
    b.near(20, 5).small_until(3000)
    b.seq(3, 1, 19 + 255 * 100000 + 17)
    b.small_until(b.cpos + 3000)
    c, o = b.end(5)
    assert (1 << 24) <= 19 + 255 * 100000 + 17 <= S.LEN_CLAMP and not exceeds_clamp(c)
    out.append(named("edge/a clean match length of 25 million", c, len(o)))
    for n, what in ((TILE, "a tile's"), (CHUNK, "a chunk's")):
        b = S.Blk(300 + n % 89)
        b.near(20, 5).small_until(n - 400).to_c(n - 8)
        c = bytes(b.c) + b"\x60" + b"sixlit" + b"\x07"       # token, six literals, one stray byte: the input's last byte is byte n - 1
        assert len(c) == n
        out.append(named(f"edge/one byte left after the literals on {what} last byte", c, len(b.o) + 6))
    return out


def long_run_case():
    """A match length of 300 000 0xFF bytes (76.5 million: beyond kLenClamp) between ordinary sequences: the one-wave kernel's."""
    b = S.Blk(401)
    b.near(20, 5).small_until(3000)
    b.seq(3, 1, 19 + 255 * 300000 + 17)
    b.small_until(b.cpos + 3000)
    c, o = b.end(5)
    assert exceeds_clamp(c)
    return named("edge/0xFF match-length run of 300 000 bytes", c, len(o))


def mutated_cases(n=200, seed=20261019):
    """n mutated blocks (decoded_size_cases.mutate) of valid blocks of one to a dozen tiles, both limits."""
    rng = np.random.default_rng(seed)
    base = []
    for k, size in enumerate((300, 2500, 5000, 9000, 24000)):
        b = S.Blk(500 + k)
        b.near(20, 5).small_until(size)
        base.append(b.end(5))
    out = []
    for i in range(n):
        c, o = base[i % len(base)]
        m = D.mutate(rng, c)
        out.append(named(f"mutated/{i}", m, len(o) if i % 2 == 0 else len(o) // 2 + 1))
    return out
