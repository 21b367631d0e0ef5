"""Handcrafted raw blocks for the SET-UP of a batch in the bitmap-fed decompress kernel (test infrastructure; used by
tests/test_fed_setup_cases_cpu.py on the CPU and tests/test_gpu_fed_setup.py on the GPU).

The set-up (lz4_decompress_batch_phase.inc under LZF_FED_DECODE, from the token decode to the error tests) reads a token's match offset
and match-length byte in one 4-byte read where all four bytes are staged, tests a batch's bounds once (where the batch ends, against
capacity and limit) and both offset errors in one compare per lane, and works out the exact status only when one of those flags
something.  Every block here puts one edge of that where it matters; `layout` is the host model of windows, batches and lanes (held to
the emulator of the window loop by the CPU test), `census` names the edges a case reaches, and the oracle gives every case's status."""
import numpy as np

from seg_stage_cases import _seq, _walk
from fed_window_cases import CARRY, ROUND

STAGED = ROUND + 128      # kCB: bytes of a window staged in LDS
SPAN_MAX = 4096 // 3      # kSpanMax
TOT_CLAMP = 1 << 25
OK, UNEXPECTED_END, MEMORY_LIMIT_EXCEEDED, ZERO_OFFSET, INVALID_OFFSET, OUTPUT_FULL, CONTRACT, OUT_CAPACITY = range(8)      # oracle_ffi

RQ_SWEEP = tuple(range(STAGED - 8, STAGED + 5))
M_KINDS = {"nibble < 15": 8, "nibble 15, m1 0": 19, "nibble 15, m1 254": 19 + 254, "nibble 15, m1 255": 19 + 255}
LANES = ("lane 0", "a middle lane", "lane nb - 1")


def staged_class(rq):
    return ("four bytes fit" if rq + 4 <= STAGED else "two fit, four do not" if rq + 2 <= STAGED else
            "straddles the staged bytes" if rq < STAGED else "past the staged bytes")


def edges():
    e = [f"offset at staged position {rq}, {k}" for rq in RQ_SWEEP for k in M_KINDS]
    e += [f"offset: {c}" for c in ("four bytes fit", "two fit, four do not", "straddles the staged bytes", "past the staged bytes")]
    e += ["end: last match's offset at len - 2", "end: last literals, q == len", "end: last literals, q + 1 == len",
          "end: extended match, q + 2 == len", "end: extended match, q + 3 == len"]
    e += ["bounds: cap == out_len", "bounds: cap == out_len - 1", "bounds: limit == out_len", "bounds: limit == out_len - 1",
          "bounds: limit below out_len by the last literals only", "bounds: a literal of lane k > 0 does not fit",
          "bounds: a match byte of lane k does not fit", "bounds: a literal of the batch's last lane does not fit",
          "bounds: a match byte of the batch's last lane does not fit"]
    for lane in LANES:
        e += [f"offsets: off == mo, no prefix, {lane}", f"offsets: off == mo + 1, no prefix, {lane}", f"offsets: off == 0, {lane}",
              f"offsets: off == 0xFFFF, {lane}"]
        for plen in (1, 300):
            e += [f"offsets: off == mo + plen, prefix {plen}, {lane}", f"offsets: off == mo + plen + 1, prefix {plen}, {lane}"]
    e += ["order: two damaged sequences in one batch, the first wins", "order: zero offset in front of an exceeded limit, one batch",
          "order: zero offset and exceeded limit in one sequence", "order: damage in the second batch of a window"]
    return e


# ---------------------------------------------------------------------------------------------------------------------- building
def enc(seqs, tail=b"tail!", have=0, seed=1):
    """seqs: (L, M) or (L, M, off) -> the block's bytes; an offset not given is drawn from the output so far (`have` bytes of prefix and
    existing output in front).  tail None: no last literals, the block ends behind its last match."""
    rng = np.random.default_rng(seed)
    out_len, blk = have, bytearray()
    for s in seqs:
        L, M = s[0], s[1]
        lit = bytes(rng.integers(0, 256, L, dtype=np.uint8))
        out_len += L
        assert out_len >= 1, "a match needs output before it"
        off = s[2] if len(s) > 2 else int(rng.integers(1, min(out_len, 3000) + 1))
        blk += _seq(lit, off, M)
        out_len += M
    if tail is not None:
        blk += _seq(tail, None, 0)
    return bytes(blk)


def layout(blk, base=0):
    """The fed kernel's windows and batches over a block whose tokens can be walked: one record per token — pos, L, M, q (where its offset
    stands), cstart of the window that decodes it, rq = q - cstart, window and batch numbers, first (the window's first batch), lane, nb (0: a
    solo sequence), lo and mo (output positions of its literals and its match, `base` bytes of existing output in front)."""
    toks, n = _walk(blk), len(blk)
    recs, i, o, win, nbatch = [], 0, base, 0, 0
    while i < len(toks):
        cstart = toks[i][0] & ~31
        lst = [t for t in toks[i:] if t[0] - cstart < ROUND]
        tc, tidx = len(lst), 0
        while tidx < tc:
            if tidx > 0 and tc - tidx <= CARRY and cstart + ROUND < n:
                break
            nb_try = min(64, tc - tidx)
            incl = np.cumsum([min(L + M, TOT_CLAMP) for _, L, M, _ in lst[tidx:tidx + nb_try]])
            over = np.nonzero(incl > SPAN_MAX)[0]
            nb = min(int(over[0]) if len(over) else 64, nb_try)
            for j in range(max(nb, 1)):
                p, L, M, _ = lst[tidx + j]
                q = p + 1 + (0 if L < 15 else 1 + (L - 15) // 255) + L
                lo = o + (int(incl[j]) - (L + M) if nb else 0)
                recs.append(dict(pos=p, L=L, M=M, q=q, cstart=cstart, rq=q - cstart, win=win, batch=nbatch, first=tidx == 0, lane=j, nb=nb, lo=lo, mo=lo + L))
            o += int(incl[max(nb, 1) - 1])
            tidx += max(nb, 1); nbatch += 1
        i += tidx; win += 1
    return recs


def case(name, blk, wants, prefix=b"", existing=b"", limit=None, cap=None, rb=0, status=OK):
    return dict(name=name, input=bytes(blk), prefix=prefix, existing=existing, limit=limit, cap=cap, rb=rb, wants=set(wants), status=status)


def _rnd(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


# ------------------------------------------------------------------------------------------------------------------------ the cases
def sweep_cases():
    """A token in the second batch of the first window (64 three-byte tokens in front of it, 44 tokens in its own batch: not carried) whose
    literal run, swept byte by byte, puts its offset at every staged position around the end of the staged bytes."""
    out = []
    for kind, M in M_KINDS.items():
        for L in range(160, 200):
            seqs = [(1, 4)] + [(0, 4)] * 63 + [(216, 4)] * 3 + [(0, 4)] * 40 + [(L, M)] + [(3, 5)] * 6
            blk = enc(seqs, seed=L)
            r = layout(blk)[64 + 43]
            assert r["L"] == L and r["M"] == M
            if r["rq"] in RQ_SWEEP and r["cstart"] == 0 and r["batch"] == 1 and r["nb"] == 44:
                out.append(case(f"sweep: rq {r['rq']}, {kind}", blk, [f"offset at staged position {r['rq']}, {kind}", f"offset: {staged_class(r['rq'])}"]))
    return out


def end_cases():
    base = [(5, 8)] * 10
    out = [case("end: block ends behind a match's offset", enc(base, tail=None), ["end: last match's offset at len - 2"]),
           case("end: last literals", enc(base, tail=b"abc"), ["end: last literals, q == len"]),
           case("end: one byte behind the last literals", enc(base, tail=b"abc") + b"\x00", ["end: last literals, q + 1 == len"])]
    blk = enc(base + [(3, 19)], tail=None)              # ... token, 3 literals, offset, m1 = 0
    out.append(case("end: extended match, its length byte the last byte", blk, ["end: extended match, q + 3 == len"]))
    out.append(case("end: extended match, its length byte missing", blk[:-1], ["end: extended match, q + 2 == len"], status=UNEXPECTED_END))
    return out


def bounds_cases(decode):
    """decode(blk) -> the oracle's output of a valid block (for out_len)."""
    seqs = [(3, 6)] * 70
    tail = b"the end!!"
    blk = enc(seqs, tail=tail)
    n = len(decode(blk))
    lay = layout(blk)
    assert lay[0]["nb"] == 64 and lay[63]["lane"] == 63
    out = [case("bounds: cap == out_len", blk, ["bounds: cap == out_len"], cap=n, limit=1 << 22),
           case("bounds: cap == out_len - 1", blk, ["bounds: cap == out_len - 1"], cap=n - 1, limit=1 << 22, status=OUT_CAPACITY),
           case("bounds: limit == out_len", blk, ["bounds: limit == out_len"], limit=n),
           case("bounds: limit == out_len - 1", blk, ["bounds: limit == out_len - 1"], limit=n - 1),
           case("bounds: limit excludes the last literals", blk, ["bounds: limit below out_len by the last literals only"], limit=n - len(tail)),
           case("bounds: limit excludes the last match byte", blk, [], limit=n - len(tail) - 1, status=MEMORY_LIMIT_EXCEEDED)]
    for k, who in ((7, "lane k"), (63, "the batch's last lane")):
        r = lay[k]
        what = "lane k > 0" if k == 7 else "the batch's last lane"
        out.append(case(f"bounds: cap cuts the literals of {who}", blk, [f"bounds: a literal of {what} does not fit"], cap=r["mo"] - 1, limit=1 << 22, status=OUT_CAPACITY))
        out.append(case(f"bounds: cap cuts the match of {who}", blk, [f"bounds: a match byte of {'lane k' if k == 7 else what} does not fit"],
                        cap=r["mo"] + r["M"] - 1, limit=1 << 22, status=OUT_CAPACITY))
    return out


def _patched(blk, rec, off):
    b = bytearray(blk)
    b[rec["q"]:rec["q"] + 2] = int(off).to_bytes(2, "little")
    return bytes(b)


def offset_cases():
    """A first batch of 64 tokens (two literals and a match of four each); the offset of lane 0, 31 or 63 patched to each edge value."""
    out = []
    for plen in (0, 1, 300):
        prefix = _rnd(plen, 77 + plen)
        blk = enc([(2, 4)] * 200, have=plen, seed=5 + plen)
        lay = layout(blk)
        assert lay[0]["nb"] == 64 and lay[0]["cstart"] == 0
        for lane, who in zip((0, 31, 63), LANES):
            r = lay[lane]
            assert r["lane"] == lane and r["batch"] == 0 and r["rq"] + 4 <= STAGED
            mo = r["mo"]
            if plen == 0:
                out += [case(f"offsets: off == mo, {who}", _patched(blk, r, mo), [f"offsets: off == mo, no prefix, {who}"]),
                        case(f"offsets: off == mo + 1, {who}", _patched(blk, r, mo + 1), [f"offsets: off == mo + 1, no prefix, {who}"], status=INVALID_OFFSET),
                        case(f"offsets: off == 0, {who}", _patched(blk, r, 0), [f"offsets: off == 0, {who}"], status=ZERO_OFFSET),
                        case(f"offsets: off == 0xFFFF, {who}", _patched(blk, r, 0xFFFF), [f"offsets: off == 0xFFFF, {who}"], status=INVALID_OFFSET)]
            else:
                out += [case(f"offsets: off == mo + plen, prefix {plen}, {who}", _patched(blk, r, mo + plen), [f"offsets: off == mo + plen, prefix {plen}, {who}"], prefix=prefix),
                        case(f"offsets: off == mo + plen + 1, prefix {plen}, {who}", _patched(blk, r, mo + plen + 1),
                             [f"offsets: off == mo + plen + 1, prefix {plen}, {who}"], prefix=prefix, status=INVALID_OFFSET)]
    return out


def order_cases():
    blk = enc([(2, 4)] * 200, seed=9)
    lay = layout(blk)
    a, b = lay[10], lay[40]
    assert a["batch"] == b["batch"] == 0 and lay[0]["nb"] == 64
    two = _patched(_patched(blk, a, 0xFFFF), b, 0)                      # the invalid offset (a later test of the chain) stands first
    out = [case("order: invalid offset at lane 10, zero offset at lane 40", two, ["order: two damaged sequences in one batch, the first wins"], status=INVALID_OFFSET)]
    # zero offset at lane 10, and the limit cuts lane 40's match: the zero offset stands first
    out.append(case("order: zero offset at lane 10, the limit cuts lane 40", _patched(blk, a, 0), ["order: zero offset in front of an exceeded limit, one batch"],
                    limit=b["mo"] + b["M"] - 1, status=ZERO_OFFSET))
    out.append(case("order: zero offset and exceeded limit at lane 10", _patched(blk, a, 0), ["order: zero offset and exceeded limit in one sequence"],
                    limit=a["mo"] + a["M"] - 1, status=MEMORY_LIMIT_EXCEEDED))
    c = lay[64 + 5]
    assert c["batch"] == 1 and c["win"] == 0 and not c["first"] and c["lane"] == 5
    out.append(case("order: zero offset in the second batch of the window", _patched(blk, c, 0), ["order: damage in the second batch of a window"], status=ZERO_OFFSET))
    return out


def corpus(decode):
    """Every case with limit and cap filled in (a generous default where the case does not set them)."""
    cs = sweep_cases() + end_cases() + bounds_cases(decode) + offset_cases() + order_cases()
    for c in cs:
        if c["limit"] is None:
            c["limit"] = 1 << 22
        if c["cap"] is None:
            c["cap"] = 8192
    assert len({c["name"] for c in cs}) == len(cs)
    return cs


def reach(cs):
    got = set()
    for c in cs:
        got |= c["wants"]
    return got
