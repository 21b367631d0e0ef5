"""Handcrafted raw blocks for the overlapping matches of period 1, 2, 4 and 8 in the bitmap-fed decompress kernel (test infrastructure; used
by tests/test_fed_periodic_cases_cpu.py on the CPU and tests/test_gpu_fed_periodic.py on the GPU).

In the match rounds of the fed kernel's copy stage (lz4_decompress_batch_phase.inc under LZF_FED_DECODE) the wavefront moves a near
overlapping match byte by byte, lane i reading source byte i mod offset.  For an offset that is a power of two — 1, 2, 4 and 8 are 95 % of
these matches on the Silesia stand-in — that is a mask and the two divisions are branched around; every other offset keeps them.  Every block here puts one edge of that where it
matters.  `tokens` is the host model: fed_setup_cases.layout (windows, batches, lanes, output positions) with the class rule and the
H-rule rounds on top; `census` names the edges a case reaches, the oracle gives every case's bytes.

Most cases start behind `existing` output of a lap of the ring or more: the ring is then full of known bytes when the block starts, so the
bytes behind a short source (the match's own destination, one lap old) are known to differ from the pattern.

Not reachable, and so not here: a straddling source (s0 < near_lo < s0 + span) of an overlapping match inside a batch — it needs
off > kNearHist - kSpanMax = 1 366 and M > off, a sequence larger than a batch, which takes the solo path."""
import numpy as np

from seg_stage_cases import _seq, _walk
from fed_window_cases import ROUND
import fed_setup_cases as S

RING = 4096
SPAN_MAX = RING // 3          # kSpanMax
NEAR_HIST = RING - SPAN_MAX   # kNearHist
SHORT = 64                    # kShort
PERIODS = (1, 2, 4, 8)
OTHER_PERIODS = (3, 5, 6, 7, 9, 16, 63)
GRID_M = (4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 63, 64, 65, 66, 127, 128, 129, 511, 512, 513, 1024)
OTHER_M = (33, 64, 65, 200)
WIDE_POW2 = (32, 64, 128, 512)     # powers of two beyond 8: the mask form too; from 128 on the wave's stride of 64 is not a multiple of the offset
RBS = (0, 1, 15)

OWN, MASK, BYTE_LOOP, COOP_PLAIN = "own-lane", "byte loop, offset a power of two", "byte loop, other offsets", "cooperative, not overlapping"
PREFIX, FAR, STRADDLING, SOLO_SEQ, NONE = "prefix source", "far", "straddling source", "sequence larger than a batch", "no match"


# --------------------------------------------------------------------------------------------------------------------------- the model
def classify(M, off, mo, ob0, rb):
    """The class of a match of a batch that starts at output position ob0 (the rule of the round loop's set-up)."""
    if M == 0:
        return NONE
    if off > mo:
        return PREFIX
    s0, span = mo - off, min(M, off)
    near_lo = max(ob0 - NEAR_HIST, 0)
    if s0 + span <= near_lo:
        return FAR
    if s0 < near_lo:
        return STRADDLING
    mi, si = (mo + rb) % RING, (s0 + rb) % RING
    mwrap = mi + M > RING
    if M <= off:
        return OWN if M <= SHORT and not mwrap and si + M <= RING else COOP_PLAIN
    return MASK if off & (off - 1) == 0 else BYTE_LOOP


def tokens(c):
    """One record per token of the case: fed_setup_cases.layout's fields + off, ob0 (where its batch starts), s0, mi, si (ring indices of
    the match and its source), cls, and round / leader (the match round it moves in and that round's first unresolved lane; None for far / no match)."""
    blk, rb = c["input"], c["rb"]
    recs = S.layout(blk, len(c["existing"]))
    by_batch = {}
    for t in recs:
        by_batch.setdefault(t["batch"], []).append(t)
    for b in by_batch.values():
        ob0 = b[0]["lo"]
        for t in b:
            t["off"] = blk[t["q"]] | (blk[t["q"] + 1] << 8) if t["M"] else 0
            t["ob0"] = ob0
            t["cls"] = SOLO_SEQ if t["nb"] == 0 else classify(t["M"], t["off"], t["mo"], ob0, rb)
            t["s0"] = t["mo"] - t["off"]
            t["mi"], t["si"] = (t["mo"] + rb) % RING, (t["s0"] + rb) % RING
            t["round"] = t["leader"] = None
        if b[0]["nb"] == 0:
            continue
        # the H rule: the first unresolved match leads; when it is an own-lane match, every own-lane match whose source ends at or below
        # its start moves with it, otherwise it moves alone
        left = [t for t in b if t["cls"] not in (NONE, FAR)]
        r = 0
        while left:
            f = left[0]
            if f["cls"] == OWN:
                movers = [t for t in left if t["cls"] == OWN and t["s0"] + t["M"] <= f["mo"]]
            else:
                movers = [f]
            for t in movers:
                t["round"], t["leader"] = r, f["lane"]
            left = [t for t in left if t["round"] is None]
            r += 1
    return recs


def masked_moves(c):
    """The overlapping cooperative matches of the case that need no division (the kernel's counter 4)."""
    return sum(t["cls"] == MASK for t in tokens(c))


def plain_geometry(t, rb):
    """An overlapping match of period 1, 2, 4 or 8, longer than 8 bytes, whose destination does not wrap the ring and whose source's first
    8 bytes lie inside the ring array (the geometry the edges below are named after)."""
    return t["off"] in PERIODS and t["M"] > max(8, t["off"]) and t["cls"] == MASK and t["mi"] + t["M"] <= RING and t["si"] + 8 <= RING


def decode(c):
    """A plain decoder over the token walk: the case's output, existing bytes included (what the CPU test holds the oracle to)."""
    pre, out, blk = c["prefix"], bytearray(c["existing"]), c["input"]
    for pos, L, M, _ in _walk(blk):
        p = pos + 1 + (0 if L < 15 else 1 + (L - 15) // 255)
        out += blk[p:p + L]
        if M:
            off = blk[p + L] | (blk[p + L + 1] << 8)
            for _ in range(M):
                k = len(out) - off
                out.append(out[k] if k >= 0 else pre[len(pre) + k])
    return bytes(out)


def edges():
    e = [f"grid: off {off}, M {M}" for off in PERIODS for M in sorted(set(GRID_M) | {max(off + 1, 4)})]
    e += [f"grid: off {off}, the largest M a batch takes" for off in PERIODS] + [f"grid: off {off}, one byte more than a batch takes" for off in PERIODS]
    e += [f"other period: off {off}, M {M}" for off in OTHER_PERIODS for M in sorted(set(OTHER_M) | {off + 1})]
    e += [f"wide power of two: off {off}, M {M}" for off in WIDE_POW2 for M in (off + 1, off + 70, off + 300)]
    e += [f"neighbours: M == off beside M == off + 1, off {off}" for off in (4, 8)]
    e += [f"bytes: old ring content behind the source differs from the pattern, off {off}" for off in (1, 2, 4)]
    e += [f"destination: ring residue {r}" for r in range(8)]
    e += ["destination: ends exactly at the ring's end", "destination: wraps by 1 byte", "destination: wraps by M - 1 bytes",
          "destination: a long match wraps (byte loop)", "destination: a long match ends exactly at the ring's end"]
    e += [f"source: its last byte is the ring's last byte, off {off}" for off in PERIODS]
    e += [f"source: the 8-byte read crosses the ring's end by {k}" for k in range(1, 8)]
    e += ["source: a long match's 8-byte read crosses the ring's end", "source: s0 == near_lo", "source: in the prefix", "source: from the prefix into the output"]
    e += [f"rb {rb}: {what}" for rb in RBS for what in ("period divides 8, M <= 64", "period divides 8, M > 64", "period divides 8, wraps")]
    e += ["lanes: periodic in lane 0 of a full batch", "lanes: periodic in lane 63 of a full batch", "lanes: two adjacent periodic lanes, the second's source in the first's output",
          "lanes: a plain own-lane match whose source is a periodic match's output in its batch", "lanes: a plain own-lane match whose source ends where a periodic match starts",
          "lanes: a batch of 64 periodic matches",
          "windows: a periodic match is the last token listed in a window", "windows: a periodic match is the first token of a carried batch"]
    return e


def census(c):
    """The edges the case reaches, by the model."""
    got, toks, blk = set(), tokens(c), c["input"]
    out = decode(c)
    batches = {}
    for t in toks:
        batches.setdefault(t["batch"], []).append(t)
    for t in toks:
        M, off, cls = t["M"], t["off"], t["cls"]
        overl = M > off > 0
        if off in PERIODS and cls in (OWN, MASK, COOP_PLAIN) and c["kind"] == "grid":
            got.add(f"grid: off {off}, M {M}")
        if off in PERIODS and t["lane"] == 0 and t["L"] + M == SPAN_MAX and t["nb"] >= 1 and cls == MASK:
            got.add(f"grid: off {off}, the largest M a batch takes")
        if off in PERIODS and cls == SOLO_SEQ and t["L"] + M == SPAN_MAX + 1:
            got.add(f"grid: off {off}, one byte more than a batch takes")
        if off in WIDE_POW2 and cls == MASK and t["lane"] == 0:
            got.add(f"wide power of two: off {off}, M {M}")
        if off in OTHER_PERIODS and cls in (BYTE_LOOP, MASK, OWN, COOP_PLAIN):
            got.add(f"other period: off {off}, M {M}")
        if plain_geometry(t, c["rb"]) and off < 8 and t["mo"] >= RING:
            old = out[t["mo"] - RING:t["mo"] - RING + 8 - off]
            if len(old) == 8 - off and all(a != b for a, b in zip(old, out[t["mo"]:t["mo"] + 8 - off])) and len(set(out[t["s0"]:t["mo"]])) == off:
                got.add(f"bytes: old ring content behind the source differs from the pattern, off {off}")
        if plain_geometry(t, c["rb"]):
            got.add(f"destination: ring residue {t['mi'] % 8}")
            if t["mi"] + M == RING:
                got.add("destination: ends exactly at the ring's end" if M <= SHORT else "destination: a long match ends exactly at the ring's end")
            if t["si"] + off == RING or (off == 8 and t["si"] + 8 == RING):
                got.add(f"source: its last byte is the ring's last byte, off {off}")
            if t["s0"] == max(t["ob0"] - NEAR_HIST, 0):
                got.add("source: s0 == near_lo")
        if cls == MASK and off in PERIODS and overl and M > 8 and not plain_geometry(t, c["rb"]):
            mwrap = t["mi"] + M > RING
            if M <= SHORT and t["mi"] + M == RING + 1:
                got.add("destination: wraps by 1 byte")
            if M <= SHORT and t["mi"] == RING - 1:
                got.add("destination: wraps by M - 1 bytes")
            if M > SHORT and mwrap:
                got.add("destination: a long match wraps (byte loop)")
            if not mwrap and t["si"] + 8 > RING:
                if M <= SHORT:
                    got.add(f"source: the 8-byte read crosses the ring's end by {t['si'] + 8 - RING}")
                    if t["si"] + off == RING:
                        got.add(f"source: its last byte is the ring's last byte, off {off}")
                else:
                    got.add("source: a long match's 8-byte read crosses the ring's end")
        if cls == PREFIX and off in PERIODS and overl:
            got.add("source: in the prefix")
            if M > off - t["mo"]:
                got.add("source: from the prefix into the output")
        if cls == MASK and off in PERIODS:
            got.add(f"rb {c['rb']}: period divides 8, " + ("wraps" if t["mi"] + M > RING else "M <= 64" if M <= SHORT else "M > 64"))
    for b in batches.values():
        if b[0]["nb"] == 64:
            if b[0]["cls"] == MASK:
                got.add("lanes: periodic in lane 0 of a full batch")
            if b[63]["cls"] == MASK:
                got.add("lanes: periodic in lane 63 of a full batch")
            if all(t["cls"] == MASK for t in b):
                got.add("lanes: a batch of 64 periodic matches")
        for a, t in zip(b, b[1:]):
            if a["off"] == t["off"] == a["M"] == t["M"] - 1 and a["cls"] == OWN and t["cls"] == MASK:
                got.add(f"neighbours: M == off beside M == off + 1, off {t['off']}")
            if a["cls"] == t["cls"] == MASK and a["mo"] <= t["s0"] < a["mo"] + a["M"]:
                got.add("lanes: two adjacent periodic lanes, the second's source in the first's output")
        for t in b:
            if t["cls"] == OWN and any(a["cls"] == MASK and a["lane"] < t["lane"] and a["mo"] <= t["s0"] and t["s0"] + t["M"] <= a["mo"] + a["M"] for a in b):
                got.add("lanes: a plain own-lane match whose source is a periodic match's output in its batch")
            if t["cls"] == OWN and any(a["cls"] == MASK and a["lane"] < t["lane"] and t["s0"] + t["M"] == a["mo"] for a in b):
                got.add("lanes: a plain own-lane match whose source ends where a periodic match starts")
    # windows: the tokens a window lists are those that start in its 1 024 bytes
    starts = []
    for t in toks:
        if not starts or starts[-1][0] != t["win"]:
            starts.append((t["win"], t["cstart"]))
    for k, (w, cstart) in enumerate(starts):
        listed = [t for t in toks if cstart <= t["pos"] < cstart + ROUND]
        if k + 1 < len(starts) and listed and listed[-1]["cls"] == MASK:
            got.add("windows: a periodic match is the last token listed in a window")
        if k > 0:
            first = [t for t in toks if t["win"] == w][0]
            if first["pos"] < starts[k - 1][1] + ROUND and first["cls"] == MASK:
                got.add("windows: a periodic match is the first token of a carried batch")
    return got


# ------------------------------------------------------------------------------------------------------------------------- building
def distinct(n, seed):
    """n bytes, any 256 in a row all different."""
    rng = np.random.default_rng(seed)
    return b"".join(bytes(rng.permutation(256).astype(np.uint8)) for _ in range(n // 256 + 1))[:n]


class Block:
    """A block built token by token; `o` is the output position (existing output in front)."""

    def __init__(self, seed, existing=0, prefix=0):
        self.seed, self.blk, self.n = seed, bytearray(), 0
        self.existing, self.prefix = distinct(existing, seed + 1000), distinct(prefix, seed + 2000)
        self.o = existing

    def seq(self, L, M, off):
        self.n += 1
        self.blk += _seq(distinct(L, self.seed * 131 + self.n), off, M)
        self.o += L
        mo = self.o
        self.o += M
        return mo

    def end(self, tail=b"tail!"):
        self.blk += _seq(tail, None, 0)
        return bytes(self.blk)


def case(name, kind, b, rb=0, wants=()):
    blk = b.end()
    return dict(name=name, kind=kind, input=blk, prefix=b.prefix, existing=b.existing, limit=1 << 22, cap=8192, rb=rb, wants=set(wants), status=S.OK)


def one(name, kind, off, M, mi, rb=0, L=None, wants=(), seed=0):
    """One match (off, M) whose destination starts at ring index mi, behind existing output (a lap or more where mi leaves room), three
    short sequences that read its output, and the last literals."""
    L = off + 3 if L is None else L
    mo = (mi - rb) % RING
    if mo - L < 2800:
        mo += RING
    b = Block(seed or (off * 1000 + M), existing=mo - L)
    assert b.seq(L, M, off) == mo
    for k in range(3):
        b.seq(3, 5 + k, min(M, 40) + k)
    return case(name, kind, b, rb=rb, wants=wants)


def grid_cases():
    out = []
    for off in PERIODS:
        for M in sorted(set(GRID_M) | {max(off + 1, 4)}):
            out.append(one(f"grid: off {off}, M {M}", "grid", off, M, (off * 131 + M * 7) % 600 + 64, wants=[f"grid: off {off}, M {M}"]))
        L = off + 3
        out.append(one(f"grid: off {off}, the largest M", "large", off, SPAN_MAX - L, 100 + off, wants=[f"grid: off {off}, the largest M a batch takes"]))
        out.append(one(f"grid: off {off}, M over a batch", "large", off, SPAN_MAX - L + 1, 100 + off, wants=[f"grid: off {off}, one byte more than a batch takes"]))
    for off in OTHER_PERIODS:
        for M in sorted(set(OTHER_M) | {off + 1}):
            out.append(one(f"other period: off {off}, M {M}", "other", off, M, (off * 57 + M * 3) % 2000 + 64, wants=[f"other period: off {off}, M {M}"]))
    for off in WIDE_POW2:
        for M in (off + 1, off + 70, off + 300):
            out.append(one(f"wide power of two: off {off}, M {M}", "wide", off, M, (off * 3 + M) % 600 + 64, L=off + 3, wants=[f"wide power of two: off {off}, M {M}"]))
    for off in (4, 8):
        b = Block(70 + off, existing=4300)
        b.seq(off + 2, off, off); b.seq(off + 2, off + 1, off); b.seq(off + 2, off, off); b.seq(3, 6, 30)
        out.append(case(f"neighbours: off {off}", "neighbours", b, wants=[f"neighbours: M == off beside M == off + 1, off {off}"]))
    return out


def position_cases():
    out = []
    for r in range(8):
        out.append(one(f"destination: residue {r}", "dest", 2, 37, 512 + r, wants=[f"destination: ring residue {r}"]))
    for off, M in ((1, 33), (2, 64), (4, 9), (8, 17)):
        out.append(one(f"destination: off {off}, M {M} ends at the ring's end", "dest", off, M, RING - M, wants=["destination: ends exactly at the ring's end"]))
        out.append(one(f"destination: off {off}, M {M} wraps by 1", "dest", off, M, RING - M + 1, wants=["destination: wraps by 1 byte"]))
        out.append(one(f"destination: off {off}, M {M} wraps by M - 1", "dest", off, M, RING - 1, wants=["destination: wraps by M - 1 bytes"]))
    out.append(one("destination: long match wraps", "dest", 2, 300, RING - 100, wants=["destination: a long match wraps (byte loop)"]))
    out.append(one("destination: long match ends at the ring's end", "dest", 4, 300, RING - 300, wants=["destination: a long match ends exactly at the ring's end"]))
    for off in PERIODS:      # destination at ring index 0: the source's last byte is the ring's last
        out.append(one(f"source: ends at the ring's end, off {off}", "src", off, 21, 0, wants=[f"source: its last byte is the ring's last byte, off {off}"]))
    for k in range(1, 8):    # si + 8 == RING + k
        off = 8 if k < 4 else 4 if k < 6 else 2 if k == 6 else 1      # (the destination behind it starts at ring index k - 8 + off >= 0)
        out.append(one(f"source: read crosses the ring's end by {k}", "src", off, 40, k - 8 + off, wants=[f"source: the 8-byte read crosses the ring's end by {k}"]))
    out.append(one("source: long match, read crosses the ring's end", "src", 4, 200, 1, wants=["source: a long match's 8-byte read crosses the ring's end"]))
    for off in PERIODS:      # the block's first bytes, nothing in front: s0 == near_lo == 0
        b = Block(300 + off)
        b.seq(off, 30 + off, off); b.seq(2, 6, 9)
        out.append(case(f"source: s0 == near_lo, off {off}", "src", b, wants=["source: s0 == near_lo"]))
    b = Block(310, prefix=300)
    b.seq(1, 3 + 1, 2); b.seq(2, 6, 5)                      # off 2 > mo 1: one byte of the prefix, then the output
    out.append(case("source: prefix, into the output", "src", b, wants=["source: in the prefix", "source: from the prefix into the output"]))
    b = Block(311, prefix=300)
    b.seq(0, 40, 8); b.seq(2, 6, 5)
    out.append(case("source: prefix, off 8 at output position 0", "src", b, wants=["source: in the prefix"]))
    for rb in RBS[1:]:
        for off, M in ((1, 64), (2, 33), (4, 9), (8, 40)):
            out.append(one(f"rb {rb}: off {off}, M {M}", "rb", off, M, 700 + off + rb, rb=rb, wants=[f"rb {rb}: period divides 8, M <= 64"]))
        out.append(one(f"rb {rb}: short", "rb", 2, 5, 700, rb=rb))
        out.append(one(f"rb {rb}: long", "rb", 2, 513, 900, rb=rb, wants=[f"rb {rb}: period divides 8, M > 64"]))
        out.append(one(f"rb {rb}: wraps", "rb", 2, 40, RING - 7, rb=rb, wants=[f"rb {rb}: period divides 8, wraps"]))
        out.append(one(f"rb {rb}: ends at the ring's end", "rb", 1, 64, RING - 64, rb=rb, wants=["destination: ends exactly at the ring's end"]))
        out.append(one(f"rb {rb}: source read ends at the ring's end", "rb", 8, 33, 0, rb=rb, wants=["source: its last byte is the ring's last byte, off 8"]))
    return out


def lane_cases():
    out = []
    # 64 periodic matches in one batch (every period, lengths of every class up to 32), a second batch behind it
    b = Block(400, existing=4200)
    for j in range(64):
        b.seq(8 if j % 3 else 0, (9, 12, 9, 16, 17, 12, 10, 10)[j % 8] if j % 3 else 9, PERIODS[j % 4] if j % 3 else 2)
    for j in range(10):
        b.seq(2, 33, 2)
    out.append(case("lanes: 64 periodic matches", "lanes", b, wants=["lanes: a batch of 64 periodic matches", "lanes: periodic in lane 0 of a full batch",
                                                                      "lanes: periodic in lane 63 of a full batch",
                                                                      "lanes: two adjacent periodic lanes, the second's source in the first's output"]))
    # twenty periodic matches of 33 .. 52 bytes, each behind literals of its own: twenty cooperative rounds
    b = Block(401, existing=4250)
    for j in range(20):
        b.seq(8, 33 + j, PERIODS[j % 4])
    out.append(case("lanes: twenty periodic rounds", "lanes", b))
    # a mixed batch: plain own-lane matches that read a periodic match's output, one of them ending exactly where a later periodic match starts
    b = Block(402, existing=4300, prefix=0)
    b.seq(5, 6, 30)
    a = b.seq(8, 24, 2)                       # periodic A
    m = b.seq(0, 8, 12)                       # plain, source inside A's output
    assert a <= m - 12 and m - 12 + 8 <= a + 24
    p = b.seq(6, 40, 4)                       # periodic P, leads a later round
    q = b.o + 3
    b.seq(3, 7, q - (p - 7))                  # plain: its source [p - 7, p) ends exactly where P starts
    b.seq(4, 9, 1); b.seq(0, 5, 3)
    out.append(case("lanes: mixed batch", "lanes", b, wants=["lanes: a plain own-lane match whose source is a periodic match's output in its batch",
                                                             "lanes: a plain own-lane match whose source ends where a periodic match starts"]))
    # windows: tokens of 15 bytes, 69 of them start in the first window: 64 go, 5 wait for the second window
    for rb in (0, 15):
        b = Block(403 + rb, existing=4120)
        for j in range(110):
            b.seq(12, 9, PERIODS[j % 4])
        out.append(case(f"windows: periodic matches across windows, rb {rb}", "windows", b, rb=rb,
                        wants=["windows: a periodic match is the last token listed in a window", "windows: a periodic match is the first token of a carried batch"]))
    return out


def corpus():
    cs = grid_cases() + position_cases() + lane_cases()
    assert len({c["name"] for c in cs}) == len(cs)
    return cs
