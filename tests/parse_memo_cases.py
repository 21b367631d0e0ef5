"""Built LZ4 blocks for the saved walks of lzf_seg_parse_kernel's fixed point (lz4_seg_front.hip, kParseMemo), and a host model of the
pass loop that keeps them: a lane whose entry changed looks the new entry up in its saved walks (newest first); a hit brings (walked
entry, exit, merge position, row B) back and the lane sits the walk out; a miss moves the live result into the first slot — the oldest
goes — clears row B and walks.  Nothing of pass 0 is saved; the slots are empty at the start of every chunk.  The walks themselves are
parse_hop_cases.Chunk's, hop for hop.  The model reports every lookup (lane, pass, entry, hit or miss, what came back, what was
displaced) and, with the slots a chunk before left behind, every lookup a slot that was NOT cleared would have answered wrongly.

The blocks: a period-4 background 0x10 0x10 0x10 0x00 — the sequence `token 0x10, one literal, offset` whose literal and offset bytes
read as tokens too, so three chains run side by side through every region and never meet — in which single bytes are replaced: a token
of another length on the true chain moves it to another phase, one on a side chain joins or parts two chains, 0xF0 starts a literal run
that jumps a region, 0x1F .. 0xFF a match length that takes the general routine.  The replacements are drawn from a seeded generator
and kept where the block still decodes; census() names the edges a block reaches, EDGES lists them, CASES says which block was chosen
for which.  Every block is at most three chunks."""
import numpy as np

import parse_hop_cases as P

CHUNK, STRIDE, REGION = P.CHUNK, P.STRIDE, P.REGION
LIMIT = 1 << 22
BG = (0x10, 0x10, 0x10, 0x00)
# 1 literal, then a match of 4 + 15 + 257 * 255 + 40 bytes at offset 1: 65 595 bytes are out, every offset two bytes can spell is valid behind it
# (262 bytes: region 0 and the first six of region 1 — lane 0 takes the general routine over them)
PREAMBLE = bytes([0x1F, 0x41, 0x01, 0x00]) + b"\xff" * 257 + bytes([40])


# ------------------------------------------------------------------------------------------------------------------ the model
class MemoChunk(P.Chunk):
    """Chunk h of buf with `depth` saved walks per lane (0: the pass loop without them).  .bits, .exit as P.Chunk; .events: one dict per
    lookup; .lookups, .hits; .slots: what the lanes' slots hold at the end; .est: the marks the chunk owns (the launch order's count).
    ghost: the .slots of the chunk before, for the stale-slot census only — the model itself always starts a chunk with empty slots."""

    def __init__(self, buf, h, depth=1, ghost=None, defect=None):
        self.buf, self.h, self.depth = buf, h, depth
        n = len(buf)
        self.cstart = cs = h * STRIDE
        self.cb = bytes(buf[cs:cs + CHUNK]) + bytes(max(0, CHUNK - (n - cs)) + 4)
        room = n - cs
        self.fe = (min(room - 24, CHUNK - 2) if room > 24 else 0)
        self.hops, self.passes, self.events, self.stale = [], 0, [], []
        A = [set() for _ in range(64)]
        B = [set() for _ in range(64)]
        in_input = [cs + REGION * i < n for i in range(64)]
        x0 = [self._walk(i, REGION * i, in_input[i], False, 0, 0, A, B)[0] for i in range(64)]
        self.x0 = x0
        # the live result of a lane: what the kernel holds in walked, X, mpos and row B (+ what the census wants to know of the walk)
        live = [dict(entry=REGION * i, X=x0[i] if in_input[i] else 0, mpos=REGION * i, B=set(), inreg=True, pss=0, general=False) for i in range(64)]
        slots = [[] for _ in range(64)]                 # newest first, at most `depth`
        if defect == "no reset" and ghost is not None:
            slots = [[dict(s) for s in g] for g in ghost]
        fresh = [True] * 64
        for pss in range(1, 81):
            entry, m = [0] * 64, 0
            for i in range(64):
                entry[i] = m; m = max(m, live[i]["X"])
            redo = [in_input[i] and entry[i] != live[i]["entry"] and i != 0 for i in range(64)]
            if not any(redo):
                break
            self.passes = pss
            for i in range(64):
                if not redo[i]:
                    continue
                end_r, e = REGION * (i + 1), entry[i]
                k = next((k for k, s in enumerate(slots[i]) if s["entry"] == e), None)
                old = live[i]
                ev = dict(lane=i, pss=pss, entry=e, hit=k is not None, slot=k, fresh=fresh[i], displaced=old, restored=None)
                self.events.append(ev)
                if k is not None:
                    live[i] = ev["restored"] = slots[i].pop(k)
                    if defect == "row without mpos":
                        live[i] = dict(live[i], mpos=old["mpos"])
                    if defect == "X without walked":
                        live[i] = dict(live[i], entry=old["entry"])
                else:
                    inreg = e < end_r and cs + e < n
                    if defect != "row B not cleared":
                        B[i] = set()
                    else:
                        B[i] = set(old["B"])
                    n_hops = len(self.hops)
                    x1, mg = self._walk(i, e if inreg else end_r, inreg, False, 1, pss, A, B)
                    general = any(r["how"] in ("parked", "step back") for r in self.hops[n_hops:])      # a 0xFF length byte
                    if not inreg:
                        X, mp = e, end_r
                    elif mg:
                        X, mp = x0[i], x1
                    else:
                        X, mp = x1, end_r
                    live[i] = dict(entry=e, X=X, mpos=mp, B=B[i], inreg=inreg, pss=pss, general=general)
                    if ghost is not None:
                        g = next((s for s in ghost[i] if s["entry"] == e), None)
                        if g is not None and (g["X"], g["mpos"], g["B"]) != (X, mp, B[i]):
                            self.stale.append(dict(lane=i, pss=pss, entry=e))
                if depth and not fresh[i]:
                    slots[i].insert(0, dict(old, left=pss))
                    del slots[i][depth:]
                fresh[i] = False
                B[i] = live[i]["B"]
        self.slots = slots
        self.lookups, self.hits = len(self.events), sum(e["hit"] for e in self.events)
        self.bits = np.zeros(CHUNK, bool)
        for i in range(64):
            if in_input[i]:
                for p in A[i]:
                    if p >= live[i]["mpos"]:
                        self.bits[p] = True
                for p in live[i]["B"]:
                    self.bits[p] = True
        self.exit = min(cs + max(l["X"] for l in live), n)
        self.est = int(self.bits.sum()) if h == 0 else int(self.bits[CHUNK - STRIDE:].sum())


def chunks(blk, depth=1, defect=None):
    """The chunks of blk in order, each with the slots of the one before as its ghost."""
    out, ghost = [], None
    for h in range(P.nch(len(blk))):
        c = MemoChunk(blk, h, depth, ghost, defect)
        out.append(c); ghost = c.slots
    return out


def expected(blk, depth=1, defect=None):
    """(rows (nch, CHUNK // 32) uint32, exits (nch,), marks the chunks own summed, lookups, hits) as the model has them."""
    cs = chunks(blk, depth, defect)
    rows = np.stack([np.packbits(c.bits, bitorder="little").view(np.uint32) for c in cs])
    return rows, np.array([c.exit for c in cs], np.uint32), sum(c.est for c in cs), sum(c.lookups for c in cs), sum(c.hits for c in cs)


# ------------------------------------------------------------------------------------------------------------------ the edges
# Lane 0 never walks again and lane 1's entry is lane 0's exit, which is final after pass 0: lane 1 looks up once and cannot hit.  Lane 2's
# entry changes in passes 1 and 2 at most (lane 1's exit changes once), and its first result is pass 0's, which is not saved: no hit
# either.  Lane 3 is the lowest lane whose entry can come back (lane 2's exit changes in pass 1 and returns in pass 2).
LOWEST_HIT_LANE = 3
EDGES = ["an entry returns after one pass", "an entry returns after two others: a hit at depth 2, a miss at depth 1",
         "a hit restores a walk that had merged", "a hit restores a walk that had left the region, and a lane above changes again",
         "a hit followed by a miss in the same lane", "a result with an entry beyond its region is displaced and restored",
         "a restored row with marks in word 0 and in word 7", f"a hit in lane {LOWEST_HIT_LANE}", "a hit in lane 63",
         "the restored walk went through the general routine", "a stale slot of the chunk before would have answered a lane's last lookup"]


def census(blk):
    got = set()
    d1, d2 = chunks(blk, 1), chunks(blk, 2)
    for c1, c2 in zip(d1, d2):
        miss1 = {(e["lane"], e["pss"]) for e in c1.events if not e["hit"]}
        for e in c2.events:
            # the second slot holds what the lane's lookup before the last displaced: its entries ran e1, e2, e3, e1
            if e["hit"] and e["slot"] == 1 and (e["lane"], e["pss"]) in miss1:
                got.add(EDGES[1])
        last = {e["lane"]: e["pss"] for e in c1.events}      # (a stale answer to an entry the lane leaves again would be walked over)
        if any(last[t["lane"]] == t["pss"] for t in c1.stale):
            got.add(EDGES[10])
        hit_at = {}
        for e in c1.events:
            i, rb0 = e["lane"], REGION * e["lane"]
            if not e["hit"]:
                if i in hit_at:
                    got.add(EDGES[4])
                continue
            r = e["restored"]
            hit_at.setdefault(i, e["pss"])
            if r["left"] == e["pss"] - 1:
                got.add(EDGES[0])
            if r["inreg"] and r["mpos"] < rb0 + REGION and r["X"] == c1.x0[i]:
                got.add(EDGES[2])
            if r["inreg"] and r["mpos"] == rb0 + REGION and r["X"] != c1.x0[i] and any(f["lane"] > i and f["pss"] == e["pss"] + 1 for f in c1.events):
                got.add(EDGES[3])
            if not r["inreg"]:
                got.add(EDGES[5])
            if any(p < rb0 + 32 for p in r["B"]) and any(p >= rb0 + 224 for p in r["B"]):
                got.add(EDGES[6])
            if i == LOWEST_HIT_LANE:
                got.add(EDGES[7])
            if i == 63:
                got.add(EDGES[8])
            if r["general"]:
                got.add(EDGES[9])
    return got


# ------------------------------------------------------------------------------------------------------------------ the blocks
PLANTS = (0x00, 0x20, 0x30, 0x40, 0x50, 0x60, 0x90)


def _draw(rng, lo, hi, count, wide=20):
    """`count` replacements in the regions lo .. hi - 1: (position, bytes); two in `wide` are a long literal run or a long match."""
    out = []
    for _ in range(count):
        p = int(rng.integers(lo * REGION, hi * REGION))
        r = int(rng.integers(0, wide))
        if r == 0:
            out.append((p, bytes([0xF0, int(rng.integers(0, 255))])))                 # 15 + b literals: a plain hop that jumps a region
        elif r == 1:
            out.append((p, bytes([0x1F])))
            out.append((p + 4, bytes([0xFF, int(rng.integers(0, 200))])))             # a match length that goes on: the general routine
        else:
            out.append((p, bytes([PLANTS[int(rng.integers(0, len(PLANTS)))]])))
    return out


def block(seed, lo, hi, count, second=None, wide=20):
    """The background over regions 0 .. hi + 1 with `count` seeded replacements in regions lo .. hi - 1; second = (count2, seed2): the same
    replacements again one chunk stride further on, count2 of them drawn anew — chunk 1 then sees chunk 0's entries over other bytes.
    Cut at the first true token behind the last region and ended with 40 literals.  None if the replacements leave no valid block."""
    rng = np.random.default_rng(seed)
    base = STRIDE if second else 0
    end = base + (hi + 2) * REGION
    b = bytearray(BG[p & 3] for p in range(end + 600))
    b[:len(PREAMBLE)] = PREAMBLE
    plants = _draw(rng, lo, hi, count, wide)
    if second:
        again = plants[:len(plants) - second[0]] + _draw(np.random.default_rng(second[1]), lo, hi, second[0], wide)
        plants = plants + [(p + STRIDE, v) for p, v in again]
    for p, v in plants:
        if p >= len(PREAMBLE):
            b[p:p + len(v)] = v
    p = 0
    while p < end:                                          # the true chain, to where the block is cut
        nx = P._token_next(b, p)
        if nx is None or nx <= p:
            return None
        p = nx
    if p > end + 300:
        return None
    return bytes(b[:p]) + bytes([0xF0, 25]) + bytes((7 * i + 3) & 0x7F for i in range(40))


# (name, arguments of block(), the edges the block was chosen for — tests/test_parse_memo_cases_cpu.py holds each to its list)
CASES = [
    ("regions 2-9, seed 2", (2, 2, 10, 40), (0, 2, 3, 6)),
    ("regions 2-9, seed 51: a long match in a restored walk", (51, 2, 10, 40), (0, 9)),
    ("regions 2-7, long runs, seed 179: an entry beyond the region comes back", (179, 2, 8, 30, None, 4), (5,)),
    ("regions 2-7, long runs, seed 215: a hit, then a miss", (215, 2, 8, 30, None, 4), (0, 4)),
    ("regions 2-7, long runs, seed 186: the walk before the last comes back", (186, 2, 8, 30, None, 4), (1,)),
    ("regions 56-62, seed 1: lane 63", (1, 56, 63, 40), (0, 3, 8)),
    (f"regions 56-62, seed 58: lane {LOWEST_HIT_LANE}", (58, 56, 63, 40), (7,)),
    ("two chunks, the same entries over other bytes", (6, 2, 9, 40, (6, 1006)), (10,)),
]


def all_cases():
    """[(name, block)]"""
    out = []
    for name, args, _ in CASES:
        blk = block(*args)
        assert blk is not None, name
        out.append((name, blk))
    return out
