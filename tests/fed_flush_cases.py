"""Handcrafted raw blocks for the DEFERRED FLUSH of the bitmap-fed decompress kernel (test infrastructure; used by
tests/test_fed_flush_cases_cpu.py on the CPU and tests/test_gpu_fed_flush.py on the GPU).

A batch of the fed kernel's copy stage (lz4_decompress_batch_phase.inc under LZF_FED_DECODE) leaves its output in the ring; the NEXT batch
writes it to `out` behind its own far phase, whole 16-byte lines only (OutRing::flush_lines), and whatever ends the window loop — a parked
piece, the job's end, a status, a bail — or a solo sequence drains what is pending, bytes and all.  Every block here puts one edge of
that where it matters.  `model` is the host model: the windows and batches of fed_setup_cases.layout, cut into pieces where the kernel
parks, with the pending range carried as the kernel carries it; `census` names the edges a case reaches at 1 and 3 pieces; the oracle
gives every case's status and bytes.

Not reachable, and so not here: a far source inside one of the TWO batches before its own (two batches span at most 2 x kSpanMax = 2 730
bytes, a far source ends kNearHist = 2 731 or more below its batch), and for the same reason a far match that reads the last batch of
the piece before; the newest batch a far source reaches is the third before its own, and the first batch of a piece reads the piece
before through near matches (the ring re-filled from `out`).  (test_fed_flush_cases_cpu.py holds that inequality to the kernel's RING.)

One case is larger than the rest: a walk-mode retry needs a bit map that is wrong about a window, which takes a block of more than a parse
chunk (walk_case: 20 KiB in, built after fed_piece_cases' "chunk 1 not in step" block — whose walked window stands directly behind a solo
sequence, with nothing pending).  Its window behind 16 384 is listed from the map, bails in its first batch's set-up and is walked, directly
behind a batch.  The emulator of the window loop proves the retry, the model the pending range it carries."""
import fed_periodic_cases as K
import fed_piece_cases as P
from fed_periodic_cases import FAR, PREFIX, STRADDLING, NEAR_HIST, SPAN_MAX, Block
from fed_setup_cases import OK, ZERO_OFFSET, INVALID_OFFSET, OUT_CAPACITY, TOT_CLAMP
import fed_window_cases as fw
from fed_window_cases import CARRY, ROUND
from seg_stage_cases import _walk

CAP = 16384
PIECES = (1, 3)
RBS = (0, 1, 15)

E_FAR_AT = "far: its source ends exactly at ob0 - kNearHist"
E_FAR_BELOW = "far: its source ends one byte below ob0 - kNearHist"
E_FAR_NEWEST = "far: its source inside the third batch before its own (the newest a far source reaches)"
E_HAND_NEAR = "hand-over: the first batch of a piece reads the last batch of the piece before"
E_PARK = "hand-over: a piece parks with a range pending"
E_SOLO_AFTER = "solo: directly after a batch, a range pending"
E_SOLO_BEFORE = "solo: directly before a batch"
E_STRADDLE = "slow: a straddling source in a batch with a range pending"
E_PREFIX = "slow: a prefix source in a batch with a range pending"
E_ONLY = "end: the job's only batch is its last"
E_CARRY = "window: its last batch is carried, a range pending"
E_WALK = "walk: a window bails in its first batch's set-up and is walked, a range pending across the retry"
E_ERR = {ZERO_OFFSET: "error after a good batch: zero offset", INVALID_OFFSET: "error after a good batch: offset beyond the prefix",
         OUT_CAPACITY: "error after a good batch: capacity"}
E_STAY = "lines: a range that does not reach its first 16-byte address stays pending"
E_HEAD = "lines: the first flush behind a misaligned start has head bytes"
E_RES = tuple(f"lines: a batch ends at output address residue {r}" for r in range(16))


def edges():
    return [E_FAR_AT, E_FAR_BELOW, E_FAR_NEWEST, E_HAND_NEAR, E_PARK, E_SOLO_AFTER, E_SOLO_BEFORE, E_STRADDLE, E_PREFIX, E_ONLY, E_CARRY, E_WALK,
            E_STAY, E_HEAD] + list(E_ERR.values()) + list(E_RES)


# --------------------------------------------------------------------------------------------------------------------------- the model
def flush_lines(a, b, rb):
    """OutRing::flush_lines: where the pending range starts after out[a, b) was flushed by whole 16-byte lines."""
    nh = -(a + rb) & 15
    if nh:
        if b - a < nh:
            return a
        a += nh
    return a + ((b - a) >> 4 << 4)


def model(c, pieces=1):
    """The job as the fed kernel runs it in `pieces` pieces -> (events, status, good_end).  events: dicts in order, kind "batch" (piece, win,
    first — the window's first batch —, nb — 0: a solo sequence —, ob0, end, toks, pend_in, pend_out, after — the kind of the event before it in
    its piece, None for a piece's first), "carry" and "park" (pending: a range is pending there).  status: OK or the first error by the
    copy stage's rules; good_end: the output position where the failing batch starts (what `out` then holds), the job's out_len if none."""
    blk, rb, n, plen = c["input"], c["rb"], len(c["input"]), len(c["prefix"])
    toks = _walk(blk)
    ev, i, o, win, piece, after = [], 0, len(c["existing"]), 0, 0, None
    pend = o
    while i < len(toks):
        expect = toks[i][0]
        while pieces > 1 and expect >= P.piece_end(n, pieces, piece):
            ev.append(dict(kind="park", piece=piece, pending=pend < o, expect=expect, o=o))
            piece += 1; pend = o; after = None
        cstart = expect & ~31
        lst = [t for t in toks[i:] if t[0] - cstart < ROUND]
        tc, tidx = len(lst), 0
        while tidx < tc:
            if tidx > 0 and tc - tidx <= CARRY and cstart + ROUND < n:
                ev.append(dict(kind="carry", piece=piece, pending=pend < o)); after = "carry"
                break
            nb_try = min(64, tc - tidx)
            incl, s = [], 0
            for _, L, M, _ in lst[tidx:tidx + nb_try]:
                s += min(L + M, TOT_CLAMP); incl.append(s)
            over = [j for j, v in enumerate(incl) if v > SPAN_MAX]
            nb = min(over[0] if over else 64, nb_try)
            recs = []
            for j in range(max(nb, 1)):
                p, L, M, _ = lst[tidx + j]
                q = p + 1 + (0 if L < 15 else 1 + (L - 15) // 255) + L
                lo = o + (incl[j] - (L + M) if nb else 0)
                off = blk[q] | (blk[q + 1] << 8) if M else 0
                recs.append(dict(pos=p, L=L, M=M, q=q, off=off, lo=lo, mo=lo + L, lane=j,
                                 cls="solo" if nb == 0 else K.classify(M, off, lo + L, o, rb)))
            for t in recs:      # the copy stage's checks, in its order
                if t["lo"] + t["L"] > c["cap"]:
                    return ev, OUT_CAPACITY, o
                if t["M"] and t["off"] == 0:
                    return ev, ZERO_OFFSET, o
                if t["M"] and t["off"] > t["mo"] + plen:
                    return ev, INVALID_OFFSET, o
                if t["M"] and t["mo"] + t["M"] > c["cap"]:
                    return ev, OUT_CAPACITY, o
            end = o + incl[max(nb, 1) - 1]
            pend_out = end if nb == 0 else flush_lines(pend, o, rb)
            ev.append(dict(kind="batch", piece=piece, win=win, first=tidx == 0, nb=nb, ob0=o, end=end, toks=recs, pend_in=pend, pend_out=pend_out, after=after))
            pend, o, after = pend_out, end, "solo" if nb == 0 else "batch"
            tidx += max(nb, 1)
        i += tidx; win += 1
    return ev, OK, o


def census(c):
    """The edges the case reaches, by the model, at 1 and 3 pieces."""
    got = set()
    for pieces in PIECES:
        ev, status, good_end = model(c, pieces)
        bs = [e for e in ev if e["kind"] == "batch"]
        if status == OK:
            # the emulator of the window loop, piece by piece: a window listed from the map (kind 0) and then walked at the same start (kind 1)
            # bailed before it ran a batch; windows of the piece in front of it ran batches; the model's batch that starts the window holds the range
            m = P.emulate_pieces(c["input"], pieces, prefix_len=len(c["prefix"]), existing_len=len(c["existing"]), limit=c["limit"], cap=c["cap"])
            for piece, log in m.log.items():
                for i in range(2, len(log)):
                    if log[i][0] == 1 and log[i - 1] == (0, log[i][1]) and any(k == 0 for k, _ in log[:i - 1]):
                        if any(e["piece"] == piece and e["first"] and e["toks"][0]["pos"] & ~31 == log[i][1] and e["after"] in ("batch", "carry")
                               and e["pend_in"] < e["ob0"] for e in bs):
                            got.add(E_WALK)
        if status != OK and bs and good_end == bs[-1]["end"] and bs[-1]["nb"] >= 1 and good_end > len(c["existing"]):
            got.add(E_ERR[status])
        if status == OK and len(bs) == 1 and bs[0]["nb"] >= 1:
            got.add(E_ONLY)
        for k, e in enumerate(ev):
            if e["kind"] == "park" and e["pending"]:
                got.add(E_PARK)
            if e["kind"] == "carry" and e["pending"]:
                got.add(E_CARRY)
            if e["kind"] != "batch":
                continue
            b = bs.index(e)
            pending = e["pend_in"] < e["ob0"]
            if e["nb"] == 0:
                if e["after"] == "batch" and pending:
                    got.add(E_SOLO_AFTER)
                if b + 1 < len(bs) and bs[b + 1]["nb"] >= 1 and bs[b + 1]["piece"] == e["piece"] and bs[b + 1]["after"] == "solo":
                    got.add(E_SOLO_BEFORE)
                continue
            got.add(E_RES[(e["end"] + c["rb"]) & 15])
            if pending and e["pend_out"] == e["pend_in"]:
                got.add(E_STAY)
            if pending and (e["pend_in"] + c["rb"]) & 15 and e["pend_out"] > e["pend_in"]:
                got.add(E_HEAD)
            near_lo = max(e["ob0"] - NEAR_HIST, 0)
            for t in e["toks"]:
                s0 = t["mo"] - t["off"]
                if t["cls"] == FAR and near_lo > 0 and pending:
                    if s0 + t["M"] == near_lo:
                        got.add(E_FAR_AT)
                    if s0 + t["M"] == near_lo - 1:
                        got.add(E_FAR_BELOW)
                    if b >= 3 and all(x["piece"] == e["piece"] and x["nb"] >= 1 for x in bs[b - 3:b]) and bs[b - 3]["ob0"] <= s0 and s0 + t["M"] <= bs[b - 3]["end"]:
                        got.add(E_FAR_NEWEST)
                if t["cls"] == STRADDLING and pending:
                    got.add(E_STRADDLE)
                if t["cls"] == PREFIX and pending:
                    got.add(E_PREFIX)
                if e["after"] is None and e["piece"] > 0 and b > 0 and t["M"] and t["off"] <= t["mo"] and bs[b - 1]["ob0"] <= s0 < bs[b - 1]["end"]:
                    got.add(E_HAND_NEAR)
    return got


# ------------------------------------------------------------------------------------------------------------------------- building
def case(name, b, rb=0, wants=(), status=OK, cap=CAP):
    return dict(name=name, input=b.end(), prefix=b.prefix, existing=b.existing, limit=1 << 22, cap=cap, rb=rb, wants=set(wants), status=status)


def dense(seed, n_tok, existing=4120, prefix=0, first_L=12):
    """n_tok sequences of 15 compressed and 21 output bytes (a batch of 64 is 1 344 bytes, a window lists 69 and carries 5)."""
    b = Block(seed, existing=existing, prefix=prefix)
    b.seq(first_L, 9, 30)
    for _ in range(n_tok - 1):
        b.seq(12, 9, 30)
    return b


def patch(c, batch, lane, off_of):
    """The match offset of one token rewritten: off_of(batch event, token record, all batch events of the whole job) -> offset."""
    bs = [e for e in model(c)[0] if e["kind"] == "batch"]
    t = bs[batch]["toks"][lane]
    off = off_of(bs[batch], t, bs)
    assert 0 <= off <= 0xFFFF
    blk = bytearray(c["input"])
    blk[t["q"]:t["q"] + 2] = off.to_bytes(2, "little")
    c["input"] = bytes(blk)
    return c


def walk_case():
    """Twenty rounds.  Two literal runs of a batch's size, token-like from the first byte of chunk 1 of the parse (14 336) on, keep that chunk's
    chain out of step until behind 16 384, where its share of the bit map starts: the first run's window and the second's (15 296, all of it
    chunk 0's share) are listed rightly and run a batch each, the window behind them comes wrong from the map, bails and is walked.  Which
    lengths of the two runs leave the false chain out of step is found by trying; the census (emulator + model) decides."""
    for L2, adj in ((L2, adj) for L2 in range(1085, 1125) for adj in range(3)):
        b = P.dense_to(P.start(140), fw.STRIDE - 200)
        L1 = 15300 - b.cpos - 6 + adj
        lit_start = b.cpos + 1 + (1 + (L1 - 15) // 255)
        lit = bytearray(x or 1 for x in P._rnd(L1, 141))
        lit[fw.STRIDE - lit_start:] = fw.token_like(L1 - (fw.STRIDE - lit_start))
        b.seq(L1, 9, 7, lit=bytes(lit))
        b.seq(L2, 11, 7, lit=fw.token_like(L2))
        if not fw.CHUNK < b.cpos < fw.CHUNK + 64:
            continue
        P.dense(b, 2)
        blk, built = P.finish(b, 20 * ROUND)
        c = dict(name="walk: chunk 1 not in step behind two batches, its share's first window is walked", input=blk, prefix=b"", existing=b"", limit=1 << 22,
                 cap=(len(built) + 255) // 256 * 256, rb=15, wants={E_WALK, E_PARK, E_CARRY}, status=OK)
        if E_WALK in census(c):
            return c
    raise AssertionError("no length of the second run keeps chunk 1 out of step")


def corpus():
    out = []
    near_lo = lambda e: e["ob0"] - NEAR_HIST      # noqa: E731
    # five windows of dense sequences: far sources at the edge of the intact history and in the newest batch they reach, parked pieces, carried batches
    for rb in RBS:
        c = case(f"dense: far sources at the edges, rb {rb}", dense(10 + rb, 300), rb=rb,
                 wants=[E_FAR_AT, E_FAR_BELOW, E_FAR_NEWEST, E_HAND_NEAR, E_PARK, E_CARRY])
        patch(c, 3, 5, lambda e, t, bs: t["mo"] - (near_lo(e) - t["M"]))
        patch(c, 3, 9, lambda e, t, bs: t["mo"] - (near_lo(e) - 1 - t["M"]))
        patch(c, 3, 20, lambda e, t, bs: t["mo"] - (bs[0]["ob0"] + 100))
        patch(c, 4, 0, lambda e, t, bs: t["mo"] - (near_lo(e) - t["M"]))
        patch(c, 1, 63, lambda e, t, bs: t["mo"] - (near_lo(e) - t["M"]))
        out.append(c)
    # a batch's end at every residue of the output address
    for r in range(16):
        rb = RBS[r % 3]
        out.append(case(f"lines: batches end at residue {r}, rb {rb}", dense(40 + r, 140, existing=4112, first_L=12 + (r - rb) % 16), rb=rb,
                        wants=[E_RES[r]] + ([E_HEAD] if rb else [])))
    # a solo sequence between two batches
    for rb in RBS:
        b = dense(60 + rb, 10, existing=4200)
        b.seq(10, 1400, 7)
        for _ in range(10):
            b.seq(12, 9, 30)
        out.append(case(f"solo: between two batches, rb {rb}", b, rb=rb, wants=[E_SOLO_AFTER, E_SOLO_BEFORE]))
    # slow matches in the second batch
    for rb in RBS:
        c = case(f"slow: straddling source, rb {rb}", dense(70 + rb, 140), rb=rb, wants=[E_STRADDLE])
        out.append(patch(c, 1, 7, lambda e, t, bs: t["mo"] - (near_lo(e) - 2)))
        c = case(f"slow: prefix source, rb {rb}", dense(80 + rb, 140, existing=0, prefix=300), rb=rb, wants=[E_PREFIX])
        out.append(patch(c, 1, 7, lambda e, t, bs: t["mo"] + 5))
    # the only batch
    for rb in RBS:
        b = Block(90 + rb, existing=4100)
        b.seq(3, 5, 9)
        out.append(case(f"end: one batch, rb {rb}", b, rb=rb, wants=[E_ONLY]))
    # an error in the batch behind a good one
    for rb in RBS:
        c = case(f"error: zero offset in the second batch, rb {rb}", dense(100 + rb, 140), rb=rb, wants=[E_ERR[ZERO_OFFSET]], status=ZERO_OFFSET)
        out.append(patch(c, 1, 6, lambda e, t, bs: 0))
        c = case(f"error: offset beyond the prefix in the second batch, rb {rb}", dense(110 + rb, 140), rb=rb, wants=[E_ERR[INVALID_OFFSET]], status=INVALID_OFFSET)
        out.append(patch(c, 1, 6, lambda e, t, bs: 0xFFFF))
        c = case(f"error: capacity in the second batch, rb {rb}", dense(120 + rb, 140), rb=rb, wants=[E_ERR[OUT_CAPACITY]], status=OUT_CAPACITY)
        t = [e for e in model(c)[0] if e["kind"] == "batch"][1]["toks"][6]
        c["cap"] = t["mo"] + 3
        out.append(c)
    # a first batch of six bytes behind a misaligned start: the range does not reach its first line and stays pending through the second batch
    for existing in (4101, 4106):
        b = Block(130 + existing, existing=existing)
        b.seq(2, 4, 9); b.seq(1356, 4, 40)
        for _ in range(10):
            b.seq(12, 9, 30)
        out.append(case(f"lines: six bytes behind out & 15 = {existing & 15}", b, wants=[E_STAY] if existing == 4101 else [E_HEAD]))
    # the walk-mode retry: the one large block (see the module's head)
    out.append(walk_case())
    assert len({c["name"] for c in out}) == len(out)
    return out
