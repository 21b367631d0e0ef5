"""Built edges of the batched kernels' copy stage (lz4_decompress_batch_phase.inc, included by the pair, staged and bitmap-fed kernels) and a host
model of it.  Plain Python and numpy: no GPU, no library (the fed geometry takes its windows from the emulator's log, fed_window_cases.emulate).

  * geometries: the ring, a batch's span, the intact history, the staged bytes and the rule by which a batch's token list is drawn — written
    here as literals next to the source line they restate, never read from the code under test;
  * model(): batch by batch what the stage does with a block — ob0, nb, solo, per lane L / M / off / lo / mo and the class of its literals and of
    its match, the fence, the rounds of the resolve loop — and the status it ends with (decompress.rs:58-138);
  * cases(geom, rb): raw blocks built sequence by sequence (the builder of seg_stage_cases.py), one group per family of edges;
  * edges(geom) / census(): the named edges and which of them a model run reaches.  A match or literal run counts for an edge only when its bytes
    tell a wrong copy apart (discriminating()).
tests/test_copy_stage_cases_cpu.py requires every edge for every geometry and residue; tests/test_gpu_copy_stage.py runs the cases on the device
and compares bytes, statuses, and the kernels' batch and round counters with the model."""
import collections
import functools

import numpy as np

from seg_stage_cases import _lsic, _seq, _block, _walk, Blk, Parse  # noqa: F401  (the one encoder)

OK, UNEXPECTED_END, MEMORY_LIMIT_EXCEEDED, ZERO_OFFSET, INVALID_OFFSET, OUTPUT_FULL, CONTRACT, OUT_CAPACITY = range(8)    # oracle_ffi
KSHORT = 64              # kShort     lzf_copy_helpers.h:13   bytes a lane moves by itself
KFARSHORT = 32           # kFarShort  lzf_copy_helpers.h:14   same for far matches
TOTCLAMP = 1 << 25       # kTotClamp  lzf_copy_helpers.h:15
INPUT_MAX, OUTPUT_MAX, JOBS_MAX = 64 << 10, 1 << 20, 400
RESIDUES = (0, 1, 15)
EXISTING = (0, 1, 17, 4095, 4096, 4097, 20000)
PREFIX_LEN = 3000

# name, RING, kSpanMax = RING / 3, kNearHist = RING - kSpanMax, kCB, the rule, bytes of input one token list covers, TOKCAP
#   paired48 / paired24  lz4_decompress_paired.hip:22-25 (kSpanMax, kNearHist, kChunk = 64 S, kCB = kChunk + 64), kernels.h:62-63 (S, TOKCAP)
#   staged16             lz4_decompress_batched.hip:55-58, kernels.h:29
#   fed                  lz4_decompress_fed.hip:50-53 (kRound = 32 W, kCB = kRound + 128), kernels.h:159 (W = 32, TOKCAP = 352)
# The chunk rule (lz4_decompress_parse_phase.inc:152-153, :233-246): a chunk lists the tokens that start in [cstart, cstart + 64 S), TOKCAP of
# them at most, and the next chunk starts at the first token it did not list.
Geom = collections.namedtuple("Geom", "name ring span hist kcb rule cover tokcap")
GEOMS = {g.name: g for g in (
    Geom("paired48", 4096, 1365, 2731, 3136, "chunk", 3072, 640),
    Geom("paired24", 4096, 1365, 2731, 1600, "chunk", 1536, 384),
    Geom("staged16", 4096, 1365, 2731, 1088, "chunk", 1024, 256),
    Geom("fed", 4096, 1365, 2731, 1152, "fed", 1024, 352))}

FAR_M = (4, 7, 8, 16, 17, 32, 33, 64, 65, 255, 256, 257, 1100)
NEAR1_M = (4, 7, 8, 16, 17, 32, 33, 64)
COOP_M = (65, 255, 256, 257)
OVER_OFF = (1, 2, 3, 4, 7, 8, 15, 16, 63, 64, 65)
LIT_L = (0, 1, 2, 3, 4, 7, 8, 16, 17, 32, 33, 64, 65, 64 + 255, 64 + 256, 64 + 257)


def over_m(off):
    """The overlapping lengths asked for at one offset: off + 1, 64, 65, 300 (those that overlap)."""
    return sorted({m for m in (off + 1, 64, 65, 300) if m > off and m >= 4})


# ------------------------------------------------------------------------------------------------------------------------- the model
def listings(geom, blk, toks):
    """[(cstart, [indices into toks], upto)]: the token lists the batches are drawn from, in order; the batches take the first `upto` of a list
    (fed: the rest is a short last batch left for the next window, which lists it again)."""
    out, n = [], len(toks)
    if geom.rule == "chunk":
        i = 0
        while i < n:
            cstart, j = toks[i][0], i
            while j < n and j - i < geom.tokcap and toks[j][0] < cstart + geom.cover:
                j += 1
            out.append((cstart, list(range(i, j)), j - i)); i = j
        return out
    # fed: the windows as the emulator logs them.  A window's `pos` is the 32-aligned position at or below the chain's next token (not that
    # token itself), and it lists the tokens that start in [pos, pos + 1 024).
    import fed_window_cases as fw
    rc, st, log = fw.emulate(blk)
    assert rc == 0 and st["walked_windows"] == 0, ("the model covers windows listed from a map that is right", rc, st)
    i = 0
    for k, (kind, pos) in enumerate(log):
        if kind == 2:
            continue
        stop = log[k + 1][1] if k + 1 < len(log) and log[k + 1][0] == 2 else None      # a short last batch left for the next window
        j = i
        while j < n and j - i < geom.tokcap and toks[j][0] < pos + geom.cover:
            j += 1
        idxs = list(range(i, j))
        upto = next((k2 for k2, q in enumerate(idxs) if toks[q][0] == stop), len(idxs))
        out.append((pos, idxs, upto)); i += upto
    assert i == n, (i, n)
    return out


def _rounds(lanes):
    """The resolve loop (`while (unresolved)`): its iterations, and what the single-lane rounds met — ("at H", lane): moved with its source's end
    exactly at H; ("H+1", lane): one byte beyond, left waiting."""
    pend = {i: (l["s0"] + l["span"] if l["m"] == "near1" else None) for i, l in enumerate(lanes) if l["m"] and (l["m"].startswith(("near", "coop", "slow")))}
    n, ev = 0, set()
    while pend:
        f = min(pend); n += 1
        if lanes[f]["m"] == "near1":
            H = lanes[f]["mo"]
            for i, e in pend.items():
                if e is not None and i != f and e == H:
                    ev.add(("at H", i))
                if e is not None and e == H + 1:
                    ev.add(("H+1", i))
            for i in [i for i, e in pend.items() if e is not None and e <= H]:
                del pend[i]
        else:
            del pend[f]
    return n, ev


Result = collections.namedtuple("Result", "batches status nbatch rounds toks")


MUTANTS = ("s0 > near_lo", "s0 + span < near_lo", "M < off", "kShort - 1", "kShort + 1", "kSpanMax + 1", "kSpanMax - 1", "kNearHist + 1", "kNearHist - 1")


def model(blk, geom, rb, prefix_len=0, existing_len=0, limit=None, cap=None, mut=""):
    """One entry per batch (a dict: cstart, ob0, nb, solo, fence, safe0, rounds, events, lanes — per lane L, M, off, has, src, lo, mo and the classes
    lit / lit_src / long_wrap / off_arm / m / mwrap / swrap / code) and the job's status, batch count and round count.  mut: one of MUTANTS, a
    comparison or a threshold of the match classification moved by one (the census test: the counts of some built block must notice)."""
    if mut.startswith("kSpanMax"):
        geom = geom._replace(span=geom.span + (1 if mut.endswith("+ 1") else -1))
    if mut.startswith("kNearHist"):
        geom = geom._replace(hist=geom.hist + (1 if mut.endswith("+ 1") else -1))
    kshort = KSHORT + (mut == "kShort + 1") - (mut == "kShort - 1")
    limit = (1 << 63) - 1 if limit is None else limit
    cap = (1 << 31) if cap is None else cap
    toks, err = Parse(blk).chain(0)
    assert not err, "the built blocks hold whole tokens"
    R, P = geom.ring, prefix_len
    ridx = lambda x: (x + rb) & (R - 1)       # noqa: E731  RIDX (lzf_out_ring.h:39)
    o = safe = existing_len
    status, batches = OK, []
    for cstart, idxs, upto in listings(geom, blk, toks):
        t = 0
        while t < upto and status == OK:
            nb_try = min(64, len(idxs) - t)
            tk = [toks[k] for k in idxs[t:t + nb_try]]
            incl = np.cumsum([min(L + M, TOTCLAMP) for _, L, M, _, _ in tk])
            over = np.nonzero(incl > geom.span)[0]
            nb = min(int(over[0]) if len(over) else nb_try, nb_try)
            ob0 = o
            B = dict(cstart=cstart, ob0=ob0, nb=nb, solo=nb == 0, fence=False, safe0=safe, rounds=0, events=set(), lanes=[], first=idxs[t],
                     incl=incl[:max(nb, 1) + 1].tolist())
            batches.append(B)
            if nb == 0:                                     # C. solo sequence (.inc:141-200)
                pos, L, M, off, src = tk[0]
                B["lanes"].append(dict(L=L, M=M, off=off, has=M > 0, src=src, lo=o, mo=o + L, nn=None))
                ln = B["lanes"][0]
                if cap - o < L:
                    status = OUT_CAPACITY; break
                if M and o + L + M > limit:
                    status = MEMORY_LIMIT_EXCEEDED; break
                o += L
                if M:
                    mlen = M
                    if off == 0:
                        status = ZERO_OFFSET; break
                    if off > o:
                        need = off - o
                        if need > P:
                            status = INVALID_OFFSET; break
                        nn = min(need, mlen); ln["nn"] = nn
                        if cap - o < nn:
                            status = OUT_CAPACITY; break
                        o += nn; mlen -= nn
                    if mlen:
                        if cap - o < mlen:
                            status = OUT_CAPACITY; break
                        if o - off + min(mlen, off) > safe:
                            B["fence"] = True
                        o += mlen
                safe = o
                t += 1
                continue
            near_lo = ob0 - geom.hist if ob0 > geom.hist else 0
            need = 0
            for j in range(nb):
                pos, L, M, off, src = tk[j]
                lo = ob0 + int(incl[j]) - min(L + M, TOTCLAMP); mo = lo + L
                has = M > 0
                ln = dict(L=L, M=M, off=off, has=has, src=src, lo=lo, mo=mo, lit=None, lit_src=None, long_wrap=False, off_arm=None, m=None,
                          mwrap=False, swrap=False, code=OK, s0=None, span=None)
                if L:
                    n1 = min(L, KSHORT)
                    ln["lit"] = "long" if L > KSHORT else "own"
                    ln["lit_src"] = "bytes-wrap" if ridx(lo) + n1 > R else "lds" if src - cstart + n1 <= geom.kcb else "global"      # .inc:263-269
                    ln["long_wrap"] = L > KSHORT and ridx(lo + KSHORT) + (L - KSHORT) > R
                if has:
                    q = src + L - cstart                                                         # .inc:206-210 (every geometry here stages)
                    ln["off_arm"] = "lds16" if q + 2 <= geom.kcb else "bytes-straddle" if q + 1 == geom.kcb else "bytes-global"
                if lo > cap or cap - lo < L:                                                     # .inc:213-219
                    ln["code"] = OUT_CAPACITY
                elif has and mo + M > limit:
                    ln["code"] = MEMORY_LIMIT_EXCEEDED
                elif has and off == 0:
                    ln["code"] = ZERO_OFFSET
                elif has and off > mo and off - mo > P:
                    ln["code"] = INVALID_OFFSET
                elif has and cap - mo < M:
                    ln["code"] = OUT_CAPACITY
                if has and off:                                                                  # .inc:225-233
                    span = min(M, off); s0 = mo - off
                    ln["span"], ln["s0"] = span, s0
                    from_prefix = off > mo
                    mi = ridx(mo)
                    ln["mwrap"] = mwrap = mi + M > R
                    if from_prefix:
                        ln["m"] = "slow-prefix"
                        ln["pre"] = off - mo                                                      # bytes the prefix can give
                        ln["glb"] = M > off - mo and near_lo > 0                                  # the rest starts at out[0], below near_lo
                        if M > off - mo:
                            need = max(need, near_lo)
                    elif s0 >= near_lo + (mut == "s0 > near_lo"):
                        ln["swrap"] = swrap = ridx(s0) + M > R
                        ln["m"] = "near1" if M <= off - (mut == "M < off") and M <= kshort and not mwrap and not swrap else "coop" if M <= off else "coop-ov"
                    elif s0 + span <= near_lo - (mut == "s0 + span < near_lo"):
                        ln["m"] = ("far-own" if M <= KFARSHORT and not mwrap else "far-wrap" if M <= KSHORT and mwrap else
                                   "far-mid" if M <= KSHORT else "far-long")
                        ln["fresh"] = s0 + M > safe
                        need = max(need, s0 + M)
                    else:
                        ln["m"] = "slow-straddle"
                        need = max(need, near_lo)
                B["lanes"].append(ln)
            bad = [ln["code"] for ln in B["lanes"] if ln["code"] != OK]
            if bad:
                status = bad[0]; break
            if min(need, ob0) > safe:                                                            # .inc:235-242
                B["fence"] = True; safe = ob0
            B["rounds"], B["events"] = _rounds(B["lanes"])
            o = ob0 + int(incl[nb - 1])
            t += nb
        if status != OK:
            break
    return Result(batches, status, len(batches), sum(b["rounds"] for b in batches), toks)


# ------------------------------------------------------------------------------------------------------------- discriminating bytes
def _copy(hist, off, M):
    """copy_overlapping (decompress.rs:80-138) of M bytes at distance off behind `hist`; None where the source does not exist."""
    if off < 1 or off > len(hist):
        return None
    if off >= M:
        s = len(hist) - off
        return bytes(hist[s:s + M])
    return (bytes(hist[-off:]) * (M // off + 1))[:M]


SEAMS = (16, 32)         # where the 8-byte pieces of a lane's own copy meet: a size class taken one byte too far leaves a hole there, not at an end


def discriminating_match(full, P, R, mo, M, off):
    """Would the output change if the match's source were moved by +-1, +-16, +-RING, or the copy were one byte short at either end?  `full` is
    prefix + output.  A moved source that does not exist (in front of the prefix, at or behind the destination) defines no bytes and is left out;
    a byte the copy leaves out — at either end, or at a seam of its 8-byte pieces — keeps what the ring held there, the byte RING earlier, where there is
    one (in the first ring of output the slot holds nothing defined)."""
    a = P + mo
    want = bytes(full[a:a + M])
    for d in (1, -1, 16, -16, R, -R):
        got = _copy(full[:a], off - d, M)
        if got is not None and got == want:
            return False
    for x in {a, a + M - 1} | {a + k for k in SEAMS if k < M}:
        if x - P - R >= 0 and full[x - R] == full[x]:          # (output positions: the prefix is never in the ring)
            return False
    return True


def discriminating_lits(full, P, R, blk, lo, L, src):
    if L == 0:
        return True
    a = P + lo
    want = bytes(full[a:a + L])
    for d in (1, -1, 16, -16, R, -R):
        if 0 <= src + d and src + d + L <= len(blk) and bytes(blk[src + d:src + d + L]) == want:
            return False
    for x in {a, a + L - 1} | {a + k for k in SEAMS if k < L}:
        if x - P - R >= 0 and full[x - R] == full[x]:
            return False
    return True


# ------------------------------------------------------------------------------------------------------------------------ the edges
def edges(geom):
    """Every named edge of the stage for one geometry."""
    e = {"cut: cumulative output == kSpanMax, no cut", "cut: cumulative output == kSpanMax + 1, cut at that lane", "cut: one sequence of kSpanMax, a batch of one",
         "cut: one sequence of kSpanMax + 1, solo", "cut: 64 short tokens", "cut: a batch behind a solo sequence", "cut: last literals at lane 0",
         "cut: last literals at lane 63",
         "class: s0 == near_lo, near", "class: s0 == near_lo, near, others share its round", "class: s0 == near_lo - 1, slow-straddle", "class: s0 + span == near_lo, far", "class: s0 + span == near_lo + 1, slow",
         "class: near_lo == 0 and s0 == 0", "far: source newer than safe, the fence runs", "far: old source, no fence",
         "near1 refused: M == off + 1", "near1 refused: M == 65", "near1 refused: mwrap", "near1 refused: source wraps",
         "near1: source ends at H, moved in that round", "near1: source ends at H + 1, waits", "near1: chain of 64, 64 rounds", "near1: every match in round one",
         "literals: own share wraps", "literals: long run wraps", "offset: in the staged bytes", "offset: straddles kCB", "offset: starts at kCB", "offset: beyond kCB",
         "solo: L > kSpanMax", "solo: offset 1, M % 16 == 0", "solo: offset 1, M % 16 == 1", "solo: offset 1, M % 16 == 15", "solo: offset 2", "solo: offset 3",
         "solo: offset 63", "solo: offset >= M", "solo: source newer than safe", "solo: output <= RING", "solo: output > RING",
         "solo: refill, then near at distance 1", "solo: refill, then near at distance kNearHist - 1", "solo: refill, then near at distance kNearHist",
         "solo: last literals > kSpanMax",
         "prefix: M == off - mo", "prefix: M == off - mo + 1", "prefix: crosses into out and overlaps itself", "prefix: off - mo == prefix_len",
         "prefix: off - mo == prefix_len + 1, InvalidDedupOffset", "prefix: off - mo == prefix_len + 1, InvalidDedupOffset, solo", "prefix: rest from out[0..] below near_lo", "prefix: solo, nn < mlen", "prefix: solo, nn == mlen",
         "existing: source crosses from existing into new output",
         "status: zero offset at lane 0", "status: zero offset at lane 63", "status: offset one beyond at lane 0", "status: offset one beyond at lane 63",
         "status: two codes, the earlier wins", "status: capacity exact, literals", "status: capacity one short, literals", "status: capacity exact, match",
         "status: capacity one short, match", "status: limit exact", "status: limit one over"}
    e |= {f"far: M={m}" for m in FAR_M} | {f"far: M={m}, mwrap" for m in FAR_M}
    e |= {f"near1: M={m}" for m in NEAR1_M}
    e |= {f"coop: M={m}{w}" for m in COOP_M for w in ("", ", mwrap", ", source wraps")}
    e |= {f"overlap: off={o} M={m}" for o in OVER_OFF for m in over_m(o)}
    e |= {f"literals: L={v}" for v in LIT_L}
    e |= {f"existing_len={v}" for v in EXISTING}
    # An own share that ends at or one byte beyond the staged bytes: a token that starts inside the list's cover (offset <= cover - 1) with 64 or more
    # literals in a batch (L <= kSpanMax: at most 1 + 6 bytes of token and length in front of them) ends its own share at cover - 1 + 7 + 64 at most.
    if geom.cover + 6 + KSHORT >= geom.kcb:
        e |= {"literals: own share ends at kCB", "literals: own share ends one byte beyond kCB"}
    return e


def census(case, geom, rb, res):
    """The named edges one model run reaches."""
    got = set()
    R, H, SP = geom.ring, geom.hist, geom.span
    P, E = len(case["prefix"]), len(case["existing"])
    full = case["prefix"] + case["output"] if case["status"] == OK else None
    blk = case["input"]
    dm = lambda ln: full is not None and discriminating_match(full, P, R, ln["mo"], ln["M"], ln["off"])              # noqa: E731
    dl = lambda ln: full is not None and discriminating_lits(full, P, R, blk, ln["lo"], ln["L"], ln["src"])         # noqa: E731
    if (P or E) and res.status == OK:
        got.add(f"existing_len={E}")
    last = len(res.toks) - 1
    for bi, B in enumerate(res.batches):
        prev = res.batches[bi - 1] if bi else None
        lanes, nb, ob0 = B["lanes"], B["nb"], B["ob0"]
        near_lo = ob0 - H if ob0 > H else 0
        failed = res.status != OK and bi == len(res.batches) - 1
        if B["solo"]:
            ln = lanes[0]
            L, M, off = ln["L"], ln["M"], ln["off"]
            if failed:
                if M and off > ln["mo"] and off - ln["mo"] == P + 1 and P:
                    got.add("prefix: off - mo == prefix_len + 1, InvalidDedupOffset, solo")
                continue
            if L + M == SP + 1:
                got.add("cut: one sequence of kSpanMax + 1, solo")
            if L > SP and dl(ln):
                got.add("solo: L > kSpanMax" if M else "solo: last literals > kSpanMax")
            if M > SP and dm(ln):
                if off == 1:
                    got.add(f"solo: offset 1, M % 16 == {M % 16}")
                if off in (2, 3, 63):
                    got.add(f"solo: offset {off}")
                if off >= M:
                    got.add("solo: offset >= M")
                if B["fence"]:
                    got.add("solo: source newer than safe")
                if ln["nn"] is not None:
                    got.add("prefix: solo, nn == mlen" if ln["nn"] == M else "prefix: solo, nn < mlen")
            if M and dm(ln):
                got.add("solo: output > RING" if L + M > R else "solo: output <= RING")
            continue
        incl = B["incl"]
        if not failed:
            if nb >= 2 and incl[nb - 1] == SP:
                got.add("cut: cumulative output == kSpanMax, no cut")
            if nb >= 1 and len(incl) > nb and incl[nb] == SP + 1:
                got.add("cut: cumulative output == kSpanMax + 1, cut at that lane")
            if nb == 1 and incl[0] == SP:
                got.add("cut: one sequence of kSpanMax, a batch of one")
            if nb == 64:
                got.add("cut: 64 short tokens")
            if prev is not None and prev["solo"]:
                got.add("cut: a batch behind a solo sequence")
            if not lanes[0]["has"]:
                got.add("cut: last literals at lane 0")
            if nb == 64 and not lanes[63]["has"]:
                got.add("cut: last literals at lane 63")
            n1 = sum(ln["m"] == "near1" for ln in lanes)
            if nb == 64 and B["rounds"] == 64:
                got.add("near1: chain of 64, 64 rounds")
            if n1 >= 8 and B["rounds"] == 1:
                got.add("near1: every match in round one")
            for what, j in B["events"]:
                if dm(lanes[j]):
                    got.add("near1: source ends at H, moved in that round" if what == "at H" else "near1: source ends at H + 1, waits")
            if any(ln["m"] and ln["m"].startswith("far") and dm(ln) for ln in lanes):
                got.add("far: source newer than safe, the fence runs" if B["fence"] and any(ln.get("fresh") for ln in lanes) else "far: old source, no fence")
        codes = [ln["code"] for ln in lanes]
        if failed:
            j = next(i for i, c in enumerate(codes) if c != OK)
            ln = lanes[j]
            if len({c for c in codes if c != OK}) >= 2:
                got.add("status: two codes, the earlier wins")
            if ln["code"] == ZERO_OFFSET and j in (0, 63):
                got.add(f"status: zero offset at lane {j}")
            if ln["code"] == INVALID_OFFSET and ln["off"] == ln["mo"] + P + 1:
                if j in (0, 63) and not P:
                    got.add(f"status: offset one beyond at lane {j}")
                if P:
                    got.add("prefix: off - mo == prefix_len + 1, InvalidDedupOffset")
            if ln["code"] == OUT_CAPACITY:
                if case["cap"] - ln["lo"] == ln["L"] - 1:
                    got.add("status: capacity one short, literals")
                elif case["cap"] - ln["mo"] == ln["M"] - 1 and ln["has"]:
                    got.add("status: capacity one short, match")
            if ln["code"] == MEMORY_LIMIT_EXCEEDED and ln["mo"] + ln["M"] == case["limit"] + 1:
                got.add("status: limit one over")
            continue
        for j, ln in enumerate(lanes):
            L, M, off, lo, mo, m = ln["L"], ln["M"], ln["off"], ln["lo"], ln["mo"], ln["m"]
            if L and case["cap"] - lo == L:
                got.add("status: capacity exact, literals")
            if M and case["cap"] - mo == M:
                got.add("status: capacity exact, match")
            if M and mo + M == case["limit"]:
                got.add("status: limit exact")
            if dl(ln):
                if L in LIT_L:
                    got.add(f"literals: L={L}")
                if ln["lit_src"] == "bytes-wrap":
                    got.add("literals: own share wraps")
                if ln["long_wrap"]:
                    got.add("literals: long run wraps")
                if L >= KSHORT and ln["src"] - B["cstart"] + KSHORT == geom.kcb and ln["lit_src"] == "lds":
                    got.add("literals: own share ends at kCB")
                if L >= KSHORT and ln["src"] - B["cstart"] + KSHORT == geom.kcb + 1 and ln["lit_src"] == "global":
                    got.add("literals: own share ends one byte beyond kCB")
            if not M or not dm(ln):
                continue
            got.add({"lds16": "offset: in the staged bytes", "bytes-straddle": "offset: straddles kCB", "bytes-global": "offset: beyond kCB"}[ln["off_arm"]])
            if ln["src"] + L - B["cstart"] == geom.kcb:
                got.add("offset: starts at kCB")
            s0, span = ln["s0"], ln["span"]
            if m == "slow-prefix":
                pre = ln["pre"]
                if M == pre:
                    got.add("prefix: M == off - mo")
                if M == pre + 1:
                    got.add("prefix: M == off - mo + 1")
                if M > pre and off < M:
                    got.add("prefix: crosses into out and overlaps itself")
                if pre == P:
                    got.add("prefix: off - mo == prefix_len")
                if ln["glb"] and ob0 > H and M - pre <= near_lo:
                    got.add("prefix: rest from out[0..] below near_lo")
                continue
            if near_lo > 0:
                if s0 == near_lo and m in ("near1", "coop", "coop-ov"):
                    got.add("class: s0 == near_lo, near")
                    if m == "near1" and j == 0 and B["rounds"] == 1 and sum(x["m"] == "near1" for x in lanes) >= 3:
                        got.add("class: s0 == near_lo, near, others share its round")
                if s0 == near_lo - 1 and span >= 2 and m == "slow-straddle":
                    got.add("class: s0 == near_lo - 1, slow-straddle")
                if s0 + span == near_lo and m.startswith("far"):
                    got.add("class: s0 + span == near_lo, far")
                if s0 + span == near_lo + 1 and m == "slow-straddle":
                    got.add("class: s0 + span == near_lo + 1, slow")
            elif s0 == 0 and m in ("near1", "coop", "coop-ov"):
                got.add("class: near_lo == 0 and s0 == 0")
            if m == "slow-straddle" and s0 < E < s0 + span:
                got.add("existing: source crosses from existing into new output")
            if m.startswith("far") and (M in FAR_M or M > 1000):
                got.add(f"far: M={M if M in FAR_M else FAR_M[-1]}" + (", mwrap" if ln["mwrap"] else ""))
            if m == "near1" and M in NEAR1_M:
                got.add(f"near1: M={M}")
            if m in ("coop", "coop-ov"):
                fine = dict(over=M <= off, big=M <= KSHORT, mwrap=not ln["mwrap"], swrap=not ln["swrap"])
                only = [k for k, v in fine.items() if not v]
                if only == ["over"] and M == off + 1:
                    got.add("near1 refused: M == off + 1")
                if only == ["big"] and M == KSHORT + 1:
                    got.add("near1 refused: M == 65")
                if only == ["mwrap"]:
                    got.add("near1 refused: mwrap")
                if only == ["swrap"]:
                    got.add("near1 refused: source wraps")
            if m == "coop" and M in COOP_M and not (ln["mwrap"] and ln["swrap"]):
                got.add(f"coop: M={M}" + (", mwrap" if ln["mwrap"] else ", source wraps" if ln["swrap"] else ""))
            if m == "coop-ov" and off in OVER_OFF and M in over_m(off):
                got.add(f"overlap: off={off} M={M}")
            if prev is not None and prev["solo"] and prev["lanes"][0]["L"] + prev["lanes"][0]["M"] > R and m in ("near1", "coop", "coop-ov"):
                d = ob0 - s0
                if d in (1, H - 1, H):
                    got.add("solo: refill, then near at distance " + {1: "1", H - 1: "kNearHist - 1", H: "kNearHist"}[d])
    return got


# ------------------------------------------------------------------------------------------------------------------------ the cases
class CB(Blk):
    """Blk with a prefix and existing output in front (positions are offsets into `out`, as the kernel counts them) and pins: a sequence larger than
    a batch's span is decoded alone, so the token behind it starts a batch whose first output byte is known."""

    def __init__(self, g, rb, salt, seed, prefix=0, existing=0):
        super().__init__(seed + 7919 * salt)      # salt: cases() draws the literals again where a byte happens not to tell a wrong copy apart
        self.g, self.rb, self.P, self.E, self.pins = g, rb, prefix, existing, 0
        self.o += self._lits(prefix + existing, None)

    @property
    def opos(self):
        return len(self.o) - self.P

    def ridx(self, x):
        return (x + self.rb) & (self.g.ring - 1)

    def pin_to(self, target):
        """One solo sequence that ends at output position `target`."""
        gap = target - self.opos
        assert gap > self.g.span + 4, gap
        if len(self.o) >= 1500:
            self.pins += 1
            return self.seq(3, 1399 + 2 * (self.pins % 40), gap - 3)      # (a period that changes from pin to pin: no output repeats at 1, 16 or the ring)
        return self.seq(gap - 4, 7, 4)

    def pin(self, beyond=0):
        return self.pin_to(max(self.opos + self.g.span + 10, beyond))

    def pin_at(self, residue):
        """... that ends at the next output position whose ring index is `residue`."""
        t = self.opos + self.g.span + 5
        return self.pin_to(t + (residue - self.ridx(t)) % self.g.ring)

    def hard_pin(self):
        """A literal run longer than a token list's cover: the token behind it starts a chunk (a window), and a batch."""
        return self.seq(max(self.g.cover, self.g.span) + 40, 9, 4)


def fin(name, b, tail=5, status=OK, limit=None, cap=None, c=None):
    cc, o = b.end(tail)
    out = o[b.P:]
    return dict(name=name, input=cc if c is None else c, output=out if status == OK else b"", prefix=o[:b.P], existing=o[b.P:b.P + b.E], status=status,
                limit=len(out) if limit is None else limit, cap=len(out) + 64 if cap is None else cap)


def _patched(b, off, behind=0):
    """The block so far with its last sequence's offset field replaced (`behind`: the match-length bytes that follow it)."""
    c = bytearray(b.c); k = len(c) - 2 - behind; c[k:k + 2] = off.to_bytes(2, "little"); b.c = c
    return b


def cut_cases(g, rb, salt):
    sp = g.span
    b = CB(g, rb, salt, 101); b.seq(300, 9, 8)
    b.hard_pin()
    for i in range(10):
        b.seq(2, 40 + i, 98)
    b.seq(2, 33, sp - 1000 - 2); b.seq(3, 50, 4)              # lane 10 ends at kSpanMax exactly; lane 11 is cut off
    b.hard_pin()
    for i in range(10):
        b.seq(2, 40 + i, 98)
    b.seq(2, 33, sp - 1000 - 1); b.seq(3, 50, 4)              # lane 10 ends at kSpanMax + 1: cut at that lane
    b.hard_pin(); b.seq(5, 200, sp - 5); b.seq(1, 9, 4)       # one sequence of exactly kSpanMax
    b.hard_pin(); b.seq(5, 200, sp - 4); b.seq(1, 9, 4)       # ... + 1: solo
    out = [fin("cuts: spans at the limit", b)]
    b = CB(g, rb, salt, 102); b.seq(400, 9, 8)
    b.hard_pin()
    for i in range(64):
        b.seq(1, 300 + i, 4)                                   # 64 short tokens, every source in front of the batch: one round
    b.seq(2, 20, 5)
    b.hard_pin(); b.seq(4, 50, 4)
    for i in range(63):
        b.seq(0, 4, 4)                                         # each reads what the lane before wrote: 64 rounds
    b.hard_pin(); b.seq(6, 30, 4); b.seq(0, 8, 4); b.seq(0, 11, 4)     # source ends at H (lane 1), one byte beyond H (lane 2)
    b.hard_pin()
    for i in range(63):
        b.seq(1, 20 + i, 4 + i % 3)
    out.append(fin("cuts: 64 tokens, chain of 64, H, last literals at lane 63", b))
    b = CB(g, rb, salt, 103); b.seq(40, 9, 8); b.hard_pin()
    out.append(fin("cuts: last literals at lane 0", b))
    return out


def class_cases(g, rb, salt):
    H = g.hist
    out = []
    # each boundary in a block of its own: a job's rounds are one sum, and two boundaries moved together can cancel in it
    for k, (name, M, off_of) in enumerate((("s0 == near_lo", 8, lambda mo, nl: mo - nl), ("s0 == near_lo - 1", 8, lambda mo, nl: mo - nl + 1),
                                           ("s0 + span == near_lo", 8, lambda mo, nl: mo - nl + 8), ("s0 + span == near_lo + 1", 8, lambda mo, nl: mo - nl + 7))):
        b = CB(g, rb, salt, 201 + k)
        b.seq(20, 20, 8)                                       # near_lo == 0, s0 == 0
        b.seq(500, 11, 9)
        b.pin(beyond=H + 1200); ob0 = b.opos
        b.seq(3, off_of(ob0 + 3, ob0 - H), M)
        b.seq(1, 30, 5); b.seq(1, 30, 5)                       # two near matches of old bytes: they share lane 0's round when it is near, and only then
        b.pin(); b.seq(4, 50, 4)
        for _ in range(3):
            b.seq(0, 4, 4)                                     # (a short chain: the job's rounds are not its batches, in any kernel)
        out.append(fin("classes: " + name, b))
    # a far source written since the last fence: four batches of near matches, then a far match into the first one's output
    b = CB(g, rb, salt, 210); b.seq(500, 11, 9)
    b.pin(beyond=H + 1200); p = b.opos
    for i in range(4):
        b.seq(2, 50 + i, 1290)
    b.seq(3, b.opos + 3 - (p + 100), 8)
    b.pin(); b.seq(3, H + 3 + 8 + 40, 8)                       # and an old one
    out.append(fin("classes: the fence in front of a far match", b))
    return out


def far_cases(g, rb, salt):
    R, H = g.ring, g.hist
    out = []
    for half, Ms in enumerate((FAR_M[:7], FAR_M[7:])):
        b = CB(g, rb, salt, 311 + half); b.seq(1500, 11, 9)
        b.pin(beyond=H + 1300)
        for M in Ms:
            for wrap in (False, True):
                L = 3
                b.pin_at((R - M // 2 - L) % R if wrap else 100)
                b.seq(L, H + L + M + 5, M)
        out.append(fin(f"far: every size, wrapped and not ({half})", b))
    return out


def near_cases(g, rb, salt):
    R = g.ring
    b = CB(g, rb, salt, 401); b.seq(600, 11, 9)
    for M in NEAR1_M:
        b.seq(3, M + 20, M)
    b.seq(3, 9, 10); b.seq(3, 100, 65)                         # refused by M == off + 1, by M == 65
    for L, off, M in ((3, 8, 8), (3, 84, 64), (3, 85, 65)):    # M == off, M == kShort, kShort + 1 first in a batch, two matches of old bytes behind:
        b.pin(); b.seq(L, off, M); b.seq(1, 120, 5); b.seq(1, 120, 5)      # one round where lane 0 moves by itself, two where the wave moves it
    b.pin_at(R - 10 - 3); b.seq(3, 50, 20)                     # ... by mwrap
    b.pin_at(R - 10 + 50 - 3); b.seq(3, 50, 20)                # ... by the source's wrap
    for M in COOP_M:
        b.pin_at(1000); b.seq(3, M + 30, M)
        b.pin_at((R - M // 2 - 3) % R); b.seq(3, M + 30, M)    # mwrap
        b.pin_at((R - M // 2 + M + 30 - 3) % R); b.seq(3, M + 30, M)      # the source wraps
    out = [fin("near: single-lane sizes and refusals, cooperative sizes and wraps", b)]
    b = CB(g, rb, salt, 402); b.seq(200, 11, 9)
    for off in OVER_OFF:
        for M in over_m(off):
            b.seq(2, off, M)
    out.append(fin("near: overlapping, every offset and length", b))
    return out


def literal_cases(g, rb, salt):
    R = g.ring
    b = CB(g, rb, salt, 501); b.seq(40, 11, 9)
    for L in LIT_L:
        b.seq(L, 20 + L % 5, 4 + L % 3)
    b.pin_at(R - 10); b.seq(30, 20, 4)                         # an own share that wraps
    b.pin_at(R - 100); b.seq(300, 20, 4)                       # a long run that wraps
    out = [fin("literals: every length, wraps", b)]
    for name, at, L in (("own share ends at kCB", g.cover - 2, 64), ("own share ends one byte beyond kCB", g.cover - 1, 64),
                        ("offset straddles kCB", g.kcb - 203, 200), ("offset beyond kCB", g.kcb - 202, 200)):
        own = "literals: own share ends at kCB" in edges(g)
        if ("own share" in name and not own) or (name == "offset beyond kCB" and own):      # (the own share that ends at kCB has its offset right behind it)
            continue
        b = CB(g, rb, salt, 510 + len(out)); b.seq(9, 5, 6)
        b.to_c(at); b.seq(L, 20, 6)
        b.near(3, 5)
        out.append(fin("literals: " + name, b))
    return out


def solo_cases(g, rb, salt):
    H = g.hist
    b = CB(g, rb, salt, 601); b.seq(1600, 11, 9)
    for M in (1376, 1377, 1391):
        b.seq(2, 1, M); b.seq(3, 40, 6)
    for off in (2, 3, 63):
        b.seq(3, off, 1400); b.seq(2, 30, 5)
    b.seq(2, 1500, 1400)                                       # offset >= M
    for i in range(5):
        b.seq(3, 30 + i, 6)
    b.seq(2, 100, 1400)                                        # a source the batch before wrote
    for d in (1, H - 1, H):
        b.seq(2, 1500, 4200)                                   # more than the ring: the refill's other arm
        b.seq(2, 2 + d, 4)
    return [fin("solo: run-length tails, offsets, refills, long last literals", b, tail=g.span + 35)]


def prefix_cases(g, rb, salt):
    H, P = g.hist, PREFIX_LEN
    out = []
    for E in EXISTING:
        b = CB(g, rb, salt, 701 + E % 97, prefix=P, existing=E)
        mo = E + 3
        if mo + 60 <= g.span // 2:
            b.seq(3, mo + 10, mo + 50)                         # ten bytes of the prefix, then out[0..], then itself
        mo = b.opos + 3; b.seq(3, mo + 50, 50)                 # wholly in the prefix, M == off - mo
        mo = b.opos + 3; b.seq(3, mo + 50, 51)                 # one byte from out
        mo = b.opos + 3; b.seq(3, mo + P, 8)                   # the prefix's first byte
        if E >= 4:
            b.pin_to(E + H + 3); b.seq(2, b.opos + 2 - (E - 4), 16)       # a straddling source from existing output into new output
        b.pin(beyond=H + 100); mo = b.opos + 2; b.seq(2, mo + 5, 40)      # five bytes of the prefix, the rest from out[0..] through global memory
        b.seq(3, 9, 5)
        mo = b.opos + 2; b.seq(2, mo + 100, 1500)              # solo: nn < mlen
        b.seq(3, 9, 5)
        mo = b.opos + 2; b.seq(2, mo + 1500, 1500)             # solo: nn == mlen
        b.seq(4, 50, 4)
        for _ in range(4):
            b.seq(0, 4, 4)                                     # (a short chain: the job's rounds are not its batches, in any kernel)
        out.append(fin(f"prefix: existing_len {E}", b))
    for solo in (False, True):
        b = CB(g, rb, salt, 790 + solo, prefix=P, existing=17)
        mo = b.opos + 3; b.seq(3, mo + P, 1500 if solo else 8)
        _patched(b, mo + P + 1, behind=len(_lsic(1500 - 19)) if solo else 0)
        out.append(fin("prefix: one byte in front of the prefix" + (", solo" if solo else ""), b, status=INVALID_OFFSET, limit=1 << 20, cap=1 << 20))
    return out


def status_cases(g, rb, salt):
    out = []
    for lane in (0, 63):
        for what in ("zero", "beyond"):
            b = CB(g, rb, salt, 801 + lane); b.seq(40, 9, 8); b.hard_pin()
            for i in range(lane):
                b.seq(1, 20 + i, 4 + i % 3)
            mo = b.opos + 2; b.seq(2, 9, 6); _patched(b, 0 if what == "zero" else mo + 1)
            out.append(fin(f"status: offset {what} at lane {lane}", b, status=ZERO_OFFSET if what == "zero" else INVALID_OFFSET, limit=1 << 20, cap=1 << 20))
    b = CB(g, rb, salt, 810); b.seq(40, 9, 8); b.hard_pin()
    for i in range(5):
        b.seq(1, 20 + i, 5)
    b.seq(2, 9, 6); _patched(b, 0)
    for i in range(3):
        b.seq(1, 20 + i, 5)
    b.seq(2, 9, 6); _patched(b, 0xFFFF)
    out.append(fin("status: zero offset in front of an offset beyond the output", b, status=ZERO_OFFSET, limit=1 << 20, cap=1 << 20))
    for tail, what in ((9, "literals"), (0, "match")):
        def blk():
            b = CB(g, rb, salt, 820 + tail); b.seq(40, 9, 8)
            for i in range(20):
                b.seq(3 + i % 4, 20 + i, 5 + i % 7)
            return b
        n = len(blk().end(tail)[1])
        out.append(fin(f"status: capacity exact, {what}", blk(), tail=tail, limit=n + 10, cap=n))
        out.append(fin(f"status: capacity one short, {what}", blk(), tail=tail, status=OUT_CAPACITY, limit=n, cap=n - 1))
    out.append(fin("status: limit exact", blk(), tail=0, limit=n))
    out.append(fin("status: limit one over", blk(), tail=0, status=MEMORY_LIMIT_EXCEEDED, limit=n - 1, cap=n + 64))
    return out


def _build(g, rb, salt):
    out = sum((f(g, rb, salt) for f in (cut_cases, class_cases, far_cases, near_cases, literal_cases, solo_cases, prefix_cases, status_cases)), [])
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases(geom_name, rb):
    """The blocks of one geometry and residue.  Their literals are random bytes, so one in a few hundred of the matches copies a byte that equals
    its neighbour or the byte a ring earlier and does not count for its edge: the literals are drawn again (the first of sixteen seeds under
    which the census is whole; the first seed's blocks, for the census test to name what is missing, where there is none)."""
    g, first = GEOMS[geom_name], None
    for salt in range(16):
        cs = _build(g, rb, salt)
        first = first or cs
        got = set()
        for c in cs:
            got |= census(c, g, rb, run_model(c, g, rb))
        if got >= edges(g):
            break
    else:
        cs = first
    return cs


def run_model(case, geom, rb):
    return model(case["input"], geom, rb, len(case["prefix"]), len(case["existing"]), case["limit"], case["cap"])


@functools.lru_cache(maxsize=None)
def reach(geom_name, rb):
    """(cases, models, edges reached) of one geometry and residue."""
    g = GEOMS[geom_name]
    cs = cases(geom_name, rb)
    ms = [run_model(c, g, rb) for c in cs]
    got = set()
    for c, m in zip(cs, ms):
        got |= census(c, g, rb, m)
    return cs, ms, got
