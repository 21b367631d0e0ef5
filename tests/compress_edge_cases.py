"""Compress inputs built for the candidate rules of raw::compress2, and the census that proves, from a trace of
the oracle, that the inputs reach the rule they were built for — job by job, or per stride / per kind of block end (CPU-side; tests/test_compress_edge_cases_cpu.py asserts the census,
tests/compress_edge_check.py and tests/test_gpu_compress_edges.py run the jobs through every compress kernel).

A natural corpus reaches these rules by chance and nothing says whether it did.  Here every class has a builder (seeded, no
randomness beyond the seed) and a census condition over the events of lzfo_compress2_trace: a kernel that differs from the oracle on
one of these inputs differs at the rule the census names.

Two rules for every builder: a planted repeat and its source each follow a short zero run (the match on the run resets the skip step
to 1, mod.rs:174-175, so the first planted position is probed and inserted), and the filler between a source and its copy is one zero
run (one match, no inserts on the way) or text, never long noise (whose stride would jump over the planted bytes).

    1  distance       a copy exactly 65534 / 65535 (legal) and 65536 / 65537 (refused, mod.rs:201) back, probed at every phase of a
                      64 KiB epoch the compact kernel's 16-bit positions + parity bit could confuse, in epochs 1..3; also behind a prefix
    2  empty slot     a never-written slot reads as position 0, a legal source (B8): offset == the probe position
    3  stale slot     a carried table whose slot is older than `offset` (saturating_sub gives 0): the same, across two calls
    4  first position the probe at the initial cursor never matches (B7), behind a prefix and with a carried table
    5  backtrack      stops at literal_start, at candidate 0 (incl. the byte in front of the input: poison under the red-zone harness)
    6  skip schedule  a six-byte plant at every position of a noise block: found or jumped over, per stride (B2)
    7  LSIC tails     15, 255 and 4 x 255 boundaries in match length, literal length between matches and final literals
    8  block end      the len - 5 / len - 12 rules and the 0-hash of a short read (B3) at lengths around 64 KiB and 128 KiB
    9  U16            every input of up to 65535 bytes again with the 16-bit table, and an offset beyond 65500 there

A job is dict(cls, name, input, cursor, kind, cap, chain, offset_add, par): `cap` None is the worst-case bound; jobs that share a
`chain` are the calls of one carried table in order, `offset_add` going to EncoderTable::offset before the call (mod.rs:72-74).
"""
import functools

import numpy as np

import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import synth

Z = bytes(24)
E = (14, 15, 16, 269, 270, 271, 524, 525, 526, 1034, 1035, 1036, 1289, 1290, 1291)
PHASES = (0, 1, 2, 15, 16, 17, 63, 64, 65, 32768, 65519, 65520, 65534, 65535)
DISTANCES = (65534, 65535, 65536, 65537)
CLASSES = ("distance", "empty slot", "stale slot", "first position", "backtrack", "skip schedule", "lsic", "block end", "u16")


def noise(seed, n):
    """n seeded bytes, none of them zero (a zero run in a builder ends where the builder says)."""
    return np.random.default_rng(seed).integers(1, 256, n, dtype=np.uint8).tobytes()


def bound(n):
    return n + n // 255 + 64


def job(cls, name, data, cursor=0, kind=o.TABLE_U32, cap=None, chain=None, offset_add=0, **par):
    return dict(cls=cls, name=name, input=bytes(data), cursor=cursor, kind=kind, cap=cap, chain=chain, offset_add=offset_add, par=par)


# ------------------------------------------------------------------------------------------------------------------------ the oracle
def run_oracle(jobs, trace=True):
    """Every job through the oracle, chains on one table in order.  Returns one dict(rc, out, events, table) per job; `table` is the
    table's bytes after the call (dict + offset), `events` None without trace."""
    tables, res = {}, []
    for j in jobs:
        if j["chain"] is None:
            t = o.new_table(j["kind"])
        else:
            t = tables.setdefault(j["chain"], o.new_table(j["kind"]))
        t.offset += j["offset_add"]
        if trace:
            rc, out, ev = o.compress2_trace(j["input"], cursor=j["cursor"], kind=j["kind"], table=t, cap=j["cap"])
        else:
            (rc, out), ev = o.compress2(j["input"], cursor=j["cursor"], kind=j["kind"], table=t, cap=j["cap"]), None
        res.append(dict(rc=rc, out=out, events=ev, table=bytes(t)))
    return res


def sequences(j, events):
    """The parse as the trace gives it: ([(literal_len, offset, match_len)], final literal run)."""
    seqs, end = [], j["cursor"]
    for e in dicts(events):
        if e["type"] != o.EV_MATCH:
            continue
        seqs.append((e["pos"] - e["backtrack"] - e["literal_start"], e["pos"] - e["candidate"], e["matching_bytes"] + e["backtrack"]))
        end = e["pos"] + e["matching_bytes"]
    return seqs, max(len(j["input"]) - end, 0)


def schedule(literal_start, end):
    """The probes of mod.rs:174-231 from literal_start while nothing matches: [(position, stride in force at that probe)]."""
    out, cursor, step, counter = [], literal_start, 1, 1 << 6
    while cursor < end:
        out.append((cursor, step))
        cursor += step
        step = counter >> 6
        if literal_start + 1 != cursor:
            counter += 1
    return out


def dicts(ev):
    """Trace events (the record array of oracle_ffi.compress2_trace) as a list of dicts."""
    return ev if isinstance(ev, list) else o.events_as_dicts(ev)


def _matches(r):
    return [e for e in dicts(r["events"]) if e["type"] == o.EV_MATCH]


def _second_run_from_position_0(j, e):
    """A match probed behind the first byte of the second zero run of zeros(40) + noise(l) + zeros(40) whose backtrack, one byte or
    more, ends because the source has reached position 0."""
    return e["pos"] > 40 + j["par"]["l"] and e["flags"] & o.STOP_CANDIDATE_ZERO and e["backtrack"] >= 1 and e["candidate"] == e["backtrack"]


def _tuned(build, want, lo, hi):
    """The first build(x), x in lo..hi, whose traced oracle run satisfies want(job, result) — lengths that depend on where the skip
    schedule lands are found by asking the oracle, not by restating the schedule."""
    for x in range(lo, hi + 1):
        j = build(x)
        if want(j, run_oracle([j])[0]):
            return j
    raise AssertionError("no parameter in %d..%d meets the condition" % (lo, hi))


# ---------------------------------------------------------------------------------------------------------------------------------- 1
def distance():
    text = synth.gen_text_zipf(61, 4 * 65536).tobytes()
    P, tail = noise(101, 24), text[1000:1100]
    jobs = []
    for cursor, phases in ((0, PHASES), (1, (0, 1, 65535)), (4096, (0, 1, 65535))):
        for e in (1, 2, 3):
            for ph in phases:
                for D in DISTANCES:
                    c = e * 65536 + ph
                    if c - D < cursor:                 # (c < D: no room for the source; a lead shorter than the prefix: source not inserted)
                        continue
                    # the lead is text, which is probed at most positions but not at all: where the parse strides over the first byte of
                    # the source, the text starts a few bytes later
                    jobs.append(_tuned(lambda x: job("distance", f"e{e} ph{ph} D{D} cursor{cursor}", text[x:x + c - D] + P + bytes(D - 24) + P + tail,
                                                     cursor=cursor, e=e, ph=ph, D=D, c=c),
                                       lambda j, r: any(e["pos"] == c and e["candidate"] == c - D for e in dicts(r["events"][r["events"]["pos"] == c])), 0, 40))
    return jobs


# ---------------------------------------------------------------------------------------------------------------------------------- 2
def empty_slot():
    Q = noise(102, 32)
    jobs = []
    for cursor in (40, 100):
        for X in (200, 65535, 65536):
            d = Q + noise(103, 8) + bytes(X - 40) + Q + noise(104, 40)
            jobs.append(job("empty slot", f"X{X} cursor{cursor}", d, cursor=cursor, X=X))
    return jobs


# ---------------------------------------------------------------------------------------------------------------------------------- 3
def stale_slot():
    Q = noise(105, 52)
    b1 = noise(106, 76) + Z + Q
    b1 += noise(107, 3980 - len(b1)) + Q
    b1 += noise(108, 5000 - len(b1))
    jobs = []
    for v in (0, 1, 2):
        ch = f"stale v{v}"
        jobs.append(job("stale slot", ch + " call 1", b1, chain=ch, v=v, call=1))
        d = b1[4000:] + noise(109, 30 + v) + Z + Q[20:52] + noise(110, 50)
        jobs.append(job("stale slot", ch + " call 2", d, cursor=1000, chain=ch, offset_add=4000, v=v, call=2))
    return jobs


# ---------------------------------------------------------------------------------------------------------------------------------- 4
def first_position():
    jobs = []
    for cursor in (32, 4096):
        head = noise(111, 32)
        d = head + noise(112, cursor - 32) + head + noise(113, 60)
        jobs.append(job("first position", f"prefix cursor{cursor}", d, cursor=cursor, how="prefix"))
    Q = noise(114, 32)
    for lead in (300, 1000):
        ch = f"first lead{lead}"
        a = noise(115, lead) + Z + Q + noise(116, 40) + Z
        jobs.append(job("first position", ch + " call 1", a, chain=ch, how="carried", call=1))
        jobs.append(job("first position", ch + " call 2", a + Q + noise(117, 60), cursor=len(a), chain=ch, how="carried", call=2))
    return jobs


# ---------------------------------------------------------------------------------------------------------------------------------- 5
def backtrack():
    jobs = []
    for s in range(4):
        W, Q, x = noise(120 + s, 16), noise(130 + s, 16), bytes([0x40 + s])
        d = W + x + b"\x01" + noise(140 + s, 30) + x + Q + noise(150 + s, 30) + W + x + Q + noise(160 + s, 20)
        jobs.append(job("backtrack", f"literal_start s{s}", d, stop="literal_start"))
    # The second zero run is matched from its second byte where the stride carries the probe past its first one: the candidate is
    # position 1, one step back reaches position 0 and the backtrack ends there although the byte in front of the probe is a zero too.
    # While the stride is 1 (the first 64 probes of the noise) the run is entered at its first byte, so l starts beyond that; of every
    # six consecutive lengths the oracle picks the first that enters behind the first byte.
    for l in range(64, 400, 6):
        jobs.append(_tuned(lambda x: job("backtrack", f"candidate 0, zeros l{x}", bytes(40) + noise(170, x) + bytes(40) + noise(171, 20), stop="candidate 0", l=x),
                           lambda j, r: any(_second_run_from_position_0(j, e) for e in _matches(r)), l, l + 5))
    Q = noise(172, 32)
    for n in range(130, 401):
        for y in (0x00, 0xFF, 0xA5):
            d = Q + noise(173, n) + bytes([y]) + Q + noise(174, 20)
            j = job("backtrack", f"over-read n{n} y{y:02x}", d, stop="over-read", n=n, y=y, q2=32 + n + 1)
            # kept where the probe lands behind the start of the second Q (the backtrack then walks to candidate 0, the byte in front
            # of the input being y's twin in a kernel that reads it): the one filter a builder has
            ev = [e for e in _matches(run_oracle([j])[0]) if e["pos"] > j["par"]["q2"] and e["candidate"] == e["backtrack"] > 0]
            if ev:
                jobs.append(j)
    return jobs


# ---------------------------------------------------------------------------------------------------------------------------------- 6
SKIP_SRC = 8
# A six-byte plant has five-byte hashes (mod.rs:41-51 hashes five bytes) at its first two positions, so a stride of 2 always probes one
# of them: at that stride the plant can only be lost to a later insert into the same slot.  With this seed the noise does that (the
# slot of position 8 is taken again before the stride reaches 3); the other strides also jump over the plant.
SKIP_SEED = 202


def skip_schedule():
    r = noise(SKIP_SEED, 4000)
    src = r[SKIP_SRC:SKIP_SRC + 6]
    return [job("skip schedule", f"p{p}", r[:p] + src + r[p + 6:], p=p) for p in range(60, 1401)]


# ---------------------------------------------------------------------------------------------------------------------------------- 7
def lsic():
    jobs = []
    for v in E:
        extra = lambda j, r, v=v: any(s[2] - 4 == v for s in sequences(j, r["events"])[0])
        jobs.append(_tuned(lambda x, v=v: job("lsic", f"match extra {v}, offset 1", noise(190, 10) + bytes(x) + noise(191, 20), field="match run", v=v),
                           extra, v, v + 8))
        far = lambda j, r, v=v: any(s[2] - 4 == v and s[1] > s[2] for s in sequences(j, r["events"])[0])
        for mid in (7, 8, 9, 10):                     # (the stride over the source decides where the second zero run is entered: two lengths to tune)
            try:
                jobs.append(_tuned(lambda x, v=v, mid=mid: job("lsic", f"match extra {v}, far source", Z + noise(192, x) + noise(193, mid) + b"\x01" + Z +
                                                               noise(192, x) + noise(194, 20), field="match far", v=v), far, max(v - 24, 1), v + 8))
                break
            except AssertionError:
                assert mid < 10, f"match extra {v}, far source: no lengths found"
        lits = lambda j, r, v=v: any(s[0] == v for s in sequences(j, r["events"])[0][1:])
        try:                                          # (the run comes out as long as the noise or one longer: the second zero run is entered at its first, second or third byte)
            jobs.append(_tuned(lambda x, v=v: job("lsic", f"literals {v}", bytes(40) + noise(195, x) + bytes(40) + noise(196, 20), field="literals", v=v),
                               lits, max(v - 8, 1), v))
        except AssertionError:                        # a length the stride leaves out: a repeat whose backtrack reaches its first byte instead
            A = noise(189, 16)
            jobs.append(_tuned(lambda x, v=v: job("lsic", f"literals {v}", Z + b"\x02" + A + noise(195, x) + A + noise(196, 20), field="literals", v=v),
                               lits, max(v - 24, 1), v))
        jobs.append(_tuned(lambda x, v=v: job("lsic", f"final literals {v}", noise(197, x), field="final", v=v),
                           lambda j, r, v=v: sequences(j, r["events"]) == ([], v), v, v))
    return jobs


# ---------------------------------------------------------------------------------------------------------------------------------- 8
def block_end():
    t = synth.gen_text_zipf(62, 3000).tobytes() * 50
    jobs = []
    for k in (1, 2):
        for r in range(-13, 21):
            n = k * 65536 + r
            for what, d in (("text", t[:n]), ("zeros", bytes(n))):
                jobs.append(job("block end", f"{what} n{n}", d, n=n, what=what))
                if k == 2:
                    jobs.append(job("block end", f"{what} n{n} cursor65536", d, cursor=65536, n=n, what=what))
                if n <= 65535:
                    jobs.append(job("block end", f"{what} n{n} u16", d, kind=o.TABLE_U16, n=n, what=what))
            # the period-3000 text and the zeros are one match up to len - 5 whatever n is; the other two ends of a block need the last
            # match cut short: at len - 11 (11 bytes are left: no probe, :178-190) and at len - 12 (one last probe, which matches)
            A = noise(210, 7)
            jobs.append(job("block end", f"text n{n}, match to len - 11", t[:n - 11] + noise(200, 11), n=n, what="final 11"))
            jobs.append(job("block end", f"text n{n}, match at len - 12", t[:n - 72] + Z + A + noise(211, 9) + bytes(20) + A + noise(212, 5), n=n, what="probe len - 12"))
            if k == 1:
                jobs.append(job("block end", f"zeros n{n}, match to len - 11", bytes(n - 11) + noise(220, 11), n=n, what="final 11"))
    return jobs


# ---------------------------------------------------------------------------------------------------------------------------------- 9
def u16(others):
    jobs = [job("u16", j["name"] + " (" + j["cls"] + ") u16", j["input"], cursor=j["cursor"], kind=o.TABLE_U16, of=j["cls"])
            for j in others if len(j["input"]) <= 65535 and j["kind"] == o.TABLE_U32 and j["chain"] is None]
    P = noise(198, 24)
    d = b"\x07" + P + bytes(65535 - 1 - 24 - 32) + P + noise(199, 8)
    assert len(d) == 65535
    jobs.append(job("u16", "last match from position 1", d, kind=o.TABLE_U16, of=None))
    return jobs


@functools.lru_cache(maxsize=None)
def corpus():
    jobs = distance() + empty_slot() + stale_slot() + first_position() + backtrack() + skip_schedule() + lsic() + block_end()
    return tuple(jobs + u16(jobs))


def of_class(jobs, *cls):
    return [j for j in jobs if j["cls"] in cls]


@functools.lru_cache(maxsize=None)
def traced():
    """run_oracle(corpus()), once per process and shared: nobody changes it."""
    return tuple(run_oracle(corpus()))


# ------------------------------------------------------------------------------------------------------------------------- the census
def census(jobs, results=None):
    """Per class: counts (what the trace shows, for the record) and `missing`, one line per census condition that some input does
    not meet.  An empty `missing` everywhere is the proof that the corpus reaches every rule in the reference."""
    results = results if results is not None else run_oracle(jobs)
    out = {c: dict(jobs=0, bytes=0, matches=0, refused=0, short_inserts=0, counts={}, missing=[]) for c in CLASSES}

    def count(c, key, n=1):
        out[c]["counts"][key] = out[c]["counts"].get(key, 0) + n

    for j, r in zip(jobs, results):
        c = out[j["cls"]]
        c["jobs"] += 1; c["bytes"] += len(j["input"])
        for key, ty in (("matches", o.EV_MATCH), ("refused", o.EV_REFUSED), ("short_inserts", o.EV_SHORT_INSERT)):
            c[key] += int((r["events"]["type"] == ty).sum())

    lsic_seen = {f: set() for f in ("match run", "match far", "literals", "final")}
    skip = {}
    end = dict(match_to_len_minus_5=0, final_5=0, final_11=0, probe_at_len_minus_12=0, short_insert=0)
    overread = 0
    for j, r in zip(jobs, results):
        cls, par, ev, d = j["cls"], j["par"], r["events"], j["input"]
        if cls == "distance":                                             # (thousands of text matches per job: only the far ones and the plant matter)
            ev = ev[(ev["pos"] >= par["c"]) | (ev["pos"] - ev["candidate"] >= 65534)]
        ev = dicts(ev)
        m = [e for e in ev if e["type"] == o.EV_MATCH]
        ref = [e for e in ev if e["type"] == o.EV_REFUSED]
        miss = out[cls]["missing"].append
        seqs, final = sequences(j, ev)
        if cls == "distance":
            c, D = par["c"], par["D"]
            if D <= 65535:
                ok = any(e["pos"] == c and e["pos"] - e["candidate"] == D and e["matching_bytes"] + e["backtrack"] == 24 for e in m)
                count(cls, "matched at offset %d" % D, ok)
                if not ok:
                    miss(f"{j['name']}: no match of 24 bytes at offset {D} probed at {c}")
            else:
                ok = any(e["pos"] == c and e["flags"] & o.REFUSED_DISTANCE and e["candidate"] == c - D for e in ref)
                far = [s for s in seqs if s[1] >= 65534]
                count(cls, "refused at distance %d" % D, ok and not far)
                if not ok or far:
                    miss(f"{j['name']}: no distance refusal at {c} of candidate {c - D}" if not ok else f"{j['name']}: a match at offset {far[0][1]}")
        elif cls == "empty slot":
            X = par["X"]
            if X <= 65535:
                ok = any(e["candidate"] == 0 and e["raw_slot"] == 0 and e["pos"] - e["candidate"] == e["pos"] == X for e in m)
                count(cls, "matched position 0 from an empty slot", ok)
            else:
                ok = any(e["pos"] == X and e["candidate"] == 0 and e["raw_slot"] == 0 and e["flags"] & o.REFUSED_DISTANCE for e in ref)
                count(cls, "position 0 refused at distance 65536", ok)
            if not ok:
                miss(f"{j['name']}: position 0 from an empty slot not {'matched' if X <= 65535 else 'refused by distance'} at {X}")
        elif cls == "stale slot" and par["call"] == 2:
            want = 1054 + par["v"]
            ok = any(0 < e["raw_slot"] < e["table_offset"] and e["candidate"] == 0 and e["pos"] == want for e in m) and (0, want, 32) in seqs
            count(cls, "matched position 0 from a slot older than offset", ok)
            if not ok:
                miss(f"{j['name']}: no match (0, {want}, 32) from a stale slot")
        elif cls == "first position" and par.get("call", 2) == 2:
            ok = any(e["pos"] == j["cursor"] and e["flags"] & o.REFUSED_FIRST_POSITION and e["matching_bytes"] >= 32 for e in ref)
            count(cls, "refused at init_cursor (%s)" % par["how"], ok)
            if not ok:
                miss(f"{j['name']}: no first-position refusal at {j['cursor']}")
        elif cls == "backtrack":
            if par["stop"] == "literal_start":
                ok = any(e["flags"] & o.STOP_LITERAL_START and e["pos"] - e["backtrack"] == e["literal_start"] and e["candidate"] > e["backtrack"] and
                         d[e["pos"] - e["backtrack"] - 1] == d[e["candidate"] - e["backtrack"] - 1] for e in m[1:])
                count(cls, "stopped at literal_start with an equal byte in front", ok)
                if not ok:
                    miss(f"{j['name']}: no zero-literal match whose backtrack literal_start alone stopped")
            elif par["stop"] == "candidate 0":
                ok = any(_second_run_from_position_0(j, e) for e in m)
                count(cls, "stopped at candidate 0, backtrack >= 1 (second zero run)", ok)
                if not ok:
                    miss(f"{j['name']}: the second zero run is not matched from behind its first byte with a backtrack that ends at candidate 0")
            else:
                ok = any(e["pos"] > par["q2"] and e["flags"] & o.STOP_CANDIDATE_ZERO and e["backtrack"] >= 1 for e in m)
                count(cls, "stopped at candidate 0, backtrack >= 1 (over-read)", ok)
                overread += ok
                if not ok:
                    miss(f"{j['name']}: kept although the backtrack does not end at candidate 0")
        elif cls == "skip schedule":
            p = par["p"]
            hit = [e for e in m if e["pos"] in (p, p + 1) and e["candidate"] == SKIP_SRC + e["pos"] - p]
            # A job without a hit leaves no event near the plant, so its stride comes from schedule(), the restated probe sequence: the
            # one in force at the probe nearest the plant.  The restatement is held to the trace wherever the trace speaks: every hit
            # must be a probe of schedule() with the stride the event records.
            if hit:
                skip.setdefault(hit[0]["step"], [0, 0, 0, 0])[0] += 1
                if m[0] is hit[0] and (hit[0]["pos"], hit[0]["step"]) not in schedule(0, p + 2):
                    miss(f"{j['name']}: the hit at {hit[0]['pos']} (stride {hit[0]['step']}) is no probe of the restated schedule")
            elif not m:
                q, step = schedule(0, p + 2)[-1]
                skip.setdefault(step, [0, 0, 0, 0])[1 if q < p else 2] += 1
            else:                                                         # (a chance match elsewhere resets the stride: in no column)
                skip.setdefault(0, [0, 0, 0, 0])[3] += 1
        elif cls == "lsic":
            got = {"match run": [s[2] - 4 for s in seqs if s[1] == 1], "match far": [s[2] - 4 for s in seqs if s[1] > s[2]],
                   "literals": [s[0] for s in seqs[1:]], "final": [final]}[par["field"]]
            if par["v"] in got:
                lsic_seen[par["field"]].add(par["v"])
        elif cls == "block end":
            n = len(d)
            end["match_to_len_minus_5"] += any(e["pos"] + e["matching_bytes"] == n - 5 for e in m)
            end["final_5"] += final == 5 and bool(m)
            end["final_11"] += final == 11 and bool(m)
            end["probe_at_len_minus_12"] += any(e["pos"] == n - 12 for e in m)
            end["short_insert"] += sum(e["type"] == o.EV_SHORT_INSERT for e in ev)
            if par["what"] == "final 11" and not (final == 11 and m):
                miss(f"{j['name']}: final literal run of {final}")
            if par["what"] == "probe len - 12" and not any(e["pos"] == n - 12 and e["literal_start"] == n - 12 for e in m):
                miss(f"{j['name']}: no match probed at len - 12")
        elif cls == "u16" and par["of"] is None:
            ok = bool(seqs) and seqs[-1][1] >= 65500 and m[-1]["candidate"] - m[-1]["backtrack"] == 1
            count(cls, "offset >= 65500 from a source at position 1", ok)
            if not ok:
                miss(f"{j['name']}: last match {seqs[-1:] or None}")

    if out["backtrack"]["jobs"]:
        out["backtrack"]["counts"]["over-read variants kept"] = overread
        if overread < 8:
            out["backtrack"]["missing"].append(f"over-read: {overread} variants kept, 8 wanted")
    if out["skip schedule"]["jobs"]:
        for step in range(2, 7):
            hit, jumped, lost, _ = skip.get(step, [0, 0, 0, 0])
            out["skip schedule"]["counts"]["stride %d: matched (stride from the trace) / jumped over / probed, slot overwritten (stride from the "
                                           "restated schedule)" % step] = (hit, jumped, lost)
            if not hit:
                out["skip schedule"]["missing"].append(f"stride {step}: the plant is never matched")
            if not jumped + lost:
                out["skip schedule"]["missing"].append(f"stride {step}: the plant is never refused")
        out["skip schedule"]["counts"]["jobs with another match and no hit, in no column"] = sum(v[3] for v in skip.values())
        out["skip schedule"]["counts"]["jobs matched at other strides (1, 7)"] = sum(v[0] for k, v in skip.items() if not 2 <= k <= 6)
    if out["lsic"]["jobs"]:
        for f, seen in lsic_seen.items():
            out["lsic"]["counts"][f] = len(seen)
            for v in E:
                if v not in seen:
                    out["lsic"]["missing"].append(f"{f}: {v} does not occur")
    if out["block end"]["jobs"]:
        out["block end"]["counts"].update(end)
        for k, v in end.items():
            if not v:
                out["block end"]["missing"].append(k)
    return out


def report(cen):
    lines = []
    for c in CLASSES:
        v = cen[c]
        lines.append(f"{c:15s} jobs {v['jobs']:5d}  bytes {v['bytes']:9d}  match events {v['matches']:7d}  refused-probe events {v['refused']:6d}  "
                     f"short-read inserts (B3, U32) {v['short_inserts']:5d}  missing {len(v['missing'])}")
        for k, n in v["counts"].items():
            lines.append(f"    {k}: {n}")
    return "\n".join(lines)

