"""The launch-order stage — what decides which job of a large call runs first — as host models, built cases and a census.  Plain Python and
numpy: no GPU, no library.  The stage is seven kernels and one accumulation of the parse kernel (aux_kernels.hip, lz4_seg_front.hip,
the dry run of lz4_compress_compact.hip); the models restate each from the source:

  cost_est        lzf_decompress_cost_kernel: tokens sampled in three windows, scaled to the input, plus the bytes' share (integer-exact);
  fed_est         the plan stage's and the parse's est[] of a fed call: the marks every chunk owns plus the bytes' share (integer-exact), and
                  for which jobs that is the block's true sequence count;
  probe_jobs      lzf_cost_probe_jobs_kernel, field by field;
  cost_estimates  the float32 estimate lzf_order_by_cost_kernel sorts by;
  order_fault     the contract of the 1024-class counting sort all three ordering kernels share (order_ok = no fault).

tests/test_launch_order_cases_cpu.py proves that every case reaches the edge it is named for (census()); tests/test_gpu_launch_order.py
compares the device's dumps (lzf_debug_order, analysis library) with the models."""
import functools

import numpy as np

import seg_stage_cases as S
from seg_stage_cases import Blk, Parse, _block, _seq, _walk, host_parse  # noqa: F401

CHUNK, OVERLAP, STRIDE = S.CHUNK, S.OVERLAP, S.STRIDE
SEG_MAX_IN = 4 * 1024 * 1024 + 32 * 1024                   # kSegMaxIn (lzf_dispatch.h): the largest input the map covers
K_SKIP, K_COUNT, K_PAD = 1024, 4096, 32                    # lzf_decompress_cost_kernel: bytes to fall in step, bytes counted, bytes staged behind
K_W = K_SKIP + K_COUNT                                     # a token that starts below this is walked
WIN = K_W + K_PAD                                          # 5 152 bytes of a window are staged
SAMPLED_FROM = 3 * WIN                                     # 15 456: shorter inputs get a guess
CLASSES = 1024                                             # order_longest_first
TABLE_U32 = 0                                              # LZF_TABLE_U32 (lzfear_hip.h)
U32, U64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
LEN_SHIFTS = (2, 0, 31, 32)
RESIDUES = (0, 1, 15)
PROBES = ((65536, 1), (16384, 3), (4096, 16))              # (piece, parts)
CJOB = np.dtype([("input", "<u8"), ("input_len", "<u8"), ("cursor", "<u8"), ("out", "<u8"), ("out_cap", "<u8"), ("table", "<u8"),
                 ("table_kind", "<u4"), ("flags", "<u4")])                               # lzf_compress_job


# ------------------------------------------------------------------------------------------------ the model: lzf_decompress_cost_kernel
def window_walk(b, start):
    """The walk of aux_kernels.hip:254-268 over one staged window b (WIN bytes); tokens count from relative position `start` on.
    Returns (cnt, span, flags): flags names what the walk met."""
    assert len(b) == WIN
    flags = set()
    rd = lambda q: b[q] if q < WIN else 0                  # noqa: E731  (both length extensions read 0 behind the staged bytes)
    p, first, cnt = 0, None, 0
    while p < K_W:
        if p >= start:
            if first is None:
                first = p
            cnt += 1
        tok = b[p]
        q, L = p + 1, tok >> 4
        if L == 15:
            while True:
                x = rd(q); q += 1; L += x
                if not (x == 255 and q < WIN):
                    break
            if x == 255:
                flags.add("literal-length run of 0xFF over the window's end")
        q += L + 2
        if (tok & 15) == 15:
            while True:
                x = rd(q); q += 1
                if not (x == 255 and q < WIN):
                    break
            if x == 255:
                flags.add("match-length run of 0xFF over the window's end")
        assert q > p and q <= U32                          # (the kernel's `q <= p` is a 32-bit wrap: no window gets there)
        p = q
    if first is None:
        return 0, 0, flags | {"never reaches its first counted byte"}
    if p > WIN:
        flags.add("span clamped")
    return cnt, min(p, WIN) - first, flags


def cost_windows(inp, length=None):
    """(third, [(cnt, span, flags)] of the three windows) of a sampled input, None for one that gets the guess."""
    n = min(len(inp) if length is None else length, 0x7FFFFFFF)
    if inp is None or n < SAMPLED_FROM:
        return None
    third = (n - WIN) // 3
    return third, [window_walk(inp[w * third:w * third + WIN], K_SKIP if w else 0) for w in range(3)]


def cost_est(inp, len_shift, length=None):
    """est[j] of lzf_decompress_cost_kernel.  inp None: a null input of `length` bytes."""
    n = min(len(inp) if length is None else length, 0x7FFFFFFF)
    cw = None if inp is None else cost_windows(inp, n)
    if cw is None:
        return n >> 4                                       # the short path: no byte share
    cnt, span = sum(w[0] for w in cw[1]), sum(w[1] for w in cw[1])
    share = n >> len_shift if len_shift < 32 else 0
    return ((((n * cnt) // span) & U32 if span else n >> 4) + share) & U32


# ------------------------------------------------------------------------------------------------------- the model: the fed estimate
def chunk_marks(P, h):
    """bool[CHUNK]: the tokens of the chain that starts at chunk h's first byte, inside the chunk and the input (lzf_seg_parse_kernel)."""
    cs = h * STRIDE
    lim = min(cs + CHUNK, P.n)
    m = np.zeros(CHUNK, bool)
    p = cs
    while p < lim:
        m[p - cs] = True
        p = P.token(p)[4]
    return m


def fed_eligible(job, min_in):
    """lzf_seg_plan_kernel (lz4_seg_front.hip:34-43) with fed = 1: prefix and existing output do not matter; the map's window, an input and an output do."""
    n = job["input_len"]
    return min_in <= n <= SEG_MAX_IN and job["input"] is not None and not job.get("null_out", False)


@functools.lru_cache(maxsize=None)
def _owned_marks(c):
    """(marks the chunks of input c own, all together; the block's sequence count where every chunk is in step by OVERLAP, else None)"""
    P = Parse(c)
    n = P.n
    truth = np.zeros(n, bool)
    toks, err = P.chain(0)
    truth[[t[0] for t in toks]] = True
    cnt, in_step = 0, not err
    for h in range(S.seg_nch(n)):
        cs = h * STRIDE
        own = 0 if h == 0 else OVERLAP                     # chunk 0 its whole row, chunk h >= 1 from OVERLAP on
        hi = min(CHUNK, n - cs)
        if hi <= own:
            continue
        m = chunk_marks(P, h)
        cnt += int(m[own:hi].sum())
        in_step = in_step and bool((m[own:hi] == truth[cs + own:cs + hi]).all())
    return cnt, (len(toks) if in_step else None)


def fed_est(job, min_in, len_shift):
    """(est, sequences): est[j] as the plan stage and the parse leave it; sequences = the block's true sequence count where the estimate
    holds it exactly (every chunk's chain in step with the block's chain by OVERLAP), None elsewhere."""
    n = job["input_len"]
    l31 = min(n, 0x7FFFFFFF)
    share = l31 >> len_shift if len_shift < 32 else 0
    if not fed_eligible(job, min_in):
        return (l31 >> 4) + share, None                     # a guess by length, and the bytes' share on top of it
    assert len(job["input"]) == n
    cnt, seqs = _owned_marks(job["input"])
    return (cnt + share) & U32, seqs


# ------------------------------------------------------------------------------------------------------ the model: the compress probes
def cost_payload(j):
    return j["input_len"] - j["cursor"] if j["cursor"] < j["input_len"] else 0


def cost_sample_len(payload, piece, parts):
    return (piece * parts) & U32 if payload >= 4 * piece * parts else 0


def probe_offset(payload, piece, parts, k):
    """Where piece k of a probed payload starts, relative to the payload."""
    return ((payload - piece) * (2 * k + 1) // (2 * parts)) & ~15


def probe_jobs(jobs, piece, parts):
    """lzf_cost_probe_jobs_kernel (aux_kernels.hip:172-187): probe i = piece (i % parts) of job (i // parts), as a CJOB array."""
    out = np.zeros(len(jobs) * parts, CJOB)
    for i in range(len(out)):
        j = jobs[i // parts]
        payload = cost_payload(j)
        sl = cost_sample_len(payload, piece, parts)
        out[i] = ((j["input"] + j["cursor"] + (probe_offset(payload, piece, parts, i % parts) if sl else 0)) & U64, piece if sl else 0, 0, 0, U64, 0,
                  TABLE_U32, 0)
    return out


def cost_estimates(jobs, reserved, piece, parts):
    """float32[n]: what lzf_order_by_cost_kernel sorts by.  reserved: uint32[n * parts], the probes' work."""
    f = np.float32
    est = np.zeros(len(jobs), np.float32)
    for i, j in enumerate(jobs):
        payload = cost_payload(j)
        sl = cost_sample_len(payload, piece, parts)
        if not sl:
            est[i] = f(payload) * f(0.1)
        else:
            kc = int(np.asarray(reserved[i * parts:(i + 1) * parts], np.uint64).sum()) & U32
            est[i] = f(kc) * (f(payload) / f(sl))
    return est


# ------------------------------------------------------------------------------------------------ the model: the 1024-class counting sort
def order_fault(est, perm, classes=CLASSES):
    """None when perm is an order the counting sort may give for est, else what is wrong with it.  Two rules: perm is a permutation of
    0..n-1; with top = max(est) and w = top / (classes - 1) * (1 + 1e-3) no job stands in front of a job whose estimate is larger by more
    than w.  (Jobs of one class differ by less than top / (classes - 1) and the classes are ordered strictly; the 1e-3 covers the float32
    rounding of the estimates and of their product with scale, about 1e-4 of a class.  Inside a class the order is free: the sort places
    jobs with atomicAdd.)  All estimates 0: only the permutation is required."""
    e = np.asarray(est, np.float64)
    perm = np.asarray(perm, np.int64)
    n = len(e)
    if len(perm) != n:
        return f"perm has {len(perm)} entries for {n} jobs"
    if n == 0:
        return None
    if perm.min() < 0 or perm.max() >= n or len(np.unique(perm)) != n:
        return "perm is not a permutation of 0..n-1"
    top = float(e.max())
    if top == 0.0:
        return None
    w = top / (classes - 1) * (1 + 1e-3)
    ep = e[perm]
    behind = np.maximum.accumulate(ep[::-1])[::-1]         # behind[k] = max(ep[k:])
    bad = np.nonzero(ep[:-1] < behind[1:] - w)[0]
    if len(bad):
        k = int(bad[0])
        return f"rank {k} (job {int(perm[k])}, estimate {ep[k]:.9g}) stands in front of an estimate of {behind[k + 1]:.9g}: more than w = {w:.6g} larger"
    return None


def order_ok(est, perm, classes=CLASSES):
    return order_fault(est, perm, classes) is None


def class_of(est, classes=CLASSES):
    """The class order_longest_first puts every estimate in (float32 arithmetic; 0 = the longest jobs)."""
    e = np.asarray(est, np.float32)
    top = e.max() if len(e) else np.float32(0)
    scale = np.float32(classes - 1) / top if top > 0 else np.float32(0)
    c = np.minimum((e * scale).astype(np.float64), classes - 1).astype(np.int64)
    return (classes - 1) - c


def model_sort(est, classes=CLASSES, ascending=False, rng=None):
    """An order the counting sort may give: by class, inside a class as the atomics fall (rng: shuffled)."""
    c = class_of(est, classes)
    key = -c if ascending else c
    tie = rng.permutation(len(c)) if rng is not None else np.arange(len(c))
    return np.lexsort((tie, key))


# ------------------------------------------------------------------------------------------------------------------ cases: the sorts
SORT_SIZES = (1, 2, 63, 1023, 1024, 1025, 2048, 2049, 4097)      # the 1024-thread stride loop: below, at, one over, two rounds, four rounds + 1
SORT_KINDS = ("all zero", "all equal", "distinct 0..n-1", "around 2^24 and up to 2^32-1", "powers of two", "one outlier")


def sort_estimates(kind, n):
    """uint32[n] for a sort case."""
    rng = np.random.default_rng(n * 131 + SORT_KINDS.index(kind))
    if kind == "all zero":
        return np.zeros(n, np.uint32)
    if kind == "all equal":
        return np.full(n, 123457, np.uint32)
    if kind == "distinct 0..n-1":
        return rng.permutation(n).astype(np.uint32)
    if kind == "around 2^24 and up to 2^32-1":
        v = np.where(rng.random(n) < 0.5, (1 << 24) + rng.integers(-300, 300, n), rng.integers(1 << 24, 1 << 32, n)).astype(np.uint32)
        v[0] = U32
        if n > 1:
            v[n - 1] = (1 << 24) + 1                        # (the first integer a float32 cannot hold)
        return v
    if kind == "powers of two":
        return (np.uint64(1) << rng.integers(0, 32, n).astype(np.uint64)).astype(np.uint32)
    if kind == "one outlier":
        v = rng.integers(0, 1000, n).astype(np.uint32)
        v[n // 2] = 4_000_000_000
        return v
    raise KeyError(kind)


def input_len_edges(n):
    """uint64[n] for the sort by input length: lengths of 0 and of 2^31 among ordinary ones."""
    rng = np.random.default_rng(n)
    v = rng.integers(0, 1 << 22, n).astype(np.uint64)
    v[::5] = 0
    v[n // 3] = 1 << 31
    if n > 2:
        v[n // 2] = (1 << 31) - 1
    return v


COST_PIECE = 4096                                          # the sort by cost: every probed job has a payload of 4 pieces


def cost_sort_jobs(est_u32, parts, mixed=True):
    """Compress jobs (pointers null: lzf_order_by_cost_kernel reads lengths and probe results only) and synthetic probe results whose
    model estimates follow est_u32: two jobs of three are probed (their `reserved` values add up to est_u32[i], cursor 0 or in the
    middle), the third is not (its payload is est_u32[i] mod 2^14, below the probed size); mixed = False: every job is probed."""
    n = len(est_u32)
    jobs, reserved = [], np.zeros(n * parts, np.uint32)
    for i, v in enumerate(est_u32.tolist()):
        if mixed and i % 3 == 2:
            jobs.append(dict(input=0, input_len=v % (1 << 14) + 77, cursor=77))
        else:
            cur = 0 if i % 3 == 0 else 4001
            jobs.append(dict(input=0, input_len=4 * COST_PIECE * parts + cur, cursor=cur))
            reserved[i * parts:(i + 1) * parts] = v // parts
            reserved[i * parts] += v % parts
    return jobs, reserved


# -------------------------------------------------------------------------------------------------------- cases: the cost sampling
def _sized(b, n, tail=5):
    """Ends block b at exactly n compressed bytes."""
    b.to_c(n - 1 - tail)
    c, o = b.end(tail)
    assert len(c) == n, (len(c), n)
    return c


def _plain(seed, n, lit=12, mat=12):
    b = Blk(seed)
    b.near(20, 6)
    while b.cpos < n - 600:
        b.near(int(b.rng.integers(0, lit)), 4 + int(b.rng.integers(0, mat)))
    return _sized(b, n)


def on_boundaries(seed, n):
    """A block of n bytes, short sequences throughout, with a token at each window's first byte."""
    third = (n - WIN) // 3
    b = Blk(seed)
    b.near(20, 6)
    for t in (third, 2 * third):
        b.small_until(t - 300).to_c(t)
    b.small_until(n - 600)
    return _sized(b, n)


@functools.lru_cache(maxsize=None)
def cost_cases():
    """[(name, input or None, input_len, edges the case is built for)]"""
    out = []
    add = lambda name, c, reaches=(), length=None: out.append(dict(name=name, input=c, input_len=len(c) if length is None else length, reaches=tuple(reaches)))   # noqa: E731
    add("cost: 15 455 bytes, the longest guess", _plain(1, SAMPLED_FROM - 1), ("guess at 15 455",))
    add("cost: 15 456 bytes, the first sampled length", _plain(2, SAMPLED_FROM), ("sampled at 15 456", "windows overlap"))
    add("cost: null input", None, ("null input",), length=40000)
    add("cost: zero length", b"", ("zero length",))
    # a token at 5 100 of window 0 whose literal length takes 60 bytes of 0xFF: the run crosses byte 5 152
    b = Blk(3); b.near(20, 6); b.small_until(4800).to_c(5100); b.near(15 + 255 * 60 + 7, 4); b.small_until(b.cpos + 9000)
    add("cost: literal-length run of 0xFF over byte 5 152", b.end(5)[0], ("literal-length run of 0xFF over the window's end",))
    b = Blk(4); b.near(20, 6); b.small_until(4800).to_c(5100); b.seq(3, 1, 19 + 255 * 60 + 9); b.small_until(b.cpos + 22000)
    add("cost: match-length run of 0xFF over byte 5 152", b.end(5)[0], ("match-length run of 0xFF over the window's end",))
    b = Blk(5); b.near(20, 6); b.small_until(2800).to_c(3000); b.near(4000, 9); b.small_until(b.cpos + 15000)
    add("cost: literals jump over the rest of window 0", b.end(5)[0], ("span clamped",))
    # windows 1 and 2 start inside a run of random literals: their walks start off the chain
    b = Blk(6); b.near(20, 6); b.small_until(5200); b.near(24000, 8); b.small_until(b.cpos + 6000)
    add("cost: windows start inside literals", b.end(5)[0], ("window starts inside literals",))
    # ... and inside literals of 0xFF: the walk's first token runs over the whole window, lanes 1 and 2 never count
    b = Blk(7); b.near(40000, 8, fill=0xFF); b.small_until(b.cpos + 5000)
    add("cost: lanes 1 and 2 never reach byte 1 024", b.end(5)[0], ("never reaches its first counted byte",))
    for k, n in enumerate((15457, 16384, 20000, 24571, 30001, 32768, 40960, 49999, 65535, 65536)):
        add(f"cost: short sequences, {n} bytes", _plain(10 + k, n, lit=6 + k, mat=6 + 3 * k))
    for k, n in enumerate((18000, 33333, 61000)):
        add(f"cost: tokens on the windows' first bytes, {n} bytes", on_boundaries(30 + k, n), ("windows start on tokens",))
    for k, (lo, hi) in enumerate(((100, 900), (300, 3000), (2000, 6000))):      # literal-heavy: few tokens per window
        b = Blk(40 + k); b.near(20, 6)
        while b.cpos < 30000 + 9000 * k:
            b.near(int(b.rng.integers(lo, hi)), 4 + int(b.rng.integers(0, 300)))
        add(f"cost: literal runs of {lo}..{hi} bytes", b.end(9)[0])
    b = Blk(50); b.near(9, 4)
    while b.cpos < 40000:
        b.near(0, 4 + b.cpos % 3)                          # 3-byte tokens throughout: the most a window holds
    add("cost: 3-byte tokens throughout", b.end(5)[0], ("3-byte tokens throughout",))
    for k in range(4):                                     # mixed: long matches and literal-length bytes of every kind
        b = Blk(60 + k); b.near(20, 6)
        while b.cpos < 20000 + 11000 * k:
            b.near(int(b.rng.choice([0, 3, 14, 15, 16, 269, 270, 271, 700])), int(b.rng.choice([4, 18, 19, 20, 273, 274, 275, 2000])))
        add(f"cost: length bytes of every kind, block {k}", b.end(7)[0])
    assert len({c["name"] for c in out}) == len(out)
    assert all(c["input_len"] <= 65536 for c in out)
    return tuple(out)


def direct_count_est(c, len_shift):
    """cost_est of a block whose windows start on tokens and hold short sequences only, from the block's token list alone."""
    n = len(c)
    third = (n - WIN) // 3
    pos = np.array([t[0] for t in _walk(c)], np.int64)
    cnt = span = 0
    for w in range(3):
        base = w * third
        assert base in pos, "the window does not start on a token"
        rel = pos[pos >= base] - base
        counted = rel[(rel >= (K_SKIP if w else 0)) & (rel < K_W)]
        behind = int(rel[rel >= K_W][0])                    # the first token the walk does not enter
        cnt += len(counted)
        span += min(behind, WIN) - int(counted[0])
    return n * cnt // span + (n >> len_shift if len_shift < 32 else 0)


# --------------------------------------------------------------------------------------------------------- cases: the fed estimate
FED_MIN_IN = 20000                                         # the cases' min_in: some blocks lie below it


@functools.lru_cache(maxsize=None)
def fed_cases():
    """Jobs of a fed call: dict(name, input, input_len, null_out, prefix_len, out_existing_len, reaches)."""
    out = []

    def add(name, c, reaches=(), **kw):
        out.append(dict(dict(name=name, input=c, input_len=len(c), null_out=False, prefix_len=0, out_existing_len=0, reaches=tuple(reaches)), **kw))
    for c in S.seam_cases():
        add("fed " + c["name"], c["input"])
    add("fed: below min_in", _plain(70, FED_MIN_IN - 1), ("below min_in",))
    add("fed: exactly min_in", _plain(71, FED_MIN_IN), ("at min_in",))
    add("fed: null out", _plain(72, 30000), ("null out",), null_out=True)
    add("fed: prefix_len set", _plain(73, 30001), ("prefix_len set",), prefix_len=777)
    add("fed: out_existing_len set", _plain(74, 30002), ("out_existing_len set",), out_existing_len=4096)
    add("fed: exactly CHUNK bytes", _plain(75, CHUNK), ("one chunk, full",))
    add("fed: CHUNK + 1 bytes", _plain(76, CHUNK + 1), ("second chunk owns nothing",))
    add("fed: two bytes into the second chunk's own region", _plain(77, STRIDE + CHUNK + 2), ("ends inside an owned region",))
    add("fed: ends inside the third chunk's own region", _plain(78, 2 * STRIDE + OVERLAP + 5000), ("ends inside an owned region",))
    for c in cost_cases():
        if c["input"] and c["input_len"] >= SAMPLED_FROM and len(out) < 40:
            add("fed " + c["name"], c["input"])
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


# ------------------------------------------------------------------------------------------------------- cases: the compress probes
def probe_cases(piece, parts, data):
    """Compress jobs for one (piece, parts): dict(name, data, cursor, reaches); data(name, n) -> n bytes."""
    T = 4 * piece * parts
    out = []
    add = lambda name, d, cursor, *reaches: out.append(dict(name=f"probe {piece}x{parts}: {name}", data=d, cursor=cursor, reaches=reaches))   # noqa: E731
    add("payload one below the probed size", data("mix", T - 1), 0, "payload 4*piece*parts - 1", "cursor 0")
    add("payload exactly the probed size", data("mix2", T), 0, "payload 4*piece*parts")
    add("cursor in the middle, payload exactly the probed size", data("mix", T + 5003), 5003, "cursor in the middle", "payload 4*piece*parts")
    add("cursor in the middle, payload one below", data("mix2", T + 5003), 5004, "payload 4*piece*parts - 1")
    add("cursor at input_len", data("mix", 70000), 70000, "cursor >= input_len")
    add("cursor behind input_len", data("mix", 70001), 70008, "cursor >= input_len")
    add("text and binary, 700 000 bytes", data("mix3", 700_000), 0)
    add("zeros", data("zeros", T + 12345), 17)
    add("noise", data("noise", T + 4321), 0)
    add("zeros, noise, text", data("zeros", 120_000) + data("noise", 150_000) + data("mix", 200_000), 1)
    assert all(len(c["data"]) <= (1 << 20) for c in out)
    return out


def synthetic_data(name, n):
    """The census' stand-in for the bytes (the probes' geometry depends on lengths alone)."""
    return bytes(n)


# --------------------------------------------------------------------------------------------------------------------- the census
SORT_EDGES = {f"n = {n}" for n in SORT_SIZES} | set(SORT_KINDS) | {
    "float32 rounds an estimate", "estimate 2^32-1", "every class but one empty behind the outlier", "more jobs than classes", "input_len 0", "input_len 2^31",
    "sum of reserved over several parts", "probed and unprobed jobs", "cursor in the middle of a sorted job"}
COST_EDGES = {"guess at 15 455", "sampled at 15 456", "windows overlap", "null input", "zero length", "literal-length run of 0xFF over the window's end",
              "match-length run of 0xFF over the window's end", "span clamped", "window starts inside literals", "never reaches its first counted byte",
              "windows start on tokens", "3-byte tokens throughout", "walk falls in step before byte 1 024", "lanes 1 and 2 with span 0"}
FED_EDGES = {"below min_in", "at min_in", "null out", "prefix_len set", "out_existing_len set", "one chunk, full", "second chunk owns nothing",
             "ends inside an owned region", "in step at every seam", "out of step through a whole chunk", "falls in step inside the overlap",
             "falls in step behind the overlap", "a chunk with no mark of its own", "more than 64 chunks"}
PROBE_EDGES = {"payload 4*piece*parts - 1", "payload 4*piece*parts", "cursor 0", "cursor in the middle", "cursor >= input_len",
               "every probe inside its payload", "every probe 16-byte aligned to the payload", "probes of a job do not overlap"}


def census_sort():
    got = set()
    for n in SORT_SIZES:
        got.add(f"n = {n}")
        if n > CLASSES:
            got.add("more jobs than classes")
        for kind in SORT_KINDS:
            e = sort_estimates(kind, n)
            assert e.dtype == np.uint32 and len(e) == n
            if kind == "all zero" and not e.any():
                got.add(kind)
            if kind == "all equal" and e[0] and (e == e[0]).all():
                got.add(kind)
            if kind == "distinct 0..n-1" and sorted(e.tolist()) == list(range(n)):
                got.add(kind)
            if kind == "around 2^24 and up to 2^32-1":
                got.add(kind)
                if (e.astype(np.float32).astype(np.float64) != e.astype(np.float64)).any():
                    got.add("float32 rounds an estimate")
                if (e == U32).any():
                    got.add("estimate 2^32-1")
            if kind == "powers of two" and ((e & (e - 1)) == 0).all():
                got.add(kind)
            if kind == "one outlier" and n >= 63:
                got.add(kind)
                rest = np.delete(class_of(e), n // 2)
                if len(np.unique(rest)) == 1:
                    got.add("every class but one empty behind the outlier")
            for parts in (1, 3):
                jobs, reserved = cost_sort_jobs(e, parts)
                sl = [cost_sample_len(cost_payload(j), COST_PIECE, parts) for j in jobs]
                if parts > 1 and any(sl) and (reserved.reshape(-1, parts)[:, 1:] > 0).any():
                    got.add("sum of reserved over several parts")
                if any(sl) and not all(sl):
                    got.add("probed and unprobed jobs")
                if any(s and j["cursor"] for s, j in zip(sl, jobs)):
                    got.add("cursor in the middle of a sorted job")
        v = input_len_edges(n)
        if n >= 63 and (v == 0).any():
            got.add("input_len 0")
        if n >= 63 and (v == 1 << 31).any():
            got.add("input_len 2^31")
    return got


def outlier_classes(n=4097):
    """How many classes the jobs behind the outlier fall into (a known coarseness of the design: DESIGN.md)."""
    e = sort_estimates("one outlier", n)
    return len(np.unique(np.delete(class_of(e), n // 2)))


def census_cost():
    got = set()
    for c in cost_cases():
        mine = set()
        n, inp = c["input_len"], c["input"]
        if inp is None:
            mine.add("null input")
        elif n == 0:
            mine.add("zero length")
        elif n == SAMPLED_FROM - 1 and cost_windows(inp) is None:
            mine.add("guess at 15 455")
        cw = cost_windows(inp, n) if inp is not None else None
        if cw is not None:
            third, wins = cw
            if n == SAMPLED_FROM:
                mine.add("sampled at 15 456")
            if third < WIN:
                mine.add("windows overlap")
            for w in wins:
                mine |= w[2] - {"never reaches its first counted byte"}
            if all("never reaches its first counted byte" in w[2] and w[1] == 0 for w in wins[1:]):
                mine |= {"never reaches its first counted byte", "lanes 1 and 2 with span 0"}
            toks = host_parse(inp)
            pos = np.array([t[0] for t in toks], np.int64)
            truth = set(pos.tolist())
            if third in truth and 2 * third in truth:
                mine.add("windows start on tokens")
            for w in (1, 2):
                base = w * third
                k = int(np.searchsorted(pos, base, side="right")) - 1
                _, L, _, _, src = toks[k]
                if base not in truth and src <= base < src + L:
                    mine.add("window starts inside literals")
                # the walk from the window's first byte steps on a true token before the counted part begins
                P, p = Parse(inp), base
                while p < base + K_SKIP and p not in truth:
                    p = P.token(p)[4]
                if base not in truth and p < base + K_SKIP:
                    mine.add("walk falls in step before byte 1 024")
            inside = pos[(pos >= 100) & (pos < K_W)]
            if len(inside) > 1 and (np.diff(inside) == 3).all():
                mine.add("3-byte tokens throughout")
        assert set(c["reaches"]) <= mine, (c["name"], sorted(set(c["reaches"]) - mine))
        got |= mine
    return got


def census_fed(min_in=FED_MIN_IN):
    got = set()
    for c in fed_cases():
        mine = set()
        n = c["input_len"]
        if n == min_in - 1 and not fed_eligible(c, min_in):
            mine.add("below min_in")
        if n == min_in and fed_eligible(c, min_in):
            mine.add("at min_in")
        if c["null_out"] and not fed_eligible(c, min_in):
            mine.add("null out")
        if c["prefix_len"] and fed_eligible(c, min_in):
            mine.add("prefix_len set")
        if c["out_existing_len"] and fed_eligible(c, min_in):
            mine.add("out_existing_len set")
        nch = S.seg_nch(n)
        if n == CHUNK and nch == 1:
            mine.add("one chunk, full")
        if n == CHUNK + 1 and nch == 2:
            mine.add("second chunk owns nothing")
        last = (nch - 1) * STRIDE
        if nch > 1 and OVERLAP < n - last < CHUNK:
            mine.add("ends inside an owned region")
        if nch > 64:
            mine.add("more than 64 chunks")
        if fed_eligible(c, min_in):
            est, seqs = fed_est(c, min_in, 32)
            if nch > 1 and seqs is not None:
                mine.add("in step at every seam")
                assert est == seqs
            P = Parse(c["input"])
            truth = np.zeros(n, bool)
            truth[[t[0] for t in P.chain(0)[0]]] = True
            for h in range(1, nch):
                cs = h * STRIDE
                hi = min(CHUNK, n - cs)
                m = chunk_marks(P, h)[:hi]
                agree = m & truth[cs:cs + hi]
                first = int(np.argmax(agree)) if agree.any() else None
                if hi > OVERLAP and not m[OVERLAP:].any():
                    mine.add("a chunk with no mark of its own")
                if first is None:
                    if m.sum() > 100:
                        mine.add("out of step through a whole chunk")
                elif 0 < first < OVERLAP and not truth[cs]:
                    mine.add("falls in step inside the overlap")
                elif first >= OVERLAP and m[OVERLAP:first].any():
                    mine.add("falls in step behind the overlap")
        assert set(c["reaches"]) <= mine, (c["name"], sorted(set(c["reaches"]) - mine))
        got |= mine
    return got


def census_probes():
    got = set()
    inside = aligned = apart = True
    for piece, parts in PROBES:
        cases = probe_cases(piece, parts, synthetic_data)
        jobs = [dict(input=0x7000_0000_0000 + 0x100000 * i + i % 16, input_len=len(c["data"]), cursor=c["cursor"]) for i, c in enumerate(cases)]
        pj = probe_jobs(jobs, piece, parts)
        T = 4 * piece * parts
        for i, (c, j) in enumerate(zip(cases, jobs)):
            mine = set()
            payload = cost_payload(j)
            if payload == T - 1:
                mine.add("payload 4*piece*parts - 1")
                assert not pj["input_len"][i * parts:(i + 1) * parts].any()
            if payload == T:
                mine.add("payload 4*piece*parts")
                assert (pj["input_len"][i * parts:(i + 1) * parts] == piece).all()
            if j["cursor"] == 0:
                mine.add("cursor 0")
            elif j["cursor"] >= j["input_len"]:
                mine.add("cursor >= input_len")
                assert payload == 0
            elif payload >= T:
                mine.add("cursor in the middle")
            assert set(c["reaches"]) <= mine, (c["name"], sorted(set(c["reaches"]) - mine))
            got |= mine
            lo = j["input"] + j["cursor"]
            starts = pj["input"][i * parts:(i + 1) * parts].astype(object) - lo
            for k in range(parts):
                if pj["input_len"][i * parts + k]:
                    inside = inside and 0 <= starts[k] and starts[k] + piece <= payload
                    aligned = aligned and starts[k] % 16 == 0
                    apart = apart and (k == 0 or starts[k] >= starts[k - 1] + piece)
    if inside:
        got.add("every probe inside its payload")
    if aligned:
        got.add("every probe 16-byte aligned to the payload")
    if apart:
        got.add("probes of a job do not overlap")
    return got
