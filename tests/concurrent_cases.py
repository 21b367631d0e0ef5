"""Call kinds of the concurrent-caller tests (tests/test_concurrent_cases_cpu.py proves them, tests/concurrent_check.py runs them on the
device): plain Python and numpy + the oracle.

A KIND is a named builder: build(kind, seed) returns a dict with the host-side inputs of one library call, the job arrays to make
of them and what the call must answer — statuses, lengths, bytes, tables, mismatch positions — from the oracle or, for a decode, the
known plaintext; never from the library.  The raw batch kinds also name the string lzf_last_*_launch must report (LAUNCH_*, copied from
rust-lz-fear_amd/csrc/lzf_dispatch.h; the CPU test compares them with the header).

Seeds 0 and 1 of a kind differ in their data and in their job counts (COUNTS): two equal calls would hide cross-talk between them.
The shapes are the smallest that reach each class on MI355X (256 CUs, 160 KiB of LDS) under the dispatch rules:

  D1  decompress_batch, max_input_len 65 535: the pair kernel alone            D2  segmented pipeline, one group (< 32 jobs)
  D3  segmented pipeline, four groups on the shared lanes (>= 32, bound 160 KiB) D4  bitmap-fed (> 3 072 jobs, bound 300 KiB)
  Z1 / Z2  decompressed_size_batch: latency class / one-wave kernel            V1 / V2  decompress_verify_batch the same way
  C1  compress_batch team kernel   C2  compact kernel, more jobs than CUs      C3  general kernels: U16 jobs, carried U32 tables
  C4  compressed_size_batch        A1  xxh32_batch, both kernels               A2  copy_ranges   A3  history trim + restore
  F1 .. F6  the device frame drivers (they wait for the caller's stream in mid-call)
  H1 / H2  the host-buffer batch calls / the host frame layer (one pinned slab, kept device scratch, the worker pool)

LONG kinds take a millisecond and more alone on MI355X (measured: profiles/concurrent_callers.txt); a pair of two long kinds must be
seen to overlap."""
import numpy as np

import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import synth

KIB = 1024
MIN_SEG_IN = 64 * KIB                       # lzf_dispatch.h kSegMinIn: smaller inputs never enter the pipeline / the latency classes
U32, U16, FRESH = 1, 2, 4                   # LZF_KINDS_*
TABLE_U32, TABLE_U16 = 0, 1
MISMATCH = 8
NO_CAP = (1 << 64) - 1
D1_BOUND, D3_BOUND, D4_BOUND = 65535, 160 * KIB, 300 * KIB

LAUNCH_PAIRED48 = "lzf_decompress_paired_kernel<4096,48,640>"
LAUNCH_SEG_128K = "segmented: lzf_seg_resolve_pair_kernel<131072> + lzf_decompress_paired_kernel<4096,48,640>"
LAUNCH_SEG_32K = "segmented: lzf_seg_resolve_pair_kernel<32768> + lzf_decompress_paired_kernel<4096,48,640>"
LAUNCH_FED = "bitmap-fed: lzf_seg_parse_kernel + lzf_decompress_fed_kernel<4096,32,352> + lzf_decompress_paired_kernel<4096,24,384>"
LAUNCH_SIZE_SEG = "latency: lzf_seg_parse_kernel + lzf_size_tile_kernel + lzf_size_finish_kernel + lzf_decoded_size_kernel<48,768>"
LAUNCH_SIZE_WAVE = "lzf_decoded_size_kernel<48,768>"
LAUNCH_VERIFY_SEG = "latency: lzf_seg_parse_kernel + lzf_size_tile_kernel + lzf_verify_finish_kernel + lzf_verify_tile_kernel + lzf_verify_kernel<48,768>"
LAUNCH_VERIFY_WAVE = "lzf_verify_kernel<48,768>"
LAUNCH_TEAM = "lzf_compress_team_kernel"
LAUNCH_TEAM_ALL = "lzf_compress_team_kernel + lzf_compress_team_carry_kernel + lzf_compress_wave_kernel"
LAUNCH_COMPACT_ALL = "lzf_compress_compact_kernel + lzf_compress_wave_kernel"

# jobs per call, seed 0 and seed 1 (A1: short buffers, long buffers).  Where a long kind took less than a millisecond alone on the device
# the count — never a block size — was raised until it did, with room for the run-to-run spread (profiles/concurrent_callers.txt):
# Z1 from 16 and 14 (0.37 and 0.50 ms; 0.58 at 512, 0.86 / 0.98 at 1 024) to 2 048 and 4 096 (1.24 and 2.20 ms; 4 096 is the class's ceiling),
# D3 from 36 and 44 (0.8 and 0.7 ms; 0.8 .. 1.7 ms, up and down, from 192 to 768 jobs) to 1 000 and 1 024, V1 from 16 and 14 (0.8 and 1.3 ms) to 1 024 and 960, C2 — one block's 1.02 ms
# whatever the count while all blocks are resident, 18 per CU — from 300 and 280 to 5 000 and 4 800: a second round of residents.
# The blocks of D3, Z1, V1 and C2 stay the 36 / 44, 16 / 14, 16 / 14 and 300 / 280 of the smaller calls; the jobs take them in turn.
COUNTS = {"D1": (40, 37), "D2": (8, 7), "D3": (1000, 1024), "D4": (3073, 3200), "Z1": (2048, 4096), "Z2": (200, 187), "V1": (1024, 960),
          "V2": (200, 187), "C1": (6, 5), "C2": (5000, 4800), "C3": (16, 14), "C4": (5000, 4800), "A1": (8193, 8200), "A1_LONG": (40, 37),
          "A2": (200, 190), "A3": (64, 60), "F1": (6, 5), "F2": (6, 5), "F3": (6, 5), "F4": (6, 5), "F5": (6, 5), "F6": (6, 5),
          "H1": (24, 21), "H2": (6, 5)}
ASYNC_KINDS = ("D1", "D2", "D3", "D4", "Z1", "Z2", "V1", "V2", "C1", "C2", "C3", "C4", "A1", "A2", "A3")
FRAME_KINDS = ("F1", "F2", "F3", "F4", "F5", "F6")
HOST_KINDS = ("H1", "H2")
KINDS = ASYNC_KINDS + FRAME_KINDS + HOST_KINDS
# D2 is not among them: one block's chain of stages bounds it (0.56 .. 0.64 ms at 7 .. 31 jobs), and it has no room for more jobs below
# the 32 at which the pipeline takes groups.  Its overlap is recorded, not required.
LONG = ("D3", "D4", "Z1", "V1", "C1", "C2", "C3") + FRAME_KINDS + ("H2",)
# which lzf_last_*_launch a kind sets, and to what
LAUNCH = {"D1": ("decompress", LAUNCH_PAIRED48), "D2": ("decompress", LAUNCH_SEG_128K), "D3": ("decompress", LAUNCH_SEG_32K),
          "D4": ("decompress", LAUNCH_FED), "Z1": ("size", LAUNCH_SIZE_SEG), "Z2": ("size", LAUNCH_SIZE_WAVE),
          "V1": ("verify", LAUNCH_VERIFY_SEG), "V2": ("verify", LAUNCH_VERIFY_WAVE), "C1": ("compress", LAUNCH_TEAM),
          "C2": ("compress", LAUNCH_COMPACT_ALL), "C3": ("compress", LAUNCH_TEAM_ALL)}
FRAME_BYTES, FRAME_BLOCK = 1536 * 1000, 64 * KIB          # "frames of 1.5 MB each in 64 KiB blocks"

_GENS = (synth.gen_text_zipf, synth.gen_records, synth.gen_log, synth.gen_markup)


def launch_of(kind, seed):
    """(which lzf_last_*_launch, the string it must report) for a call of (kind, seed), or None."""
    if kind not in LAUNCH:
        return None
    return LAUNCH[kind]


def _dims(bound):
    """lzf_dispatch.h seg_dims: the largest input the scratch is sized for, its chunks and its tiles."""
    m = min(max(bound if bound is not None else 1 << 62, 16384), 4 * 1024 * 1024 + 32 * 1024)
    return m, (1 if m <= 16384 else 1 + -(-(m - 16384) // 14336)), -(-m // 2048)


def pool_request(kind, seed):
    """Bytes of the largest scratch allocation a call of (kind, seed) asks the device's stream-ordered pool for, to the areas' alignment
    (lzf_dispatch.h: seg_layout, fed_layout, size_layout, verify_layout; the CPU test holds these to the emulated layouts).  Kinds
    whose scratch is a launch order or nothing: 0."""
    n = count(kind, seed)
    bound = {"D2": None, "D3": D3_BOUND, "D4": D4_BOUND, "Z1": None, "V1": None}.get(kind, 0)
    if bound == 0:
        return 0
    m, nch, tiles = _dims(bound)
    if kind in ("D2", "D3"):
        return 48 * n + 8 + 8 * n * nch + 8 * n * tiles + 2048 * n * nch + 16 * n * min(m // 3 + 192, 448 * 1024) + 12 * n
    if kind == "D4":
        return 48 * n + 8 + 2048 * n * nch + 4096 + 16 * n
    size = 48 * n + 8 * n * nch + 16 * n * tiles + 2048 * n * nch + 4 * n
    return size if kind == "Z1" else size + 8 * n * tiles + 8 * n


def count(kind, seed):
    return COUNTS[kind][seed & 1]


def plain(seed, k, n, tag=0, gen=None):
    """n bytes of compressible data, a function of (seed, k, tag) alone; the generator turns with k unless one is given."""
    return (gen or _GENS[(k + seed) % len(_GENS)])(0xC0CA11E5 + (tag << 40) + (seed << 20) + k, n).tobytes()


def _compress(data, **kw):
    rc, c = o.compress2(data, **kw)
    assert rc == 0, rc
    return c


def _linked(prefix, existing, data):
    """`data` compressed behind prefix + existing with a table carried over them (the linked-block case): the block's matches reach
    into both."""
    hist = prefix + existing
    t = o.new_table(TABLE_U32)
    assert o.compress2(hist, table=t)[0] == 0
    rc, c = o.compress2(hist + data, cursor=len(hist), table=t)
    assert rc == 0
    return c


def _first_offset_at(c):
    """Position of the match offset of a block's first sequence."""
    L, p = c[0] >> 4, 1
    if L == 15:
        while True:
            b = c[p]; p += 1; L += b
            if b != 255:
                break
    return p + L


def damaged(c, n_plain, status):
    """(input, limit) made of the valid block `c` (it decodes to n_plain bytes) that the oracle answers with `status` 1..4."""
    if status == 1:                                              # UnexpectedEnd: cut inside a sequence (a block cut behind a literal run ends Ok)
        for cut in range(len(c) - len(c) // 3, len(c)):
            if o.decompress_raw(c[:cut], limit=n_plain, cap=n_plain + len(c) + 64)[0] == 1:
                return c[:cut], n_plain
    if status == 2:
        return c, n_plain // 2                                   # MemoryLimitExceeded: the limit is half the output
    at = _first_offset_at(c)
    off = b"\0\0" if status == 3 else b"\xff\xff"                # ZeroDeduplicationOffset / InvalidDeduplicationOffset: far in front of the output
    return c[:at] + off + c[at + 2:], n_plain


def _djob(inp, limit, prefix=b"", existing=b"", cap=None):
    """limit: output_limit, which the decoder compares with output.len() — the existing output included."""
    return dict(inp=inp, prefix=prefix, existing=existing, limit=limit, cap=cap if cap is not None else limit + 64)


def _finish_decode(case):
    """out_cap >= output_limit + input_len: LZF_OUT_CAPACITY cannot happen."""
    for j in case["jobs"]:
        j["cap"] = j["limit"] + len(case["inputs"][j["inp"]]) + 64
    return case


# ------------------------------------------------------------------------------------------------------------------ decode kinds
def _decode_case(kind, seed, sizes, history_jobs=(), max_input_len=None):
    """One job per entry of `sizes` (plaintext bytes); the jobs in history_jobs get a prefix and existing output that their block
    refers to.  expect[i] = (0, index into plains): plains[i] = existing + plaintext."""
    inputs, jobs, plains, expect = [], [], [], []
    for k, n in enumerate(sizes):
        d = plain(seed, k, n, tag=ord(kind[1]))
        if k in history_jobs:
            pre, ex = plain(seed, k, 3000 + 7 * k, tag=90), plain(seed, k, 5000 + 11 * k, tag=91)
            c = _linked(pre, ex, d)
        else:
            pre, ex, c = b"", b"", _compress(d)
        inputs.append(c); plains.append(ex + d); expect.append((0, k))
        jobs.append(_djob(k, len(ex) + len(d), pre, ex))
    return _finish_decode(dict(kind=kind, seed=seed, family="decode", inputs=inputs, jobs=jobs, plains=plains, expect=expect,
                               max_input_len=max_input_len))


def build_d1(seed):
    n = count("D1", seed)
    sizes = [2 * KIB + (k * 977 + seed * 131) % (38 * KIB) for k in range(n)]
    sizes[0], sizes[-1] = 2 * KIB, 40 * KIB
    return _decode_case("D1", seed, sizes, history_jobs=(3, 11), max_input_len=D1_BOUND)


def _big_sizes(n, seed):
    return [256 * KIB + ((k * 7919 + seed * 4099) % 64) * KIB + k for k in range(n)]


def build_d2(seed):
    return _decode_case("D2", seed, _big_sizes(count("D2", seed), seed), history_jobs=(1, 5))


D3_BLOCKS = (36, 44)


def build_d3(seed):
    """36 and 44 blocks, taken in turn by the call's jobs (inputs are read-only: jobs may share them); every job has its own output.
    The caller bounds its inputs at 160 KiB (lzf_decompress_batch_sized), as a caller of a thousand blocks would: without a bound the
    call's scratch is sized for 4 MiB blocks at their worst — 7.6 GiB from the stream-ordered pool, and the runtime's allocator has
    kept an entry point on the host for up to 1.9 s over a request of that size (pool_request, profiles/concurrent_callers.txt)."""
    case = _decode_case("D3", seed, _big_sizes(D3_BLOCKS[seed & 1], seed), max_input_len=D3_BOUND)
    nb = len(case["jobs"])
    for k in range(nb, count("D3", seed)):
        case["jobs"].append(dict(case["jobs"][k % nb])); case["expect"].append(case["expect"][k % nb])
    return case


def build_d4(seed):
    """About 6 distinct inputs of 64 to 128 KiB shared by all jobs, every job with its own output slot of the same capacity."""
    n, nd = count("D4", seed), 6 + (seed & 1)
    sizes = [140 * KIB + ((k * 37 + seed * 11) % 100) * KIB + 13 * k for k in range(nd)]
    plains = [plain(seed, k, s, tag=4, gen=synth.gen_text_zipf) for k, s in enumerate(sizes)]             # (text: about 2.1 : 1)
    inputs = [_compress(d) for d in plains]
    cap = max(len(d) + len(c) for d, c in zip(plains, inputs)) + 64
    jobs, expect = [], []
    for i in range(n):
        k = (i * 5 + seed) % nd
        jobs.append(_djob(k, len(plains[k]), cap=cap)); expect.append((0, k))
    return dict(kind="D4", seed=seed, family="decode", inputs=inputs, jobs=jobs, plains=plains, expect=expect, max_input_len=D4_BOUND,
                uniform_cap=cap)


# ---------------------------------------------------------------------------------------------------------- size and verify kinds
def _size_case(kind, seed, sizes, max_input_len, n_jobs=None):
    """Valid blocks with, from job 2 on, one damaged block of every status 1..4; two jobs behind a prefix and existing output.
    expect[i] = (status, output.len() or None) — the plaintext's length for a valid block, the oracle's word for a damaged one."""
    inputs, jobs, expect, plains = [], [], [], []
    for k, n in enumerate(sizes):
        d = plain(seed, k, n, tag=ord(kind[0]) + int(kind[1]))
        pre, ex = (plain(seed, k, 2000 + k, tag=92), plain(seed, k, 3000 + k, tag=93)) if k in (0, 7) else (b"", b"")
        c = _linked(pre, ex, d) if pre else _compress(d)
        limit, st = len(ex) + len(d), 0
        if 2 <= k <= 5:
            st = k - 1
            c, limit = damaged(c, len(d), st)
        inputs.append(c); plains.append(ex + d)
        jobs.append(_djob(k, limit, pre, ex))
        expect.append((st, len(ex) + len(d) if st == 0 else None))
    for k in range(len(sizes), n_jobs or 0):                     # more jobs than blocks: the blocks again, in turn (read-only, they may be shared)
        jobs.append(dict(jobs[k % len(sizes)])); expect.append(expect[k % len(sizes)])
    return dict(kind=kind, seed=seed, family="size", inputs=inputs, jobs=jobs, plains=plains, expect=expect, max_input_len=max_input_len)


def _small_sizes(n, seed):
    return [600 + (k * 677 + seed * 211) % 9000 for k in range(n)]


Z1_BLOCKS = (16, 14)


def build_z1(seed):
    """16 and 14 blocks, taken in turn where the call has more jobs."""
    return _size_case("Z1", seed, _big_sizes(Z1_BLOCKS[seed & 1], seed), None, n_jobs=count("Z1", seed))


def build_z2(seed):
    return _size_case("Z2", seed, _small_sizes(count("Z2", seed), seed), D1_BOUND)


def _verify_case(kind, seed, sizes, max_input_len, n_jobs=None):
    """The size case with the expected bytes in every job's `out` (out_cap = their length; outs[j["inp"]]).  Block 6's expected bytes
    differ from the decoded ones at mismatch_at: LZF_MISMATCH with out_len = existing + that position."""
    case = _size_case(kind, seed, sizes, max_input_len, n_jobs)
    case["family"] = "verify"
    outs = []
    for k in range(len(sizes)):
        want, j = bytearray(case["plains"][k]), case["jobs"][k]
        if k == 6:
            at = len(j["existing"]) + mismatch_at(len(want) - len(j["existing"]), seed)
            want[at] ^= 0x40
        outs.append(bytes(want))
    for k, j in enumerate(case["jobs"]):
        j["cap"] = len(outs[j["inp"]])
        if j["inp"] == 6:
            case["expect"][k] = (MISMATCH, len(j["existing"]) + mismatch_at(len(outs[6]) - len(j["existing"]), seed))
    case["outs"] = outs
    return case


def mismatch_at(n, seed):
    return (n * (3 + seed)) // 7


def build_v1(seed):
    """16 and 14 blocks as Z1's, taken in turn by a few hundred jobs."""
    return _verify_case("V1", seed, _big_sizes(Z1_BLOCKS[seed & 1], seed), None, n_jobs=count("V1", seed))


def build_v2(seed):
    return _verify_case("V2", seed, _small_sizes(count("V2", seed), seed), D1_BOUND)


# ------------------------------------------------------------------------------------------------------------------- compress kinds
def _cjob(data, kind=TABLE_U32, cursor=0, cap=None, table=None):
    return dict(input=data, kind=kind, cursor=cursor, cap=cap if cap is not None else len(data) + len(data) // 255 + 64, table=table)


def _table_bytes(t):
    return bytes(memoryview(t).cast("B"))


def _expect_compress(jobs):
    """[(status, bytes)] and the tables after the call, from the oracle; the jobs' own `table` bytes stay as they are before the call."""
    expect, tables, seen = [], [], {}
    for j in jobs:
        key = (id(j["input"]), j["cursor"], j["kind"], j["cap"]) if j["table"] is None else None      # (C2: thousands of jobs over a few hundred inputs)
        if key not in seen:
            t = o.new_table(j["kind"])
            if j["table"] is not None:
                memoryview(t).cast("B")[:] = j["table"]
            rc, c = o.compress2(j["input"], cursor=j["cursor"], kind=j["kind"], table=t, cap=j["cap"])
            seen[key] = ((rc, c if rc == 0 else None), _table_bytes(t) if j["table"] is not None else None)
        expect.append(seen[key][0]); tables.append(seen[key][1])
        if key is None:
            del seen[key]
    return expect, tables


def _compress_case(kind, seed, jobs, kinds, family="compress"):
    expect, tables = _expect_compress(jobs)
    if family == "csize":
        expect = [(st, len(c) if st == 0 else None) for st, c in expect]
    return dict(kind=kind, seed=seed, family=family, jobs=jobs, kinds=kinds, expect=expect, tables_after=tables)


def build_c1(seed):
    n = count("C1", seed)
    sizes = [64 * KIB + ((k * 53 + seed * 17) % 192) * KIB + 3 * k for k in range(n)]
    sizes[0], sizes[-1] = 64 * KIB, 256 * KIB
    return _compress_case("C1", seed, [_cjob(plain(seed, k, s, tag=11)) for k, s in enumerate(sizes)], U32 | FRESH)


C2_BLOCKS = (300, 280)


def _c2_jobs(seed):
    """Blocks of 16 KiB, taken in turn by the call's jobs (the inputs are read-only: jobs may share them); every job has its own output."""
    blocks = [plain(seed, k, 16 * KIB, tag=12) for k in range(C2_BLOCKS[seed & 1])]
    return [_cjob(blocks[k % len(blocks)]) for k in range(count("C2", seed))]


def build_c2(seed):
    return _compress_case("C2", seed, _c2_jobs(seed), U32)


def build_c3(seed):
    """U16 jobs of up to 65 535 bytes with fresh tables, then 4 U32 jobs that continue a stream: cursor behind the first part and the
    writable table the oracle carried over it."""
    n = count("C3", seed)
    jobs = [_cjob(plain(seed, k, 65535 - ((k * 4111 + seed * 977) % 40000), tag=13), kind=TABLE_U16) for k in range(n - 4)]
    for k in range(4):
        d = plain(seed, 100 + k, 96 * KIB + 1000 * k + 64 * seed, tag=13)
        cur = 32 * KIB + 512 * k
        t = o.new_table(TABLE_U32)
        assert o.compress2(d[:cur], table=t)[0] == 0
        jobs.append(_cjob(d, cursor=cur, table=_table_bytes(t)))
    return _compress_case("C3", seed, jobs, U32 | U16)


def build_c4(seed):
    """C2's jobs through the size call; jobs 1 and 9 with a capacity of half their compressed length: LZF_OUTPUT_FULL."""
    jobs = _c2_jobs(seed)
    for j in jobs:
        j["cap"] = NO_CAP
    for k in (1, 9):
        jobs[k]["cap"] = len(_compress(jobs[k]["input"])) // 2
    case = _compress_case("C4", seed, [dict(j, cap=min(j["cap"], 1 << 20)) for j in jobs], U32, family="csize")
    case["jobs"] = jobs
    return case


# ---------------------------------------------------------------------------------------------------------------------- the helpers
def build_a1(seed):
    """Two xxh32_batch calls behind one another: more than 8 192 short buffers (the kernel of 16 hashes per wavefront) and 40 buffers
    of 1 to 300 KiB (the kernel of one wavefront per buffer)."""
    calls = []
    for name, lens in (("A1", [(k * 37 + seed * 5) % 200 for k in range(count("A1", seed))]),
                       ("A1_LONG", [1 * KIB + (k * 7727 + seed * 1013) % (299 * KIB) for k in range(count("A1_LONG", seed))])):
        lens[-1] = 300 * KIB if name == "A1_LONG" else lens[-1]
        offs = np.cumsum([0] + [ln + 1 + k % 3 for k, ln in enumerate(lens)])[:-1]
        arena = np.frombuffer(plain(seed, len(calls), int(offs[-1]) + lens[-1] + 16, tag=21), dtype=np.uint8)
        hashes = np.array([o.xxh32(arena[a:a + ln].tobytes()) for a, ln in zip(offs, lens)], dtype=np.uint32)
        calls.append(dict(arena=arena, offs=np.asarray(offs, dtype=np.uint64), lens=np.asarray(lens, dtype=np.uint64), hashes=hashes))
    return dict(kind="A1", seed=seed, family="xxh", calls=calls)


def build_a2(seed):
    """Ranges of 0 to about 40 KiB at turning residues, gaps of poison between the destinations.  expect = the whole destination."""
    n = count("A2", seed)
    lens = [(k * 2711 + seed * 313) % (40 * KIB) if k % 9 else k % 2 for k in range(n)]
    so = np.cumsum([0] + [ln + k % 5 for k, ln in enumerate(lens)])[:-1]
    do = np.cumsum([64] + [ln + 33 + k % 7 for k, ln in enumerate(lens)])[:-1]
    src = np.frombuffer(plain(seed, 0, int(so[-1]) + lens[-1] + 8, tag=22), dtype=np.uint8)
    return dict(kind="A2", seed=seed, family="copy", src=src, so=np.asarray(so, dtype=np.uint64), do=np.asarray(do, dtype=np.uint64),
                lens=np.asarray(lens, dtype=np.uint64), total=int(do[-1]) + lens[-1] + 64, max_len=max(lens))


def copy_expect(case, poison):
    out = np.full(case["total"], poison, dtype=np.uint8)
    for s, d, ln in zip(case["so"].tolist(), case["do"].tolist(), case["lens"].tolist()):
        out[d:d + ln] = case["src"][s:s + ln]
    return out


TRIM_FROM = 1 << 30                          # lzfear_hip.h: jobs with less than 1 GiB of existing output, or more than out_cap, are copied as they are


def build_a3(seed):
    """lzf_history_trim_batch over job records alone (nothing is decoded, the addresses are never followed): existing output below
    and beyond 1 GiB.  lzf_history_restore_batch over results of every status with the shifts of the trim.  The expectation is the
    header's rule: shift = (existing - 65 536) & ~15 from 1 GiB on, 0 below."""
    n = count("A3", seed)
    rows, results = [], []
    for k in range(n):
        ex = (TRIM_FROM - 3 + k + seed) if k % 4 == 1 else (TRIM_FROM * (2 + k % 3) + 12345 * k + seed) if k % 4 == 3 else 1000 * k + seed
        rows.append(dict(input=0x1000 * (k + 1), input_len=100 + k, prefix=0x7000000 + k, prefix_len=k % 5, out=0x100000000 + 64 * k,
                         out_existing_len=ex, out_cap=ex - 1 if k % 16 == 7 else ex + 70000 + k, output_limit=(ex + 5000 if k % 6 else ex // 2)))
        results.append(((k * 3 + seed) % 5 if k % 3 == 0 else 0, 4096 + k))                     # (status, trimmed out_len)
    return dict(kind="A3", seed=seed, family="trim", rows=rows, results=results)


def trim_expect(row):
    """(trimmed job, shift) by the rule of include/lzfear_hip.h."""
    ex = row["out_existing_len"]
    if ex < TRIM_FROM or ex > row["out_cap"]:
        return dict(row), 0
    shift = (ex - 65536) & ~15
    t = dict(row, out=row["out"] + shift, out_existing_len=ex - shift, out_cap=row["out_cap"] - shift,
             output_limit=max(row["output_limit"] - shift, 0))
    return t, shift


# ------------------------------------------------------------------------------------------------------------------- frames
def frames(seed, tag):
    """count frames of 1.5 MB in 64 KiB blocks by the oracle: frame 1 linked, frame 2 with a content checksum, frame 3 damaged (the
    match offset of its first block's first sequence is zero).  [(plaintext, frame, settings keywords)]."""
    out = []
    for k in range(count("F1", seed)):
        d = plain(seed, k, FRAME_BYTES + 4096 * k + seed, tag=tag)
        kw = dict(block_size=FRAME_BLOCK, independent_blocks=k != 1, content_checksum=k == 2)
        rc, f = o.frame_compress(d, o.make_settings(**kw))
        assert rc == 0
        if k == 3:
            assert f[4] & 0x09 == 0 and not f[10] & 0x80, "7-byte header, first block compressed"
            at = 11 + _first_offset_at(f[11:])
            f = f[:at] + b"\0\0" + f[at + 2:]
        out.append((d, f, kw))
    return out


def _frame_case(kind, seed, family, **more):
    fr = frames(seed, tag=30 + int(kind[1]))
    dec = [o.frame_decompress(f, cap=len(d) + 65536) for d, f, _ in fr]            # (status, bytes, consumed)
    return dict(kind=kind, seed=seed, family=family, plains=[d for d, _, _ in fr], frames=[f for _, f, _ in fr], decoded=dec, **more)


def build_f1(seed):
    """frame_decompress_many: expect = the oracle's (status, bytes, consumed) of every frame."""
    return _frame_case("F1", seed, "frame_decompress")


def build_f2(seed):
    """frame_compress_many: one settings per call — seed 0 independent blocks with a content checksum, seed 1 linked blocks; expect =
    the oracle's frames of the plaintexts."""
    kw = dict(block_size=FRAME_BLOCK, independent_blocks=not seed & 1, content_checksum=not seed & 1)
    case = _frame_case("F2", seed, "frame_compress", settings=kw)
    case["expect"] = [o.frame_compress(d, o.make_settings(**kw)) for d in case["plains"]]
    return case


def build_f3(seed):
    """stream_decompress: the valid frames back to back in two streams; expect = the plaintexts behind one another."""
    case = _frame_case("F3", seed, "stream_decompress")
    ok = [k for k, d in enumerate(case["decoded"]) if d[0] == 0]
    case["streams"] = [ok[:len(ok) // 2], ok[len(ok) // 2:]]
    return case


def build_f4(seed):
    """frame_verify against the plaintexts; frame 0's expected bytes differ at FRAME_MISMATCH_AT."""
    case = _frame_case("F4", seed, "frame_verify")
    at = mismatch_at(len(case["plains"][0]), seed)
    want = [bytearray(d) for d in case["plains"]]
    want[0][at] ^= 0x01
    case["wanted"] = [bytes(w) for w in want]
    case["expect"] = [(MISMATCH, at) if k == 0 else (st, len(b)) for k, (st, b, _) in enumerate(case["decoded"])]
    return case


def build_f5(seed):
    """frame_block_index, then frame_decompress_blocks over all blocks of every valid frame."""
    return _frame_case("F5", seed, "frame_blocks")


def build_f6(seed):
    """frame_decompressed_size: (status, size, consumed) of every frame; the content checksum is not verified."""
    return _frame_case("F6", seed, "frame_size")


# ------------------------------------------------------------------------------------------------------------------- host buffers
def build_h1(seed):
    """lzf_decompress_batch_host and lzf_compress_batch_host over the same plaintexts of 1 to 200 KiB."""
    n = count("H1", seed)
    plains = [plain(seed, k, 1 * KIB + (k * 9173 + seed * 577) % (199 * KIB), tag=41) for k in range(n)]
    comp = [o.compress2(d) for d in plains]
    return dict(kind="H1", seed=seed, family="host_batch", plains=plains, comp=comp)


def build_h2(seed):
    """framed compress_many / decompress_frames over host buffers: F-like frames of 1.5 MB, independent blocks of 64 KiB."""
    kw = dict(block_size=FRAME_BLOCK, independent_blocks=True, content_checksum=True)
    plains = [plain(seed, k, FRAME_BYTES + 1000 * k + seed, tag=42) for k in range(count("H2", seed))]
    fr = [o.frame_compress(d, o.make_settings(**kw)) for d in plains]
    return dict(kind="H2", seed=seed, family="host_frames", plains=plains, frames=[f for _, f in fr], settings=kw)


BUILDERS = {"D1": build_d1, "D2": build_d2, "D3": build_d3, "D4": build_d4, "Z1": build_z1, "Z2": build_z2, "V1": build_v1,
            "V2": build_v2, "C1": build_c1, "C2": build_c2, "C3": build_c3, "C4": build_c4, "A1": build_a1, "A2": build_a2,
            "A3": build_a3, "F1": build_f1, "F2": build_f2, "F3": build_f3, "F4": build_f4, "F5": build_f5, "F6": build_f6,
            "H1": build_h1, "H2": build_h2}
_CACHE = {}


def build(kind, seed):
    """The case of (kind, seed), built once per process and never changed afterwards."""
    if (kind, seed) not in _CACHE:
        _CACHE[kind, seed] = BUILDERS[kind](seed)
    return _CACHE[kind, seed]


def job_count(case):
    f = case["family"]
    return (len(case["calls"][0]["lens"]) if f == "xxh" else len(case["lens"]) if f == "copy" else len(case["rows"]) if f == "trim"
            else len(case["frames"]) if f.startswith("frame") or f == "stream_decompress" or f == "host_frames"
            else len(case["plains"]) if f == "host_batch" else len(case["jobs"]))


def job_bytes(case):
    """One bytes object per job: what the CPU test compares between two seeds."""
    f = case["family"]
    if f in ("decode", "size", "verify"):
        return [case["inputs"][j["inp"]] for j in case["jobs"]]
    if f in ("compress", "csize"):
        return [j["input"] for j in case["jobs"]]
    if f == "xxh":
        c = case["calls"][0]
        return [c["arena"][a:a + n].tobytes() for a, n in zip(c["offs"].tolist(), c["lens"].tolist())]
    if f == "copy":
        return [case["src"][a:a + n].tobytes() for a, n in zip(case["so"].tolist(), case["lens"].tolist())]
    if f == "trim":
        return [repr(sorted(r.items())).encode() for r in case["rows"]]
    if f == "host_batch":
        return case["plains"]
    return case["frames"]


# ------------------------------------------------------------------------------------------------------------------- the pairs
def _self(kinds):
    return [((k, 0), (k, 1)) for k in kinds]


def _with(kinds, other):
    return [((k, 0), (other, 1)) for k in kinds if k != other]


def _dedup(pairs):
    seen, out = set(), []
    for p in pairs:
        if p not in seen and (p[1], p[0]) not in seen:
            seen.add(p); out.append(p)
    return out


def stream_pairs():
    """One thread, two caller streams: every asynchronous kind with itself (other seed), with D3 and with D4; D3 with D3 in both
    enqueue orders.  ((kind, seed) first enqueued, (kind, seed) second)."""
    return _dedup(_self(ASYNC_KINDS) + _with(ASYNC_KINDS, "D3") + _with(ASYNC_KINDS, "D4")) + [(("D3", 1), ("D3", 0))]


def thread_pairs():
    """Two threads: every kind with itself (other seed), with D3, with F1 and with H2."""
    return _dedup(_self(KINDS) + _with(KINDS, "D3") + _with(KINDS, "F1") + _with(KINDS, "H2"))


THREAD_MIX = (("D3", 0), ("C2", 0), ("F1", 0), ("H2", 0))


def slices(pairs, size):
    return [pairs[a:a + size] for a in range(0, len(pairs), size)]


def both_long(pair):
    return pair[0][0] in LONG and pair[1][0] in LONG
