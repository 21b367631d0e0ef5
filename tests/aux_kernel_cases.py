"""Built cases for the small kernels around the codec (rust-lz-fear_amd/csrc/aux_kernels.hip), behind the public entry points
lzf_xxh32_batch, lzf_chain_decompress_step, lzf_table_offset(_batch), lzf_table_seed_from_dictionary and lzf_copy_ranges.

Every builder is seeded and needs neither a GPU nor torch: a case is host bytes (an arena) and offsets into it.  The GPU test
(tests/test_gpu_aux_kernels.py) puts an arena at a 256-byte boundary of device memory, so `offset & 15` is the pointer's residue;
the CPU test (tests/test_aux_kernel_cases_cpu.py) proves that the cases reach the edges named here and pins every expectation
to the oracle.
"""
import functools

import numpy as np

from seg_stage_cases import _seq      # one LZ4 sequence (the hand-built block of the chain frames)

M64 = (1 << 64) - 1
NONE = 0xFFFFFFFF                      # UINT32_MAX: "no job" in lzf_chain_step
ZONE = 4096                            # red zones, as tests/redzone.py
OUT_POISON = 0xA5                      # tests/redzone.py: what surrounds every output
IN_POISONS = (0x00, 0xFF)              # tests/redzone.py: what surrounds every input, one run each

# lzf_xxh32_batch hashes up to this many buffers with one wavefront per buffer (lzf_xxh32_wave_kernel) and more with 16 hashes per
# wavefront (lzf_xxh32_kernel).  The same number is a literal in capi.hip (lzf_xxh32_batch); tests/test_gpu_aux_kernels.py:
# test_xxh32_lane_kernel_on_both_sides_of_the_switch calls with this many buffers and with one more.  Move both together.
XXH32_WAVE_KERNEL_MAX_N = 8192


# ------------------------------------------------------------------------------------------------------------------- XXH32
XXH_LONG = (1024, 1025, 1039) + tuple(range(1040, 1056)) + (2047, 2048, 2049, 2064, 3071, 3072, 3073, 3088) + \
    tuple(4096 + 16 * k + r for k in (0, 1, 5) for r in (0, 3, 4, 15)) + (65536 + 1024 + 17,)
XXH_SHORT = tuple(range(49)) + (63, 64, 65, 255, 256, 257, 1008, 1023)
XXH_SHORT_RESIDUES = (0, 1, 2, 3, 15)


def xxh_shape(n):
    """How the wave kernel splits a length: 1 KiB chunks (0, 1, 2, 3, "many"), the 16-byte stripes behind the last chunk, the
    bytes behind the last stripe."""
    chunks = n >> 10
    return ("many" if chunks > 3 else chunks), (n >> 4) - (chunks << 6), n & 15


def _place(lens, residues, rng, gap=48):
    """An arena of random bytes and one offset per buffer: buffer i at `residues[i]` modulo 16, `gap` bytes or more apart."""
    offs, pos = [], gap
    for n, r in zip(lens, residues):
        pos = (pos + 15) // 16 * 16 + r
        offs.append(pos)
        pos += n + gap
    return rng.integers(0, 256, pos + 16, dtype=np.uint8), offs


@functools.lru_cache(maxsize=None)
def xxh_wave_case():
    """Every length of XXH_LONG at all 16 pointer residues and of XXH_SHORT at XXH_SHORT_RESIDUES: one call of the wave kernel."""
    jobs = [(n, r) for n in XXH_LONG for r in range(16)] + [(n, r) for n in XXH_SHORT for r in XXH_SHORT_RESIDUES]
    rng = np.random.default_rng(3201)
    order = rng.permutation(len(jobs))
    jobs = [jobs[i] for i in order]
    arena, offs = _place([n for n, _ in jobs], [r for _, r in jobs], rng)
    return dict(name="wave", arena=arena, offs=offs, lens=[n for n, _ in jobs])


LANE_HANDFUL = (1024, 2049, 3088, 4096 + 19, 5000)      # the few 1 KiB .. 5 KiB buffers of a lane-kernel list
LANE_FIRST_WAVE = (0, 5, 16, 0, 15, 16, 1, 17, 16, 0, 3, 32, 16, 15, 0, 48)      # 0, below 16 and exactly 16 next to each other


def _lane_list(seed, n):
    """n buffers for the kernel of 16 hashes per wavefront, all inside one pool of random bytes (the buffers alias: they are only
    read).  Buffer g is group g % 16 of wavefront g // 16.  Most wavefronts get 16 pairwise different stripe counts out of 0..16
    in a random order, so every group ends its loops before, with and after each of its neighbours somewhere; every eighth
    wavefront draws with repeats; the first is LANE_FIRST_WAVE; LANE_HANDFUL is spread over groups in the middle of wavefronts."""
    rng = np.random.default_rng(seed)
    lens = []
    for w in range((n + 15) // 16):
        if w == 0:
            lens += LANE_FIRST_WAVE
        elif w % 8 == 7:
            lens += [int(x) for x in rng.choice(XXH_SHORT[:55], 16)]
        else:
            for k in rng.permutation(17)[:16]:
                lens.append(16 * int(k) + int(rng.integers(0, 16 if k < 16 else 2)))      # (16 stripes: 256 or 257 bytes)
    lens = lens[:n]
    for k, big in enumerate(LANE_HANDFUL):
        lens[16 * (40 + 97 * k) + (3 + 5 * k) % 16] = big
    pool = rng.integers(0, 256, 8192 + max(LANE_HANDFUL), dtype=np.uint8)
    offs = [int(rng.integers(0, len(pool) - ln + 1)) for ln in lens]
    return dict(name=f"lane{n}", arena=pool, offs=offs, lens=lens)


@functools.lru_cache(maxsize=None)
def xxh_lane_cases():
    """(the list of XXH32_WAVE_KERNEL_MAX_N buffers — the wave kernel's last n —, the same with one buffer appended, a longer list whose
    last wavefront has idle groups)."""
    at = XXH32_WAVE_KERNEL_MAX_N
    more = _lane_list(3202, at + 1)
    same = dict(name=f"lane{at}", arena=more["arena"], offs=more["offs"][:at], lens=more["lens"][:at])
    return same, more, _lane_list(3203, at + 16 * 3 + 9)


def xxh_buffers(case):
    a = case["arena"]
    return [a[o:o + n].tobytes() for o, n in zip(case["offs"], case["lens"])]


# ------------------------------------------------------------------------------------------------------------ the chain step
STEP = np.dtype([("prev_job", "<u4"), ("job", "<u4"), ("stored_len", "<u8"), ("stored_src", "<u8"), ("out", "<u8"),
                 ("block_maxsize", "<u8")])                                                       # lzf_chain_step
STATE = np.dtype([("length", "<u8"), ("dead", "<u4"), ("reserved", "<u4")])                       # lzf_chain_state
DJOB = np.dtype([("input", "<u8"), ("input_len", "<u8"), ("prefix", "<u8"), ("prefix_len", "<u8"), ("out", "<u8"),
                 ("out_existing_len", "<u8"), ("out_cap", "<u8"), ("output_limit", "<u8")])       # lzf_decompress_job
RES = np.dtype([("out_len", "<u8"), ("status", "<i4"), ("reserved", "<u4")])                      # lzf_job_result
assert (STEP.itemsize, STATE.itemsize, DJOB.itemsize, RES.itemsize) == (40, 16, 64, 16)
F_BLOCK_SIZE_OVERFLOW = 22


def chain_model(length, dead, block_maxsize, prev=None, job=None, stored_len=0, count_only=False):
    """What LZ4FrameReader::decode_block (src/framed/decompress.rs:238-274) does to one linked-block stream between two blocks, for a
    stream whose whole output is one buffer: `length` bytes of it are the history (it covers the carry-over window of :253-269), so
    the next block is decoded behind them with a limit counted from there.

    prev: (status, out_len) of the block decoded last, None if there was none or it was a stored one.  job: input_len of the
    block to decode next, None if there is none.  Returns (length, dead, job fields or None, copy or None, error): the job's
    (input_len, out_existing_len, out_cap, output_limit); copy = (position in the output, bytes) of a stored block; error = the
    status that ended the stream in this step (F_BLOCK_SIZE_OVERFLOW for :272-274), 0 otherwise.  count_only: the history is kept
    as a length alone, so a stored block copies nothing."""
    error = 0
    if prev is not None and not dead:
        status, out_len = prev
        if status != 0:                           # :248: decompress_raw(..)? — the error leaves decode_block, the reader is done
            dead, error = 1, status
        else:                                     # :253-269: the block is in `output` and in the window before :272 looks at its size
            grown = (out_len - length) & M64
            length = out_len
            if grown > block_maxsize:             # :272-274
                dead, error = 1, F_BLOCK_SIZE_OVERFLOW
    fields = copy = None
    if job is not None:
        if dead:
            fields = (0, 0, 0, 0)                 # nothing to decode, nowhere to write
        else:                                     # :248: an empty Vec and block_maxsize become "behind `length`, at most block_maxsize more";
            limit = (length + block_maxsize) & M64      # literals are not limit-checked (src/raw/decompress.rs:55-57): input_len more room
            fields = (job, length, (limit + job) & M64, limit)
    elif stored_len and not dead:                 # :250: output.extend_from_slice(buf)
        if not count_only:
            copy = (length, stored_len)
        length = (length + stored_len) & M64
    return length, dead, fields, copy, error


STORED_SIZES = (1, 255, 256, 257, 4096 + 1, 65536 + 3)
STORED_RESIDUES = (0, 1, 15)
BM = 65536


@functools.lru_cache(maxsize=None)
def chain_case():
    """One call of lzf_chain_decompress_step over every named stream.  Returns the four arrays as the host writes them (pointers are
    offsets into `src` / `out`, to be rebased; `out` of a stream that must never be dereferenced is `wild`), and the names."""
    rng = np.random.default_rng(3301)
    streams = []

    def add(name, length=1000, dead=0, bm=BM, prev=None, job=None, stored=0, sr=0, dr=0, wild=False):
        streams.append(dict(name=name, length=length, dead=dead, bm=bm, prev=prev, job=job, stored=stored, sr=sr, dr=dr, wild=wild))

    add("prev none, job", job=777)
    add("prev none, job, nothing decoded yet", length=0, job=12345)
    add("prev ok, job", prev=(0, 1000 + 4321), job=999)
    for s in range(1, 8):
        add(f"prev status {s}, job emptied", prev=(s, 1000 + 50), job=100 + s)
    add("prev status 4, stored block not copied", prev=(4, 1234), stored=300)
    add("prev ok, grown by block_maxsize: alive", prev=(0, 1000 + BM), job=31)
    add("prev ok, grown by block_maxsize + 1: dead, length updated", prev=(0, 1000 + BM + 1), job=32)
    add("prev ok, grown by block_maxsize + 1, stored block not copied", prev=(0, 1000 + BM + 1), stored=64)
    add("prev ok, 4 MiB blocks, grown by block_maxsize: alive", bm=4 << 20, prev=(0, 1000 + (4 << 20)), job=33, wild=True)
    add("prev ok, 4 MiB blocks, grown by block_maxsize + 1: dead", bm=4 << 20, prev=(0, 1001 + (4 << 20)), job=34, wild=True)
    add("dead on entry, job emptied, prev ignored", dead=1, prev=(0, 5000), job=55)
    add("dead on entry, stored block not copied", dead=1, stored=700, sr=1, dr=15)
    add("job none, stored_len 0", length=4242)
    add("prev ok, job none, stored_len 0: the chain's last step", prev=(0, 1000 + 17))
    add("prev ok, stored block behind the new length", prev=(0, 1000 + 333), stored=500, sr=15, dr=1)
    for n in STORED_SIZES:
        for sr in STORED_RESIDUES:
            for dr in STORED_RESIDUES:
                add(f"stored {n}, source & 15 = {sr}, destination & 15 = {dr}", length=int(rng.integers(0, 3000)), stored=n, sr=sr, dr=dr)
    add("length above 4 GiB, job", length=(5 << 32) + 77, job=(1 << 20) + 3, wild=True)
    add("length across 4 GiB, prev ok grown by block_maxsize: alive", length=(1 << 32) - 5, prev=(0, (1 << 32) - 5 + BM), job=9, wild=True)
    add("length above 4 GiB, prev ok grown by block_maxsize + 1: dead", length=(7 << 32) + 1, prev=(0, (7 << 32) + 2 + BM), job=10, wild=True)

    n = len(streams)
    n_jobs = 2 * n + 7                                   # the jobs and results of this step and the last, and some that belong to no stream
    slots = [int(x) for x in rng.permutation(n_jobs)]
    jobs = np.zeros(n_jobs, dtype=DJOB)
    for f in DJOB.names:                                 # every field starts as something to tell from whatever the step writes
        jobs[f] = rng.integers(1, 1 << 40, n_jobs, dtype=np.uint64)
    res = np.zeros(n_jobs, dtype=RES)
    res["out_len"] = rng.integers(0, 1 << 40, n_jobs, dtype=np.uint64)
    res["status"] = rng.integers(0, 8, n_jobs)
    res["reserved"] = rng.integers(0, 1 << 32, n_jobs, dtype=np.uint64)
    steps = np.zeros(n, dtype=STEP)
    state = np.zeros(n, dtype=STATE)
    state["reserved"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    src_sizes, src_res, out_sizes, out_res = [], [], [], []
    for i, s in enumerate(streams):
        steps["prev_job"][i] = steps["job"][i] = NONE
        if s["prev"] is not None:
            k = slots.pop()
            steps["prev_job"][i] = k
            res["status"][k], res["out_len"][k] = s["prev"]
        if s["job"] is not None:
            k = slots.pop()
            steps["job"][i] = k
            jobs["input_len"][k] = s["job"]
        steps["stored_len"][i] = s["stored"]
        steps["block_maxsize"][i] = s["bm"]
        state["length"][i], state["dead"][i] = s["length"], s["dead"]
        src_sizes.append(s["stored"]); src_res.append(s["sr"])
        # room for the history, for what a previous block may have added and for the stored block; the end of the history
        # (where a stored block lands) at the destination residue
        after_prev = s["prev"][1] if s["prev"] is not None and s["prev"][0] == 0 and not s["dead"] else s["length"]
        out_sizes.append(0 if s["wild"] else max(after_prev, s["length"]) + s["stored"])
        out_res.append((s["dr"] - after_prev) % 16)
    assert len(slots) == n_jobs - sum((s["prev"] is not None) + (s["job"] is not None) for s in streams) >= 7
    src, src_offs = _place(src_sizes, src_res, rng, gap=ZONE)
    out, out_offs = _place(out_sizes, out_res, rng, gap=ZONE)
    src_mask = np.zeros(len(src), dtype=bool)            # the bytes that are stored blocks; everything else is IN-poison on the device
    out_mask = np.zeros(len(out), dtype=bool)            # the bytes that are history on entry; everything else is OUT_POISON
    for i, s in enumerate(streams):
        src_mask[src_offs[i]:src_offs[i] + s["stored"]] = True
        if not s["wild"]:
            out_mask[out_offs[i]:out_offs[i] + out_sizes[i] - s["stored"]] = True
    steps["stored_src"] = src_offs
    steps["out"] = out_offs
    return dict(names=[s["name"] for s in streams], streams=streams, steps=steps, state=state, jobs=jobs, results=res,
                src=src, src_mask=src_mask, out=out, out_mask=out_mask, wild=[s["wild"] for s in streams])


WILD_OUT = 0x00007F0000000010      # `out` of a stream whose output is never dereferenced (no device allocation is there to hit by luck)


def chain_arenas(case, in_poison):
    """(src, out) as they are uploaded: the stored blocks inside `in_poison`, the histories inside OUT_POISON."""
    return np.where(case["src_mask"], case["src"], np.uint8(in_poison)), np.where(case["out_mask"], case["out"], np.uint8(OUT_POISON))


def chain_rebase(case, src_base, out_base):
    steps = case["steps"].copy()
    steps["stored_src"] += np.uint64(src_base)
    steps["out"] = [WILD_OUT if w else out_base + int(o) for w, o in zip(case["wild"], case["steps"]["out"])]
    return steps


def chain_expect(case, in_poison):
    """The model over the call: (state, jobs, out) afterwards; `steps`, `results` and `src` stay as they are."""
    steps, state, jobs, res = case["steps"], case["state"].copy(), case["jobs"].copy(), case["results"]
    src, out = chain_arenas(case, in_poison)
    for i in range(len(steps)):
        st = steps[i]
        prev = None if st["prev_job"] == NONE else (int(res["status"][st["prev_job"]]), int(res["out_len"][st["prev_job"]]))
        job = None if st["job"] == NONE else int(jobs["input_len"][st["job"]])
        length, dead, fields, copy, _ = chain_model(int(state["length"][i]), int(state["dead"][i]), int(st["block_maxsize"]), prev, job,
                                                    int(st["stored_len"]))
        state["length"][i], state["dead"][i] = length, dead
        if fields is not None:
            k = st["job"]
            jobs["input_len"][k], jobs["out_existing_len"][k], jobs["out_cap"][k], jobs["output_limit"][k] = fields
        if copy is not None:
            assert not case["wild"][i]
            a, b = int(st["out"]) + copy[0], int(st["stored_src"])
            out[a:a + copy[1]] = src[b:b + copy[1]]
    return state, jobs, out


# ---- frames of linked blocks, walked block by block (the CPU test drives chain_model with the oracle's decompress_raw over them)
def frame_walk(frame):
    """(linked, block_maxsize, [(stored, bytes)]) of an LZ4 frame without block checksums and content size."""
    flg, bd = frame[4], frame[5]
    assert not flg & 0x18, "no content size, no block checksums"
    p = 4 + 2 + (4 if flg & 1 else 0) + 1
    blocks = []
    while True:
        w = int.from_bytes(frame[p:p + 4], "little"); p += 4
        if w == 0:
            return not flg & 0x20, 1 << (((bd >> 4) & 7) * 2 + 8), blocks
        blocks.append((bool(w >> 31), frame[p:p + (w & 0x7FFFFFFF)]))
        p += w & 0x7FFFFFFF


def frame_with_block(frame, k, block):
    """The frame with its k-th block replaced by the compressed `block`."""
    p = 4 + 2 + (4 if frame[4] & 1 else 0) + 1
    for _ in range(k):
        p += 4 + (int.from_bytes(frame[p:p + 4], "little") & 0x7FFFFFFF)
    old = int.from_bytes(frame[p:p + 4], "little") & 0x7FFFFFFF
    return frame[:p] + len(block).to_bytes(4, "little") + block + frame[p + 4 + old:]


def overflowing_block(block_maxsize):
    """A block every sequence of which passes decompress_raw's limit check and whose last literals, which are not checked
    (src/raw/decompress.rs:63-67), carry it 8 bytes past block_maxsize."""
    return _seq(b"abcd", 4, block_maxsize - 6) + _seq(b"0123456789", None, 0)


def run_chain(frame, dictionary, decompress_raw):
    """A linked-block frame through chain_model in lock step, as the frame layer does it: step k finishes block k - 1 and prepares
    block k; a compressed block is then decoded by `decompress_raw(block, prefix, existing, limit, cap)` -> (status, bytes).
    Returns dict(status, out: the bytes delivered, done: the blocks finished, trace: (length, dead) after every step, results: what
    every step was given as the previous block's result)."""
    linked, bm, blocks = frame_walk(frame)
    assert linked
    out, length, dead, prev, delivered = b"", 0, 0, None, 0
    trace, results = [], []
    for k in range(len(blocks) + 1):
        stored, data = blocks[k] if k < len(blocks) else (False, None)
        job = len(data) if data is not None and not stored else None
        results.append(prev)
        length, dead, fields, copy, error = chain_model(length, dead, bm, prev, job, len(data) if stored else 0)
        trace.append((length, dead))
        if error:
            return dict(status=error, out=out[:delivered], done=k - 1, trace=trace, results=results)
        if copy is not None:
            assert copy == (len(out), len(data))
            out += data
        assert length == len(out)
        delivered, prev = length, None
        if fields is not None:
            assert fields[:2] == (len(data), len(out))
            rc, got = decompress_raw(data, dictionary, out, fields[3], fields[2])
            if rc == 0:
                assert got[:len(out)] == out
                out = got
            prev = (rc, len(got))
    return dict(status=0, out=out, done=len(blocks), trace=trace, results=results)


def run_chain_count_only(frame, results):
    """The same steps by the count-only rule (the frame layer's size query: lzf_chain_size_step_kernel), given each block's
    (status, out_len): the (length, dead) trace; nothing is ever copied."""
    _, bm, blocks = frame_walk(frame)
    length, dead, trace = 0, 0, []
    for k, prev in enumerate(results):
        stored, data = blocks[k] if k < len(blocks) else (False, None)
        job = len(data) if data is not None and not stored else None
        length, dead, _, copy, _ = chain_model(length, dead, bm, prev, job, len(data) if stored else 0, count_only=True)
        assert copy is None
        trace.append((length, dead))
    return trace


# ---------------------------------------------------------------------------------------------------------- table helpers
TABLE_BYTES = 16384 + 8            # lzf_u32_table and lzf_u16_table alike: the slots, then the offset
OFFSET_ADDS = (0, 1, 65536, (1 << 32) + 5, 1 << 63)
OFFSET_BATCH_N = (1, 255, 256, 257, 1000)


@functools.lru_cache(maxsize=None)
def offset_tables():
    """max(OFFSET_BATCH_N) tables of random bytes, offsets included, back to back."""
    return np.random.default_rng(3401).integers(0, 256, (max(OFFSET_BATCH_N), TABLE_BYTES), dtype=np.uint8)


def offset_adds(n, rnd):
    """The adds of the rnd-th batch call over n tables: OFFSET_ADDS in turn, from another start every call."""
    return np.array([OFFSET_ADDS[(i + 2 * rnd) % len(OFFSET_ADDS)] for i in range(n)], dtype=np.uint64)


def offset_expect(tables, adds):
    """`tables` with adds[i] added to the offset of table i modulo 2^64 (tables beyond len(adds) as they are)."""
    t = tables.copy()
    off = np.ascontiguousarray(t[:, 16384:]).view("<u8").reshape(-1)
    off[:len(adds)] += adds                                                    # (uint64 arrays wrap)
    t[:, 16384:] = off.view(np.uint8).reshape(-1, 8)
    return t


SEED_GRID_ITEMS = 1024 * 256       # windows one pass of lzf_seed_table_kernel's grid takes (1 024 workgroups of 256: capi.hip)


def seed_windows(n):
    return (n - 8) // 3 + 1 if n >= 8 else 0


def seed_expect(dictionary):
    """The template table of src/framed/compress.rs:202-211 restated with numpy: hash_for_u32 (src/raw/compress/mod.rs:40-51) of
    the 8-byte window at every third position; the last position with a hash wins, and positions only grow: a per-slot maximum."""
    d = np.frombuffer(bytes(dictionary), dtype=np.uint8)
    table = np.zeros(4096, dtype=np.uint32)
    if len(d) >= 8:
        v = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(d, 8)[::3]).view("<u8")[:, 0]
        h = ((v << np.uint64(24)) * np.uint64(889523592379)) >> np.uint64(52)
        np.maximum.at(table, h.astype(np.int64), (np.arange(len(v), dtype=np.uint64) * 3).astype(np.uint32))
    return table.tobytes() + bytes(8)


def seed_hashes(dictionary):
    d = np.frombuffer(bytes(dictionary), dtype=np.uint8)
    v = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(d, 8)[::3]).view("<u8")[:, 0]
    return ((v << np.uint64(24)) * np.uint64(889523592379)) >> np.uint64(52)


@functools.lru_cache(maxsize=None)
def seed_cases():
    """[(name, dictionary bytes, pointer residue)]"""
    rng = np.random.default_rng(3402)
    big = rng.integers(0, 256, 2 * 786432 + 8 + 2, dtype=np.uint8).tobytes()
    cases = [(f"dict_len {n}", big[100:100 + n], 0) for n in range(41)]
    cases += [(f"dict_len 1000 at residue {r}", big[3000 + r:4000 + r], r) for r in range(8)]
    cases.append(("one full pass of the grid", big[:786432 + 7], 0))
    for base, what in ((786432 + 8, "grid-stride loop, second pass of one window"), (2 * 786432 + 8, "grid-stride loop, third pass of one window")):
        cases += [(f"{what}, (dict_len - 8) % 3 = {k}", big[:base + k], 3 + k) for k in range(3)]
    cases.append(("all zero", bytes(100), 0))
    k = 0
    while True:                                   # a dictionary whose first window's slot is hit by no other window
        lonely = big[5000 + 200 * k:5200 + 200 * k]
        h = seed_hashes(lonely)
        if h[0] not in h[1:]:
            break
        k += 1
    cases.append(("window 0 alone in its slot", lonely, 0))
    cases.append(("four symbols", rng.integers(0, 4, 5000, dtype=np.uint8).tobytes(), 5))
    return cases


# ----------------------------------------------------------------------------------------------------------- lzf_copy_ranges
COPY_LAUNCH = 65535                # ranges per launch of lzf_copy_ranges_kernel (grid.y: capi.hip)
COPY_N = 2 * COPY_LAUNCH + 3
COPY_SMALL = (0, 1, 15, 16, 17, 33)
COPY_BIG = {0: 65535, COPY_LAUNCH - 1: 65536, COPY_LAUNCH: 65537, COPY_LAUNCH + 1: 65535, COPY_N - 1: 65537}
COPY_MAX_LEN = 65537


@functools.lru_cache(maxsize=None)
def copy_case():
    """One call of three launches: COPY_SMALL in turn, source residues that turn once per round of lengths and destination residues with period 17, and a
    range of 64 KiB - 1, 64 KiB or 64 KiB + 1 (two pieces with max_len COPY_MAX_LEN) first and last in the call and on both sides of
    the first relaunch.  About 2.1 MB copied, inside arenas of 5 MB.  Returns src bytes, the ranges' (source offset, destination offset, length) as three arrays
    and the size of the destination."""
    lens = np.array([COPY_BIG.get(i, COPY_SMALL[i % len(COPY_SMALL)]) for i in range(COPY_N)], dtype=np.int64)
    i = np.arange(COPY_N, dtype=np.int64)
    slot = (lens + 16 + 15) // 16 * 16                   # a byte or more between two ranges, whatever their residues
    base = np.concatenate(([0], np.cumsum(slot)[:-1])) + 16
    so, do = base + (i // len(COPY_SMALL)) % 16, base + (i % 17) % 16      # (every length meets every residue: 6 and 17 share no factor)
    total = int(base[-1] + slot[-1] + 32)
    src = np.random.default_rng(3501).integers(0, 256, total, dtype=np.uint8)
    return dict(src=src, so=so, do=do, lens=lens, total=total)


def copy_expect(case):
    exp = np.full(case["total"], OUT_POISON, dtype=np.uint8)
    src = case["src"]
    for a, b, n in zip(case["so"].tolist(), case["do"].tolist(), case["lens"].tolist()):
        exp[b:b + n] = src[a:a + n]
    return exp
