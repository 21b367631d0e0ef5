"""CPU test (no GPU) of the frame layer's one compress plan, lzf_frame_jobs::compress_plan and fill_compress_job
(rust-lz-fear_amd/csrc/frame_jobs.h), compiled here with g++: both compress drivers (lzf_frame_compress_many and
lzf_frame_compress_device_many) take their jobs from it.  Held to a Python model written from the block loop of
src/framed/compress.rs:217-275, not from the C++:

  in_buffer starts as the dictionary (:217-218).  Every round reads up to block_size bytes behind it (:227); compress2 runs over
  the whole in_buffer from window_offset = its length before the read (:222,:243) into out_buffer[..read_bytes] (:242).  With
  independent blocks in_buffer goes back to the dictionary and the table to the template's clone (:265-270); otherwise, once
  in_buffer is longer than WINDOW_SIZE, the excess is drained from its front and the table is offset by as much (:271-275).

The plan states where in_buffer stands in S = dict ++ data as [lo, lo + hist + n): for linked blocks lo is everything drained
so far; for independent blocks the header's convention is S = dict ++ this block (lo = 0) with a dictionary and S = data
(lo = the block's offset) without.  Launch order is the drivers': independent blocks in frame order in one step, linked streams
in lock-step — block k of every stream that has one in step k — with the table offset of block k due before step k."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BS = 65536
WINDOW_SIZE = 64 * 1024                 # src/framed/mod.rs:20
LZF_OK, NOT_OK = 0, -7                  # any status but LZF_OK keeps a frame out
LZF_TABLE_U32, LZF_CJOB_TABLE_READONLY = 0, 1


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cplan") / "libemu_compress_plan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(HERE, "emu", "emu_compress_plan.cpp")])
    L = C.CDLL(so)
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.lzf_emu_compress_plan.restype = C.c_int64
    L.lzf_emu_compress_plan.argtypes = [C.c_uint32, u64p, C.POINTER(C.c_int32), C.c_uint64, C.c_uint64, C.c_int, u64p, u64p, u32p, u64p]
    L.lzf_emu_compress_plan_steps.argtypes = [u64p]
    L.lzf_emu_compress_plan_frames.argtypes = [u64p, u64p]
    L.lzf_emu_compress_plan_job.argtypes = [C.c_uint64, u64p]

    def run(in_len, part, bs, dict_len, indep):
        n = len(in_len)
        lens = (C.c_uint64 * max(n, 1))(*in_len)
        st = (C.c_int32 * max(n, 1))(*[LZF_OK if p else NOT_OK for p in part])
        n_steps, max_nb, slots, n_linked = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        nj = L.lzf_emu_compress_plan(n, lens, st, bs, dict_len, int(indep), C.byref(n_steps), C.byref(max_nb), C.byref(n_linked), C.byref(slots))
        assert nj >= 0
        step_off = (C.c_uint64 * (n_steps.value + 1))()
        L.lzf_emu_compress_plan_steps(step_off)
        nb, job_of = (C.c_uint64 * max(n, 1))(), (C.c_uint64 * max(nj, 1))()
        L.lzf_emu_compress_plan_frames(nb, job_of)
        jobs = []
        for q in range(nj):
            w = (C.c_uint64 * 15)()
            L.lzf_emu_compress_plan_job(q, w)
            jobs.append(dict(zip(("frame", "block", "off", "n", "lo", "hist", "add", "slot", "table",
                                  "input_len", "cursor", "out_cap", "table_kind", "flags_ro", "flags_rw"), list(w))))
        return dict(jobs=jobs, step_off=list(step_off), nb=list(nb)[:n], job_of=list(job_of)[:nj], max_nb=max_nb.value,
                    n_linked=n_linked.value, slots=slots.value)
    return run


def model_blocks(in_len, bs, dict_len, indep):
    """compress.rs:217-275 for one input, as positions in S = dict ++ data: per block (off, n, lo, hist, add, input_len, cursor,
    out_cap), add = what table.offset() got since the block before."""
    out = []
    drained, buf_len = 0, dict_len              # in_buffer = S[drained, drained + buf_len)  (:217-218)
    off, add = 0, 0
    while True:
        window_offset = buf_len                 # :222
        n = min(bs, in_len - off)               # :227
        if n == 0:                              # :229
            break
        buf_len += n
        lo = (0 if dict_len else off) if indep else drained
        out.append(dict(off=off, n=n, lo=lo, hist=window_offset, add=add, input_len=buf_len, cursor=window_offset, out_cap=n))   # :242-243
        off += n
        add = 0
        if indep:
            buf_len = dict_len                  # :267-268
        elif buf_len > WINDOW_SIZE:             # :271-274
            add = buf_len - WINDOW_SIZE
            drained += add; buf_len = WINDOW_SIZE
    return out


def model_plan(in_len, part, bs, dict_len, indep):
    frames = [model_blocks(n, bs, dict_len, indep) if p else [] for n, p in zip(in_len, part)]
    table, linked = {}, 0
    for f, blocks in enumerate(frames):
        if blocks and not indep:
            table[f] = linked; linked += 1
    order = []
    if indep:
        order = [(f, k) for f, blocks in enumerate(frames) for k in range(len(blocks))]
        step_off = [0, len(order)]
    else:
        step_off = []
        for k in range(max([len(b) for b in frames], default=0)):
            step_off.append(len(order))
            order += [(f, k) for f, blocks in enumerate(frames) if k < len(blocks)]
        step_off.append(len(order))
    jobs, slot = [], 0
    for f, k in order:
        jobs.append(dict(frames[f][k], frame=f, block=k, slot=slot, table=table.get(f, 0)))
        slot += frames[f][k]["n"]
    return dict(jobs=jobs, step_off=step_off, nb=[len(b) for b in frames], n_linked=linked, slots=slot)


def check(plan, in_len, part, dict_len, indep, bs=BS):
    got, want = plan(in_len, part, bs, dict_len, indep), model_plan(in_len, part, bs, dict_len, indep)
    assert got["nb"] == want["nb"]
    assert got["step_off"] == want["step_off"]
    assert got["max_nb"] == max(want["nb"], default=0) and got["n_linked"] == want["n_linked"] and got["slots"] == want["slots"]
    assert len(got["jobs"]) == len(want["jobs"])
    for q, (g, w) in enumerate(zip(got["jobs"], want["jobs"])):
        for key in ("frame", "block", "off", "n", "lo", "hist", "slot", "input_len", "cursor", "out_cap"):
            assert g[key] == w[key], (q, key, g, w)
        if not indep:
            assert g["table"] == w["table"] and g["add"] == w["add"], (q, g, w)
        assert g["table_kind"] == LZF_TABLE_U32 and g["flags_ro"] == LZF_CJOB_TABLE_READONLY and g["flags_rw"] == 0
    # slots: the running sum of the blocks' lengths in job order
    at = 0
    for g in got["jobs"]:
        assert g["slot"] == at
        at += g["n"]
    # every frame's jobs in block order; a frame that takes no part has none
    at = 0
    for f, nb in enumerate(got["nb"]):
        assert nb == ((in_len[f] + bs - 1) // bs if part[f] else 0)
        for k in range(nb):
            j = got["jobs"][got["job_of"][at + k]]
            assert (j["frame"], j["block"]) == (f, k)
        at += nb
    assert at == len(got["jobs"])
    assert all(part[g["frame"]] for g in got["jobs"])
    return got


SIZES = [0, 1, BS, BS + 1, 3 * BS + 5]
MIXED = [3 * BS + 5, 0, BS + 1, 1, BS]
SETTINGS = [("independent", True, 0), ("independent, dictionary 100", True, 100), ("linked", False, 0),
            ("linked, dictionary 4", False, 4), ("linked, dictionary 100", False, 100)]


@pytest.mark.parametrize("name,indep,dict_len", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_compress_plan_against_model(plan, name, indep, dict_len):
    for sizes in (SIZES, MIXED):
        got = check(plan, sizes, [True] * len(sizes), dict_len, indep)
        assert len(got["jobs"]) == 8                                   # 0 + 1 + 1 + 2 + 4 blocks
    # one frame that takes no part between frames that do: no job, no table, no slot — and the others as without it
    sizes, part = [BS + 1, 3 * BS + 5, 1, 3 * BS + 5, 0, BS], [True, False, True, True, True, True]
    got = check(plan, sizes, part, dict_len, indep)
    assert got["nb"][1] == 0 and len(got["jobs"]) == 8
    without = check(plan, [n for n, p in zip(sizes, part) if p], [True] * 5, dict_len, indep)
    renumber = {0: 0, 2: 1, 3: 2, 4: 3, 5: 4}
    assert [dict(g, frame=renumber[g["frame"]]) for g in got["jobs"]] == without["jobs"] and got["step_off"] == without["step_off"]


def test_compress_plan_linked_steps_and_forgetting(plan):
    """Spelled out for the mixed order, linked, no dictionary: four steps with gaps, and the window of the 3 * bs + 5 input
    forgets a whole block from block 2 on."""
    got = check(plan, MIXED, [True] * 5, 0, False)
    assert got["step_off"] == [0, 4, 6, 7, 8]
    assert [(g["frame"], g["block"]) for g in got["jobs"]] == [(0, 0), (2, 0), (3, 0), (4, 0), (0, 1), (2, 1), (0, 2), (0, 3)]
    assert [g["table"] for g in got["jobs"]] == [0, 1, 2, 3, 0, 1, 0, 0] and got["n_linked"] == 4
    big = [g for g in got["jobs"] if g["frame"] == 0]
    assert [(g["lo"], g["hist"], g["add"]) for g in big] == [(0, 0, 0), (0, BS, 0), (BS, BS, BS), (2 * BS, BS, BS)]
    # with a 100-byte dictionary the window is over 64 KiB after block 0 already: block 1 forgets the dictionary
    got = check(plan, [3 * BS + 5], [True], 100, False)
    assert [(g["lo"], g["hist"], g["add"]) for g in got["jobs"]] == [(0, 100, 0), (100, BS, 100), (100 + BS, BS, BS), (100 + 2 * BS, BS, BS)]


def test_compress_plan_nothing_to_do(plan):
    for indep in (True, False):
        for sizes, part in (([], []), ([0, 0], [True, True]), ([5, BS], [False, False])):
            got = check(plan, sizes, part, 100, indep)
            assert got["jobs"] == [] and got["slots"] == 0 and got["n_linked"] == 0
