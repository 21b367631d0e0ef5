"""Decode jobs and linked-block frames with more history than the decode kernels' 31-bit positions hold (-m gpu).

raw          jobs whose existing output ends at 1 GiB, on both sides of 2 GiB - 256, past 2 GiB and past 4 GiB inside one real buffer of
             4 GiB + 64 MiB that is never filled: only the 64 KiB below each job's end are written.  The blocks are built against exactly
             that history.  Trim -> lzf_decompress_batch_sized -> restore (pair kernel and segmented pipeline), the size call the same way,
             and lzf_decompress_batch_host over host copies of the tails give the oracle's status, its out_len + (E - 65536) and its bytes;
             nothing is written outside [E, E + room) of a job.
             (Status 4, InvalidDeduplicationOffset, cannot occur here: an offset is below 65 536 and every job has that much history.)
chain_step   lzf_chain_decompress_step_trimmed, the frame layer's step, against the frame reader's model on lengths on both sides of
             2^30: below it the jobs are lzf_chain_decompress_step's (`out` untouched), from it on the trimmed ones, and the finish adds
             the shift back.  lzf_chain_decompress_step itself, on the same streams with absolute results, writes what it always wrote.
linked_frame one hand-built linked-block frame of 516 blocks of 4 MiB block size — 513 blocks of a period-251 pattern, 4 MiB each, then
             three blocks whose payload (a match at offset 65 535, then 1 MiB of compressed corpus) is large enough for the segmented
             pipeline — 2 055 MiB of content, across 2^30, 2 GiB - 256 and 2^31, through every frame driver; the expectation is the
             oracle's lzfo_frame_decompress of the same bytes, built once and compared on the device."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import oracle_ffi as o
import aux_kernel_cases as K
import history_trim_cases as H
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi, framed, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MiB = 1 << 20
KEEP = 65536
ZONE = 4096
POISON = 0xA5
NO_LIMIT = (1 << 63) - 1
BASES = (1 << 30, 0x7FFFFF00 - 1, 0x7FFFFF00, (1 << 31) + 7, (1 << 32) + 12345)
N_SLOTS = 8
ENDS = tuple(BASES[i % 5] + i * 8 * MiB for i in range(N_SLOTS))           # E_i: no job's output meets another job's history
BIG = (4 << 30) + 64 * MiB


def _timed(name, t0):
    print(f"[long history] {name}: {time.time() - t0:.2f} s")


@pytest.fixture(scope="module")
def big():
    """The buffer every raw job decodes into (`out` = its base), with the 64 KiB below every E_i written and poison around them."""
    torch.cuda.set_device(0)
    buf = torch.empty(BIG, dtype=torch.uint8, device=DEV)
    hist = [synth.silesia_mix((3 + i) * MiB, (3 + i) * MiB + KEEP).tobytes() for i in range(N_SLOTS)]
    for E, h in zip(ENDS, hist):
        assert E + 7 * MiB < BIG
        buf[E - KEEP - ZONE:E + 7 * MiB].fill_(POISON)
        buf[E - KEEP:E].copy_(torch.frombuffer(bytearray(h), dtype=torch.uint8))
    torch.cuda.synchronize()
    return buf, hist


def _upload(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(DEV)


def _pair_blocks(hist):
    lit = bytes(range(65, 65 + 26))
    small = o.compress2(synth.silesia_mix(40 * MiB, 40 * MiB + 32768).tobytes())[1]
    items = [
        dict(name="deep offsets", block=H.seq(lit, 65535, 300) + H.seq(lit[:7], 65000, 40) + H.seq(b"tail!")),
        dict(name="a match that straddles E", block=H.seq(b"", 10, 100) + H.seq(b"ab", 50, 200) + H.seq(b"tail!")),
        dict(name="offset 1 from the first byte", block=H.seq(b"", 1, 5000) + H.seq(b"tail!")),
        dict(name="offset 65535 first, then a compressed block", block=H.seq(b"", 65535, 1000) + small),
        dict(name="truncated: UnexpectedEnd", block=(H.seq(lit, 65535, 40) + H.seq(b"0123456789"))[:-4], status=o.UNEXPECTED_END),
        dict(name="MemoryLimitExceeded at the second match", block=H.seq(lit, 65535, 20) + H.seq(b"xy", 3, 100) + H.seq(b"tail!"), limit=26 + 20 + 50,
             status=o.MEMORY_LIMIT_EXCEEDED),
        dict(name="zero offset", block=H.seq(lit, 0, 8) + H.seq(b"tail!"), status=o.ZERO_DEDUP_OFFSET),
        dict(name="a limit below the shift: MemoryLimitExceeded at the first match", block=H.seq(lit, 100, 8) + H.seq(b"tail!"), abs_limit=12345,
             status=o.MEMORY_LIMIT_EXCEEDED),
    ]
    assert len(items) == N_SLOTS and max(len(it["block"]) for it in items) < 65536
    return items


def _seg_blocks(hist):
    items = []
    for i in range(N_SLOTS):
        body = o.compress2(synth.silesia_mix((50 + 2 * i) * MiB, (51 + 2 * i) * MiB).tobytes())[1]
        block = H.seq(b"", 65535, 70000) + H.seq(b"", 10 + i, 100) + body
        it = dict(name=f"offset 65535 x 70000, straddle, 1 MiB compressed ({i})", block=block)
        if i == 6:
            it = dict(name="the same, truncated", block=block[:-3], status=o.UNEXPECTED_END)
        assert len(it["block"]) >= 65536
        items.append(it)
    return items


def _expect(items, hist):
    """Per job the oracle on the 64 KiB-history job: (status, absolute out_len, decoded bytes); and the job's absolute limit and room."""
    out = []
    for i, (it, h) in enumerate(zip(items, hist)):
        E = ENDS[i]
        limit = it.get("abs_limit", E + it["limit"] if "limit" in it else NO_LIMIT)
        rel = limit - (E - KEEP) if limit > E - KEEP else 0
        st, full = o.decompress_raw(it["block"], b"", h, rel, KEEP + 6 * MiB)
        assert st == it.get("status", o.OK), (it["name"], st)
        room = (len(full) - KEEP if st == o.OK else 2 * MiB) + len(it["block"]) + 64
        out.append(dict(status=st, out_len=len(full) + E - KEEP, data=full[KEEP:], limit=limit, room=room))
    return out


def _device_jobs(buf, items, exp):
    d_in = [_upload(it["block"]) for it in items]
    dj = np.zeros(len(items), dtype=device.DJOB)
    for i, (it, e) in enumerate(zip(items, exp)):
        dj[i] = (d_in[i].data_ptr(), len(it["block"]), 0, 0, buf.data_ptr(), ENDS[i], ENDS[i] + e["room"], e["limit"])
    return device.to_device(dj, DEV), d_in


def _reset(buf, exp):
    for E, e in zip(ENDS, exp):
        buf[E:E + e["room"] + ZONE].fill_(POISON)


def _check_memory(buf, hist, exp, what):
    for i, (E, h, e) in enumerate(zip(ENDS, hist, exp)):
        n = e["out_len"] - E if e["status"] == o.OK else 0
        if e["status"] == o.OK:
            got = buf[E:E + n].cpu().numpy().tobytes()
            assert got == e["data"], f"{what}: job {i}: decoded bytes differ from the oracle's"
            # behind the decoded bytes the room may hold scratch of the decode (literals run past the limit), never the zone behind it
        assert (buf[E + e["room"]:E + e["room"] + ZONE] == POISON).all().item(), f"{what}: job {i}: written behind out + out_cap"
        assert (buf[E - KEEP - ZONE:E - KEEP] == POISON).all().item(), f"{what}: job {i}: written in front of the history"
        assert buf[E - KEEP:E].cpu().numpy().tobytes() == h, f"{what}: job {i}: the history changed"


def _check_results(res, exp, what):
    for i, e in enumerate(exp):
        assert int(res["status"][i]) == e["status"], f"{what}: job {i}: status {res['status'][i]}, oracle {e['status']}"
        if e["status"] == o.OK:
            assert int(res["out_len"][i]) == e["out_len"], f"{what}: job {i}: out_len {res['out_len'][i]}, oracle {e['out_len']}"


def _raw_call(big, make_items, want_segmented):
    buf, hist = big
    items = make_items(hist)
    exp = _expect(items, hist)
    assert {e["status"] for e in exp} == ({0, 1} if want_segmented else {0, 1, 2, 3})
    n = len(items)
    max_in = max(len(it["block"]) for it in items)
    d_jobs, keep = _device_jobs(buf, items, exp)
    lib = ffi.lib()
    # the jobs as they are: out of the decoder's contract from 2 GiB - 256 on, and said so
    _reset(buf, exp)
    d_res = torch.zeros(n * device.RES.itemsize, dtype=torch.uint8, device=DEV)
    device.decompress_batch(d_jobs, d_res, n, max_input_len=max_in)
    torch.cuda.synchronize()
    plain = device.results_to_host(d_res, n)
    for i, E in enumerate(ENDS):
        if E >= 0x7FFFFF00:
            assert plain["status"][i] == ffi.CONTRACT, (i, plain["status"][i])
    # trim, decode, restore
    _reset(buf, exp)
    d_res.fill_(0x5A)
    t0 = time.time()
    d_trimmed, d_shift = device.decompress_batch_long_history(d_jobs, d_res, n, max_input_len=max_in)
    torch.cuda.synchronize()
    _timed(f"raw decode of {n} jobs ({'segmented' if want_segmented else 'pair'})", t0)
    launch = lib.lzf_last_decompress_launch().decode()
    assert launch.startswith("segmented") == want_segmented, launch
    shifts = d_shift.cpu().numpy().view(np.uint64)
    assert [int(s) for s in shifts] == [H.shift_of(E) for E in ENDS] and all(s % 16 == 0 and s > 0 for s in shifts)
    tj = d_trimmed.cpu().numpy().view(device.DJOB)
    assert ((tj["out"] & 15) == (buf.data_ptr() & 15)).all() and (tj["out_existing_len"] < KEEP + 16).all()
    _check_results(device.results_to_host(d_res, n), exp, "decode")
    _check_memory(buf, hist, exp, "decode")
    # the size call over the same jobs
    d_res.fill_(0x5A)
    device.decompressed_size_batch_long_history(d_jobs, d_res, n, max_input_len=max_in)
    torch.cuda.synchronize()
    _check_results(device.results_to_host(d_res, n), exp, "size")
    assert lib.lzf_history_trim_batch(d_jobs.data_ptr(), d_jobs.data_ptr(), d_shift.data_ptr(), n, None) == ffi.E_INVALID
    # the host entry points over host copies of the tails: `out` is where the Vec would begin, only its tail is there
    jobs = (ffi.DecompressJob * n)()
    res = (ffi.JobResult * n)()
    tails = []
    for i, (it, h, e) in enumerate(zip(items, hist, exp)):
        s = H.shift_of(ENDS[i])
        front = ENDS[i] - s - KEEP                                 # 0 .. 15 bytes of the kept history that no offset reaches
        tail = np.full(front + KEEP + e["room"] + ZONE, POISON, np.uint8)
        tail[front:front + KEEP] = np.frombuffer(h, np.uint8)
        tails.append(tail)
        jobs[i].input = ffi._bytes_address(it["block"]); jobs[i].input_len = len(it["block"])
        jobs[i].out = tail.ctypes.data - s
        jobs[i].out_existing_len = ENDS[i]; jobs[i].out_cap = ENDS[i] + e["room"]; jobs[i].output_limit = e["limit"]
    t0 = time.time()
    ffi.check(lib.lzf_decompress_batch_host(jobs, res, n))
    _timed(f"raw host decode of {n} jobs", t0)
    for i, (tail, h, e) in enumerate(zip(tails, hist, exp)):
        front = len(tail) - KEEP - e["room"] - ZONE
        assert res[i].status == e["status"], ("host", i, res[i].status)
        if e["status"] == o.OK:
            assert res[i].out_len == e["out_len"], ("host", i)
            assert tail[front + KEEP:front + KEEP + len(e["data"])].tobytes() == e["data"], ("host", i)
        assert tail[front:front + KEEP].tobytes() == h and (tail[:front] == POISON).all() and (tail[-ZONE:] == POISON).all(), ("host", i)
    sres = (ffi.JobResult * n)()
    ffi.check(lib.lzf_decompressed_size_batch_host(jobs, sres, n))
    for i, e in enumerate(exp):
        assert sres[i].status == e["status"] and (e["status"] != o.OK or sres[i].out_len == e["out_len"]), ("host size", i)
    del keep


def test_raw_jobs_through_the_pair_kernel(big):
    _raw_call(big, _pair_blocks, want_segmented=False)


def test_raw_jobs_through_the_segmented_pipeline(big):
    _raw_call(big, _seg_blocks, want_segmented=True)


# ------------------------------------------------------------------------------------------------------------------ chain_step
def test_chain_step_on_both_sides_of_one_gib(big):
    buf, _ = big
    NONE, BM = K.NONE, 4 * MiB
    T = H.THRESHOLD
    stored_at = ENDS[4] + 3 * MiB                                   # a stored block appended past 4 GiB, inside the big buffer
    streams = [                                                     # (length, dead, prev (status, absolute out_len) or None, job input_len or None, stored)
        (T - 1, 0, None, 777, 0), (T, 0, None, 778, 0), (T + 15, 0, None, 779, 0), (T + 16, 0, None, 780, 0),
        (0x7FFFFF00 - 1, 0, None, 16500, 0), (0x7FFFFF00, 0, None, 16501, 0), ((1 << 31) + 7, 0, None, 16502, 0), ((1 << 32) + 12345, 0, None, 70000, 0),
        (T - 100, 0, (0, T - 100 + 99), 31, 0),                     # finishes below the threshold
        (T - 100, 0, (0, T + 50), 32, 0),                           # grows across it: an untrimmed result, a trimmed job
        (1 << 31, 0, (0, (1 << 31) + BM), 33, 0),                   # trimmed result, grown by exactly block_maxsize: alive
        (1 << 31, 0, (0, (1 << 31) + BM + 1), 34, 0),               # ... by one more: dead, the job emptied
        ((1 << 32) + 5, 0, (3, 12345), 35, 0),                      # the job before failed
        ((1 << 33) + 1, 1, (0, (1 << 33) + 500), 36, 0),                        # dead on entry
        (stored_at - 1000, 0, (0, stored_at), None, 3000),          # a stored block behind a trimmed result: absolute, 64-bit
    ]
    n = len(streams)
    rng = np.random.default_rng(77)
    jobs = np.zeros(2 * n, dtype=K.DJOB)
    for f in K.DJOB.names:
        jobs[f] = rng.integers(1, 1 << 40, 2 * n, dtype=np.uint64)
    res = np.zeros(2 * n, dtype=K.RES)
    res["status"] = 7
    steps = np.zeros(n, dtype=K.STEP); state = np.zeros(n, dtype=K.STATE)
    stored_src = _upload(bytes(rng.integers(0, 256, 3000, dtype=np.uint8)))
    e_jobs, e_state = jobs.copy(), state.copy()
    for i, (length, dead, prev, job, stored) in enumerate(streams):
        steps[i] = (NONE, NONE, stored, stored_src.data_ptr() if stored else 0, buf.data_ptr() if stored else K.WILD_OUT + 16 * i, BM)
        state[i] = (length, dead, 0)
        if prev is not None:
            steps["prev_job"][i] = 2 * i
            # what the job made from `length` reports: counted from its shift
            res[2 * i] = (prev[1] - (H.shift_of(length) if prev[0] == 0 else 0), prev[0], 0)
        if job is not None:
            steps["job"][i] = 2 * i + 1
            jobs["input_len"][2 * i + 1] = job
    e_jobs = jobs.copy()
    for i, (length, dead, prev, job, stored) in enumerate(streams):
        nl, nd, fields, copy, _ = K.chain_model(length, dead, BM, prev, job, stored)
        e_state[i] = (nl, nd, 0)
        if fields is not None:
            k = 2 * i + 1
            t, s = H.trim(dict(out=int(steps["out"][i]), out_existing_len=fields[1], out_cap=fields[2], output_limit=fields[3]))
            assert (s > 0) == (fields[1] >= T)
            e_jobs["input_len"][k], e_jobs["out_existing_len"][k], e_jobs["out_cap"][k], e_jobs["output_limit"][k] = fields[0], t["out_existing_len"], t["out_cap"], t["output_limit"]
            if s:
                e_jobs["out"][k] = t["out"]
                assert t["out_existing_len"] < KEEP + 16 and t["output_limit"] == t["out_existing_len"] + BM
        if copy is not None:
            assert copy == (stored_at, 3000)
    assert [int(x) for x in e_state["dead"]] == [0] * 11 + [1, 1, 1, 0]
    assert int(e_jobs["out_existing_len"][1]) == T - 1 and int(e_jobs["out"][1]) == int(jobs["out"][1])          # below: as ever
    assert int(e_jobs["out_existing_len"][3]) == KEEP and int(e_jobs["out"][3]) == K.WILD_OUT + 16 + T - KEEP     # at 2^30: trimmed
    buf[stored_at - ZONE:stored_at + 3000 + ZONE].fill_(POISON)
    # the untrimmed step over the same streams, given the results as untrimmed jobs report them: the model as it is, at every length
    res_abs, u_jobs = res.copy(), jobs.copy()
    for i, (length, dead, prev, job, stored) in enumerate(streams):
        if prev is not None:
            res_abs["out_len"][2 * i] = prev[1]
        fields = K.chain_model(length, dead, BM, prev, job, stored)[2]
        if fields is not None:
            k = 2 * i + 1
            u_jobs["input_len"][k], u_jobs["out_existing_len"][k], u_jobs["out_cap"][k], u_jobs["output_limit"][k] = fields
    d = [device.to_device(a, DEV) for a in (steps, state, jobs, res_abs)]
    ffi.check(ffi.lib().lzf_chain_decompress_step(d[0].data_ptr(), d[1].data_ptr(), n, d[2].data_ptr(), d[3].data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert (d[1].cpu().numpy().view(K.STATE) == e_state).all() and (d[2].cpu().numpy().view(K.DJOB) == u_jobs).all()
    assert int(u_jobs["out_existing_len"][15]) == (1 << 32) + 12345 and int(u_jobs["out"][15]) == int(jobs["out"][15])
    buf[stored_at - ZONE:stored_at + 3000 + ZONE].fill_(POISON)
    d = [device.to_device(a, DEV) for a in (steps, state, jobs, res)]
    ffi.check(ffi.lib().lzf_chain_decompress_step_trimmed(d[0].data_ptr(), d[1].data_ptr(), n, d[2].data_ptr(), d[3].data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g_state, g_jobs = d[1].cpu().numpy().view(K.STATE), d[2].cpu().numpy().view(K.DJOB)
    for i in range(n):
        assert g_state[i] == e_state[i], (i, g_state[i], e_state[i])
        assert g_jobs[2 * i + 1] == e_jobs[2 * i + 1], (i, g_jobs[2 * i + 1], e_jobs[2 * i + 1])
    assert (g_jobs == e_jobs).all()
    assert torch.equal(buf[stored_at:stored_at + 3000], stored_src)
    assert (buf[stored_at - ZONE:stored_at] == POISON).all().item() and (buf[stored_at + 3000:stored_at + 3000 + ZONE] == POISON).all().item()


# ---------------------------------------------------------------------------------------------------------------- linked_frame
N_PERIODIC, N_BLOCKS, BM4 = 513, 516, 4 * MiB
F_INPUT_ERROR = 16


def _linked_frame():
    pat = bytes((37 * k + 11) % 256 for k in range(251))
    flg, bd = 0x40, 0x70                                               # version 01, linked blocks, no checksums, no content size; 4 MiB blocks
    parts = [b"\x04\x22\x4d\x18", bytes([flg, bd, (o.xxh32(bytes([flg, bd])) >> 8) & 0xFF])]
    sizes, starts = [], []

    def add(payload, n):
        assert len(payload) < BM4
        starts.append(sum(len(p) for p in parts) + 4)
        parts.append(len(payload).to_bytes(4, "little")); parts.append(payload); sizes.append(n)

    for k in range(N_PERIODIC):
        end = (k + 1) * BM4
        last5 = bytes(pat[(end - 5 + t) % 251] for t in range(5))
        if k == 0:
            add(H.seq(pat, 251, BM4 - 251 - 5) + H.seq(last5), BM4)
        else:
            add(H.seq(b"", 251, BM4 - 5) + H.seq(last5), BM4)           # a source in the block before
    for k in range(3):
        body = o.compress2(synth.silesia_mix((90 + k) * MiB, (91 + k) * MiB).tobytes())[1]
        payload = H.seq(b"", 65535, 70000) + body
        assert len(payload) >= 65536                                    # the segmented pipeline's window, with history past 2 GiB
        add(payload, 70000 + MiB)
    parts.append(b"\0\0\0\0")
    return b"".join(parts), sizes, starts


@pytest.fixture(scope="module")
def linked():
    torch.cuda.set_device(0)
    t0 = time.time()
    frame, sizes, starts = _linked_frame()
    total = sum(sizes)
    assert len(sizes) == N_BLOCKS and total > (1 << 31) + 4 * MiB and 16000 < starts[2] - starts[1] < 17500
    exp = np.empty(total + 4096, np.uint8)
    n, used = C.c_size_t(0), C.c_size_t(0)
    rc = o.lib().lzfo_frame_decompress(frame, len(frame), b"", 0, exp.ctypes.data, len(exp), C.byref(n), C.byref(used))
    assert (rc, n.value, used.value) == (0, total, len(frame))
    d_exp = torch.from_numpy(exp[:total]).to(DEV)
    d_frame = _upload(frame)
    _timed("linked frame and the oracle's expectation", t0)
    return dict(frame=frame, sizes=sizes, starts=starts, total=total, exp=exp[:total], d_exp=d_exp, d_frame=d_frame)


def test_linked_frame_decompress_frames_device(linked):
    t0 = time.time()
    (st, out, used), = framed.decompress_frames_device([linked["d_frame"]])
    _timed("decompress_frames_device", t0)
    assert (st, out.numel(), used) == (0, linked["total"], len(linked["frame"]))
    assert torch.equal(out, linked["d_exp"])


def test_linked_frame_sizes_and_block_index(linked):
    t0 = time.time()
    assert framed.decompressed_sizes_device([linked["d_frame"]]) == [(0, linked["total"], len(linked["frame"]))]
    _timed("decompressed_sizes_device", t0)
    t0 = time.time()
    ix, = framed.block_index_device([linked["d_frame"]])
    _timed("block_index_device", t0)
    assert (ix.status, ix.out_len, ix.consumed, len(ix.blocks)) == (0, linked["total"], len(linked["frame"]), N_BLOCKS)
    offs = np.concatenate(([0], np.cumsum(linked["sizes"])[:-1]))
    for k in range(N_BLOCKS - 10, N_BLOCKS):
        e = ix.blocks[k]
        assert (int(e["out_off"]), int(e["out_len"]), int(e["in_off"]), int(e["status"])) == (int(offs[k]), linked["sizes"][k], linked["starts"][k], 0), k
        assert int(e["flags"]) == ffi.FBLOCK_LINKED | ffi.FBLOCK_DELIVERED, k
    assert [int(x) for x in ix.blocks["out_off"]] == [int(x) for x in offs]


def test_linked_frame_in_a_stream_behind_it_a_small_frame(linked):
    content = synth.silesia_mix(7 * MiB, 7 * MiB + 50000).tobytes()
    rc, small = o.frame_compress(content)
    assert rc == 0
    d_stream = torch.cat([linked["d_frame"], _upload(small)])
    t0 = time.time()
    (st, out, used, nf), = framed.decompress_streams_device([d_stream])
    _timed("decompress_streams_device", t0)
    assert (st, out.numel(), used, nf) == (0, linked["total"] + len(content), d_stream.numel(), 2)
    assert torch.equal(out[:linked["total"]], linked["d_exp"]) and out[linked["total"]:].cpu().numpy().tobytes() == content


def test_linked_frame_over_host_buffers(linked):
    t0 = time.time()
    (st, out), = framed.decompress_frames([linked["frame"]], caps=[linked["total"] + 64])
    _timed("decompress_frames (host buffers)", t0)
    assert st == 0 and len(out) == linked["total"]
    assert np.array_equal(np.frombuffer(out, np.uint8), linked["exp"])


def test_linked_frame_truncated_inside_its_first_large_block(linked):
    cut = linked["starts"][N_PERIODIC] + 40000                           # inside the payload of the block behind the 513 periodic ones
    d_cut = linked["d_frame"][:cut].clone()
    want = N_PERIODIC * BM4
    t0 = time.time()
    (st, out, used), = framed.decompress_frames_device([d_cut])
    _timed("decompress_frames_device, truncated", t0)
    assert (st, out.numel()) == (F_INPUT_ERROR, want)
    assert torch.equal(out, linked["d_exp"][:want])
    (st, size, _), = framed.decompressed_sizes_device([d_cut])
    assert (st, size) == (F_INPUT_ERROR, want)
