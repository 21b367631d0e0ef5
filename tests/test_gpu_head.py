"""GPU tests (-m gpu) of lzf_decompress_head_batch / _host: the head of every job's block, out_cap being the target.  Held to
head_cases.py's expectations (the oracle's decode cut at the target): status, out_len and the bytes of out[existing, out_len), with
every other byte of every arena unchanged; on one job array the call is also compared with lzf_decompressed_size_batch and
lzf_decompress_batch.  Damaged inputs here are data errors that end in a status."""
import ctypes as C

import numpy as np
import pytest
import torch

import head_cases as cases
import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ZONE = 4096


@pytest.fixture(scope="module")
def rows():
    r = cases.all_cases()
    cases.assert_covers(r)
    return r


def _arena(blobs, poison, residues=None, gap=64):
    """The blobs in one device tensor, each at a 256-aligned place + its residue, at least `gap` bytes of `poison` around each:
    (tensor, offsets, host copy)."""
    residues = residues if residues is not None else [0] * len(blobs)
    offs, at = [], 256
    for b, r in zip(blobs, residues):
        offs.append(at + r)
        at = (at + r + len(b) + gap + 255) // 256 * 256
    h = np.full(at + 256, poison, dtype=np.uint8)
    for b, a in zip(blobs, offs):
        h[a:a + len(b)] = np.frombuffer(b, dtype=np.uint8)
    t = torch.from_numpy(h).to(DEV)
    assert t.data_ptr() % 256 == 0
    return t, np.array(offs, dtype=np.uint64), h


def build_jobs(cs, poison=0xA5, residues=None, which=None):
    """The job array of the cases: inputs and prefixes in two arenas, every job's `out` — existing output, then room(c) bytes of poison —
    in a third, poison around each.  residues: per job (input, prefix, out) byte offsets from a 256-aligned address.  which: the jobs
    are cs[which[i]], ALIASING the inputs and prefixes of cs; every job has an `out` of its own.  A prefix_len without prefix bytes
    (LZF_CONTRACT) gets a NULL prefix; a job with an origin points `out` that far in front of its memory (never touched there)."""
    aliased = which is not None
    which = [int(k) for k in which] if aliased else list(range(len(cs)))
    res = residues or [(0, 0, 0)] * len(which)
    assert not (aliased and residues)
    d_in, in_off, _ = _arena([c["input"] for c in cs], poison, None if aliased else [r[0] for r in res])
    d_pre, pre_off, _ = _arena([c["prefix"] for c in cs], poison, None if aliased else [r[1] for r in res])
    js = [cs[k] for k in which]
    rooms = [cases.room(c) for c in js]
    d_out, out_off, h_out = _arena([c["existing"] + bytes([poison]) * rm for c, rm in zip(js, rooms)], poison, [r[2] for r in res])
    j = np.zeros(len(js), dtype=device.DJOB)
    j["input"] = np.uint64(d_in.data_ptr()) + in_off[which]
    j["input_len"] = [len(c["input"]) for c in js]
    j["prefix"] = [int(d_pre.data_ptr()) + int(pre_off[k]) if cs[k]["prefix_len"] == len(cs[k]["prefix"]) else 0 for k in which]
    j["prefix_len"] = [c["prefix_len"] for c in js]
    j["out"] = [int(d_out.data_ptr()) + int(a) - c["origin"] for c, a in zip(js, out_off)]
    j["out_existing_len"] = [c["origin"] + len(c["existing"]) for c in js]
    j["out_cap"] = [min(c["origin"] + c["target"], (1 << 64) - 1) for c in js]
    j["output_limit"] = [c["origin"] + c["limit"] for c in js]
    return j, (d_in, d_pre, d_out), (out_off, h_out, rooms)


def run_head(j, stream=None, long_history=False):
    n = len(j)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    d_j = device.to_device(j, DEV)
    keep = (device.decompress_head_batch_long_history if long_history else device.decompress_head_batch)(d_j, d_res, n, stream=stream)
    (stream or torch.cuda.current_stream()).synchronize()
    del keep
    return device.results_to_host(d_res, n)


def check(js, exps, res, d_out, layout, what=""):
    """Status, out_len and bytes of every job; and the whole `out` arena against its picture before the call with the expected bytes
    put in: everything outside [existing, out_len) is unchanged — below the existing output, [out_len, out_cap), the poison behind.
    Where a codec status is expected the room in front of the target is unspecified and left out of the comparison."""
    out_off, h_out, rooms = layout
    got = d_out.cpu().numpy()
    want = h_out.copy()
    bad = []
    for i, (c, e) in enumerate(zip(js, exps)):
        st, ln = int(res["status"][i]), int(res["out_len"][i]) - c["origin"]
        a, ex = int(out_off[i]), len(c["existing"])
        if st != e[0] or (e[0] == 0 and ln != e[1]):
            bad.append((what, c["name"], (st, ln), e[:2]))
            continue
        if e[0] == 0:
            want[a + ex:a + ex + len(e[2])] = np.frombuffer(e[2], dtype=np.uint8)
        else:
            want[a + ex:a + ex + rooms[i]] = got[a + ex:a + ex + rooms[i]]
    assert not bad, bad[:10]
    if not np.array_equal(got, want):
        d = np.flatnonzero(got != want)
        i = int(np.searchsorted(out_off, d[0], side="right")) - 1
        raise AssertionError((what, js[i]["name"], "byte", int(d[0]) - int(out_off[i]), "of out", int(got[d[0]]), "expected", int(want[d[0]]), len(d), "bytes differ"))


@pytest.mark.parametrize("poison", [0xA5, 0x5A])
def test_every_case_by_the_device_call_with_red_zones(rows, poison):
    """Every case in one call, two poisons: status, length, bytes; nothing outside [existing, out_len) of any `out`, no input, no
    prefix, not the job array and nothing around the results is written."""
    cs, exp = [c for c, _ in rows], [e for _, e in rows]
    n = len(cs)
    j, keep, layout = build_jobs(cs, poison=poison)
    before = [t.clone() for t in keep[:2]]
    resbuf = torch.full((2 * ZONE + 16 * n,), poison, dtype=torch.uint8, device=DEV)
    d_j = device.to_device(j, DEV)
    device.decompress_head_batch(d_j, resbuf[ZONE:ZONE + 16 * n], n)
    torch.cuda.synchronize()
    check(cs, exp, device.results_to_host(resbuf[ZONE:ZONE + 16 * n].clone(), n), keep[2], layout)
    assert torch.equal(before[0], keep[0]) and torch.equal(before[1], keep[1]), "the call wrote to an input or a prefix"
    assert bool((resbuf[:ZONE] == poison).all()) and bool((resbuf[ZONE + 16 * n:] == poison).all()), "red zone around the results"
    assert np.array_equal(d_j.cpu().numpy(), np.ascontiguousarray(j).view(np.uint8).reshape(-1)), "the job array was written to"


def test_every_case_by_the_host_call(rows):
    """Every case through lzf_decompress_head_batch_host in one call, held to the same expectations; of each job's host `out` nothing
    but [existing, out_len) changes.  Class (i) stays out: its lengths have no buffers (a NULL with a length is refused outright), and
    existing output at the contract is what the host call trims away.  Class (j) runs as it is: the host call stages the last
    65 535 bytes of the history, so the memory handed in starts that far in front of the existing output."""
    some = [(c, e) for c, e in rows if c["cls"] != "i"]
    n = len(some)
    jobs, res, keep = (ffi.DecompressJob * n)(), (ffi.JobResult * n)(), []
    PAD, POISON = 65535, 0x3C
    for i, (c, _) in enumerate(some):
        ex, rm = len(c["existing"]), cases.room(c)
        pad = PAD if c["origin"] else 0
        ob = C.create_string_buffer(bytes(pad) + c["existing"] + bytes([POISON]) * (rm + 64), pad + ex + rm + 64)
        keep.append((c["input"], c["prefix"], ob, pad))
        jobs[i].input = ffi._bytes_address(c["input"]); jobs[i].input_len = len(c["input"])
        jobs[i].prefix = ffi._bytes_address(c["prefix"]); jobs[i].prefix_len = c["prefix_len"]
        jobs[i].out = C.addressof(ob) + pad - c["origin"]
        jobs[i].out_existing_len = c["origin"] + ex
        jobs[i].out_cap = min(c["origin"] + c["target"], (1 << 64) - 1)
        jobs[i].output_limit = c["origin"] + c["limit"]
    ffi.check(ffi.lib().lzf_decompress_head_batch_host(jobs, res, n))
    bad = []
    for i, (c, e) in enumerate(some):
        ob, pad = keep[i][2], keep[i][3]
        raw, ex, rm = ob.raw[pad:], len(c["existing"]), cases.room(c)
        st, ln = res[i].status, res[i].out_len - c["origin"]
        if st != e[0] or (st == 0 and (ln != e[1] or raw[ex:ln] != e[2])):
            bad.append((c["name"], (st, ln), e[:2]))
        keep_from = max(ln, ex) if st == 0 else ex + rm
        if raw[:ex] != c["existing"] or raw[keep_from:] != bytes([POISON]) * (ex + rm + 64 - keep_from):
            bad.append((c["name"], "bytes outside [existing, out_len) changed"))
    assert not bad, bad[:10]
    got = ffi.block_heads_host([dict(input=c["input"], prefix=c["prefix"], existing=c["existing"], nbytes=c["target"] - len(c["existing"]), limit=c["limit"])
                                for c, _ in some[:40] if c["target"] < cases.FAR])
    want = [(e[0], e[1] if e[0] == 0 else None, e[2] if e[0] == 0 else b"") for c, e in some[:40] if c["target"] < cases.FAR]
    assert [(s, l if s == 0 else None, b) for s, l, b in got] == want


def _aligned_cases(rows):
    """Classes (a) and (b): one case per block and kind, each at 16 targets in a row (every residue of the target relative to out)."""
    seen, out = set(), []
    for c, _ in rows:
        if c["cls"] not in "ab" or (c["input"], c["sub"]) in seen or len(c["input"]) > 700:
            continue
        seen.add((c["input"], c["sub"]))
        ex = len(c["existing"])
        end = cases.ref_walk(c["input"], c["prefix_len"], ex, c["limit"])[1]
        base = max(ex + 1, min(c["target"], end - 16))
        out += [dict(c, name=f"{c['name']} -> {base + r}", target=base + r) for r in range(16)]
    return out


def test_alignment_of_out_input_prefix_and_target(rows):
    """Classes (a) and (b): `out` at all 16 address residues and the target at all 16 residues relative to out (every pair), input and
    prefix at residues 0, 1, 3 and 15."""
    base = _aligned_cases(rows)
    assert len(base) >= 16 * 40 and {c["cls"] for c in base} == {"a", "b"} and {"own-lane", "wave-wide", "apart", "prefix into out", "overlap 1", "overlap 3", "overlap 8"} <= {c["sub"] for c in base}
    cs, res = [], []
    for k, c in enumerate(base):
        for ro in range(16):
            cs.append(c); res.append(((0, 1, 3, 15)[(k + ro) % 4], (0, 1, 3, 15)[(k // 4 + ro // 4) % 4], ro))
    exp = [e for e in map(cases.expect, base) for _ in range(16)]
    j, keep, layout = build_jobs(cs, poison=0xEE, residues=res)
    assert {int(x) % 16 for x in j["out"]} == set(range(16)) and {int(x) % 16 for x in j["input"]} == {0, 1, 3, 15} == {int(x) % 16 for x in j["prefix"] if x}
    assert {(int(a) % 16, int(t) % 16) for a, t in zip(j["out"], j["out_cap"])} == {(a, t) for a in range(16) for t in range(16)}
    check(cs, exp, run_head(j), keep[2], layout)


def test_agreement_with_the_size_call_and_the_decoder_on_one_job_array(rows):
    """One job array, three calls.  Where the target is at or beyond the size call's out_len the head call's status is the size call's
    (and a block the size call fails is failed by the head call at a target far past it); on clean jobs the bytes are the first
    out_cap - existing bytes lzf_decompress_batch writes."""
    some = [(c, e) for c, e in rows if c["origin"] == 0 and c["prefix_len"] == len(c["prefix"])]
    cs, exp = [c for c, _ in some], [e for _, e in some]
    n = len(cs)
    j, keep, layout = build_jobs(cs)
    head = run_head(j)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    device.decompressed_size_batch(device.to_device(j, DEV), d_res, n, max_input_len=max(len(c["input"]) for c in cs))
    torch.cuda.synchronize()
    size = device.results_to_host(d_res, n)
    seen = 0
    for i, c in enumerate(cs):
        ss, sl = int(size["status"][i]), int(size["out_len"][i])
        if (ss == 0 and c["target"] >= sl) or (ss != 0 and c["target"] >= cases.FAR):
            assert int(head["status"][i]) == ss, c["name"]
            assert ss != 0 or int(head["out_len"][i]) == max(sl, 0), c["name"]
            seen += 1
    assert seen >= 30
    # the decoder, into fresh memory with room for the whole block
    clean = [i for i in range(n) if int(size["status"][i]) == 0 and cs[i]["target"] > len(cs[i]["existing"])]
    caps = [int(size["out_len"][i]) + 64 for i in clean]
    offs = np.cumsum([0] + [(cap + 255) // 256 * 256 for cap in caps])
    h = np.zeros(int(offs[-1]), dtype=np.uint8)
    for i, a in zip(clean, offs):
        h[a:a + len(cs[i]["existing"])] = np.frombuffer(cs[i]["existing"], dtype=np.uint8)
    d_dec = torch.from_numpy(h).to(DEV)
    jd = j[clean].copy()
    jd["out"] = np.uint64(d_dec.data_ptr()) + offs[:-1].astype(np.uint64)
    jd["out_cap"] = caps
    r_dec = torch.zeros(len(clean) * 16, dtype=torch.uint8, device=DEV)
    device.decompress_batch(device.to_device(jd, DEV), r_dec, len(clean))
    torch.cuda.synchronize()
    rd = device.results_to_host(r_dec, len(clean))
    d_out, out_off = keep[2], layout[0]
    for k, i in enumerate(clean):
        c, ex = cs[i], len(cs[i]["existing"])
        assert int(rd["status"][k]) == 0 and int(head["status"][i]) == 0, c["name"]
        ln = int(head["out_len"][i])
        assert ln == min(int(rd["out_len"][k]), c["target"]), c["name"]
        a, b = int(offs[k]), int(out_off[i])
        assert torch.equal(d_dec[a + ex:a + ln], d_out[b + ex:b + ln]), c["name"]


def test_more_jobs_than_the_device_holds_at_once_on_two_streams(rows):
    """6 000 jobs aliasing a few dozen small blocks at mixed targets, every job with an `out` of its own: the ticket past one
    residency of workgroups, every result in its own place — on the current stream and on a stream of its own."""
    small = [(c, e) for c, e in rows if c["origin"] == 0 and c["prefix_len"] == len(c["prefix"]) and cases.room(c) <= 600 and len(c["input"]) <= 4000]
    clean = [x for x in small if x[1][0] == 0]
    pick = [x for st in (1, 2, 3, 4) for x in [y for y in small if y[1][0] == st][:5]] + clean[::max(1, len(clean) // 24)][:24]
    assert len(pick) >= 36 and {e[0] for _, e in pick} >= {0, 1, 2, 3, 4}
    cs, exp = [c for c, _ in pick], [e for _, e in pick]
    which = np.random.default_rng(6000).integers(0, len(cs), 6000)
    js, ex_js = [cs[k] for k in which], [exp[k] for k in which]
    for stream in (None, torch.cuda.Stream(device=DEV)):
        j, keep, layout = build_jobs(cs, which=which)
        assert len(set(j["input"].tolist())) <= len(cs) and len(set(j["out"].tolist())) == 6000
        torch.cuda.synchronize()
        check(js, ex_js, run_head(j, stream=stream), keep[2], layout, what="own stream" if stream else "current stream")


def test_long_history_directly_and_through_trim_and_restore(rows):
    """Class (j): more than 1 GiB of existing output, stated over its tail — by the call itself (64-bit positions) and through
    lzf_history_trim_batch / lzf_history_restore_batch, which move the target with the origin; out_len comes back absolute."""
    some = [(c, e) for c, e in rows if c["cls"] == "j"]
    cs, exp = [c for c, _ in some], [e for _, e in some]
    for long_history in (False, True):
        j, keep, layout = build_jobs(cs)
        check(cs, exp, run_head(j, long_history=long_history), keep[2], layout, what=f"long_history={long_history}")


def test_block_heads():
    """device.block_heads: 64-byte heads of blocks that decode to more, to less and to nothing; a dictionary as prefix; on a stream."""
    text = synth.gen_text_zipf(71, 40_000).tobytes()
    plains = [text[:5000], text[5000:5040], b"", text[6000:6064], text[7000:7065], text[8000:30_000]]
    blocks = [torch.from_numpy(np.frombuffer(o.compress2(p)[1], dtype=np.uint8).copy()).to(DEV) for p in plains]
    heads, lens, statuses = device.block_heads(blocks, 64)
    torch.cuda.synchronize()
    assert heads.shape == (len(plains), 64) and statuses.tolist() == [0] * len(plains)
    assert lens.tolist() == [min(64, len(p)) for p in plains]
    for row, p in zip(heads.cpu().numpy(), plains):
        assert row.tobytes() == p[:64] + bytes(64 - min(64, len(p)))
    dic = text[30_000:40_000]
    raw = [cases.seq(b"ab", 2 + 500, 70) + cases.seq(b"x", None, 0), cases.seq(b"", 10, 90) + cases.seq(text[:50], 3, 9) + cases.seq(b"", None, 0)]
    payloads = [o.decompress_raw(b, prefix=dic, existing=b"", limit=1 << 20, cap=1 << 12)[1] for b in raw]
    assert all(len(p) > 64 for p in payloads) and payloads[0][:2] == b"ab" and payloads[0][2:64] == dic[-500:-438]
    blocks = [torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(DEV) for b in raw]
    d_dic = torch.from_numpy(np.frombuffer(dic, dtype=np.uint8).copy()).to(DEV)
    s = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    heads, lens, statuses = device.block_heads(blocks, 64, prefix=d_dic, stream=s)
    s.synchronize()
    assert statuses.tolist() == [0, 0] and lens.tolist() == [64, 64]
    assert [r.tobytes() for r in heads.cpu().numpy()] == [p[:64] for p in payloads]
    # without the dictionary the second block's first match reaches in front of out[0]: a status, not a head
    heads, lens, statuses = device.block_heads(blocks[1:], 64)
    torch.cuda.synchronize()
    assert statuses.tolist() == [ffi.INVALID_DEDUP_OFFSET]
    assert device.block_heads([], 64)[0].shape == (0, 64)
