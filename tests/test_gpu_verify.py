"""GPU tests (-m gpu) of lzf_decompress_verify_batch / _host: does a job decode to exactly the bytes its `out` holds — nothing decoded,
nothing but the results written.  Held to verify_cases.py's expectations (decode-then-compare by the oracle); on LZF_OK and on every
codec status the verdict is also compared with lzf_decompressed_size_batch on the same job array, and on a sample with
lzf_decompress_batch + torch.equal.  Damaged inputs here are data errors that end in a status."""
import numpy as np
import pytest
import torch

import verify_cases as cases
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ZONE = 4096
KERNEL = "lzf_verify_kernel<48,768>"
LATENCY = "latency: lzf_seg_parse_kernel + lzf_size_tile_kernel + lzf_verify_finish_kernel + lzf_verify_tile_kernel + " + KERNEL
CLASS_MAX_JOBS = 16 * 256         # the class: up to 16 jobs per CU (MI355X: 4 096) with an input bound of 64 KiB or more


@pytest.fixture(scope="module")
def rows():
    r = cases.block_cases()
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


def build_jobs(cs, poison=0, residues=None):
    """The job array of the cases: inputs, prefixes and `out` memories (history, expected bytes, what lies behind out_cap) in three
    arenas.  residues: per case (input, prefix, out) byte offsets from a 256-aligned address.  A prefix_len without prefix bytes (the
    LZF_CONTRACT case) gets a NULL prefix."""
    res = residues or [(0, 0, 0)] * len(cs)
    d_in, in_off, h_in = _arena([c["input"] for c in cs], poison, [r[0] for r in res])
    d_pre, pre_off, h_pre = _arena([c["prefix"] for c in cs], poison, [r[1] for r in res])
    d_out, out_off, h_out = _arena([c["mem"] for c in cs], poison, [r[2] for r in res])
    j = np.zeros(len(cs), dtype=device.DJOB)
    j["input"] = np.uint64(d_in.data_ptr()) + in_off
    j["input_len"] = [len(c["input"]) for c in cs]
    j["prefix"] = [int(d_pre.data_ptr()) + int(a) if c["prefix_len"] == len(c["prefix"]) else 0 for c, a in zip(cs, pre_off)]
    j["prefix_len"] = [c["prefix_len"] for c in cs]
    j["out"] = np.uint64(d_out.data_ptr()) + out_off
    j["out_existing_len"] = [c["existing_len"] for c in cs]
    j["out_cap"] = [c["out_cap"] for c in cs]
    j["output_limit"] = [c["limit"] for c in cs]
    return j, (d_in, d_pre, d_out), (h_in, h_pre, h_out)


def _tuples(res, with_len):
    return [(int(s), int(l) if s in with_len else None) for s, l in zip(res["status"], res["out_len"])]


def launch_by_rule(n, max_input_len):
    return LATENCY if n <= CLASS_MAX_JOBS and (max_input_len is None or max_input_len >= cases.CLASS_MIN_IN) else KERNEL


def run_verify(j, d_res=None, max_input_len=None, reserved=None):
    """The verdicts; the launch string is held to the rule either way: a class that declines silently fails here.  reserved (a list):
    filled with results[].reserved."""
    n = len(j)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=DEV) if d_res is None else d_res
    d_j = device.to_device(j, DEV)
    device.decompress_verify_batch(d_j, d_res, n, max_input_len=max_input_len)
    torch.cuda.synchronize()
    assert device.last_verify_launch() == launch_by_rule(n, max_input_len)
    res = device.results_to_host(d_res.clone(), n)
    if reserved is not None:
        reserved[:] = res["reserved"].tolist()
    return _tuples(res, (0, cases.MISMATCH))


def run_size(j):
    n = len(j)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    device.decompressed_size_batch(device.to_device(j, DEV), d_res, n)
    torch.cuda.synchronize()
    return _tuples(device.results_to_host(d_res, n), (0,))


def check(cs, exp, got, sizes=None):
    bad = [(c["name"], g, e) for c, e, g in zip(cs, exp, got) if g != e]
    assert not bad, bad[:10]
    if sizes is not None:
        for c, g, s in zip(cs, got, sizes):
            if g[0] == 0:
                assert s == g, c["name"]                     # LZF_OK: the size call's length
            elif g[0] != cases.MISMATCH:
                assert s[0] == g[0], c["name"]               # a codec status or LZF_CONTRACT: the size call's
            else:
                assert s[0] == 0, c["name"]                  # a mismatch is a block that decodes cleanly


def test_every_case_against_decode_then_compare_and_the_size_call(rows):
    cs, exp = [c for c, _ in rows], [e for _, e in rows]
    j, keep, _ = build_jobs(cs)
    got = run_verify(j)                                     # (bound unknown: the class in front, these small jobs left to the one-wave kernel)
    check(cs, exp, got, run_size(j))
    assert run_verify(j, max_input_len=max(len(c["input"]) for c in cs)) == got
    assert run_verify(j, max_input_len=cases.CLASS_MIN_IN - 1) == got          # the one-wave kernel alone


def test_sample_against_the_decoder(rows):
    """Every fifth case decoded into fresh output by lzf_decompress_batch and compared with torch.equal: LZF_OK exactly when the
    decode is clean, as long as out_cap says and equal to the expected bytes; a mismatch's position is the first unequal byte."""
    some = [(c, e) for c, e in rows[::5] if c["prefix_len"] == len(c["prefix"])]
    cs = [c for c, _ in some]
    j, keep, _ = build_jobs(cs)
    got = run_verify(j)
    # room for the decode: what the size call says where the block is clean, the decoder's worst case where it is not
    caps = [s[1] + 64 if s[0] == 0 else c["existing_len"] + c["limit"] + len(c["input"]) + 64 for c, s in zip(cs, run_size(j))]
    offs = np.cumsum([0] + [(cap + 255) // 256 * 256 for cap in caps])
    h = np.zeros(int(offs[-1]), dtype=np.uint8)
    for c, a in zip(cs, offs):
        h[a:a + c["existing_len"]] = np.frombuffer(c["mem"][:c["existing_len"]], dtype=np.uint8)
    d_dec = torch.from_numpy(h).to(DEV)
    jd = j.copy()
    jd["out"] = np.uint64(d_dec.data_ptr()) + offs[:-1].astype(np.uint64)
    jd["out_cap"] = caps
    r_dec = torch.zeros(len(cs) * 16, dtype=torch.uint8, device=DEV)
    device.decompress_batch(device.to_device(jd, DEV), r_dec, len(cs))
    torch.cuda.synchronize()
    rd = device.results_to_host(r_dec, len(cs))
    d_out = keep[2]
    out_base = j["out"] - np.uint64(d_out.data_ptr())
    for k, c in enumerate(cs):
        st, n = int(rd["status"][k]), int(rd["out_len"][k])
        if st != 0:
            assert got[k] == (st, None), c["name"]
            continue
        ex, cap = c["existing_len"], c["out_cap"]
        m = min(n, cap)
        a, b = int(offs[k]), int(out_base[k])
        same = torch.equal(d_dec[a + ex:a + m], d_out[b + ex:b + m])
        assert (got[k][0] == 0) == (same and n == cap), c["name"]
        if not same:
            first = int(torch.nonzero(d_dec[a + ex:a + m] != d_out[b + ex:b + m])[0])
            assert got[k] == (cases.MISMATCH, ex + first), c["name"]


def test_alignment_of_input_prefix_and_out(rows):
    """input, prefix and out each at residues 0, 1, 15 and 16 of a 256-aligned address: own-lane runs, wave-wide runs, a source that
    comes out of the prefix, the token beyond a chunk and a block of text, equal and with a planted difference."""
    names = ("match/prefix, existing output and out, 10 + 50 + 300", "match/prefix, existing output and out, 63 + 50 + 65, flip",
             "match/source from the prefix into out, 10 + 20, flip at 12", "match/source wholly in the prefix, M 64",
             "tokens/beyond a chunk first, literals, flip at 4100", "tokens/beyond a chunk first, match",
             "planted/text, flip at 17", "tokens/input of 3073")
    by = {c["name"]: (c, e) for c, e in rows}
    cs, exp, res = [], [], []
    for nm in names:
        for ri in (0, 1, 15, 16):
            for rp in (0, 1, 15, 16):
                for ro in (0, 1, 15, 16):
                    cs.append(by[nm][0]); exp.append(by[nm][1]); res.append((ri, rp, ro))
    j, keep, _ = build_jobs(cs, poison=0xEE, residues=res)
    assert {int(x) % 256 for x in j["out"]} == {0, 1, 15, 16} and {int(x) % 256 for x in j["input"]} == {0, 1, 15, 16}
    check(cs, exp, run_verify(j))


@pytest.mark.parametrize("poison", [0xA5, 0x5A])
def test_nothing_but_the_results_is_written_and_nothing_outside_is_looked_at(rows, poison):
    """Poison around every input, prefix and `out`, red zones around the result array: after the call every arena, the job array and
    the red zones are what they were, and the verdicts do not depend on the poison (two of them)."""
    cs, exp = [c for c, _ in rows], [e for _, e in rows]
    n = len(cs)
    j, keep, host = build_jobs(cs, poison=poison)
    resbuf = torch.full((2 * ZONE + 16 * n,), poison, dtype=torch.uint8, device=DEV)
    d_j = device.to_device(j, DEV)
    device.decompress_verify_batch(d_j, resbuf[ZONE:ZONE + 16 * n], n)
    torch.cuda.synchronize()
    for t, h in zip(keep, host):
        assert np.array_equal(t.cpu().numpy(), h), "the call wrote to an input, a prefix or an `out`"
    assert bool((resbuf[:ZONE] == poison).all()) and bool((resbuf[ZONE + 16 * n:] == poison).all()), "red zone around the results"
    assert np.array_equal(d_j.cpu().numpy(), np.ascontiguousarray(j).view(np.uint8).reshape(-1)), "the job array was written to"
    got = _tuples(device.results_to_host(resbuf[ZONE:ZONE + 16 * n].clone(), n), (0, cases.MISMATCH))
    check(cs, exp, got)


def test_more_jobs_than_the_device_holds_at_once(rows):
    """20 000 jobs aliasing the cases: the launch order by input length and the ticket, every job's result in its own place."""
    cs, exp = [c for c, _ in rows], [e for _, e in rows]
    j, keep, _ = build_jobs(cs)
    which = np.random.default_rng(20000).integers(0, len(cs), 20000)
    got = run_verify(j[which])
    bad = [(i, cs[k]["name"], got[i], exp[k]) for i, k in enumerate(which) if got[i] != exp[k]]
    assert not bad, bad[:10]


def test_host_helper_equals_the_device_call(rows):
    some = [(c, e) for c, e in rows[::4] if c["prefix_len"] == len(c["prefix"])]
    items = [dict(input=c["input"], prefix=c["prefix"], existing=c["mem"][:c["existing_len"]],
                  expected=c["mem"][c["existing_len"]:c["out_cap"]], limit=c["limit"]) for c, _ in some]
    got = [(s, l if s in (0, cases.MISMATCH) else None) for s, l in ffi.verify_blocks_host(items)]
    bad = [(c["name"], g, e) for (c, e), g in zip(some, got) if g != e]
    assert not bad, bad[:10]


# ---------------------------------------------------------------------------------------------------- the latency class
@pytest.fixture(scope="module")
def class_rows():
    return cases.class_cases()


@pytest.mark.parametrize("n_jobs", [2, 16, 300])
def test_latency_class_answers_the_clean_jobs_and_leaves_the_error(class_rows, n_jobs):
    """2, 16 and 300 jobs of 64 KiB .. 200 KiB of compressed text through the class: a difference in tile 0, in the last tile, in the
    last byte of a tile's output and the first of the next, in a match whose source lies in the tile before; a prefix, existing
    output.  Every clean job is answered by the class itself (reserved = its tiles), the job with an error comes back from the
    one-wave kernel with the size call's status."""
    cs, exp = [c for c, _ in class_rows], [e for _, e in class_rows]
    j, keep, _ = build_jobs(cs)
    which = np.array([0, 4]) if n_jobs == 2 else np.arange(len(cs) - 16, len(cs)) if n_jobs == 16 else np.arange(300) % len(cs)
    reserved = []
    got = run_verify(j[which], max_input_len=max(len(c["input"]) for c in cs), reserved=reserved)
    assert device.last_verify_launch() == LATENCY
    bad = [(cs[k]["name"], got[i], exp[k]) for i, k in enumerate(which) if got[i] != exp[k]]
    assert not bad, bad[:10]
    for i, k in enumerate(which):
        if exp[k][0] in (0, cases.MISMATCH):
            assert reserved[i] == (len(cs[k]["input"]) + cases.TILE - 1) // cases.TILE, (cs[k]["name"], "not answered by the class")
    if n_jobs > 2:
        assert any(exp[k][0] == 3 for k in which)
    sizes = run_size(j[which])
    for i, k in enumerate(which):
        assert sizes[i][0] == (0 if exp[k][0] in (0, cases.MISMATCH) else exp[k][0])


def test_class_cases_by_the_one_wave_kernel_alone(class_rows):
    """The same cases in a call too large for the class (one job more than 16 per CU), and with a bound below the class's smallest
    input: the one-wave kernel does them all, with the same verdicts."""
    cs, exp = [c for c, _ in class_rows], [e for _, e in class_rows]
    j, keep, _ = build_jobs(cs)
    which = np.arange(CLASS_MAX_JOBS + 1) % len(cs)
    got = run_verify(j[which], max_input_len=max(len(c["input"]) for c in cs))
    assert device.last_verify_launch() == KERNEL
    assert all(got[i] == exp[k] for i, k in enumerate(which))
    assert run_verify(j, max_input_len=cases.CLASS_MIN_IN - 1) == exp and device.last_verify_launch() == KERNEL


def test_history_restore_moves_a_mismatch_position_back_with_the_origin():
    """lzf_history_restore_batch on verify results: the shift is added to the length of an LZF_OK and to the position of an
    LZF_MISMATCH, and to nothing else."""
    res = np.zeros(4, dtype=device.RES)
    res["status"] = [0, cases.MISMATCH, 3, cases.MISMATCH]
    res["out_len"] = [70_000, 65_540, 123, 9]
    shift = np.array([(1 << 30) + 16, (1 << 31) + 32, 1 << 30, 0], dtype=np.uint64)
    d_res = device.to_device(res, DEV)
    device.history_restore_batch(d_res, torch.from_numpy(shift.view(np.int64)).to(DEV), 4)
    torch.cuda.synchronize()
    got = device.results_to_host(d_res, 4)
    assert got["out_len"].tolist() == [70_000 + (1 << 30) + 16, 65_540 + (1 << 31) + 32, 123, 9] and got["status"].tolist() == res["status"].tolist()
