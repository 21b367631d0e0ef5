"""GPU tests (-m gpu) of the decoded-size query: lzf_decompressed_size_batch / _host (the status and output.len() of
decompress_raw for every job, nothing decoded) against the oracle and against lzf_decompress_batch on the same job array, and
lzf_frame_decompressed_size_device against lzf_frame_decompress_device_many.  Damaged inputs here are data errors that end in
a status."""
import numpy as np
import pytest
import torch

import decoded_size_cases as cases
import oracle_ffi as o
import vectors
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi, framed, synth
from test_oracle import fuzz_corpus

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NO_LIMIT = (1 << 63) - 1
CHUNK = 3072          # compressed bytes one parse of lzf_decoded_size_kernel<48, 768> covers
TOKCAP = 768          # tokens one parse lists
N_FF = 4000           # 0xFF length bytes of a token that reaches beyond a whole chunk
BS = 4 << 20
ZONE = 4096
LAST_KCYCLES = []


def dev(b):
    b = bytes(b)
    if not b:
        return torch.empty(0, dtype=torch.uint8, device=DEV)
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(DEV)


def _arena(blobs, poison=0, gap=64):
    """The blobs in one device tensor, `gap` bytes of `poison` behind each: (tensor, offsets)."""
    offs = np.cumsum([0] + [len(b) + gap for b in blobs])
    h = np.full(int(offs[-1]) + gap, poison, dtype=np.uint8)
    for b, a in zip(blobs, offs):
        h[a:a + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return torch.from_numpy(h).to(DEV), offs[:-1].astype(np.uint64)


def size_jobs(cs, in_poison=0):
    """Job array of the cases for the size call alone: inputs in an arena, prefix NULL, out NULL, out_cap 0."""
    d_in, offs = _arena([c["input"] for c in cs], in_poison)
    j = np.zeros(len(cs), dtype=device.DJOB)
    j["input"] = np.uint64(d_in.data_ptr()) + offs
    j["input_len"] = [len(c["input"]) for c in cs]
    j["prefix_len"] = [c["prefix_len"] for c in cs]
    j["out_existing_len"] = [c["existing_len"] for c in cs]
    j["output_limit"] = [c["limit"] for c in cs]
    return j, d_in


def run_size(j, max_input_len=None, stream=None):
    n = len(j)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    d_j = device.to_device(j, DEV)
    device.decompressed_size_batch(d_j, d_res, n, stream=stream, max_input_len=max_input_len)
    torch.cuda.synchronize()
    res = device.results_to_host(d_res, n)
    global LAST_KCYCLES
    LAST_KCYCLES = res["reserved"].tolist()          # diagnostic: kilo-cycles per job
    return [(int(s), int(l) if s == 0 else None) for s, l in zip(res["status"], res["out_len"])]


def sizes(cs, max_input_len=None):
    j, keep = size_jobs(cs)
    return run_size(j, max_input_len=max_input_len)


# ---------------------------------------------------------------------------------------------------- raw blocks, sequence by sequence
def _lsic(v):
    return b"\xff" * (v // 255) + bytes([v % 255])


def _seq(lit, off, mlen):
    """One sequence (off None: the last literals, no match)."""
    L = len(lit)
    b = bytearray([(min(L, 15) << 4) | (0 if off is None else min(mlen - 4, 15))])
    if L >= 15:
        b += _lsic(L - 15)
    b += lit
    if off is not None:
        b += off.to_bytes(2, "little")
        if mlen - 4 >= 15:
            b += _lsic(mlen - 19)
    return bytes(b)


def _fill(n_bytes):
    """Exactly n_bytes (>= 4) of input: one sequence with 1..3 literals, then 3-byte sequences (no literals, a match of 4 at
    offset 1)."""
    pad = (n_bytes - 4) % 3
    return _seq(b"x" * (1 + pad), 1, 4) + _seq(b"", 1, 4) * ((n_bytes - 4 - pad) // 3)


def _fill8(n_bytes):
    """Exactly n_bytes (>= 8) of input in 8-byte sequences (5 literals, a match of 4), the first one longer by n_bytes % 8: 128
    tokens per KiB, so a parse of the size kernel is never cut by its token list and its first chunk ends at CHUNK bytes."""
    return _seq(b"abcde" + b"x" * (n_bytes % 8), 1, 4) + _seq(b"abcde", 1, 4) * (n_bytes // 8 - 1)


# ---------------------------------------------------------------------------------------------------- blocks
def test_block_cases_match_oracle_and_decoder():
    """The CPU file's block cases, one batch: the oracle's status (and length when Ok), and the status / length lzf_decompress_batch
    writes for the same job array with out_cap = output_limit + input_len + 64."""
    blocks = cases.block_cases()
    cases.assert_all_kinds(blocks)
    cs = [c for _, c, _ in blocks]
    n = len(cs)
    caps = [c["limit"] + len(c["input"]) + 64 for c in cs]
    d_in, in_offs = _arena([c["input"] for c in cs])
    d_pre, pre_offs = _arena([c["prefix"] for c in cs])
    out_offs = np.cumsum([0] + [cap + 64 for cap in caps])
    h_out = np.zeros(int(out_offs[-1]), dtype=np.uint8)
    for c, a in zip(cs, out_offs):
        h_out[a:a + len(c["existing"])] = np.frombuffer(c["existing"], dtype=np.uint8)
    d_out = torch.from_numpy(h_out).to(DEV)
    j = np.zeros(n, dtype=device.DJOB)
    j["input"] = np.uint64(d_in.data_ptr()) + in_offs
    j["input_len"] = [len(c["input"]) for c in cs]
    j["prefix"] = np.uint64(d_pre.data_ptr()) + pre_offs
    j["prefix_len"] = [c["prefix_len"] for c in cs]
    j["out"] = np.uint64(d_out.data_ptr()) + out_offs[:-1].astype(np.uint64)
    j["out_existing_len"] = [c["existing_len"] for c in cs]
    j["out_cap"] = caps
    j["output_limit"] = [c["limit"] for c in cs]
    d_j = device.to_device(j, DEV)
    r_size = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    r_dec = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    device.decompressed_size_batch(d_j, r_size, n)
    device.decompress_batch(d_j, r_dec, n)
    torch.cuda.synchronize()
    rs, rd = device.results_to_host(r_size, n), device.results_to_host(r_dec, n)
    for k, (name, c, exp) in enumerate(blocks):
        got = (int(rs["status"][k]), int(rs["out_len"][k]) if rs["status"][k] == 0 else None)
        print(name, got, exp, int(rd["status"][k]))
        assert got == exp, name
        assert int(rd["status"][k]) == got[0], name
        if got[0] == 0:
            assert int(rd["out_len"][k]) == got[1], name


def test_block_that_decodes_to_more_than_4_gib():
    """~17 MB of 0xFF match-length bytes, half of them spread over 2 125 sequences and half as one run: the length, computed here
    from the bytes written, is beyond 32 bits (the oracle cannot hold the output); one byte less of limit is MemoryLimitExceeded."""
    blk, total = bytearray(), 0
    for _ in range(2125):
        blk += bytes([0x1F]) + b"a" + (1).to_bytes(2, "little") + b"\xff" * 4000 + bytes([3])
        total += 1 + 4 + 15 + 255 * 4000 + 3
    blk += bytes([0x0F]) + (7).to_bytes(2, "little") + b"\xff" * 8_500_000 + bytes([200])
    total += 4 + 15 + 255 * 8_500_000 + 200
    assert total > 1 << 32 and 16_900_000 < len(blk) < 17_100_000
    blk = bytes(blk)
    got = sizes([cases.make_case(blk, NO_LIMIT), cases.make_case(blk, total), cases.make_case(blk, total - 1)])
    print(total, got, "kilo-cycles per job:", LAST_KCYCLES)
    assert got == [(0, total), (0, total), (ffi.MEMORY_LIMIT_EXCEEDED, None)]


def _edge_cases():
    """(name, case, expected status or None) — every case is also held to the oracle."""
    out = []
    # a 0xFF match-length run that crosses the first chunk's end: the token 10 and 4 bytes before it, and further on
    for start in (CHUNK - 10, CHUNK - 3 - 1, 2 * CHUNK - 7, 5 * CHUNK - 2):
        blk = _fill8(start) + _seq(b"", 2, 19 + 255 * 40 + 7) + _fill8(400) + _seq(b"end", None, 0)
        out.append((f"match run over a chunk end, token at {start}", cases.make_case(blk, 1 << 20), 0))
    # a literal-length run that crosses a chunk end
    lit = bytes(range(256)) * 4
    for start in (CHUNK - 4, CHUNK - 2, 3 * CHUNK - 3):
        blk = _fill8(start) + _seq(lit[:15 + 255 * 3 + 9], 5, 8) + _fill8(100) + _seq(b"", None, 0)
        out.append((f"literal run over a chunk end, token at {start}", cases.make_case(blk, 1 << 20), 0))
    # a token as the last byte of a chunk (its offset and length bytes in the next one), plain and with a 0xFF run
    for k in (1, 2, 7):
        for m in (30, 19 + 255 * 2):
            blk = _fill8(k * CHUNK - 1) + _seq(b"", 3, m) + _fill8(40) + _seq(b"z", None, 0)
            assert blk[k * CHUNK - 1] & 0xF0 == 0 and len(_fill8(k * CHUNK - 1)) == k * CHUNK - 1
            out.append((f"token in the last byte of chunk {k}, match {m}", cases.make_case(blk, 1 << 20), 0))
    # a sequence whose match ends exactly at the limit / one byte past it (no last literals: the block ends with the match)
    blk = _fill(700) + _seq(b"abc", 2, 77)
    n = 1 + 4 * 233 + 3 + 77
    out.append(("match ends at the limit", cases.make_case(blk, n), 0))
    out.append(("match ends one byte past the limit", cases.make_case(blk, n - 1), ffi.MEMORY_LIMIT_EXCEEDED))
    out.append(("literals are not limit-checked", cases.make_case(_fill(40) + _seq(b"q" * 500, None, 0), 60), 0))
    # an offset equal to / one more than position + existing + prefix_len
    pre, ex = bytes(range(100)), bytes(range(50))
    for tag, p, e in (("", b"", b""), (" with prefix", pre, b""), (" with existing output", b"", ex), (" with both", pre, ex)):
        reach = 4 + len(p) + len(e)
        out.append(("offset reaches the first byte" + tag, cases.make_case(_seq(b"lit!", reach, 9) + _seq(b"", None, 0), 1 << 16, p, e), 0))
        out.append(("offset one beyond" + tag, cases.make_case(_seq(b"lit!", reach + 1, 9) + _seq(b"", None, 0), 1 << 16, p, e),
                    ffi.INVALID_DEDUP_OFFSET))
    # a zero offset in lane 0 and in lane 63 of a round (3-byte sequences: token k of a chunk is lane k % 64 of round k // 64),
    # with a later invalid offset that must not win
    for k in (0, 63, 64, 127, TOKCAP - 1, TOKCAP, TOKCAP + 63):
        b = bytearray(_fill(4 + 3 * 1200) + _seq(b"", None, 0))
        at = 0 if k == 0 else 4 + 3 * (k - 1)                  # token k (token 0 is 4 bytes long)
        o_at = at + (2 if k == 0 else 1)
        b[o_at:o_at + 2] = b"\x00\x00"
        later = 4 + 3 * (k + 70) + 1
        b[later:later + 2] = b"\xff\xff"
        out.append((f"zero offset in token {k}", cases.make_case(bytes(b), 1 << 20), ffi.ZERO_DEDUP_OFFSET))
    # tokens that reach beyond a whole chunk (the kernel decodes them ahead of its parse): by match length, by literals, first in
    # the block, cut inside the run, with a zero offset, past the limit
    giant_m = _seq(b"", 2, 19 + 255 * N_FF + 7)
    giant_l = _seq(bytes(range(250)) * 20, 7, 8)
    for tag, g in (("match run", giant_m), ("literals", giant_l)):
        blk = _fill8(500) + g + _fill8(100) + _seq(b"end", None, 0)
        out.append((f"token over whole chunks, {tag}", cases.make_case(blk, 1 << 20), 0))
        out.append((f"token over whole chunks first, {tag}", cases.make_case(b"\x1fa\x01\x00" + g[3:] if tag == "match run" else g + _fill8(64), 1 << 20), 0))
        out.append((f"token over whole chunks cut, {tag}", cases.make_case(blk[:500 + 2000], 1 << 20), ffi.UNEXPECTED_END))
    blk = _fill8(500) + giant_m + _fill8(100)
    out.append(("token over whole chunks ends at the limit", cases.make_case(blk[:500 + len(giant_m)], 9 * 62 + 9 + 4 + 19 + 255 * N_FF + 7), 0))
    out.append(("token over whole chunks ends one byte past the limit", cases.make_case(blk, 9 * 62 + 9 + 4 + 19 + 255 * N_FF + 7 - 1), ffi.MEMORY_LIMIT_EXCEEDED))
    out.append(("token over whole chunks past the limit", cases.make_case(blk, 200_000), ffi.MEMORY_LIMIT_EXCEEDED))
    b = bytearray(blk); b[501:503] = b"\x00\x00"
    out.append(("token over whole chunks, zero offset", cases.make_case(bytes(b), 1 << 20), ffi.ZERO_DEDUP_OFFSET))
    b = bytearray(blk); b[501:503] = b"\xff\xff"
    out.append(("token over whole chunks, offset beyond the output", cases.make_case(bytes(b), 1 << 20), ffi.INVALID_DEDUP_OFFSET))
    out.append(("one token", cases.make_case(_seq(b"hello", None, 0), 100), 0))
    out.append(("one token with a match", cases.make_case(_seq(b"hello", 5, 4), 100), 0))
    out.append(("empty input", cases.make_case(b"", 0), 0))
    out.append(("empty input behind existing output", cases.make_case(b"", 10, b"", b"0123456"), 0))
    out.append(("one byte left after the literals", cases.make_case(_seq(b"hello", None, 0) + b"\x07", 100), 0))
    out.append(("one byte left after the literals, later chunk", cases.make_case(_fill8(CHUNK + 40) + _seq(b"hello", None, 0) + b"\x07", 1 << 16), 0))
    out.append(("token byte alone", cases.make_case(b"\x00", 100), 0))
    out.append(("missing length byte", cases.make_case(b"\xf0", 100), ffi.UNEXPECTED_END))
    out.append(("missing match length byte", cases.make_case(_seq(b"ab", 1, 4) + bytes([0x2F]) + b"ab\x01\x00", 100), ffi.UNEXPECTED_END))
    return out


def test_tokens_on_the_kernels_edges():
    ec = _edge_cases()
    exp = [cases.expect(c) for _, c, _ in ec]
    got = sizes([c for _, c, _ in ec])
    for (name, c, want), e, g in zip(ec, exp, got):
        print(name, g, e)
        assert g == e, name
        if want is not None:
            assert g[0] == want, name
    assert {0, 1, 2, 3, 4} <= {e[0] for e in exp}


@pytest.mark.parametrize("poison", [0xA5, 0x5A])
def test_nothing_but_the_results_is_written(poison):
    """`out` of every job points into a poisoned buffer between red zones, `prefix` is NULL with prefix_len > 0, the result array
    lies between red zones: after the call everything but the results is intact, and the results do not depend on the bytes behind
    input_len (two poisons)."""
    blocks = cases.block_cases()
    blocks = blocks[::3] + [b for b in blocks if b[0].startswith("dict/")]
    cs = [c for _, c, _ in blocks]
    n = len(cs)
    j, keep = size_jobs(cs, in_poison=poison)
    outbuf = torch.full((2 * ZONE + 64 * n,), poison, dtype=torch.uint8, device=DEV)
    j["out"] = np.uint64(outbuf.data_ptr()) + np.uint64(ZONE) + np.arange(n, dtype=np.uint64) * np.uint64(64)
    j["out_cap"] = 64
    assert any(c["prefix_len"] > 0 for c in cs) and not j["prefix"].any()
    resbuf = torch.full((2 * ZONE + 16 * n,), poison, dtype=torch.uint8, device=DEV)
    d_res = resbuf[ZONE:ZONE + 16 * n]
    d_j = device.to_device(j, DEV)
    h_in = keep.cpu().numpy().copy()
    device.decompressed_size_batch(d_j, d_res, n)
    torch.cuda.synchronize()
    assert bool((outbuf == poison).all()), "the size call wrote to a job's `out`"
    assert bool((resbuf[:ZONE] == poison).all()) and bool((resbuf[ZONE + 16 * n:] == poison).all()), "red zone around the results"
    assert np.array_equal(keep.cpu().numpy(), h_in), "the input arena was written to"
    assert np.array_equal(d_j.cpu().numpy(), np.ascontiguousarray(j).view(np.uint8).reshape(-1)), "the job array was written to"
    res = device.results_to_host(d_res.clone(), n)
    for k, (name, c, exp) in enumerate(blocks):
        got = (int(res["status"][k]), int(res["out_len"][k]) if res["status"][k] == 0 else None)
        assert got == exp, name


def _damage(rng, c):
    b = bytearray(c)
    kind = int(rng.integers(0, 3))
    if kind == 0:
        for _ in range(int(rng.integers(1, 6))):
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
    elif kind == 1:
        del b[int(rng.integers(1, len(b))):]
    else:
        i = int(rng.integers(len(b) // 3, len(b)))
        b[i:] = bytes(rng.integers(0, 256, len(b) - i, dtype=np.uint8))
    return bytes(b)


def test_scale_aliased_4mib_jobs():
    """3 400 jobs of 4 MiB aliasing 32 distinct blocks, a tenth of them damaged (8 distinct damaged blocks), against the oracle;
    with the input bound given and unknown."""
    rng = np.random.default_rng(3400)
    n_jobs, n_good, n_bad = 3400, 32, 8
    raws = [synth.silesia_mix(k * BS, (k + 1) * BS).tobytes() for k in range(n_good)]
    comps = [o.compress2(d)[1] for d in raws]
    bads = [_damage(rng, comps[k % n_good]) for k in range(n_bad)]
    exp = [(0, BS)] * n_good + [cases.expect(cases.make_case(m, BS)) for m in bads]
    assert len({e[0] for e in exp}) >= 3
    inputs = comps + bads
    d_in, offs = _arena(inputs)
    which = np.array([n_good + (i // 10) % n_bad if i % 10 == 3 else i % n_good for i in range(n_jobs)])
    j = np.zeros(n_jobs, dtype=device.DJOB)
    j["input"] = np.uint64(d_in.data_ptr()) + offs[which]
    j["input_len"] = [len(inputs[k]) for k in which]
    j["output_limit"] = BS
    for bound in (max(len(c) for c in inputs), None):
        got = run_size(j, max_input_len=bound)
        for i, k in enumerate(which):
            assert got[i] == exp[k], (i, k, bound)


def test_scale_30000_small_jobs():
    """30 000 jobs of at most 64 KiB aliasing 300 distinct blocks (a third of them mutated), against the oracle."""
    rng = np.random.default_rng(30000)
    text = synth.silesia_mix(50 << 20, (50 << 20) + (8 << 20)).tobytes()
    distinct = []
    for k in range(200):
        n = int(rng.integers(1, 65537))
        a = int(rng.integers(0, len(text) - n))
        distinct.append((o.compress2(text[a:a + n])[1], n))
    distinct += [(cases.mutate(rng, c), n if k % 2 else n // 2 + 1) for k, (c, n) in enumerate(distinct[:100])]
    assert max(len(c) for c, _ in distinct) <= 65536 + 300
    exp = [cases.expect(cases.make_case(c, n)) for c, n in distinct]
    assert len({e[0] for e in exp}) >= 4
    d_in, offs = _arena([c for c, _ in distinct])
    which = rng.integers(0, len(distinct), 30000)
    j = np.zeros(30000, dtype=device.DJOB)
    j["input"] = np.uint64(d_in.data_ptr()) + offs[which]
    j["input_len"] = [len(distinct[k][0]) for k in which]
    j["output_limit"] = [distinct[k][1] for k in which]
    for bound in (1 << 17, None):
        got = run_size(j, max_input_len=bound)
        for i, k in enumerate(which):
            assert got[i] == exp[k], (i, k, bound)


def test_host_helper_equals_the_device_call():
    blocks = cases.block_cases()[::5] + [(n, c, cases.expect(c)) for n, c, _ in _edge_cases()]
    cs = [c for _, c, _ in blocks]
    host = ffi.decompressed_sizes_host(cs)
    devr = sizes(cs)
    assert [(s, l if s == 0 else None) for s, l in host] == devr
    assert devr == [e for _, _, e in blocks]


# ---------------------------------------------------------------------------------------------------- frames
def frame_sizes(frames, dictionary_len=0):
    return framed.decompressed_sizes_device([dev(f) for f in frames], dictionary_len=dictionary_len)


def frame_decodes(frames, dictionary=b""):
    """(status, out_len, consumed) of lzf_frame_decompress_device_many with caps from lzf_frame_decompress_bound_device."""
    d = dev(dictionary) if dictionary else None
    res = framed.decompress_frames_device([dev(f) for f in frames], dictionary=d)
    return [(st, int(t.numel()), used) for st, t, used in res]


def check_frames(frames, dictionary=b"", label=""):
    """The size call equals the decode, except that FrameChecksumFail there is Ok here.  Returns the decode's results."""
    got = frame_sizes(frames, dictionary_len=len(dictionary))
    dec = frame_decodes(frames, dictionary)
    for k, (g, d) in enumerate(zip(got, dec)):
        want = (0,) + d[1:] if d[0] == o.F_FRAME_CHECKSUM_FAIL else d
        assert tuple(g) == tuple(want), (label, k, g, d)
        assert g[0] not in (ffi.OUT_CAPACITY, ffi.E_NO_MEMORY)
    return dec


def mutate_frame(rng, frame):
    b = bytearray(frame)
    kind = rng.integers(0, 5)
    if kind == 0 and len(b) > 8:
        del b[rng.integers(7, len(b)):]
    elif kind == 1 and b:
        i = rng.integers(0, len(b)); b[i] ^= 1 << rng.integers(0, 8)
    elif kind == 2 and len(b) > 5:
        i = rng.integers(4, min(len(b), 12)); b[i] = rng.integers(0, 256)
    elif kind == 3 and b:
        i = rng.integers(0, len(b)); b[i] = 0 if rng.integers(0, 2) else 0xFF
    elif b:
        for _ in range(3):
            i = rng.integers(0, len(b)); b[i] = rng.integers(0, 256)
    return bytes(b)


def _inputs():
    mix = synth.silesia_mix(20 << 20, (20 << 20) + 900_000).tobytes()
    return [mix[:300_000], b"", mix[300_000:300_017], vectors.rng_bytes(9, 150_000), mix[100_000:760_001],
            synth.repeat256(5 * 65536 + 1234).tobytes()]


FLAVOURS = [dict(block_size=64 << 10), dict(block_size=64 << 10, independent_blocks=False),
            dict(block_size=64 << 10, independent_blocks=False, block_checksums=True),
            dict(block_size=256 << 10, content_checksum=False, block_checksums=True),
            dict(block_size=64 << 10, content_size=True), dict(block_size=4 << 20),
            dict(block_size=1 << 20, independent_blocks=False), dict(block_size=256 << 10, independent_blocks=False, content_checksum=False),
            dict(block_size=1 << 20, block_checksums=True), dict(block_size=4 << 20, independent_blocks=False, block_checksums=True)]


def _flavour_frames():
    frames = []
    for kw in FLAVOURS:
        kw = dict(kw)
        cs = kw.pop("content_size", False)
        for d in _inputs():
            frames.append(o.frame_compress(d, o.make_settings(content_size=len(d) if cs else None, **kw))[1])
    return frames


def test_frames_flag_matrix_mixed_damaged_and_with_dictionary():
    """Independent / linked, block checksums, content checksum, content size, the four block sizes, stored blocks (random data),
    empty and tiny frames, three damaged copies of each and trailing bytes — mixed in one call; then frames with a dictionary
    (longer than the 64 KiB window), independent and linked."""
    rng = np.random.default_rng(77)
    frames = _flavour_frames()
    damaged = [mutate_frame(rng, f) for f in frames for _ in range(3)]
    allf = frames + damaged + [frames[0] + b"trailing bytes"]
    dec = check_frames(allf, label="matrix")
    assert len({d[0] for d in dec}) >= 6, {d[0] for d in dec}
    assert all(d[0] == 0 for d in dec[:len(frames)])
    dct = synth.gen_text_zipf(3, 70000).tobytes()
    dframes = [o.frame_compress(d, o.make_settings(block_size=64 << 10, dictionary=dct, dictionary_id=9, **extra))[1]
               for d in _inputs() for extra in (dict(), dict(independent_blocks=False), dict(independent_blocks=False, block_checksums=True))]
    dframes += [mutate_frame(rng, f) for f in dframes]
    ddec = check_frames(dframes, dictionary=dct, label="dictionary")
    assert all(d[0] == 0 for d in ddec[:len(dframes) // 2])
    # the same frames sized with too short a dictionary: what the decode reports with that dictionary
    check_frames(dframes, dictionary=dct[:1000], label="short dictionary")


def _patch_bd(frame, bd_code):
    """The frame with another block-size code in its BD byte (header checksum fixed): blocks may now decode past block_maxsize."""
    b = bytearray(frame)
    flg = b[4]
    hlen = 2 + (8 if flg & 0x08 else 0) + (4 if flg & 0x01 else 0)
    b[5] = (b[5] & 0x8F) | (bd_code << 4)
    b[4 + hlen] = (o.xxh32(bytes(b[4:4 + hlen])) >> 8) & 0xFF
    return bytes(b)


def hdr_of(o_, bd_code):
    """A 7-byte frame header: independent blocks, no checksums, the given block-size code."""
    return _patch_bd(o_.frame_compress(b"", o_.make_settings(block_size=64 << 10, content_checksum=False))[1], bd_code)[:7]


def _frame_block(raw_block):
    return len(raw_block).to_bytes(4, "little") + raw_block


def test_frames_that_stop_early():
    """Truncated frames, a damaged block checksum, a damaged block in the middle, a block that decodes past block_maxsize, an
    empty block: the partial length, status and consumed of the decode — and one frame with a damaged content checksum, where
    the decode says FrameChecksumFail and the size call Ok."""
    data = synth.silesia_mix(7 << 20, (7 << 20) + 700_000).tobytes()
    frames, names = [], []
    for kw in (dict(), dict(independent_blocks=False), dict(block_checksums=True), dict(independent_blocks=False, block_checksums=True)):
        f = o.frame_compress(data, o.make_settings(block_size=64 << 10, **kw))[1]
        for cut in (len(f) - 1, len(f) - 4, len(f) - 5, len(f) // 2, len(f) // 3 + 1, 11, 7, 6):
            frames.append(f[:cut]); names.append(("truncated", cut, kw))
        mid = bytearray(f); mid[len(f) // 2] ^= 0x40
        frames.append(bytes(mid)); names.append(("damaged in the middle", kw))
        zero = bytearray(f); zero[len(f) // 2: len(f) // 2 + 8] = bytes(8)
        frames.append(bytes(zero)); names.append(("zeroed bytes in the middle", kw))
    rep = synth.repeat256(700_000).tobytes()              # 256 KiB blocks of it compress to less than 64 KiB each
    big = o.frame_compress(rep, o.make_settings(block_size=256 << 10))[1]
    frames.append(_patch_bd(big, 4)); names.append(("blocks decode past block_maxsize",))
    bigl = o.frame_compress(rep, o.make_settings(block_size=256 << 10, independent_blocks=False))[1]
    frames.append(_patch_bd(bigl, 4)); names.append(("blocks decode past block_maxsize",))
    # a match up to just under the limit, then 100 literals (not limit-checked): BlockSizeOverflow after the decode
    lits = hdr_of(o, 4) + _frame_block(_seq(b"ok", None, 0)) + _frame_block(_seq(b"a", 1, 65_530) + _seq(bytes(100), None, 0)) + bytes(4)
    frames.append(lits); names.append(("literals past block_maxsize",))
    empty_block = hdr_of(o, 4) + _frame_block(b"\x00") + _frame_block(b"\x30abc") + bytes(4)
    frames.append(empty_block); names.append(("a block that decodes to nothing",))
    dec = check_frames(frames, label="early stops")
    by = {}
    for nm, d in zip(names, dec):
        by.setdefault(nm[0], set()).add(d[0])
    assert o.F_BLOCK_CHECKSUM_FAIL in by["damaged in the middle"] and o.F_INPUT_ERROR in by["truncated"]
    assert by["blocks decode past block_maxsize"] == {o.MEMORY_LIMIT_EXCEEDED} and by["literals past block_maxsize"] == {o.F_BLOCK_SIZE_OVERFLOW}
    assert any(0 < d[1] < len(data) for d in dec), "no frame stopped with a partial length"
    # the documented exception
    f = o.frame_compress(data, o.make_settings(block_size=64 << 10))[1]
    csum = bytearray(f); csum[-1] ^= 1
    assert frame_decodes([bytes(csum)]) == [(o.F_FRAME_CHECKSUM_FAIL, len(data), len(f))]
    assert [tuple(g) for g in frame_sizes([bytes(csum)])] == [(0, len(data), len(f))]


def test_frames_of_65_blocks_cross_the_delivery_round():
    """65 blocks of 64 KiB per frame, independent and linked, block checksums on: the count-only delivery takes 64 blocks per
    round, block 64 is counted behind the first round's total.  Whole frames, and the last block's checksum damaged: the frame
    stops in the second round with 64 blocks counted."""
    data = synth.silesia_mix(9 << 20, (9 << 20) + 65 * 65536).tobytes()
    frames = [o.frame_compress(data, o.make_settings(block_size=64 << 10, block_checksums=True, independent_blocks=ib))[1] for ib in (True, False)]
    for f in list(frames):
        b = bytearray(f); b[-9] ^= 1                      # (... block 64 | its checksum | EndMark | content checksum)
        frames.append(bytes(b))
    dec = check_frames(frames, label="65 blocks")
    assert dec == [tuple(x if i != 1 else len(x) for i, x in enumerate(o.frame_decompress(f))) for f in frames]
    assert [d[:2] for d in dec] == [(0, len(data))] * 2 + [(o.F_BLOCK_CHECKSUM_FAIL, 64 * 65536)] * 2


def test_frames_decode_corpus():
    files = fuzz_corpus("decode")
    assert len(files) == 830
    dec = check_frames([d for _, d in files], label="decode corpus")
    assert len({d[0] for d in dec}) >= 8


def test_frame_over_the_memory_budget_still_gets_its_size():
    data = synth.silesia_mix(0, 40 << 20).tobytes()
    big = o.frame_compress(data, o.make_settings(block_size=1 << 20))[1]
    small = o.frame_compress(data[:900_000], o.make_settings(block_size=64 << 10, independent_blocks=False))[1]
    try:
        ffi.lib().lzf_frame_set_memory_budget(64 << 20)
        dec = frame_decodes([small, big])
        got = frame_sizes([small, big])
    finally:
        ffi.lib().lzf_frame_set_memory_budget(0)
    assert dec[1] == (ffi.E_NO_MEMORY, 0, 0) and dec[0] == (0, 900_000, len(small))
    assert [tuple(g) for g in got] == [(0, 900_000, len(small)), (0, len(data), len(big))]


def _cap_bytes(res):
    return sum(t.untyped_storage().nbytes() for _, t, _ in res)


def test_exact_outputs():
    """decompress_frames_device(exact=True): the bytes and statuses of the default call; and 2 000 frames of ~10 KB of text with
    4 MiB blocks get outputs as long as their content, not as long as the bound."""
    rng = np.random.default_rng(2000)
    frames = _flavour_frames()
    frames += [mutate_frame(rng, f) for f in frames]
    dfr = [dev(f) for f in frames]
    a = framed.decompress_frames_device(dfr)
    b = framed.decompress_frames_device(dfr, exact=True)
    for (sa, ta, ua), (sb, tb, ub) in zip(a, b):
        assert (sa, ua) == (sb, ub) and torch.equal(ta, tb)
    assert _cap_bytes(b) == sum(t.numel() for _, t, _ in b) <= _cap_bytes(a)
    text = synth.gen_text_zipf(11, 24 << 20).tobytes()
    plains = [text[k * 10_007: k * 10_007 + 9_000 + (k * 37) % 2_000] for k in range(2000)]
    shards = framed.CompressionSettings().compress_many(plains)                    # default settings: 4 MiB blocks
    dsh = [dev(f) for f in shards]
    bound = sum(device.frame_decompress_bound(dsh))
    res = framed.decompress_frames_device(dsh, exact=True)
    exact = _cap_bytes(res)
    print("bound", bound, "exact", exact)
    assert exact == sum(len(p) for p in plains) < bound // 50
    assert all(st == 0 for st, _, _ in res)
    for k in range(0, 2000, 97):
        assert bytes(res[k][1].cpu().numpy().tobytes()) == plains[k]


def test_stream_order_side_stream():
    """The call on a side stream behind the copies that produce the frames; the results are read after an event of that stream,
    with no device-wide synchronisation in between."""
    data = [synth.silesia_mix((20 + 2 * k) << 20, ((20 + 2 * k) << 20) + 1_500_000).tobytes() for k in range(6)]
    frames = framed.CompressionSettings().block_size(64 << 10).compress_many(data)
    frames += framed.CompressionSettings().block_size(64 << 10).independent_blocks(False).compress_many(data)
    srcs = [dev(f) for f in frames]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    done = torch.cuda.Event()
    with torch.cuda.stream(side):
        dsts = [torch.empty_like(s) for s in srcs]
        for d_, s_ in zip(dsts, srcs):
            d_.copy_(s_, non_blocking=True)
        status, out_len, used = device.frame_decompressed_size(dsts, stream=side)
        h = [torch.empty_like(t, device="cpu").pin_memory() for t in (status, out_len, used)]
        for a, b in zip(h, (status, out_len, used)):
            a.copy_(b, non_blocking=True)
        done.record(side)
    done.synchronize()
    assert h[0].tolist() == [0] * len(frames) and h[1].tolist() == [len(x) for x in data] * 2
    assert h[2].tolist() == [len(f) for f in frames]
