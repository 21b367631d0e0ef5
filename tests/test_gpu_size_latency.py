"""GPU tests (-m gpu) of the size call's latency class (lz4_decoded_size_seg.hip: a block summed up by many wavefronts).

The kernels' edges — the seam, tile and damaged cases of seg_stage_cases.py (one tile up to 67 chunks), the CPU file's boundary cases,
inputs of a tile's and a chunk's length and one byte more, 65 tiles, one 4 MiB block, an empty and a one-token input, one stray byte
on a tile's and a chunk's last byte, a length beyond the clamp — go through the analysis library in child processes
(tests/size_latency_check.py; LZF_SIZE_SEG=force, LZF_SIZE_SEG_MIN_IN=0), which check parity with the oracle and the decoder, who
finished what, red zones, alignment and a side stream.  The product library, with nothing forced, takes a mixed call, the same call
among 5 000 small jobs, and the frame layer.  Damaged blocks here are data errors that end in a status."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import decoded_size_cases as D
import oracle_ffi as o
import seg_stage_cases as S
import size_latency_cases as Z
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import build, device, framed, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device("cuda", 0)
S_CLASS = "latency: lzf_seg_parse_kernel + lzf_size_tile_kernel + lzf_size_finish_kernel + lzf_decoded_size_kernel<48,768>"
S_WAVE = "lzf_decoded_size_kernel<48,768>"
SEG_MAX_IN = 4 * 1024 * 1024 + 32 * 1024


def _compress(data):
    rc, c = o.compress2(data)
    assert rc == 0
    return c


@pytest.fixture(scope="module")
def four_mib():
    d = synth.silesia_mix(0, 4 << 20).tobytes()
    return Z.named("edge/one 4 MiB block", _compress(d), len(d))


@pytest.fixture(scope="module")
def corpus(tmp_path_factory, four_mib):
    """[(case, the oracle's (status, length), must the class finish it)], once for the module; the children read the file."""
    cases = Z.stage_cases() + Z.boundary_cases() + Z.size_edge_cases() + [four_mib, Z.long_run_case()]
    assert len(four_mib["input"]) > 1 << 20
    rows = []
    for c in cases:
        exp = D.expect(c)
        rows.append((c, exp, Z.finishes(c, exp)))
    assert {e[0] for _, e, _ in rows} == {0, 1, 2, 3, 4}
    assert any(e[0] == 0 and not fin for _, e, fin in rows)                  # (the length beyond the clamp)
    path = tmp_path_factory.mktemp("size_latency") / "corpus.pkl"
    path.write_bytes(pickle.dumps(rows))
    return str(path)


def _child(what, corpus, **env):
    e = dict(os.environ, LZF_LIB_PATH=build.build_analysis_library(), SIZE_LATENCY_CORPUS=corpus, LZF_SIZE_SEG="force", LZF_SIZE_SEG_MIN_IN="0", **env)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(HERE, "size_latency_check.py"), what], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "size latency ok" in r.stdout, r.stdout[-2000:]
    print(r.stdout.strip().splitlines()[-2], f"[{time.time() - t0:.1f} s]")


def test_parity_alignment_side_stream(corpus):
    _child("parity", corpus)


def test_who_finished_what(corpus):
    """LZF_SIZE_FORCE=2: no one-wave kernel behind the class.  Every job the oracle calls Ok with all lengths within the clamp is finished
    by the class; every other job keeps its sentinel.  No slack: valid input never fails the seam or the tile pass."""
    _child("who", corpus, LZF_SIZE_FORCE="2")


def test_red_zones_two_poisons(corpus):
    _child("redzone", corpus)


def test_scratch_refused(corpus):
    _child("refused", corpus, LZF_SIZE_FORCE="1")


# ------------------------------------------------------------------------------------------------ the product library, nothing forced
def _arena(blobs):
    offs = np.cumsum([0] + [len(b) + 64 for b in blobs])
    h = np.zeros(int(offs[-1]) + 64, dtype=np.uint8)
    for b, a in zip(blobs, offs):
        h[a:a + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return torch.from_numpy(h).to(DEV), offs[:-1].astype(np.uint64)


def _size_call(cases, max_input_len=None):
    d_in, offs = _arena([c["input"] for c in cases])
    n = len(cases)
    j = np.zeros(n, dtype=device.DJOB)
    j["input"] = [0 if c.get("null_input") else int(d_in.data_ptr()) + int(a) for c, a in zip(cases, offs)]
    j["input_len"] = [len(c["input"]) for c in cases]
    j["prefix_len"] = [c["prefix_len"] for c in cases]
    j["out_existing_len"] = [c["existing_len"] for c in cases]
    j["output_limit"] = [c["limit"] for c in cases]
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    device.decompressed_size_batch(device.to_device(j, DEV), d_res, n, max_input_len=max_input_len)
    torch.cuda.synchronize()
    res = device.results_to_host(d_res, n)
    return [(int(s), int(l) if s == 0 else None) for s, l in zip(res["status"], res["out_len"])]


@pytest.fixture(scope="module")
def mixed(four_mib):
    """A few jobs of 64 KiB and more beside jobs below it, one above the class's largest input, an empty job with a NULL input, and a job
    the decoder refuses (a prefix of 2 GiB): [(case, expectation)]."""
    mix = synth.silesia_mix(8 << 20, 10 << 20).tobytes()
    big = [Z.named(f"mixed/1 MiB block {k}", _compress(mix[k << 20:(k + 1) << 20]), 1 << 20) for k in range(2)]
    assert all(len(c["input"]) >= 64 * 1024 for c in big)
    small = [Z.named(f"mixed/small {k}", _compress(mix[k * 5000:k * 5000 + 3000 + 700 * k]), 3000 + 700 * k) for k in range(4)]
    damaged = [c for c in Z.stage_cases() if "damaged" in c["name"]]
    noise = np.random.default_rng(5).integers(0, 256, SEG_MAX_IN + 70000, dtype=np.uint8).tobytes()
    above = Z.named("mixed/above the class's largest input", _compress(noise), len(noise))
    assert len(above["input"]) > SEG_MAX_IN
    rows = [(c, D.expect(c)) for c in big + small + damaged + [four_mib, above]]
    empty = dict(Z.named("mixed/empty, NULL input", b"", 100), null_input=True)
    rows.append((empty, (0, 0)))
    rows.append((dict(Z.named("mixed/prefix of 2 GiB", small[0]["input"], 1 << 20), prefix_len=1 << 31), (6, None)))      # LZF_CONTRACT
    return rows


def test_mixed_call_through_the_product(mixed):
    """Fails on a tree without the class: lzf_last_size_launch does not exist there."""
    cases = [c for c, _ in mixed]
    got = _size_call(cases)
    assert device.last_size_launch() == S_CLASS
    for (c, exp), g in zip(mixed, got):
        assert g == exp, (c["name"], g, exp)
    assert {e[0] for _, e in mixed} >= {0, 1, 3, 4, 6}
    # a caller's bound below 64 KiB keeps the call out of the class; the answers are the same
    assert _size_call([c for c in cases if len(c["input"]) < 65536], max_input_len=65535) == [e for c, e in mixed if len(c["input"]) < 65536]
    assert device.last_size_launch() == S_WAVE


def test_the_same_jobs_among_5000_small_ones(mixed):
    tiny = Z.named("tiny", _compress(b"small block " * 40), 480)
    exp_tiny = D.expect(tiny)
    cases = [c for c, _ in mixed] + [tiny] * 5000
    got = _size_call(cases)
    assert device.last_size_launch() == S_WAVE
    assert got == [e for _, e in mixed] + [exp_tiny] * 5000


def _zero_first_offset(frame):
    """The frame with the match offset of its first block's first sequence set to 0: a data error (ZeroDedupOffset) in a compressed block,
    whatever the bytes are.  Header: magic, FLG, BD, HC (no content size, no dictionary id); then the block's u32 length and its data."""
    assert frame[4] & 0x09 == 0 and not frame[10] & 0x80, "7-byte header, first block compressed"
    p = 11
    L = frame[p] >> 4; p += 1
    if L == 15:
        while True:
            b = frame[p]; p += 1; L += b
            if b != 255:
                break
    p += L
    bad = bytearray(frame); bad[p:p + 2] = b"\0\0"
    return bytes(bad)


def test_frame_layer():
    """framed.decompressed_sizes_device over 8 frames of four 256 KiB blocks, one linked and one damaged, against the decode; and
    stream_index_device over 2 streams x 3 frames against decompress_streams_device."""
    mix = synth.silesia_mix(40 << 20, 48 << 20).tobytes()
    frames = []
    for k in range(8):
        kw = dict(block_size=256 << 10, independent_blocks=k != 3)
        frames.append(o.frame_compress(mix[k << 20:(k + 1) << 20], o.make_settings(**kw))[1])
    frames[5] = _zero_first_offset(frames[5])
    tens = [torch.frombuffer(bytearray(f), dtype=torch.uint8).to(DEV) for f in frames]
    got = framed.decompressed_sizes_device(tens)
    assert device.last_size_launch() == S_CLASS
    dec = [(st, int(t.numel()), used) for st, t, used in framed.decompress_frames_device(tens)]
    for k, (g, d) in enumerate(zip(got, dec)):
        want = (0,) + d[1:] if d[0] == o.F_FRAME_CHECKSUM_FAIL else d
        assert tuple(g) == tuple(want), (k, g, d)
    assert [d[0] for d in dec[:5]] == [0] * 5 and dec[3][1] == 1 << 20 and dec[5][0] not in (0, o.F_FRAME_CHECKSUM_FAIL)
    streams = [torch.frombuffer(bytearray(b"".join(frames[a:a + 3])), dtype=torch.uint8).to(DEV) for a in (0, 2)]
    index = framed.stream_index_device(streams)
    decoded = framed.decompress_streams_device(streams)
    for g, (st, t, used, nf) in zip(index, decoded):
        assert (g.status, g.out_len, g.consumed, g.n_frames) == (st, t.numel(), used, nf)
    assert [(g.status, g.n_frames, g.out_len) for g in index] == [(0, 3, 3 << 20)] * 2
