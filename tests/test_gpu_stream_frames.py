"""GPU tests (-m gpu) of the streams of back-to-back frames in device memory (include/lzfear_frame.h:
lzf_frame_stream_bound_device / lzf_frame_decompress_stream_device / lzf_frame_compress_stream_device).

Decode: status, bytes, `consumed` and the frame count of every stream are those of the loop a caller writes over
decompress_frame with `consumed` (the oracle; the host driver lzf_frame_decompress_many where the output capacity binds).
Compress: the bytes are the host driver's frames of the pieces, concatenated."""
import ctypes as C

import numpy as np
import pytest
import torch

import liblz4_ffi
import oracle_ffi as o
import redzone
import vectors
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi, framed, synth
from test_stream_frames_cpu import ended_at_endmark, lz4f_frames

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def dev(b):
    b = bytes(b)
    if not b:
        return torch.empty(0, dtype=torch.uint8, device=DEV)
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(DEV)


def mk(data, **kw):
    rc, f = o.frame_compress(data, o.make_settings(**kw))
    assert rc == 0
    return f


def ref_stream(data, dictionary=b"", cap=None, ocap=8 << 20):
    """The stream rule, restated: (status, bytes, consumed, frames).  Every frame through the oracle; through the host driver
    with the remaining capacity where the frame's output does not fit it (a frame whose output fits is never stopped by the
    capacity: the capacity is looked at block by block, behind the block's own errors)."""
    pos = out = good = 0
    parts, status = [], 0
    while pos < len(data):
        rest = data[pos:]
        rc, b, used = o.frame_decompress(rest, dictionary=dictionary, cap=ocap)
        if cap is not None and len(b) > cap - out:
            rc, b, used = framed.decompress_frames([rest], dictionary=dictionary, caps=[cap - out], with_consumed=True)[0]
        parts.append(b); out += len(b); pos += used
        if rc != 0:
            status = rc
            break
        if not ended_at_endmark(rest, used):
            break
        good += 1
    return status, b"".join(parts), pos, good


def run(streams, dictionary=b"", caps=None):
    """[(status, bytes, consumed, frames)] of lzf_frame_decompress_stream_device over byte strings."""
    d = dev(dictionary) if dictionary else None
    res = framed.decompress_streams_device([dev(s) for s in streams], dictionary=d, caps=caps)
    return [(st, bytes(t.cpu().numpy().tobytes()), used, nf) for st, t, used, nf in res]


def small_inputs():
    mix = synth.silesia_mix(30 << 20, (30 << 20) + 400_000).tobytes()
    return [mix[:5000], b"", mix[5000:5017], vectors.rng_bytes(3, 3000), mix[10_000:10_000 + 70_001], synth.repeat256(2 * 65536 + 77).tobytes(),
            mix[100_000:100_001], mix[200_000:330_000]]


FLAVOURS = [dict(block_size=64 << 10), dict(block_size=64 << 10, independent_blocks=False),
            dict(block_size=64 << 10, independent_blocks=False, block_checksums=True),
            dict(block_size=256 << 10, content_checksum=False, block_checksums=True),
            dict(block_size=64 << 10, content_checksum=False), dict(block_size=1 << 20)]


def pool():
    out = []
    for k, kw in enumerate(FLAVOURS):
        for d in small_inputs():
            out.append(mk(d, content_size=len(d) if k == 4 else None, **kw))
    return out


def test_streams_of_1_2_65_and_1100_frames_one_call():
    """Independent and linked frames, block and content checksums, content sizes and frames of empty content mixed in every
    stream; the empty stream; liblz4's own frames."""
    p = pool()
    rng = np.random.default_rng(11)
    streams = [p[0], p[9] + p[2], b"".join(p[int(i)] for i in rng.integers(0, len(p), 65)),
               b"".join(p[(7 * i) % len(p)] for i in range(1100)), b"", mk(b""), mk(b"") * 3, b"".join(lz4f_frames())]
    got = run(streams)
    for s, g in zip(streams, got):
        assert g == ref_stream(s, ocap=1 << 20)
        assert g[0] == 0 and g[2] == len(s)
    assert [g[3] for g in got] == [1, 2, 65, 1100, 0, 1, 3, 8]
    assert got[4] == (0, b"", 0, 0)


def test_dictionary_streams_linked_and_independent():
    dct = synth.gen_text_zipf(3, 70000).tobytes()
    ins = small_inputs()
    frames = [mk(d, block_size=64 << 10, dictionary=dct, dictionary_id=9, independent_blocks=bool((i + j) % 2))
              for i, d in enumerate(ins) for j in range(2)]
    streams = [b"".join(frames), b"".join(reversed(frames)), frames[4] + frames[5] + b"\x00"]
    got = run(streams, dictionary=dct)
    for s, g in zip(streams, got):
        assert g == ref_stream(s, dictionary=dct)
    assert [g[0] for g in got] == [0, 0, 16] and got[0][3] == len(frames) and got[2][2:] == (len(streams[2]), 2)
    assert got[0][1] == b"".join(d for d in ins for _ in range(2))


def test_trailing_bytes_and_foreign_magics():
    p = pool()
    two = p[5] + p[12]
    tails = [b"\x04", b"\x04\x22", b"\x04\x22\x4d", b"\x00\x00\x00\x00", b"\x00" * 7, b"\x50\x2a\x4d\x18\x04\x00\x00\x00abcd",
             b"\x02\x21\x4c\x18" + b"\x00" * 9]
    got = run([two + t for t in tails])
    for t, g in zip(tails, got):
        assert g == ref_stream(two + t)
        assert g[0] == (16 if len(t) < 4 else 17) and g[2] == len(two) + min(len(t), 4) and g[3] == 2


def test_damage_in_first_middle_and_last_frame():
    """A damaged block (codec error), a bad block checksum and a bad content checksum, each in the first, a middle and the last
    of five frames."""
    mix = synth.silesia_mix(41 << 20, (41 << 20) + 200_000).tobytes()
    plain = mk(mix, block_size=64 << 10, content_checksum=False)
    sums = mk(mix, block_size=64 << 10, block_checksums=True)
    hdr = 7
    assert plain[hdr + 3] == 0 and plain[hdr + 4] >= 0x10               # (block 0 is compressed and opens with literals)
    codec = bytearray(plain); codec[hdr + 4: hdr + 7] = b"\x00\x00\x00"    # block 0 opens with a match at offset 0
    second = hdr + 4 + int.from_bytes(plain[hdr:hdr + 4], "little")
    codec2 = bytearray(plain); codec2[second + 4: second + 7] = b"\x00\x00\x00"                    # block 1 does
    bsum = bytearray(sums); bsum[len(sums) // 2] ^= 0x40
    csum = bytearray(sums); csum[-1] ^= 1
    good = [plain, sums, mk(mix[:70_000], block_size=64 << 10, independent_blocks=False), mk(b"")]
    streams = []
    for bad in (bytes(codec), bytes(codec2), bytes(bsum), bytes(csum)):
        for at in (0, 2, 4):
            fr = [good[(k + at) % 4] for k in range(5)]
            fr[at] = bad
            streams.append(b"".join(fr))
    got = run(streams)
    kinds = set()
    for s, g in zip(streams, got):
        assert g == ref_stream(s)
        kinds.add(g[0])
    assert 19 in kinds and 20 in kinds and kinds & {1, 2, 3, 4}, kinds
    assert all(g[0] != 0 for g in got)
    assert [g[3] for g in got] == [0, 2, 4] * 4


def test_truncation_everywhere_in_a_middle_frame():
    """A + B[:k] for every k — every header byte, every length word, the payloads, the block checksum words, the EndMark and
    the content checksum of B cut short — and A + B[:k] + C at a few k: the bytes of C are then read as B's."""
    a = mk(synth.silesia_mix(0, 30_000).tobytes(), block_size=64 << 10)
    data = synth.repeat256(2 * 65536 + 500).tobytes()
    b = mk(data, block_size=64 << 10, block_checksums=True, content_size=len(data), independent_blocks=False)
    c = mk(b"tail frame", block_size=64 << 10)
    assert len(b) < 2000
    streams = [a + b[:k] for k in range(len(b) + 1)] + [a + b[:k] + c for k in (0, 3, 4, 7, 14, 15, 16, 19, 20, 100, len(b) - 8, len(b) - 4, len(b))]
    got = run(streams)
    kinds = set()
    for s, g in zip(streams, got):
        assert g == ref_stream(s, ocap=1 << 20), len(s)
        kinds.add(g[0])
    assert got[0][:1] + got[0][2:] == (0, len(a), 1) and got[len(b)][0] == 0 and got[len(b)][3] == 2
    assert all(g[0] == 16 and g[2] == len(a) + k for k, g in enumerate(got[:len(b) + 1]) if 0 < k < len(b))
    assert got[-1][0] == 0 and got[-1][3] == 3 and 16 in kinds


def test_capacity_at_the_total_and_around_every_frame_boundary():
    mix = synth.silesia_mix(50 << 20, (50 << 20) + 600_000).tobytes()
    datas = [mix[:150_000], mix[150_000:150_000 + 65536], b"", mix[300_000:300_001], mix[300_001:600_000]]
    frames = [mk(d, block_size=64 << 10, independent_blocks=bool(i % 2), block_checksums=i == 4) for i, d in enumerate(datas)]
    s = b"".join(frames)
    total = sum(len(d) for d in datas)
    edges = np.cumsum([len(d) for d in datas]).tolist()
    caps = sorted({max(0, e + k) for e in [0] + edges for k in (-1, 0, 1)} | {total + 1000, 65536, 65535})
    assert total in caps and total - 1 in caps
    got = run([s] * len(caps), caps=caps)
    for cap, g in zip(caps, got):
        assert g == ref_stream(s, cap=cap), cap
        assert g[0] == (0 if cap >= total else ffi.OUT_CAPACITY), cap
        assert len(g[1]) <= cap
    (bound,) = device.stream_decompress_bound([dev(s)])
    assert bound >= total and bound == sum(device.frame_decompress_bound([dev(f) for f in frames]))
    assert run([s]) == [(0, b"".join(datas), len(s), 5)]


def test_many_streams_aliasing_one_buffer():
    p = pool()
    order = [(5 * i + 1) % len(p) for i in range(40)]
    s = b"".join(p[i] for i in order)
    buf = dev(s + b"\x07\x07")
    starts = np.concatenate([[0], np.cumsum([len(p[i]) for i in order])]).tolist()
    views, want = [], []
    for k in range(0, 40, 3):
        for end in (starts[40], starts[min(k + 4, 40)], len(s) + 2):
            views.append(buf[starts[k]:end]); want.append(s[starts[k]:end] if end <= len(s) else s[starts[k]:] + b"\x07\x07")
    views += [buf[:len(s)]] * 20; want += [s] * 20
    res = framed.decompress_streams_device(views)
    assert len(res) == len(want) > 60
    for w, (st, t, used, nf) in zip(want, res):
        assert (st, bytes(t.cpu().numpy().tobytes()), used, nf) == ref_stream(w, ocap=1 << 20)


def test_memory_budget_passes_and_a_frame_over_the_budget():
    """Nine frames of 900 000 bytes in 64 KiB blocks ask for about 3.5 MB of the budget each (the frame, twice its blocks'
    slots): a budget of 8 MiB takes them two at a time, five passes for the one stream.  A budget below one frame ends the
    stream at that frame with LZF_E_NO_MEMORY, the frames before it stand."""
    data = [synth.silesia_mix((100 + k) << 20, ((100 + k) << 20) + 900_000).tobytes() for k in range(9)]
    frames = [mk(x, block_size=64 << 10, independent_blocks=bool(k % 2)) for k, x in enumerate(data)]
    small = mk(b"small frame in front", block_size=64 << 10)
    s = b"".join(frames)
    damaged = bytearray(s); damaged[sum(len(f) for f in frames[:6]) + len(frames[6]) - 1] ^= 1      # frame 6's content checksum
    try:
        ffi.lib().lzf_frame_set_memory_budget(8 << 20)
        got = run([s, bytes(damaged), s + b"\x01"], caps=[len(b"".join(data))] * 3)
        ffi.lib().lzf_frame_set_memory_budget(1 << 20)
        refused = run([small + small + frames[0] + small, frames[0], small], caps=[1 << 20] * 3)
    finally:
        ffi.lib().lzf_frame_set_memory_budget(0)
    assert got[0] == (0, b"".join(data), len(s), 9)
    assert got[1] == ref_stream(bytes(damaged)) and got[1][0] == 20 and got[1][3] == 6
    assert got[2] == (16, b"".join(data), len(s) + 1, 9)
    assert refused[0] == (ffi.E_NO_MEMORY, b"small frame in front" * 2, 2 * len(small), 2)
    assert refused[1] == (ffi.E_NO_MEMORY, b"", 0, 0)
    assert refused[2] == (0, b"small frame in front", len(small), 1)
    assert run([s])[0] == got[0]


def place(sizes, residues, fill, seed):
    """tests/redzone.py's layout: an arena filled with `fill` and the offsets of buffers of `sizes` bytes in it, each behind
    redzone.ZONE bytes and at an address whose low four bits are its entry of `residues` (the bits above them vary)."""
    rng = np.random.default_rng(seed)
    lows = [16 * int(rng.integers(0, 16)) + r for r in residues]
    offs, _, arena = redzone._place(sizes, lows, rng, DEV, True)
    arena.fill_(fill)
    assert [(arena.data_ptr() + at) & 15 for at in offs] == list(residues)
    return arena, offs


@pytest.mark.parametrize("in_poison", [0x00, 0xFF])
def test_decode_red_zones_at_all_16_residues(in_poison):
    """Sixteen streams in one call, stream i with its input at address residue i and its output at residue 5 i + 3 (mod 16):
    whole streams, a bad block checksum in a middle frame, capacities that end inside a frame, trailing bytes.  Everything
    outside [0, out_len) of every output is still redzone.OUT_POISON, and the results are the reference's under both input
    poisons: they do not depend on the bytes behind the streams."""
    p = pool()
    streams, caps, want = [], [], []
    for i in range(16):
        fr = [p[(3 * i + 5 * k) % len(p)] for k in range(3 + i % 4)]
        if i % 4 == 1:
            bad = bytearray(p[21]); bad[len(bad) // 2] ^= 0x10           # (flavour 2: linked, block checksums)
            fr[1] = bytes(bad)
        s = b"".join(fr) + (b"\x04\x22\x4d" if i % 4 == 3 else b"")
        full = ref_stream(s, ocap=1 << 20)
        cap = len(full[1]) + 100 if i % 4 != 2 else max(len(full[1]) - 1 - 1000 * i, 0)
        streams.append(s); caps.append(cap); want.append(ref_stream(s, cap=cap, ocap=1 << 20))
    poison = redzone.OUT_POISON
    in_arena, in_offs = place([len(s) for s in streams], list(range(16)), in_poison, 1)
    for s, at in zip(streams, in_offs):
        in_arena[at:at + len(s)] = dev(s)
    out_arena, out_offs = place(caps, [(5 * i + 3) % 16 for i in range(16)], poison, 2)
    ins = [in_arena[at:at + len(s)] for s, at in zip(streams, in_offs)]
    outs = [out_arena[at:at + c] for at, c in zip(out_offs, caps)]
    assert sorted(t.data_ptr() & 15 for t in ins) == list(range(16)) == sorted(t.data_ptr() & 15 for t in outs)
    status, out_len, used, nf = device.stream_decompress(ins, outs)
    torch.cuda.synchronize()
    h = out_arena.cpu().numpy()
    expect = np.full_like(h, poison)
    kinds = set()
    for at, w, st, ln, u, n in zip(out_offs, want, status.tolist(), out_len.tolist(), used.tolist(), nf.tolist()):
        assert (st, ln, u, n) == (w[0], len(w[1]), w[2], w[3])
        expect[at:at + ln] = np.frombuffer(w[1], dtype=np.uint8)
        kinds.add(st)
    assert kinds == {0, 16, 19, ffi.OUT_CAPACITY}, kinds
    assert np.array_equal(h, expect)


# ---- the write side --------------------------------------------------------------------------------------------------------

def pieces_of(data, fb):
    return [data[k:k + fb] for k in range(0, len(data), fb)] or [b""]


def settings(block_size, independent=True, block_checksums=False, dictionary=None):
    cs = framed.CompressionSettings().block_size(block_size).independent_blocks(independent).block_checksums(block_checksums)
    if dictionary is not None:
        cs.dictionary(77, dictionary)
    return cs


def host_stream(cs, data, fb, with_size):
    ps = pieces_of(data, fb)
    return b"".join(cs.compress_with_size(x) for x in ps) if with_size else b"".join(cs.compress_many(ps))


def test_compress_streams_are_the_host_frames_concatenated():
    mix = synth.silesia_mix(60 << 20, (60 << 20) + (9 << 20) + 12345).tobytes()
    noise = vectors.rng_bytes(5, 300_000)
    dct = synth.gen_text_zipf(3, 70000).tobytes()
    cases = []
    for bs in (64 << 10, 256 << 10, 1 << 20, 4 << 20):
        for indep in (True, False):
            cases.append((settings(bs, indep), [mix[:2 * bs + bs // 2 + 17], mix[bs:2 * bs]], bs + bs // 3, False))
    cases.append((settings(4 << 20), [mix], 5 << 20, False))                                      # pieces of more than one 4 MiB block
    cases.append((settings(64 << 10, block_checksums=True), [mix[:300_000], b"", mix[:1], mix[:40_000]], 40_000, False))   # frame_bytes < a block
    cases.append((settings(64 << 10, False, True), [mix[:100_000] + noise + mix[:100_000], noise], 100_000, True))    # stored blocks, content size
    cases.append((settings(64 << 10, True, dictionary=dct), [mix[:400_000], mix[400_000:500_001]], 150_000, True))
    cases.append((settings(64 << 10, False, dictionary=dct), [mix[:400_000], b""], 150_000, False))
    for cs, datas, fb, with_size in cases:
        got = cs.compress_streams_device([dev(d) for d in datas], fb, with_size=with_size)
        for d, t in zip(datas, got):
            b = bytes(t.cpu().numpy().tobytes())
            assert b == host_stream(cs, d, fb, with_size), (fb, len(d))
            # round trip through the stream decode, and frame by frame through liblz4's own frame reader
            dd = cs._dictionary or b""
            assert run([b], dictionary=dd) == [(0, d, len(b), len(pieces_of(d, fb)))]
            if liblz4_ffi.available() and not dd:
                pos = 0
                for x in pieces_of(d, fb):
                    _, _, used = o.frame_decompress(b[pos:], cap=len(x) + 64)
                    assert liblz4_ffi.lz4f_decompress(b[pos:pos + used], len(x) + 64) == (True, x)
                    pos += used
                assert pos == len(b)


@pytest.mark.parametrize("indep", [True, False])
def test_compress_streams_of_65_frames_cross_the_packing_round(indep):
    """65 frames of one 64 KiB block per stream, block checksums on: the packing kernel places 64 frames per round, so frame 64
    goes behind the first round's total (the carry of the wave scan); the stream decode then places the same 65 frames.  A
    second stream of 66 pieces, the last one short, in the same call."""
    mix = synth.silesia_mix(80 << 20, (80 << 20) + 65 * 65536 + 1234).tobytes()
    datas = [mix[:65 * 65536], mix]
    fb = 64 << 10
    cs = settings(64 << 10, indep, True)
    got = cs.compress_streams_device([dev(d) for d in datas], fb)
    for d, t, nf in zip(datas, got, (65, 66)):
        b = bytes(t.cpu().numpy().tobytes())
        assert b == host_stream(cs, d, fb, False)
        assert run([b]) == [ref_stream(b, ocap=1 << 20)] == [(0, d, len(b), nf)]


@pytest.mark.parametrize("in_poison", [0x00, 0xFF])
def test_compress_capacity_edge_under_red_zones(in_poison):
    """out_cap one below lzf_frame_compress_stream_bound: LZF_OUT_CAPACITY and not a byte written; at the bound: the stream, and
    nothing outside [0, out_len).  Inputs and outputs at odd addresses."""
    mix = synth.silesia_mix(70 << 20, (70 << 20) + 500_000).tobytes()
    datas = [mix[:300_001], mix[300_001:], b"", vectors.rng_bytes(8, 150_000), mix[:300_001]]
    fb = 70_000
    cs = settings(64 << 10, block_checksums=True)
    s = cs._struct(None); s.dictionary = None; s.dictionary_len = 0
    bounds = [ffi.lib().lzf_frame_compress_stream_bound(C.byref(s), fb, len(d)) for d in datas]
    caps = [b - 1 if i % 2 else b for i, b in enumerate(bounds)]
    poison = redzone.OUT_POISON
    in_arena, in_offs = place([len(d) for d in datas], [1, 7, 3, 15, 10], in_poison, 3)
    for d, at in zip(datas, in_offs):
        in_arena[at:at + len(d)] = dev(d)
    out_arena, out_offs = place(caps, [13, 2, 5, 9, 0], poison, 4)
    ins = [in_arena[at:at + len(d)] for d, at in zip(datas, in_offs)]
    outs = [out_arena[at:at + c] for at, c in zip(out_offs, caps)]
    status, out_len = device.stream_compress(s, fb, ins, outs)
    torch.cuda.synchronize()
    h = out_arena.cpu().numpy()
    expect = np.full_like(h, poison)
    for i, (d, at, st, ln) in enumerate(zip(datas, out_offs, status.tolist(), out_len.tolist())):
        if i % 2:
            assert (st, ln) == (ffi.OUT_CAPACITY, 0)
        else:
            w = host_stream(cs, d, fb, False)
            assert (st, ln) == (0, len(w))
            expect[at:at + ln] = np.frombuffer(w, dtype=np.uint8)
    assert np.array_equal(h, expect)
