"""GPU tests (-m gpu) of the exact sizes and the frame index of streams of back-to-back frames in device memory
(include/lzfear_frame.h: lzf_frame_stream_count_device / lzf_frame_stream_decompressed_size_device / lzf_stream_index_locate) and
of what Python builds on them (framed.stream_index_device, read_stream_range_device, decompress_streams_device(exact=True)).

Per stream the results are the decode call's (framed.decompress_streams_device).  Per frame: the start is the CPU walk's, the
size results are framed.decompressed_sizes_device's on stream[in_off:], and place and flags follow the stream rule of
lzfear_frame.h, restated here over those per-frame results."""
import struct

import numpy as np
import pytest
import torch

import oracle_ffi as o
import redzone
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi, framed, synth
from test_device_frames_cpu import py_scan_blocks
from test_gpu_stream_frames import FLAVOURS
from test_stream_frames_cpu import lz4f_frames
from test_stream_index_cpu import py_header

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
COMPLETE, BEHIND = ffi.SFRAME_COMPLETE, ffi.SFRAME_BEHIND_STOP
NO_SIZE = ffi.STREAM_NO_CONTENT_SIZE
FIELDS = ("in_off", "consumed", "out_off", "out_len", "content_size", "status", "flags")


def dev(b):
    b = bytes(b)
    if not b:
        return torch.empty(0, dtype=torch.uint8, device=DEV)
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(DEV)


def mk(data, **kw):
    rc, f = o.frame_compress(data, o.make_settings(**kw))
    assert rc == 0
    return f


def structure(data):
    """The CPU walk: [(start, where the frame's structural walk ends at its EndMark or None, the header's content size)] of every
    frame found, the failing last one included."""
    out, pos, view = [], 0, memoryview(data)
    while pos < len(data):
        rest = view[pos:]
        hst, hlen, flg = py_header(rest)
        if hst:
            out.append((pos, None, NO_SIZE))
            break
        werr, wcons = py_scan_blocks(rest, hlen, flg, 1 << (((rest[5] >> 4) & 7) * 2 + 8))[1]
        out.append((pos, None if werr else wcons, struct.unpack_from("<Q", rest, 6)[0] if flg & 8 else NO_SIZE))
        if werr:
            break
        pos += wcons
    return out


def rule(frames, sizes):
    """The stream rule of lzfear_frame.h over per-frame results: `frames` from structure(), `sizes` [(status, out_len, consumed)].
    Returns (entries as dicts, (status, out_len, consumed, n_frames))."""
    run = cons = good = status = 0
    stopped, entries = False, []
    for (start, full, csize), (st, n, c) in zip(frames, sizes):
        complete = st == 0 and full is not None and c == full
        entries.append(dict(in_off=start, consumed=c, out_off=run, out_len=n, content_size=csize, status=st,
                            flags=(COMPLETE if complete else 0) | (BEHIND if stopped else 0)))
        if stopped:
            continue
        run += n; cons += c
        if complete:
            good += 1
        else:
            status, stopped = st, True
    return entries, (status, run, cons, good)


def check(streams, dictionary=b"", same_as_decode=True):
    """The size + index call over byte strings against the rule; returns ([StreamIndex], [the rule's stream results])."""
    tens = [dev(s) for s in streams]
    got = framed.stream_index_device(tens, dictionary_len=len(dictionary))
    frames = [structure(s) for s in streams]
    views = [t[start:] for t, fr in zip(tens, frames) for start, _, _ in fr]
    sizes = framed.decompressed_sizes_device(views, dictionary_len=len(dictionary))
    decoded = framed.decompress_streams_device(tens, dictionary=dev(dictionary) if dictionary else None) if same_as_decode else None
    at, results = 0, []
    for k, (s, fr, g) in enumerate(zip(streams, frames, got)):
        want, res = rule(fr, sizes[at:at + len(fr)])
        at += len(fr)
        assert len(g.frames) == len(want), k
        for f in FIELDS:
            assert g.frames[f].tolist() == [e[f] for e in want], (k, f)
        assert (g.status, g.out_len, g.consumed, g.n_frames) == res, k
        if decoded is not None:
            st, t, used, nf = decoded[k]
            assert (g.status, g.out_len, g.consumed, g.n_frames) == (st, t.numel(), used, nf), k
        results.append(res)
    return got, results


def small_inputs():
    mix = synth.silesia_mix(30 << 20, (30 << 20) + 400_000).tobytes()
    return [mix[:5000], b"", mix[5000:5017], mix[10_000:10_000 + 70_001], mix[100_000:100_001], mix[200_000:330_000]]


@pytest.fixture(scope="module")
def pool():
    return [mk(d, content_size=len(d) if k == 4 else None, **kw) for k, kw in enumerate(FLAVOURS) for d in small_inputs()]


def flip_payload(frame, header_len=7):
    """One payload byte of the frame's first block flipped (under its block checksum)."""
    bad = bytearray(frame); bad[header_len + 4 + 2] ^= 0x20
    return bytes(bad)


# ---- 1. sizes equal the decode ---------------------------------------------------------------------------------------------

def test_sizes_and_entries_of_streams_of_1_2_65_and_1100_frames(pool):
    p = pool
    rng = np.random.default_rng(11)
    streams = [p[0], p[9] + p[2], b"".join(p[int(i)] for i in rng.integers(0, len(p), 65)),
               b"".join(p[(7 * i) % len(p)] for i in range(1100)), b"", mk(b""), mk(b"") * 3, b"".join(lz4f_frames())]
    got, res = check(streams)
    assert [r[3] for r in res] == [1, 2, 65, 1100, 0, 1, 3, 8] == [len(g.frames) for g in got]
    assert all(r[0] == 0 and r[2] == len(s) for r, s in zip(res, streams))
    assert res[4] == (0, 0, 0, 0)
    assert all((g.frames["flags"] == COMPLETE).all() for g in got)
    sized = set(got[3].frames["content_size"].tolist())
    assert NO_SIZE in sized and {len(d) for d in small_inputs()} < sized
    assert framed.stream_index_device([]) == [] and device.stream_count([]) == []


def test_dictionary_stream_of_linked_and_independent_frames():
    dct = synth.gen_text_zipf(3, 70000).tobytes()
    ins = small_inputs()
    frames = [mk(d, block_size=64 << 10, dictionary=dct, dictionary_id=9, independent_blocks=bool((i + j) % 2))
              for i, d in enumerate(ins) for j in range(2)]
    streams = [b"".join(frames), b"".join(reversed(frames)), frames[4] + frames[5] + b"\x00"]
    got, res = check(streams, dictionary=dct)
    assert [r[0] for r in res] == [0, 0, 16] and res[0][1] == 2 * sum(len(d) for d in ins) and res[2][2:] == (len(streams[2]), 2)


# ---- 2. round carries ------------------------------------------------------------------------------------------------------

def test_the_running_length_and_the_stop_carry_from_round_to_round():
    """63, 64, 65, 128 and 129 frames, the ending frame (one payload byte flipped under a block checksum) at index 0, 62, 63,
    64, 65 and last: the kernel takes 64 frames per round."""
    mix = synth.silesia_mix(7 << 20, (7 << 20) + 4000).tobytes()
    kinds = [mk(mix[:300 + 211 * k], block_size=64 << 10, block_checksums=True, independent_blocks=bool(k % 2)) for k in range(4)] + [mk(b"")]
    bad = flip_payload(kinds[1])
    streams, where = [], []
    for n in (63, 64, 65, 128, 129):
        for at in sorted({0, 62, 63, 64, 65, n - 1}):
            if at < n:
                fr = [kinds[(3 * k + n) % 5] for k in range(n)]
                fr[at] = bad
                streams.append(b"".join(fr)); where.append((n, at))
    assert len(streams) == 21
    got, res = check(streams)
    for (n, at), g, r in zip(where, got, res):
        assert len(g.frames) == n and r[0] == 19 and r[3] == at, (n, at)
        assert (g.frames["flags"] & BEHIND != 0).tolist() == [k > at for k in range(n)], (n, at)
        assert (g.frames["flags"] & COMPLETE != 0).tolist() == [k != at for k in range(n)], (n, at)
        assert (g.frames["out_off"][at + 1:] == r[1]).all(), (n, at)
        assert r[1] == int(g.frames["out_len"][:at + 1].sum()), (n, at)


# ---- 3. every kind of stop -------------------------------------------------------------------------------------------------

def test_every_kind_of_stop(pool):
    mix = synth.silesia_mix(41 << 20, (41 << 20) + 100_000).tobytes()
    plain = mk(mix, block_size=64 << 10, content_checksum=False)
    assert plain[7 + 3] == 0 and plain[7 + 4] >= 0x10               # (block 0 is compressed and opens with literals)
    codec = bytearray(plain); codec[7 + 4: 7 + 7] = b"\x00\x00\x00"  # block 0 opens with a match at offset 0
    empty_block = plain[:7] + (1).to_bytes(4, "little") + b"\x00" + plain[7:]          # a compressed block of one token: no bytes
    rc, out, used = o.frame_decompress(empty_block, cap=1 << 20)
    assert (rc, out, used) == (0, b"", 12)                          # the reader stops there with LZF_OK, in front of the EndMark
    a, b, c = pool[0], pool[9], pool[27]
    streams = [a + bytes(codec) + b, bytes(codec) + a, a + b[:len(b) // 2], a + b + c[:5], a + empty_block + b + c, empty_block]
    tails = [b"\x04", b"\x04\x22", b"\x04\x22\x4d", b"\x00\x00\x00\x00", b"\x00" * 7, b"\x50\x2a\x4d\x18\x04\x00\x00\x00abcd"]
    streams += [a + b + t for t in tails]
    got, res = check(streams)
    assert res[0][0] in (1, 2, 3, 4) and res[0][3] == 1 and len(got[0].frames) == 3 and got[0].frames["flags"].tolist() == [COMPLETE, 0, COMPLETE | BEHIND]
    assert res[1][0] in (1, 2, 3, 4) and res[1][3] == 0
    assert res[2][0] == 16 and res[2][2] == len(streams[2]) and got[2].frames["flags"].tolist() == [COMPLETE, 0]
    assert res[3][0] == 16 and res[3][3] == 2
    assert res[4] == (0, len(small_inputs()[0]), len(a) + 12, 1)    # LZF_OK in mid-frame: the stream ends, the walk lists what follows
    assert got[4].frames["flags"].tolist() == [COMPLETE, 0, COMPLETE | BEHIND, COMPLETE | BEHIND] and got[4].frames["status"].tolist() == [0] * 4
    assert res[5] == (0, 0, 12, 0)
    for t, g, r in zip(tails, got[6:], res[6:]):
        assert len(g.frames) == 3                                   # trailing bytes are listed as a frame
        assert (r[0], r[2], r[3]) == ((16, len(a + b) + len(t), 2) if len(t) < 4 else (17, len(a + b) + 4, 2)), t
        assert g.frames["content_size"][2] == NO_SIZE and g.frames["flags"][2] == 0 and g.frames["out_len"][2] == 0


# ---- 4. the documented exception -------------------------------------------------------------------------------------------

def test_a_content_checksum_is_not_verified(pool):
    a, b, c = pool[0], pool[5], pool[3]
    bad = bytearray(b); bad[-1] ^= 1
    s = a + bytes(bad) + c
    (st, t, used, nf), = framed.decompress_streams_device([dev(s)])
    assert (st, nf, used) == (20, 1, len(a) + len(b))
    got, res = check([s], same_as_decode=False)
    assert res[0] == (0, sum(len(small_inputs()[k]) for k in (0, 5, 3)), len(s), 3)
    assert got[0].frames["flags"].tolist() == [COMPLETE] * 3 and got[0].frames["status"].tolist() == [0] * 3
    assert got[0].out_len >= t.numel()


# ---- 5. capacity -----------------------------------------------------------------------------------------------------------

def test_index_capacity_under_red_zones(pool):
    s = b"".join(pool[(5 * k + 1) % len(pool)] for k in range(70)) + b"\x00\x01\x02\x03\x04"
    t = dev(s)
    full = framed.stream_index_device([t])[0]
    found = len(full.frames)
    assert found == 71 and device.stream_count([t, t[:0], t[len(pool[1]):]]) == [71, 0, 70]
    caps = [0, 1, found - 1, found, found + 5]
    rng = np.random.default_rng(3)
    lows = [16 * int(rng.integers(0, 16)) + r for r in (0, 8, 8, 0, 8)]
    offs, _, arena = redzone._place([48 * c for c in caps], lows, rng, DEV, True)
    arena.fill_(redzone.OUT_POISON)
    rooms = [arena[at:at + 48 * c] for at, c in zip(offs, caps)]
    status, out_len, consumed, n_frames, n_listed = device.stream_decompressed_size([t] * 5, index=rooms)
    plain = device.stream_decompressed_size([t] * 5)                 # d_index / index_cap both NULL: sizes only
    torch.cuda.synchronize()
    assert n_listed.tolist() == [found] * 5 == plain[4].tolist()
    for x, y in zip((status, out_len, consumed, n_frames), plain):
        assert x.tolist() == y.tolist() == [x.tolist()[0]] * 5
    assert (status[0].item(), out_len[0].item(), consumed[0].item(), n_frames[0].item()) == (full.status, full.out_len, full.consumed, full.n_frames)
    h = arena.cpu().numpy()
    expect = np.full_like(h, redzone.OUT_POISON)
    for at, c in zip(offs, caps):
        k = min(c, found)
        expect[at:at + 48 * k] = full.frames[:k].view(np.uint8)
    assert np.array_equal(h, expect)                                # exactly min(cap, found) entries, nothing else


# ---- 6. many streams -------------------------------------------------------------------------------------------------------

def test_130_streams_some_aliasing_one_tensor_some_empty(pool):
    p = pool
    order = [(5 * i + 1) % len(p) for i in range(40)]
    s = b"".join(p[i] for i in order)
    buf = dev(s + b"\x07\x07")
    starts = np.concatenate([[0], np.cumsum([len(p[i]) for i in order])]).tolist()
    views, data = [], []
    for k in range(130):
        if k % 9 == 4:
            views.append(buf[:0]); data.append(b"")
        elif k % 3 == 0:
            a, b = starts[k % 40], (len(s) + 2 if k % 2 else starts[min(k % 40 + 1 + k % 7, 40)])
            views.append(buf[a:b]); data.append((s + b"\x07\x07")[a:b])
        else:
            d = p[k % len(p)] + p[(k * 7) % len(p)] * (k % 4)
            views.append(dev(d)); data.append(d)
    got = framed.stream_index_device(views)
    decoded = framed.decompress_streams_device(views)
    sizes_at = [structure(d) for d in data]
    for k, (g, (st, t, used, nf), fr) in enumerate(zip(got, decoded, sizes_at)):
        assert (g.status, g.out_len, g.consumed, g.n_frames) == (st, t.numel(), used, nf), k
        assert g.frames["in_off"].tolist() == [x[0] for x in fr], k
        ok = g.frames["flags"] & BEHIND == 0
        assert int(g.frames["out_len"][ok].sum()) == g.out_len, k
    assert {g.status for g in got} == {0, 16} and sum(len(g.frames) == 0 for g in got) >= 14


# ---- 7. range reads --------------------------------------------------------------------------------------------------------

def test_range_reads_decode_only_the_frames_they_need(pool, monkeypatch):
    p = pool
    order = [(7 * i + 3) % len(p) for i in range(40)]
    order[10] = order[11] = 1; order[25] = 7                        # frames of zero length inside, two of them in a row
    frames = [p[i] for i in order]
    s = b"".join(frames)
    t = dev(s)
    (index,) = framed.stream_index_device([t])
    (st, whole, used, nf), = framed.decompress_streams_device([t])
    assert (st, nf, index.out_len) == (0, 40, whole.numel()) and (index.frames["out_len"] == 0).sum() >= 3
    plain = whole.cpu().numpy()
    seen = []
    real = device.stream_decompress
    monkeypatch.setattr(device, "stream_decompress", lambda streams, *a, **kw: (seen.append([x.numel() for x in streams]), real(streams, *a, **kw))[1])
    off = index.frames["out_off"].tolist() + [index.out_len]
    con = index.frames["consumed"].tolist()
    edges = sorted(set(off))
    ranges = [(max(e + d, 0), e2 + d2) for e, e2, d, d2 in zip(edges, edges[1:] + [edges[-1]], (-1, 0, 1) * 20, (1, 0, -1, 0) * 20)]
    ranges += [(e - 1, e + 1) for e in edges[1:]] + [(e, e) for e in edges[:3]]
    ranges += [(off[11], off[12]), (off[10], off[10]), (off[20] + 5, off[20] + 9), (5, 5), (9, 3), (index.out_len - 7, index.out_len + 100),
               (index.out_len, index.out_len + 5), (0, index.out_len), (0, 1 << 62), (off[9] - 1, off[12] + 1), (off[13] + 1, off[30])]
    assert len(ranges) >= 60
    for a, b in ranges:
        seen.clear()
        got = framed.read_stream_range_device(t, index, a, b)
        assert np.array_equal(got.cpu().numpy(), plain[a:b] if a < b else plain[:0]), (a, b)
        hit = [k for k in range(40) if off[k] < min(b, index.out_len) and off[k + 1] > a and off[k + 1] > off[k]]
        assert seen == ([[sum(con[hit[0]:hit[-1] + 1])]] if hit and a < b else []), (a, b)
    # a damaged frame: reads that touch it fail, reads wholly in front of it do not
    two = p[15]                                                     # (flavour 2: linked, block checksums; two blocks)
    assert two[4] & 0x10 and len(small_inputs()[3]) > 65536
    second = 7 + 4 + int.from_bytes(two[7:11], "little") + 4
    bad = list(frames); bad[20] = flip_payload(two, header_len=second)      # block 0 is delivered, block 1 fails its checksum
    tb = dev(b"".join(bad))
    (ib,) = framed.stream_index_device([tb])
    assert ib.status == 19 and ib.n_frames == 20 and ib.frames["flags"][21] & BEHIND and ib.frames["out_len"][20] == 65536
    ob = ib.frames["out_off"].tolist()
    front = framed.read_stream_range_device(tb, ib, 3, ob[20])
    assert np.array_equal(front.cpu().numpy(), plain[3:ob[20]])
    for a, b in ((ob[20] - 1, ob[20] + 1), (0, ib.out_len), (ob[20] + 100, ob[20] + 200)):
        with pytest.raises(framed.FrameError) as e:
            framed.read_stream_range_device(tb, ib, a, b)
        assert e.value.code == 19


# ---- 8. exact outputs ------------------------------------------------------------------------------------------------------

def test_decompress_streams_device_exact(pool):
    p = pool
    streams = [b"".join(p[(3 * i) % len(p)] for i in range(20)), b"", p[5] + flip_payload(p[14]) + p[0], p[4] + b"\x01\x02", mk(b"")]
    tens = [dev(s) for s in streams]
    default = framed.decompress_streams_device(tens)
    exact = framed.decompress_streams_device(tens, exact=True)
    assert {d[0] for d in default} == {0, 16, 19}
    for (st, t, used, nf), (est, et, eused, enf) in zip(default, exact):
        assert (st, used, nf) == (est, eused, enf) and torch.equal(t, et)
        assert et.untyped_storage().nbytes() == et.numel() == t.numel()
    assert any(t.untyped_storage().nbytes() > t.numel() for _, t, _, _ in default)
