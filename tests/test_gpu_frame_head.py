"""GPU tests (-m gpu) of lzf_frame_head_device: the first bytes of every frame held in device memory.  Held to frame_head_cases.py's
expectations (the walk restated in Python over the oracle's block decodes): status, out_len and bytes, with every other byte of
every arena unchanged; at every alignment of output, target, frame and dictionary; against lzf_frame_decompressed_size_device and
lzf_frame_decompress_device_many on one set of frames; with more frames than the device holds wavefronts; and through the Python
layer.  Damaged inputs here are data errors that end in a status."""
import numpy as np
import pytest
import torch

import block_index_cases as B
import frame_head_cases as cases
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi, framed

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


def run(frames, which, targets, exps, dictionary=b"", poison=0xA5, in_res=None, out_res=None, dict_res=0, null_out=(), stream=None, what=""):
    """One lzf_frame_head_device: job i reads frames[which[i]] (the jobs ALIAS the frames) and writes an output of its own —
    exps[i][3] bytes of poison, poison around — at targets[i].  Checks status, out_len and bytes of every job; the whole output
    arena against its picture before the call with the expected bytes put in (where a status other than LZF_OK is expected, the
    room below the target is unspecified and left out); the frames, the dictionary and the red zones around the two result arrays."""
    n = len(which)
    d_in, in_off, _ = _arena(frames, poison, in_res)
    d_dic, dic_off, _ = _arena([dictionary], poison, [dict_res])
    dic = d_dic[int(dic_off[0]):int(dic_off[0]) + len(dictionary)] if dictionary else None
    rooms = [e[3] for e in exps]
    d_out, out_off, h_out = _arena([bytes([poison]) * r for r in rooms], poison, out_res)
    res = torch.full((3 * ZONE + 12 * n,), poison, dtype=torch.uint8, device=DEV)
    d_len, d_st = res[ZONE:ZONE + 8 * n].view(torch.int64), res[2 * ZONE + 8 * n:2 * ZONE + 12 * n].view(torch.int32)
    before = d_in.clone(), d_dic.clone()
    s = stream or torch.cuda.current_stream()
    s.wait_stream(torch.cuda.current_stream())
    device.frame_head_raw([d_in.data_ptr() + int(in_off[k]) for k in which], [len(frames[k]) for k in which],
                          [0 if i in null_out else d_out.data_ptr() + int(a) for i, a in enumerate(out_off)], targets, d_len, d_st, dictionary=dic, stream=s)
    s.synchronize()
    st, ln = d_st.cpu().numpy(), d_len.cpu().numpy()
    got, want, bad = d_out.cpu().numpy(), h_out.copy(), []
    for i, e in enumerate(exps):
        a = int(out_off[i])
        if (int(st[i]), int(ln[i])) != tuple(e[:2]):
            bad.append((what, i, which[i], targets[i], (int(st[i]), int(ln[i])), e[:2]))
        elif e[2] is not None:
            want[a:a + len(e[2])] = np.frombuffer(e[2], dtype=np.uint8)
        else:
            want[a:a + rooms[i]] = got[a:a + rooms[i]]
    assert not bad, (len(bad), bad[:10])
    if not np.array_equal(got, want):
        d = np.flatnonzero(got != want)
        i = int(np.searchsorted(out_off, d[0], side="right")) - 1
        raise AssertionError((what, "job", i, "target", targets[i], "byte", int(d[0]) - int(out_off[i]), "of out", int(got[d[0]]), "expected", int(want[d[0]]), len(d), "bytes differ"))
    assert torch.equal(before[0], d_in) and torch.equal(before[1], d_dic), "the call wrote to a frame or to the dictionary"
    r = res.cpu().numpy()
    assert (r[:ZONE] == poison).all() and (r[ZONE + 8 * n:2 * ZONE + 8 * n] == poison).all() and (r[2 * ZONE + 12 * n:] == poison).all(), "red zone around the results"
    return st, ln


def _by_dictionary(rows):
    groups = {}
    for c, e in rows:
        groups.setdefault(c["dict"], []).append((c, e))
    return groups


@pytest.mark.parametrize("poison", [0xA5, 0x5A])
def test_every_case_with_red_zones(rows, poison):
    """Every case, one call per dictionary, two poisons.  A job that asks for nothing hands in a NULL output every other time."""
    groups = _by_dictionary(rows)
    assert len(groups) == 2
    for dic, some in groups.items():
        cs, exps = [c for c, _ in some], [e for _, e in some]
        null_out = {i for i, c in enumerate(cs) if c["target"] == 0 and i % 2 == 0}
        run([c["frame"] for c in cs], list(range(len(cs))), [c["target"] for c in cs], exps, dictionary=dic, poison=poison, null_out=null_out,
            what="with the dictionary" if dic else "no dictionary")


def test_every_alignment():
    """16 clean frames, the output at all 16 address residues x the target at all 16 residues, the frames at residues 0, 1, 3, 15,
    the dictionary at 0 and 5."""
    clean = cases.clean_frames()
    assert len(clean) == 16
    done = 0
    for dic in (b"", cases.dictionary_bytes()):
        some = [(f, d) for _, f, d in clean if d == dic]
        frames, in_res = [], []
        for f, _ in some:
            for r in (0, 1, 3, 15):
                frames.append(f); in_res.append(r)
        which, targets, exps, out_res = [], [], [], []
        for k, (f, _) in enumerate(some):
            starts, _total = cases.block_starts(f, dic)
            base = starts[2] + 40 + k                       # inside block 2: a stored block and a compressed block lie in front
            for o_r in range(16):
                for t_r in range(16):
                    which.append(4 * k + (o_r + t_r) % 4); targets.append(base + t_r); out_res.append(o_r)
                    exps.append(cases.model(f, dic, base + t_r))
        assert all(e[0] == 0 and e[1] == t for e, t in zip(exps, targets))
        for dict_res in ((0, 5) if dic else (0,)):
            run(frames, which, targets, exps, dictionary=dic, in_res=in_res, out_res=out_res, dict_res=dict_res, what=f"dictionary at {dict_res}")
            done += len(which)
    assert done == 3 * 8 * 256


def test_agrees_with_the_size_query_and_the_decode(rows):
    """On one set of frames at the far target: where the frame has no block checksums, status and out_len are
    lzf_frame_decompressed_size_device's; on clean frames the bytes are the first out_len bytes lzf_frame_decompress_device_many
    writes."""
    n_size = n_bytes = 0
    for dic, some in _by_dictionary(rows).items():
        seen, cs = set(), []
        for c, _ in some:
            if c["cls"] in ("contract", "header") or (c["cls"] == "cut" and len(c["frame"]) % 40) or c["frame"] in seen:
                continue
            seen.add(c["frame"]); cs.append(c)
        frames = [c["frame"] for c in cs]
        names = [c["name"] for c in cs]
        if not dic:                                                # twenty more clean frames
            frames += [B.good_frame(3, seed, content_checksum=bool(seed % 2)) for seed in range(5, 25)]
            names += [f"a clean frame of three blocks, seed {seed}" for seed in range(5, 25)]
        exps = [cases.model(f, dic, cases.FAR) for f in frames]
        d_in, in_off, _ = _arena(frames, 0xA5)
        views = [d_in[int(a):int(a) + len(f)] for a, f in zip(in_off, frames)]
        d_dic = torch.frombuffer(bytearray(dic), dtype=torch.uint8).to(DEV) if dic else None
        s_st, s_len, _ = device.frame_decompressed_size(views, dictionary_len=len(dic))
        outs = [torch.zeros(e[3] + 16, dtype=torch.uint8, device=DEV) for e in exps]
        d_st, d_len, _ = device.frame_decompress_many(views, outs, dictionary=d_dic)
        heads, h_len, h_st = device.frame_heads(views, 4096, dictionary=d_dic)
        st, ln = run(frames, list(range(len(frames))), [cases.FAR] * len(frames), exps, dictionary=dic, what="agreement")
        torch.cuda.synchronize()
        s_st, s_len, d_st, d_len, h_len, h_st = (t.cpu().numpy() for t in (s_st, s_len, d_st, d_len, h_len, h_st))
        for i, f in enumerate(frames):
            if not B.walk(f)["flg"] & 0x10:
                assert (int(st[i]), int(ln[i])) == (int(s_st[i]), int(s_len[i])), (i, names[i])
                n_size += 1
            if int(d_st[i]) == 0:                               # a clean frame: the decode wrote its bytes
                assert int(st[i]) == 0 and int(ln[i]) == int(d_len[i]) and exps[i][2] == bytes(outs[i][:int(d_len[i])].cpu().numpy()), names[i]
                k = min(4096, int(d_len[i]))
                assert int(h_st[i]) == 0 and int(h_len[i]) == k and torch.equal(heads[i, :k], outs[i][:k]) and not bool(heads[i, k:].any()), names[i]
                n_bytes += 1
    assert n_size >= 30 and n_bytes >= 30, (n_size, n_bytes)
    # the documented contract: block checksums are not verified here.  A flipped literal byte under a sound checksum word reads
    # LZF_OK with the flipped byte in the head, while the size query refuses the frame
    f, lit_at = cases.flipped_frame()
    t = torch.frombuffer(bytearray(f), dtype=torch.uint8).to(DEV)
    heads, h_len, h_st = device.frame_heads([t], 64)
    s_st, _, _ = device.frame_decompressed_size([t])
    sound = B.assemble([B.good_blocks(4, 0)[0][1], B.good_blocks(4, 0)[0][2]], block_checksums=True)
    whole = cases.model(sound, b"", 64)[2]
    assert int(h_st[0]) == 0 and int(h_len[0]) == 64 and int(s_st[0]) == cases.BLOCK_CHECKSUM_FAIL
    got = bytes(heads[0].cpu().numpy())
    assert got == cases.model(f, b"", 64)[2] and got != whole and sum(a != b for a, b in zip(got, whole)) >= 1


def _many():
    """About 40 small frames without a dictionary and, for 6 000 jobs aliasing them, mixed targets with the model's expectations."""
    rows = cases.all_cases()
    pick, seen = [], set()
    for c, _ in rows:
        if c["dict"] or c["cls"] in ("contract", "cut", "header") or len(c["frame"]) > 20_000 or c["frame"] in seen or "past block_maxsize" in c["name"]:
            continue
        seen.add(c["frame"]); pick.append(c["frame"])
    pick = pick[::max(1, len(pick) // 40)][:40]
    memo = {}
    which, targets, exps = [], [], []
    for i in range(6000):
        k = i % len(pick)
        t = (0, 1, 64, 65, 200, 1000, 1500, 3000, 4096, cases.FAR)[(i // len(pick)) % 10]
        if (k, t) not in memo:
            memo[(k, t)] = cases.model(pick[k], b"", t)
        which.append(k); targets.append(t); exps.append(memo[(k, t)])
    return pick, which, targets, exps


def test_more_frames_than_one_residency():
    """6 000 frames aliasing about 40 small ones at mixed targets, every frame with an output of its own: the ticket goes past what
    the device holds at once.  On the current stream and on a stream of its own."""
    pick, which, targets, exps = _many()
    assert 30 <= len(pick) <= 40 and len({e[0] for e in exps}) >= 4
    run(pick, which, targets, exps, what="current stream")
    run(pick, which, targets, exps, poison=0x5A, stream=torch.cuda.Stream(), what="own stream")


def test_python_layer():
    """device.frame_heads / framed.frame_heads_device: frames that decode to more than, less than and exactly nbytes, and to
    nothing; with a dictionary; on a stream; an empty list."""
    blocks, data = B.good_blocks(4, 0)
    plain = b"".join(data)
    short = B.assemble(blocks[:1], data[0])
    frames = [B.assemble(blocks, plain), short, B.assemble([]), B.stop_frame("codec 3", 1, n=4)]
    nbytes = len(data[0])                                         # the second frame's length exactly
    ts = [torch.frombuffer(bytearray(f), dtype=torch.uint8).to(DEV) for f in frames]
    want = [(0, plain[:nbytes]), (0, data[0]), (0, b""), (0, data[0])]
    for stream in (None, torch.cuda.Stream()):
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        heads, lens, statuses = device.frame_heads(ts, nbytes, stream=stream)
        (stream or torch.cuda.current_stream()).synchronize()
        assert heads.shape == (4, nbytes) and statuses.cpu().tolist() == [0, 0, 0, 0] and lens.cpu().tolist() == [nbytes, nbytes, 0, nbytes]
        assert not bool(heads[2].any())
        got = framed.frame_heads_device(ts, nbytes, stream=stream)
        assert [(st, bytes(h.cpu().numpy())) for st, h in got] == want
    more = framed.frame_heads_device(ts, nbytes + 10)
    assert [(st, bytes(h.cpu().numpy())) for st, h in more] == [(0, plain[:nbytes + 10]), (0, data[0]), (0, b""), (3, data[0])]
    heads, lens, _ = device.frame_heads(ts[:2], nbytes + 10)
    assert lens.cpu().tolist() == [nbytes + 10, nbytes] and not bool(heads[1, nbytes:].any())
    dic = cases.dictionary_bytes()
    dblocks, ddata = B.good_blocks(4, 0, dic)
    fd = torch.frombuffer(bytearray(B.assemble(dblocks, b"".join(ddata), dictionary_id=7)), dtype=torch.uint8).to(DEV)
    (st, h), = framed.frame_heads_device([fd], 3000, dictionary=dic)
    assert st == 0 and bytes(h.cpu().numpy()) == b"".join(ddata)[:3000]
    (st, h), = framed.frame_heads_device([fd], 3000, dictionary=torch.frombuffer(bytearray(dic), dtype=torch.uint8).to(DEV))
    assert st == 0 and bytes(h.cpu().numpy()) == b"".join(ddata)[:3000]
    assert framed.frame_heads_device([], 64) == []
    heads, lens, statuses = device.frame_heads([], 64)
    assert heads.shape == (0, 64) and lens.numel() == 0 and statuses.numel() == 0
    heads, lens, statuses = device.frame_heads(ts, 0)
    torch.cuda.synchronize()
    assert heads.shape == (4, 0) and lens.cpu().tolist() == [0, 0, 0, 0] and statuses.cpu().tolist() == [0, 0, 0, 0]


def test_heads_of_the_frames_of_a_stream():
    """A stream of five frames, the fourth of which stops the stream: the heads of the four frames the index lists as reached, the
    stopping frame's status among them; the frame behind it is not read."""
    pieces = [B.good_frame(3, seed) for seed in (1, 2, 3)] + [B.stop_frame("codec 3", 0, n=4), B.good_frame(3, 4)]
    t = torch.frombuffer(bytearray(b"".join(pieces)), dtype=torch.uint8).to(DEV)
    index, = framed.stream_index_device([t])
    assert len(index.frames) == 5 and index.status == 3 and int(index.frames[4]["flags"]) & ffi.SFRAME_BEHIND_STOP
    got = framed.stream_frame_heads_device(t, index, 64)
    want = [(0, cases.model(f, b"", 64)[2]) for f in pieces[:3]] + [(3, b"")]
    assert [(st, bytes(h.cpu().numpy())) for st, h in got] == want
