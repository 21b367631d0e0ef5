"""GPU tests (-m gpu) of the block index of frames in device memory and of the decode of runs of their blocks
(include/lzfear_frame.h: lzf_frame_block_count_device / lzf_frame_block_index_device / lzf_block_index_locate /
lzf_frame_decompress_blocks_device) and of what Python builds on them (framed.block_index_device, locate_blocks,
read_frame_range_device).

Expected entries, sizes and bytes are tests/block_index_cases.py's: the oracle decoding every block behind a host walk.  The
frames are put together from small blocks under a block_maxsize of 64 KiB — the rules depend on the number of blocks — except
in the test of the decoder classes, whose frames the device compresses and whose bytes are the whole-frame decode's."""
import ctypes as C

import numpy as np
import pytest
import torch

import block_index_cases as bc
import redzone
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi, framed

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
STORED, HAS_SUM, LINKED, DELIVERED, BEHIND = bc.STORED, bc.HAS_SUM, bc.LINKED, bc.DELIVERED, bc.BEHIND_STOP


def dev(b):
    b = bytes(b)
    if not b:
        return torch.empty(0, dtype=torch.uint8, device=DEV)
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(DEV)


def dev_poisoned(frames, poison):
    """Every frame in one input arena, 4 KiB of `poison` in front of it and behind it (tests/redzone.py's input arena: the bytes
    behind in_len are 0x00 in one run and 0xFF in another, and nothing may depend on them)."""
    offs, total = redzone._layout([len(f) for f in frames], redzone.ZONE, np.random.default_rng(17))
    h = np.full(total, poison, dtype=np.uint8)
    for at, f in zip(offs, frames):
        h[at:at + len(f)] = np.frombuffer(bytes(f), dtype=np.uint8)
    arena = torch.from_numpy(h).to(DEV)
    return [arena[at:at + len(f)] for at, f in zip(offs, frames)]


def check_index(frames, dictionary=b"", names=None, poison=None):
    """The index call over byte strings against the expected index and against the size query; returns ([FrameBlockIndex],
    [expected entries], tensors).  `poison`: the frames lie in an input arena with that byte behind each of them."""
    tens = [dev(f) for f in frames] if poison is None else dev_poisoned(frames, poison)
    got = framed.block_index_device(tens, dictionary_len=len(dictionary))
    sizes = framed.decompressed_sizes_device(tens, dictionary_len=len(dictionary))
    assert device.frame_block_count(tens) == [len(g.blocks) for g in got]
    wants = []
    for k, (f, g) in enumerate(zip(frames, got)):
        name = names[k] if names else k
        want, res = bc.ref_index(f, dictionary)
        assert (g.status, g.out_len, g.consumed) == res == sizes[k], name
        assert len(g.blocks) == len(want), name
        for i, e in enumerate(want):
            for fld in bc.comparable(e):
                assert int(g.blocks[fld][i]) == e[fld], (name, i, fld)
        wants.append(want)
    return got, wants, tens


def guarded_outs(sizes, lows, seed=0):
    """Output tensors of `sizes` bytes at the low address bits `lows`, carved out of one poisoned arena."""
    offs, _, arena = redzone._place(list(sizes), list(lows), np.random.default_rng(seed), DEV, True)
    arena.fill_(redzone.OUT_POISON)
    return [arena[at:at + n] for at, n in zip(offs, sizes)], offs, arena


def assert_only(arena, offs, written, name=""):
    """Every byte of the arena is poison but `written[k]` at offs[k]."""
    h = arena.cpu().numpy()
    expect = np.full_like(h, redzone.OUT_POISON)
    for at, b in zip(offs, written):
        expect[at:at + len(b)] = np.frombuffer(b, dtype=np.uint8)
    bad = np.nonzero(h != expect)[0]
    assert len(bad) == 0, (name, int(bad[0]), len(bad))


def plain_of(want, a, b):
    return b"".join(e["plain"] for e in want[a:b])


@pytest.fixture(scope="module")
def frame130():
    """One frame of 130 blocks with block checksums, indexed: (bytes, tensor, FrameBlockIndex, expected entries, plain bytes)."""
    f = bc.good_frame(130, block_checksums=True)
    (g,), (want,), (t,) = check_index([f])
    return f, t, g, want, plain_of(want, 0, 130)


# ---- 1. entries and sizes --------------------------------------------------------------------------------------------------

def test_entries_and_sizes_of_frames_of_0_to_130_blocks():
    frames = [bc.good_frame(n, block_checksums=sums, content_checksum=bool(n % 3)) for n in bc.COUNTS for sums in (False, True)]
    got, wants, _ = check_index(frames)
    assert [len(g.blocks) for g in got] == [n for n in bc.COUNTS for _ in (0, 1)]
    for g, want in zip(got, wants):
        assert all(e["flags"] & DELIVERED for e in want) and g.status == 0
        if len(want):
            assert any(e["flags"] & STORED for e in want)               # every frame has a stored block
            assert g.out_len == int(g.blocks["out_off"][-1] + g.blocks["out_len"][-1])
    dct = bc.dictionary_bytes()
    frames = [bc.good_frame(n, seed=1, dictionary=dct, block_checksums=True) for n in (1, 2, 65)]
    got, wants, _ = check_index(frames, dictionary=dct)
    assert [len(g.blocks) for g in got] == [1, 2, 65]
    assert framed.block_index_device([]) == [] and device.frame_block_count([]) == []
    # a header that fails lists nothing
    (g,), _, _ = check_index([b"\x00" * 11])
    assert (g.status, len(g.blocks)) == (17, 0)


# ---- 2. every kind of stop, on both sides of a round -----------------------------------------------------------------------

def test_stop_kinds_at_block_0_63_64_and_last():
    names = [(kind, at) for kind in bc.STOP_KINDS for at in bc.STOP_PLACES]
    frames = [bc.stop_frame(kind, at) for kind, at in names]
    # both input poisons: where the input is cut inside a block an over-read of the walk would show in what is listed
    other, _, _ = check_index(frames, names=names, poison=0x00)
    got, wants, _ = check_index(frames, names=names, poison=0xFF)
    for g, h in zip(got, other):
        assert (g.status, g.out_len, g.consumed) == (h.status, h.out_len, h.consumed) and g.blocks.tobytes() == h.blocks.tobytes()
    kinds = set()
    for (kind, at), g, want in zip(names, got, wants):
        if kind == "truncated":
            assert len(g.blocks) == at and g.status == 16 and (g.blocks["flags"] & DELIVERED != 0).all(), (kind, at)
            continue
        assert len(g.blocks) == 130
        assert (g.blocks["flags"] & DELIVERED != 0).tolist() == [k < at for k in range(130)], (kind, at)
        assert (g.blocks["flags"] & BEHIND != 0).tolist() == [k > at for k in range(130)], (kind, at)
        assert (g.blocks["out_off"][at:] == g.out_len).all() and int(g.blocks["status"][at]) == g.status, (kind, at)
        kinds.add(g.status)
    assert kinds == {19, 1, 2, 3, 4, 22, 0}


# ---- 3. a linked-block frame -----------------------------------------------------------------------------------------------

def test_a_linked_frame_is_indexed_and_its_runs_are_refused():
    dct = bc.dictionary_bytes()
    frames = [bc.linked_frame(), bc.linked_frame(150_000, block_checksums=True)]
    got, wants, tens = check_index(frames)
    (gd,), _, _ = check_index([bc.linked_frame(150_000, dictionary=dct)], dictionary=dct)
    for g in got + [gd]:
        assert len(g.blocks) >= 3 and (g.blocks["flags"] & LINKED != 0).all() and (g.blocks["flags"] & DELIVERED != 0).all()
        assert g.out_len == int(g.blocks["out_len"].sum()) and (g.blocks["out_len"][:-1] == bc.BMAX).all()
    out = torch.empty(got[0].out_len, dtype=torch.uint8, device=DEV)
    for run in (got[0].blocks, got[0].blocks[1:2]):
        with pytest.raises(ffi.LzfError) as e:
            device.frame_decompress_blocks([tens[0]], [run], [out])
        assert e.value.code == ffi.E_INVALID
    with pytest.raises(ffi.LzfError):
        framed.read_frame_range_device(tens[0], got[0], 10, 20)


# ---- 4. index capacity -----------------------------------------------------------------------------------------------------

def test_index_capacity_under_red_zones(frame130):
    """The entry rooms in an arena of OUT_POISON; the frames — a whole one and one cut inside block 64 — in an input arena with
    0x00 behind them in one run and 0xFF in the other: the same entries, results and counts under both."""
    f, _, full, _, _ = frame130
    cut = bc.stop_frame("truncated", 64)
    (cut_full,), _, _ = check_index([cut])
    seen = []
    for poison in (0x00, 0xFF):
        for frame, whole in ((f, full), (cut, cut_full)):
            (t,) = dev_poisoned([frame], poison)
            found = len(whole.blocks)
            assert found == (130 if frame is f else 64)
            caps = [0, 1, found - 1, found, found + 5]
            rng = np.random.default_rng(3)
            lows = [16 * int(rng.integers(0, 16)) + r for r in (0, 8, 8, 0, 8)]
            rooms, offs, arena = guarded_outs([48 * c for c in caps], lows, seed=3)
            status, out_len, consumed, n_listed = device.frame_block_index_raw([t] * 5, index=rooms)
            plain = device.frame_block_index_raw([t] * 5)                # d_index / index_cap both NULL: sizes only
            torch.cuda.synchronize()
            assert n_listed.tolist() == [found] * 5 == plain[3].tolist() and device.frame_block_count([t]) == [found]
            for x, y in zip((status, out_len, consumed), plain):
                assert x.tolist() == y.tolist() == [x.tolist()[0]] * 5
            assert (status[0].item(), out_len[0].item(), consumed[0].item()) == (whole.status, whole.out_len, whole.consumed)
            assert_only(arena, offs, [whole.blocks[:min(c, found)].tobytes() for c in caps])      # exactly min(cap, found) entries, nothing else
            seen.append((status.tolist(), out_len.tolist(), consumed.tolist(), n_listed.tolist(), arena.cpu().numpy().tobytes()))
    assert seen[0] == seen[2] and seen[1] == seen[3]                     # nothing depends on the bytes behind in_len


# ---- 5. runs ---------------------------------------------------------------------------------------------------------------

def test_runs_decode_to_the_slice_of_the_oracles_output(frame130):
    f, t, g, want, plain = frame130
    stored = next(k for k in range(8, 130) if want[k]["flags"] & STORED)
    runs = [(0, 1), (41, 42), (stored, stored + 1), (stored - 2, stored + 3), (30, 100), (63, 65), (0, 130), (129, 130), (64, 129)]
    plain_frame = bc.good_frame(130)                                     # and the same blocks without checksums
    (g2,), (want2,), (t2,) = check_index([plain_frame])
    for tensor, index, exp, label in ((t, g, want, "checksums"), (t2, g2, want2, "plain")):
        sizes = [int(index.blocks["out_len"][a:b].sum()) for a, b in runs]
        outs, offs, arena = guarded_outs(sizes, [16 * (3 * k % 16) + r for k, r in enumerate((0, 1, 7, 8, 15, 3, 4, 9, 2))], seed=5)
        status, out_len = device.frame_decompress_blocks([tensor] * len(runs), [index.blocks[a:b] for a, b in runs], outs)
        torch.cuda.synchronize()
        assert status.tolist() == [0] * len(runs) and out_len.tolist() == sizes, label
        assert_only(arena, offs, [plain_of(exp, a, b) for a, b in runs], label)
        for (a, b), n in zip(runs, sizes):
            lo = exp[a]["out_off"]
            assert plain_of(exp, a, b) == plain[lo:lo + n]
    # behind a dictionary
    dct = bc.dictionary_bytes()
    fd = bc.good_frame(65, seed=1, dictionary=dct, block_checksums=True)
    (gd,), (wd,), (td,) = check_index([fd], dictionary=dct)
    outs, offs, arena = guarded_outs([gd.out_len, int(gd.blocks["out_len"][3:9].sum())], [5, 130], seed=6)
    status, out_len = device.frame_decompress_blocks([td, td], [gd.blocks, gd.blocks[3:9]], outs, dictionary=dev(dct))
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0]
    assert_only(arena, offs, [plain_of(wd, 0, 65), plain_of(wd, 3, 9)], "dictionary")


# ---- 6. many runs ----------------------------------------------------------------------------------------------------------

def test_130_runs_aliasing_one_frame_some_empty_one_short_of_capacity(frame130):
    f, t, g, want, plain = frame130
    runs, sizes, caps = [], [], []
    for r in range(130):
        a, b = (r, r) if r % 9 == 4 else (r, min(130, r + 1 + r % 3 + (66 if r == 20 else 0)))
        runs.append((a, b))
        sizes.append(int(g.blocks["out_len"][a:b].sum()))
        caps.append(sizes[-1] - 1 if r == 50 else sizes[-1] + (3 if r % 5 == 0 else 0))
    assert sizes[50] > 0 and runs[20][1] - runs[20][0] > 64
    outs, offs, arena = guarded_outs(caps, [(37 * r) % 256 for r in range(130)], seed=7)
    status, out_len = device.frame_decompress_blocks([t] * 130, [g.blocks[a:b] for a, b in runs], outs)
    torch.cuda.synchronize()
    assert status.tolist() == [ffi.OUT_CAPACITY if r == 50 else 0 for r in range(130)]
    assert out_len.tolist() == [0 if r == 50 else n for r, n in enumerate(sizes)]
    assert_only(arena, offs, [b"" if r == 50 else plain_of(want, a, b) for r, (a, b) in enumerate(runs)])     # a short run: no writes
    # an empty call, and a call of empty runs alone
    assert device.frame_decompress_blocks([], [], [])[0].numel() == 0
    status, out_len = device.frame_decompress_blocks([t, t], [g.blocks[:0], g.blocks[5:5]], [outs[0], outs[1]])
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0] and out_len.tolist() == [0, 0]


# ---- 7. only the run's blocks are read -------------------------------------------------------------------------------------

def test_damage_outside_the_run_goes_unnoticed(frame130):
    f, _, g, want, plain = frame130
    t = dev(f)
    for k in (10, 99):                                                   # in front of the run and behind it
        t[int(g.blocks["in_off"][k]) + 5] ^= 0x21
    a, b = 40, 80
    total = int(g.blocks["out_len"][a:b].sum())
    outs, offs, arena = guarded_outs([total], [9], seed=8)
    status, out_len = device.frame_decompress_blocks([t], [g.blocks[a:b]], outs)
    torch.cuda.synchronize()
    assert (status.item(), out_len.item()) == (0, total)
    assert_only(arena, offs, [plain_of(want, a, b)])
    (st, out, used), = framed.decompress_frames_device([t])
    assert st == 19 and out.numel() == want[10]["out_off"]               # the whole-frame decode stops at block 10


# ---- 8. a stale index ------------------------------------------------------------------------------------------------------

def test_a_block_damaged_after_indexing_fails_its_run_where_it_is(frame130):
    f, _, g, want, plain = frame130
    a, b, k = 20, 100, 92                                                # the damaged block is in the run's second round of 64
    assert not want[k]["flags"] & STORED
    total = int(g.blocks["out_len"][a:b].sum())
    front = int(g.blocks["out_off"][k] - g.blocks["out_off"][a])
    t = dev(f)
    t[int(g.blocks["in_off"][k]) + 3] ^= 0x04
    outs, offs, arena = guarded_outs([total], [3], seed=9)
    status, out_len = device.frame_decompress_blocks([t], [g.blocks[a:b]], outs)
    torch.cuda.synchronize()
    assert (status.item(), out_len.item()) == (19, front)
    h = arena.cpu().numpy()
    assert h[offs[0]:offs[0] + front].tobytes() == plain_of(want, a, k)
    keep = np.ones(len(h), dtype=bool); keep[offs[0]:offs[0] + total] = False
    assert (h[keep] == redzone.OUT_POISON).all()                         # nothing beyond the run's total
    # a damaged checksum word alone: the word is read from the input, not from the entry
    t = dev(f)
    t[int(g.blocks["in_off"][k] + g.blocks["in_len"][k]) + 1] ^= 0x80
    status, out_len = device.frame_decompress_blocks([t], [g.blocks[a:b]], [torch.empty(total, dtype=torch.uint8, device=DEV)])
    assert (status.item(), out_len.item()) == (19, front)
    # without checksums: a codec status, or LZF_CONTRACT where the block decodes to another length
    import oracle_ffi as o
    pf = bc.good_frame(130)
    (g2,), (w2,), _ = check_index([pf])
    off, ln, n = int(g2.blocks["in_off"][k]), int(g2.blocks["in_len"][k]), int(g2.blocks["out_len"][k])
    seen = set()
    for want_ok in (False, True):                                        # a damage the decoder refuses, and one it decodes to another length
        for pos, x in ((p, x) for p in range(0, min(ln, 40)) for x in (0x0F, 0xF0, 0x01, 0x10, 0x55)):
            bad = bytearray(pf[off:off + ln]); bad[pos] ^= x
            rc, out = o.decompress_raw(bytes(bad), limit=bc.BMAX)
            if (rc == 0 and len(out) != n) if want_ok else rc in (1, 2, 3, 4):
                break
        else:
            continue
        t = dev(pf)
        t[off + pos] ^= x
        outs, offs, arena = guarded_outs([total], [11], seed=10)
        status, out_len = device.frame_decompress_blocks([t], [g2.blocks[a:b]], outs)
        torch.cuda.synchronize()
        print("stale block:", "another length" if want_ok else "refused", "oracle", rc, len(out), "indexed", n, "run status", status.item())
        assert status.item() in (1, 2, 3, 4, ffi.CONTRACT) and out_len.item() == front
        seen.add(want_ok)
        h = arena.cpu().numpy()
        assert h[offs[0]:offs[0] + front].tobytes() == plain_of(w2, a, k)
        keep = np.ones(len(h), dtype=bool); keep[offs[0]:offs[0] + total] = False
        assert (h[keep] == redzone.OUT_POISON).all()
    assert seen, "no damage found that changes the block's result"


# ---- 9. exact capacity in every decoder class ------------------------------------------------------------------------------

def poor_block(n, seed):
    """n poorly compressible bytes: random, with 64 zeros every 4 KiB (compressed, but barely)."""
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    x = torch.randint(0, 256, (n,), dtype=torch.uint8, device=DEV, generator=g)
    x.view(-1, 4096)[:, :64] = 0
    return x


def device_frame(data, block_size):
    s = ffi.Settings()
    ffi.lib().lzf_settings_default(C.byref(s))
    s.block_size, s.content_checksum = block_size, 0
    out = torch.empty(ffi.lib().lzf_frame_compress_bound(C.byref(s), data.numel()), dtype=torch.uint8, device=DEV)
    status, out_len = device.frame_compress_many(s, [data], [out])
    torch.cuda.synchronize()
    assert status.item() == 0
    return out[:out_len.item()]


CLASSES = {
    # blocks of 4 MiB that compress to 64 KiB and more, up to four per compute unit: the segmented pipeline
    "segmented": (4 << 20, 8, "segmented"),
    # 256 KiB blocks, more than four per compute unit: beyond the pipeline the call goes to the pair kernel
    # (the bitmap-fed path wants inputs above 256 KiB and more blocks than the pair kernel holds at once, lzf_dispatch.h)
    "pair": (256 << 10, 1100, "lzf_decompress_paired_kernel"),
    # blocks of 1 MiB, more than twelve per compute unit, inputs above 256 KiB: the bitmap-fed path (3 GiB of payload: the
    # smallest call the path takes; the payload, the frame, the guarded output and the whole-frame decode's output are held one
    # after the other where they can be, and the test ran in under a second on an MI355X)
    "fed": (1 << 20, 3100, "bitmap-fed"),
}


@pytest.mark.parametrize("name", list(CLASSES))
def test_a_whole_frame_run_at_exact_capacity_in_every_decoder_class(name):
    block_size, n_blocks, launch = CLASSES[name]
    if name == "segmented":
        from rust_lz_fear_amd import synth
        base = torch.from_numpy(synth.silesia_mix(0, block_size).copy()).to(DEV)
    else:
        base = torch.cat([poor_block(block_size, s) for s in range(4)])
    data = base.repeat((n_blocks * block_size + base.numel() - 1) // base.numel())[:n_blocks * block_size - 1000]     # (the last block is short)
    del base
    frame = device_frame(data, block_size)
    frame = frame.clone()                                                # (the bound-sized buffer it was a view of goes)
    (g,) = framed.block_index_device([frame])
    assert g.status == 0 and g.out_len == data.numel() and len(g.blocks) == n_blocks
    assert (g.blocks["flags"] == DELIVERED).all(), "every block is compressed and delivered"
    assert int(g.blocks["in_len"].min()) >= 64 << 10 or name == "pair"
    outs, offs, arena = guarded_outs([g.out_len], [7], seed=11)
    status, out_len = device.frame_decompress_blocks([frame], [g.blocks], outs)
    got_launch = ffi.lib().lzf_last_decompress_launch().decode()
    torch.cuda.synchronize()
    print(name, n_blocks, "blocks:", got_launch)
    assert (status.item(), out_len.item()) == (0, g.out_len)
    assert got_launch.startswith(launch) and (name != "pair" or "fed" not in got_launch), got_launch
    lo, hi = offs[0], offs[0] + g.out_len
    assert (arena[:lo] == redzone.OUT_POISON).all() and (arena[hi:] == redzone.OUT_POISON).all()
    assert torch.equal(outs[0], data)
    del data
    (st, whole, used), = framed.decompress_frames_device([frame], caps=[g.out_len])
    assert st == 0 and used == frame.numel()
    assert torch.equal(outs[0], whole)


# ---- 10. Python ------------------------------------------------------------------------------------------------------------

def test_read_frame_range_device(frame130, monkeypatch):
    f, t, g, want, plain = frame130
    off = g.blocks["out_off"].tolist() + [g.out_len]
    stored = next(k for k in range(8, 130) if want[k]["flags"] & STORED)
    seen = []
    real = device.frame_decompress_blocks
    monkeypatch.setattr(device, "frame_decompress_blocks", lambda fr, runs, *a, **kw: (seen.append([len(r) for r in runs]), real(fr, runs, *a, **kw))[1])
    ranges = [(off[5] + 3, off[5] + 9), (off[5] + 3, off[6] + 1), (off[stored] - 1, off[stored + 1] + 1), (off[stored], off[stored + 1]), (7, 7), (9, 3),
              (off[100], 1 << 62), (g.out_len - 1, g.out_len), (g.out_len, g.out_len + 5), (0, g.out_len), (off[63] - 1, off[64] + 1), (off[64], off[64] + 1)]
    for a, b in ranges:
        seen.clear()
        got = framed.read_frame_range_device(t, g, a, b)
        assert got.cpu().numpy().tobytes() == (plain[a:b] if a < b else b""), (a, b)
        hit = [k for k in range(130) if off[k] < min(b, g.out_len) and off[k + 1] > a]
        assert seen == ([[len(hit)]] if hit and a < b else []), (a, b)
        assert framed.locate_blocks(g, a, b) == ((hit[0], len(hit)) if hit and a < b else (0, 0))
    # behind a stop only the delivered blocks are there to read
    sf = bc.stop_frame("codec 3", 64)
    (gs,), (ws,), (ts,) = check_index([sf])
    assert framed.read_frame_range_device(ts, gs, 0, 1 << 40).cpu().numpy().tobytes() == plain_of(ws, 0, 64)
    # a block damaged since the index was taken
    bad = dev(f)
    bad[int(g.blocks["in_off"][70]) + 2] ^= 1
    assert framed.read_frame_range_device(bad, g, 0, off[70]).numel() == off[70]
    with pytest.raises(framed.FrameError) as e:
        framed.read_frame_range_device(bad, g, off[70] + 1, off[70] + 2)
    assert e.value.code == 19
