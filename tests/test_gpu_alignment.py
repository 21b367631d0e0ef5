"""Buffer-alignment sweep (-m gpu): every decompress and compress kernel with its input, prefix and output at every address residue.

The decompress kernels flush their LDS ring to `out` as a byte-wise head, 16-byte vector stores and a byte-wise tail computed from
rb = out & 15 (four separately maintained copies: the pair kernel, the bitmap-fed kernel, the segmented pipeline's stager, staged16).
Host-buffer entry points stage every job at a 256-byte multiple and the seeded red-zone layout reaches rb in {0, 1, 2, 4, 8} only, so
the other residues never ran in most kernels.  Here the jobs of tests/alignment_cases.py (checked on the CPU by
tests/test_alignment_cases_cpu.py) go through tests/redzone.py with explicit placement — both input poisons, 4 KiB zones intact, bytes
and statuses equal to the oracle's — in batch sizes that make the product dispatch launch each kernel class; every test asserts the
launch string and recomputes from the device addresses really used that every required residue occurred.  The same jobs run under
the analysis library's forced kernels (tests/alignment_check.py), and lzf_copy_ranges, lzf_xxh32_batch and the device frame calls get
a residue sweep of their own."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import alignment_cases as ac
import alignment_check as chk
import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi, framed, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))

PAIRED48 = "lzf_decompress_paired_kernel<4096,48,640>"
PAIRED24 = "lzf_decompress_paired_kernel<4096,24,384>"
STAGED16 = "lzf_decompress_batched_kernel<4096,16,256,staged>"


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


_SHAPES = {}


def _shape(name):
    if name not in _SHAPES:
        _SHAPES[name] = {"TEH": lambda: ac.concat(ac.tiny(), ac.existing_prefix(), ac.handcrafted()),
                         "TH": lambda: ac.concat(ac.tiny(), ac.handcrafted()),
                         "S": ac.segmented, "C": ac.compress}[name]()
    return _SHAPES[name]


def _rb_of_every_kind(shape):
    """(from the shape's own low bits, which chk._check_pointers has held against the device addresses)"""
    kinds = {}
    for m, ol in zip(shape.meta, shape.out_low):
        kinds.setdefault(m["kind"], set()).add(ol & 15)
    return kinds


# --------------------------------------------------------------------------------------------------------------- the pair kernel, staged16
def test_pair_kernel_48_byte_form():
    """T + E + H, no more than eight blocks per CU in a call: lzf_decompress_paired_kernel<4096,48,640>."""
    s = _shape("TEH")
    hist = chk.sweep(s, "pair kernel, 48-byte form", 0, 8 * _cus(), lambda l: l == PAIRED48, max_input_len=chk.max_in(s))
    assert (hist > 0).all()                                              # all 256 (input & 15, out & 15) pairs
    assert all(v == set(range(16)) for v in _rb_of_every_kind(s).values())


def test_pair_kernel_24_byte_form():
    """The same jobs in calls of more than eight and at most twelve blocks per CU: lzf_decompress_paired_kernel<4096,24,384>."""
    s = _shape("TEH")
    hist = chk.sweep(s, "pair kernel, 24-byte form", 8 * _cus(), 12 * _cus(), lambda l: l == PAIRED24, max_input_len=chk.max_in(s))
    assert (hist > 0).all()


def test_staged16():
    """T + H in one call of more than 64 blocks per CU whose inputs are too small for the bitmap-fed path:
    lzf_decompress_batched_kernel<4096,16,256,staged>."""
    s = _shape("TH")
    assert chk.max_in(s) < 65536
    hist = chk.sweep(s, "staged16", 64 * _cus(), 1 << 20, lambda l: l == STAGED16, max_input_len=chk.max_in(s))
    assert (hist > 0).all()
    assert all(v == set(range(16)) for v in _rb_of_every_kind(s).values())


# --------------------------------------------------------------------------------------------------------------- the segmented pipeline
def _segmented(lo, hi, ring, label):
    s = _shape("S")
    rings = [r for r in (32768, 65536, 131072) if r >= ring]            # (a device with more LDS or CUs than the sizes assume picks a larger ring)
    want = [f"segmented: lzf_seg_resolve_pair_kernel<{r}> + {PAIRED48}" for r in rings]
    hist = chk.sweep(s, label, lo, hi, lambda l: l in want, max_input_len=chk.max_in(s))
    assert (hist > 0).all()
    text = [i for i, m in enumerate(s.meta) if m["kind"] == "text 1 MiB" and m["exact"]]
    assert {(s.in_low[i] & 15, s.out_low[i] & 15) for i in text} == {(a, b) for a in range(16) for b in range(16)}
    kinds = _rb_of_every_kind(s)
    assert all(kinds[k] == set(range(16)) for k in kinds if k not in ("damaged", "short")), kinds


def test_segmented_pipeline_128k_ring():
    _segmented(0, _cus(), 131072, "segmented, 128 KiB ring")


def test_segmented_pipeline_64k_ring():
    _segmented(_cus(), 2 * _cus(), 65536, "segmented, 64 KiB ring")


def test_segmented_pipeline_32k_ring_grouped():
    _segmented(2 * _cus(), 4 * _cus(), 32768, "segmented, 32 KiB ring, grouped")


# --------------------------------------------------------------------------------------------------------------- the bitmap-fed kernel
_RESIDENT = []


def _resident_workgroups():
    """How many workgroups of the fed kernel the device holds at once, as the library counted it: the F batch of 24 blocks per CU
    and more through the analysis library, nothing forced, LZF_FED_VERBOSE=1 (one run for both tests)."""
    if not _RESIDENT:
        from rust_lz_fear_amd import build
        env = dict(os.environ, LZF_LIB_PATH=build.build_analysis_library(), LZF_FED_VERBOSE="1")
        for k in ("LZF_DECOMPRESS_KERNEL", "LZF_FED_PIECES", "LZF_FED_SLOTS", "LZF_FED_MIN_IN", "LZF_SEG_FORCE"):
            env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.join(HERE, "alignment_check.py"), "pieces"], env=env, capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "alignment pieces ok" in r.stdout
        print(r.stdout)
        m = re.search(r"bitmap-fed kernel: (\d+) workgroups resident at once \((\d+) compute units\), XCD mask 0x([0-9a-f]+)", r.stderr)
        assert m, r.stderr[-2000:]
        assert int(m.group(2)) == _cus() and int(m.group(3), 16) != 0   # (no XCD mask: the library leaves every job whole)
        _RESIDENT.append(int(m.group(1)))
        print(f"[alignment] the fed kernel's resident workgroups, counted by the library: {_RESIDENT[0]}")
    return _RESIDENT[0]


def _fed(n, label):
    s = ac.fed(n)
    hist, launch = chk.run_decompress(s, label, max_input_len=chk.max_in(s), alias_inputs=True)
    assert launch == f"bitmap-fed: lzf_seg_parse_kernel + lzf_decompress_fed_kernel<4096,32,352> + {PAIRED24}", launch
    chk.report(label, hist, 1)
    assert (hist > 0).all()
    assert chk.max_in(s) > 262144


def test_bitmap_fed_whole_jobs():
    """More jobs than the 24-byte pair kernel holds (13 per CU), no more than the fed kernel's resident workgroups: jobs stay whole."""
    n = 14 * _cus()
    assert 13 * _cus() < n <= 20 * _cus()
    _fed(n, "bitmap-fed, whole jobs")
    assert n <= _resident_workgroups()


def test_bitmap_fed_16_pieces():
    """More jobs than resident workgroups (24 per CU is beyond what 160 KiB of LDS hold of a 6 912-byte footprint): every job in 16
    pieces — the hand-over of fs->o, the ring re-fill from `out` at an arbitrary o + rb, the flag protocol."""
    n = chk.pieces_jobs(_cus())
    assert n > 24 * _cus()
    _fed(n, "bitmap-fed, 16 pieces")
    assert n > _resident_workgroups()


# --------------------------------------------------------------------------------------------------------------- compress
def _compress(shape, label, lo, hi, expect_launch):
    hist = np.zeros((16, 16), dtype=np.int64)
    parts = ac.chunks(shape, lo, hi)
    for k, part in enumerate(parts):
        h, launch = chk.run_compress(part, f"{label}, call {k} of {len(parts)} ({len(part.items)} jobs)")
        assert expect_launch(launch, len(part.items)), (label, len(part.items), launch)
        hist += h
    chk.report(label, hist, len(parts))
    return hist


def _kind(shape, *kinds):
    return ac.take(shape, [i for i, m in enumerate(shape.meta) if m["kind"] in kinds])


def test_compress_team_kernel():
    s = _kind(_shape("C"), "u32")
    hist = _compress(s, "compress, team", 0, _cus(), lambda l, n: l.startswith("lzf_compress_team_kernel"))
    assert (hist > 0).all()


def test_compress_compact_kernel():
    s = _kind(_shape("C"), "u32", "cursor")
    hist = _compress(s, "compress, compact", _cus(), 1 << 20, lambda l, n: l.startswith("lzf_compress_compact_kernel"))
    assert (hist > 0).all()


def test_compress_general_kernel():
    """The U16 jobs (the general kernel alone) and the jobs with a cursor, the ones beyond their input's end among them (a call of
    their own: the team or the compact kernel in front of the general one, as the dispatch reports for that many jobs)."""
    s = _kind(_shape("C"), "u16")
    hist = _compress(s, "compress, general <U16>", 0, 1 << 20, lambda l, n: l == "lzf_compress_wave_kernel<U16>")
    assert (hist.sum(axis=0) > 0).all() and (hist.sum(axis=1) > 0).all()
    s = _kind(_shape("C"), "cursor")
    assert any(it["cursor"] > len(it["input"]) for it in s.items)
    hist = _compress(s, "compress, cursor > 0", 0, 1 << 20, lambda l, n: l == ("lzf_compress_team_kernel + lzf_compress_team_carry_kernel + lzf_compress_wave_kernel" if n <= _cus()
                                                                              else "lzf_compress_compact_kernel + lzf_compress_wave_kernel"))
    assert (hist.sum(axis=0) > 0).all() and (hist.sum(axis=1) > 0).all()


# --------------------------------------------------------------------------------------------------------------- the analysis library
def _child(mode, needle, **env):
    from rust_lz_fear_amd import build
    e = dict(os.environ, LZF_LIB_PATH=build.build_analysis_library(), **env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "alignment_check.py"), mode], env=e, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert needle in r.stdout
    print(r.stdout)


@pytest.mark.parametrize("variant", ["paired48", "paired24", "staged16", "seg", "fed", "fed3"])
def test_forced_kernel(variant):
    env = dict(LZF_DECOMPRESS_KERNEL=variant)
    if variant == "seg":
        env["LZF_SEG_MIN_IN"] = "0"
    if variant in ("fed", "fed3"):
        env = dict(LZF_DECOMPRESS_KERNEL="fed", LZF_FED_MIN_IN="1", **({"LZF_FED_PIECES": "3"} if variant == "fed3" else {}))
    _child("variant", "alignment variant ok", **env)


@pytest.mark.parametrize("force", ["noscratch", "stager", "resolver"])
def test_forced_fallbacks_of_the_segmented_pipeline(force):
    _child("force", "alignment force ok", LZF_SEG_FORCE=force)


# --------------------------------------------------------------------------------------------------------------- copies, checksums, frames
def _as_dev(a):
    return torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def test_copy_ranges_every_residue():
    """lzf_copy_ranges: 16 x 16 source / destination residues x the lengths around its 16-byte steps; nothing outside a range moves."""
    lens = [0, 1, 15, 16, 17, 31, 33, 255, 4097]
    slot = 8192
    jobs = [(n, sr, dr) for n in lens for sr in range(16) for dr in range(16)]
    rng = np.random.default_rng(16)
    h_src = rng.integers(0, 256, slot * (len(jobs) + 1) + 256, dtype=np.uint8)
    src = torch.empty(len(h_src) + 256, dtype=torch.uint8, device=DEV)
    dst = torch.full((len(h_src) + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    s0, d0 = (-src.data_ptr()) % 256, (-dst.data_ptr()) % 256            # 256-aligned bases inside the allocations
    src[s0:s0 + len(h_src)] = torch.from_numpy(h_src).to(DEV)
    so = [slot * (k + 1) + sr for k, (n, sr, dr) in enumerate(jobs)]
    do = [slot * (k + 1) + 256 * (k % 3) + dr for k, (n, sr, dr) in enumerate(jobs)]
    sp = [src.data_ptr() + s0 + x for x in so]
    dp = [dst.data_ptr() + d0 + x for x in do]
    assert (ac.residues(sp, dp) == len(lens)).all()
    device.copy_ranges(_as_dev(sp), _as_dev(dp), _as_dev([n for n, _, _ in jobs]), len(jobs), max(lens))
    torch.cuda.synchronize()
    exp = np.full(len(h_src), 0xA5, dtype=np.uint8)
    for (n, _, _), a, b in zip(jobs, so, do):
        exp[b:b + n] = h_src[a:a + n]
    got = dst.cpu().numpy()[d0:d0 + len(h_src)]
    bad = np.nonzero(got != exp)[0]
    assert not len(bad), f"first difference at destination offset {int(bad[0])}: range {int(bad[0]) // slot - 1} = {jobs[int(bad[0]) // slot - 1]}"


def test_xxh32_batch_every_residue():
    lens = [0, 1, 15, 16, 17, 31, 32, 33, 1000]
    jobs = [(n, r) for n in lens for r in range(16)]
    slot = 2048
    h = np.random.default_rng(32).integers(0, 256, slot * (len(jobs) + 1), dtype=np.uint8)
    d = torch.empty(len(h) + 256, dtype=torch.uint8, device=DEV)
    b0 = (-d.data_ptr()) % 256
    d[b0:b0 + len(h)] = torch.from_numpy(h).to(DEV)
    offs = [slot * k + r for k, (n, r) in enumerate(jobs)]
    ptrs = [d.data_ptr() + b0 + x for x in offs]
    assert {(p & 15, n) for p, (n, _) in zip(ptrs, jobs)} == {(r, n) for n in lens for r in range(16)}
    out = torch.zeros(len(jobs), dtype=torch.int32, device=DEV)
    device.xxh32_batch(_as_dev(ptrs), _as_dev([n for n, _ in jobs]), out, len(jobs))
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    for g, x, (n, r) in zip(got, offs, jobs):
        assert int(g) == o.xxh32(h[x:x + n].tobytes()), (n, r)


FRAME_SIZES = [0, 1, 17, 1000, 65535, 65536, 15, 16, 33, 65537, 100_001, 300_003, 700_000, 4097, 200_000, 131_072]


def _frame_datas():
    """Text, so that every frame of more than a few bytes holds compressed blocks; the sizes too small to compress sit where the
    residue maps below never pair two of them.  (The frame layer codes into slots of its own and moves bytes between them and the
    caller's buffers with lzf_copy_ranges, lzf_xxh32_batch reads the caller's buffers: those are what the caller's residues reach.)"""
    return [synth.gen_text_zipf(40 + i, max(n, 1)).tobytes()[:n] for i, n in enumerate(FRAME_SIZES)]


def _two_rounds(n, mul, add):
    """Low bits for 2 x 16 buffers: every residue twice, from buffers three places apart in the size list."""
    return [((k * mul + add + (3 if mul == 1 else 1) * (k // 16)) % 16) | ((k % 5) << 4) for k in range(n)]


def _arena(total, poison):
    t = torch.full((total + 256,), poison, dtype=torch.uint8, device=DEV)
    b0 = (-t.data_ptr()) % 256
    return t[b0:b0 + total]


def _place(sizes, low, zone=4096):
    offs, pos = [], 0
    for sz, lo in zip(sizes, low):
        pos = (pos + zone + 255) // 256 * 256 + lo
        offs.append(pos); pos += sz
    return offs, pos + zone


def test_device_frames_every_residue():
    """lzf_frame_compress_device_many and lzf_frame_decompress_device_many with one frame per input residue and per output residue
    (32 frames each: every residue of either side twice, in different pairs), held to the host frame calls; the bytes around every
    output stay poison."""
    from test_gpu_device_compress import bounds, device_struct, gsettings, host_many
    datas = _frame_datas() * 2
    n = len(datas)
    in_low = [v & 15 for v in _two_rounds(n, 1, 0)]
    out_low = _two_rounds(n, 5, 1)
    for low in (in_low, out_low):
        assert {v & 15 for v in low[:16]} == set(range(16)) == {v & 15 for v in low[16:]}
        assert all(max(len(datas[k]) for k in range(n) if low[k] & 15 == r) >= 1000 for r in range(16))      # a compressible input at every residue
    poison = 0xA5
    for g in (gsettings(block_size=64 << 10, block_checksums=True), gsettings(block_size=64 << 10, independent_blocks=False), gsettings(block_size=1 << 20)):
        # compress
        caps = bounds(g, [len(x) for x in datas])
        ioffs, itot = _place([len(x) for x in datas], in_low)
        ooffs, otot = _place(caps, out_low)
        ia, oa = _arena(itot, 0x5A), _arena(otot, poison)
        for a, x in zip(ioffs, datas):
            if x:
                ia[a:a + len(x)] = torch.frombuffer(bytearray(x), dtype=torch.uint8).to(DEV)
        ins = [ia[a:a + len(x)] for a, x in zip(ioffs, datas)]
        outs = [oa[a:a + c] for a, c in zip(ooffs, caps)]
        assert all(t.data_ptr() & 15 == lo for t, lo in zip(ins, in_low) if t.numel()) and [t.data_ptr() & 255 for t in outs] == out_low
        status, out_len = device.frame_compress_many(device_struct(g), ins, outs)
        torch.cuda.synchronize()
        host = host_many(g, datas, caps=caps)
        expect = np.full(otot, poison, dtype=np.uint8)
        for a, (hs, hb), s_, l_ in zip(ooffs, host, status.tolist(), out_len.tolist()):
            assert (s_, l_) == (hs, len(hb)) and hs == 0
            expect[a:a + len(hb)] = np.frombuffer(hb, dtype=np.uint8)
        assert np.array_equal(oa.cpu().numpy(), expect), "device frames differ from the host call's, or bytes outside them were written"
        # decompress what the host call made: the frames where the compress half wrote them, the outputs on another residue map
        frames = [hb for _, hb in host]
        fl = [v & 15 for v in out_low]
        dl = _two_rounds(n, 11, 1)
        assert {v & 15 for v in dl[:16]} == set(range(16)) == {v & 15 for v in dl[16:]}
        assert all(max(len(datas[k]) for k in range(n) if dl[k] & 15 == r) >= 1000 for r in range(16))
        assert len({(a, b & 15) for a, b in zip(fl, dl)}) >= 24                                                  # (not the same residue on both sides)
        assert all(len(f) < len(x) for f, x in zip(frames, datas) if len(x) >= 1000)                             # (compressed blocks, not stored ones)
        caps = [max(len(x), 1) if k % 4 else len(x) + 100 for k, x in enumerate(datas)]
        foffs, ftot = _place([len(f) for f in frames], fl)
        doffs, dtot = _place(caps, dl)
        fa, da = _arena(ftot, 0x5A), _arena(dtot, poison)
        for a, f in zip(foffs, frames):
            fa[a:a + len(f)] = torch.frombuffer(bytearray(f), dtype=torch.uint8).to(DEV)
        fin = [fa[a:a + len(f)] for a, f in zip(foffs, frames)]
        dout = [da[a:a + c] for a, c in zip(doffs, caps)]
        assert [t.data_ptr() & 15 for t in fin] == fl and [t.data_ptr() & 255 for t in dout] == dl
        status, out_len, used = device.frame_decompress_many(fin, dout)
        torch.cuda.synchronize()
        hostd = framed.decompress_frames(frames, caps=caps, with_consumed=True)
        expect = np.full(dtot, poison, dtype=np.uint8)
        for a, x, (st, out, u), s_, l_, c_ in zip(doffs, datas, hostd, status.tolist(), out_len.tolist(), used.tolist()):
            assert (s_, l_, c_) == (st, len(out), u) and st == 0 and out == x
            expect[a:a + len(out)] = np.frombuffer(out, dtype=np.uint8)
        assert np.array_equal(da.cpu().numpy(), expect), "decoded frames differ from the host call's, or bytes outside them were written"
