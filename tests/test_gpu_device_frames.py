"""GPU tests (-m gpu) of the frame layer for frames in device memory (include/lzfear_frame.h, "frames in device memory":
lzf_frame_decompress_bound_device / lzf_frame_decompress_device_many): per frame the status, bytes and `consumed` of the
oracle's decompress_frame and of the host driver lzf_frame_decompress_many, with frames and outputs in HBM."""
import json
import os

import numpy as np
import pytest
import torch

import oracle_ffi as o
import vectors
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi, framed, synth
from test_oracle import fuzz_corpus

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = torch.device("cuda", 0)


def dev(b):
    b = bytes(b)
    if not b:
        return torch.empty(0, dtype=torch.uint8, device=DEV)
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(DEV)


def run(frames, dictionary=b"", caps=None):
    """[(status, bytes, consumed)] of lzf_frame_decompress_device_many over byte strings."""
    d = dev(dictionary) if dictionary else None
    res = framed.decompress_frames_device([dev(f) for f in frames], dictionary=d, caps=caps)
    return [(st, bytes(t.cpu().numpy().tobytes()), used) for st, t, used in res]


def mutate(rng, frame):
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
            dict(block_size=64 << 10, content_size=True), dict(block_size=4 << 20)]


def test_every_flavour_matches_oracle_and_host_path():
    rng = np.random.default_rng(77)
    frames = []
    for kw in FLAVOURS:
        kw = dict(kw)
        cs = kw.pop("content_size", False)
        for d in _inputs():
            frames.append(o.frame_compress(d, o.make_settings(content_size=len(d) if cs else None, **kw))[1])
    dct = synth.gen_text_zipf(3, 70000).tobytes()
    dframes = [o.frame_compress(d, o.make_settings(block_size=64 << 10, dictionary=dct, dictionary_id=9, **extra))[1]
               for d in _inputs()[:3] for extra in (dict(), dict(independent_blocks=False))]
    damaged = [mutate(rng, f) for f in frames for _ in range(3)]
    allf = frames + damaged + [frames[0] + b"trailing bytes"]
    bounds = device.frame_decompress_bound([dev(f) for f in allf])
    caps = [max(int(b), 1) for b in bounds]
    got = run(allf, caps=caps)
    host = framed.decompress_frames(allf, caps=caps, with_consumed=True)
    kinds = set()
    for f, g, h in zip(allf, got, host):
        assert g == o.frame_decompress(f)
        assert g == h
        kinds.add(g[0])
    assert len(kinds) >= 6, kinds
    dgot = run(dframes, dictionary=dct)
    for f, g in zip(dframes, dgot):
        assert g == o.frame_decompress(f, dictionary=dct) and g[0] == 0


def test_decode_corpus_one_call():
    J = json.load(open(os.path.join(GOLD, "corpus_frames.json")))["per_file"]
    files = fuzz_corpus("decode")
    got = run([d for _, d in files])
    for (name, data), g in zip(files, got):
        erc, eout, eused = o.frame_decompress(data)
        assert o.STATUS_NAMES[g[0]] == J[name], name
        assert g == (erc, eout, eused), name


def test_header_truncations():
    data = synth.silesia_mix(0, 200_000).tobytes()
    f = o.frame_compress(data, o.make_settings(block_size=64 << 10, content_size=len(data), dictionary=b"abcdefgh", dictionary_id=12345))[1]
    hdr = 4 + 2 + 8 + 4 + 1
    prefixes = [f[:k] for k in range(hdr + 9)]
    got = run(prefixes, dictionary=b"abcdefgh", caps=[1 << 20] * len(prefixes))
    for p, (st, out, used) in zip(prefixes, got):
        erc, eout, eused = o.frame_decompress(p, dictionary=b"abcdefgh")
        assert (st, used) == (erc, eused), len(p)
        assert out == eout


def test_capacity_edges():
    data = synth.silesia_mix(3 << 20, (3 << 20) + 5 * 65536 + 999).tobytes()
    frames = [o.frame_compress(data, o.make_settings(block_size=64 << 10, **kw))[1] for kw in (dict(), dict(independent_blocks=False, block_checksums=True))]
    for f in frames:
        caps = sorted({max(0, k * 65536 + e) for k in range(0, 7) for e in (-1, 0, 1)})
        got = run([f] * len(caps), caps=caps)
        host = framed.decompress_frames([f] * len(caps), caps=caps, with_consumed=True)
        assert got == host
        assert any(g[0] == ffi.OUT_CAPACITY for g in got)
        (b,) = device.frame_decompress_bound([dev(f)])
        assert run([f], caps=[b]) == [o.frame_decompress(f)]


def test_frames_of_65_blocks_cross_the_delivery_round():
    """65 blocks of 64 KiB per frame, independent and linked, block checksums on: the delivery kernel takes 64 blocks per round,
    so block 64 goes behind the first round's total (the carry of the wave scan).  Whole frames; the last block's checksum
    damaged, which stops the frame in the second round with the first round's 64 blocks delivered; and capacities that end
    inside block 63, between the rounds, and inside block 64."""
    data = synth.silesia_mix(9 << 20, (9 << 20) + 65 * 65536).tobytes()
    frames = [o.frame_compress(data, o.make_settings(block_size=64 << 10, block_checksums=True, independent_blocks=ib))[1] for ib in (True, False)]
    damaged = []
    for f in frames:
        b = bytearray(f); b[-9] ^= 1                      # (... block 64 | its checksum | EndMark | content checksum)
        damaged.append(bytes(b))
    got = run(frames + damaged)
    for f, g in zip(frames + damaged, got):
        assert g == o.frame_decompress(f)
    assert [g[:2] for g in got[:2]] == [(0, data)] * 2
    assert [(g[0], len(g[1])) for g in got[2:]] == [(19, 64 * 65536)] * 2
    caps = [64 * 65536 - 1, 64 * 65536, 64 * 65536 + 1, 65 * 65536 - 1, 65 * 65536]
    for f in frames:
        capped = run([f] * len(caps), caps=caps)
        assert capped == framed.decompress_frames([f] * len(caps), caps=caps, with_consumed=True)
        assert [g[0] for g in capped] == [ffi.OUT_CAPACITY] * 4 + [0]
        assert [len(g[1]) for g in capped] == [63 * 65536, 64 * 65536, 64 * 65536, 64 * 65536, 65 * 65536]


@pytest.mark.parametrize("poison", [0xA5, 0x5A])
def test_red_zones(poison):
    rng = np.random.default_rng(poison)
    base = [o.frame_compress(d, o.make_settings(block_size=64 << 10, **kw))[1] for d in _inputs()
            for kw in (dict(), dict(independent_blocks=False))]
    frames = base + [mutate(rng, f) for f in base]
    bounds = device.frame_decompress_bound([dev(f) for f in frames])
    caps = [int(b) if i % 3 else max(int(b) // 2, 1) for i, b in enumerate(bounds)]          # every third one short
    zone = 4096
    offs, pos = [], 0
    for c in caps:
        pos += zone + int(rng.integers(0, 64))
        offs.append(pos)
        pos += c
    arena = torch.full((pos + zone,), poison, dtype=torch.uint8, device=DEV)
    outs = [arena[o_:o_ + c] for o_, c in zip(offs, caps)]
    ins = [dev(f) for f in frames]
    status, out_len, used = device.frame_decompress_many(ins, outs)
    torch.cuda.synchronize()
    host = framed.decompress_frames(frames, caps=caps, with_consumed=True)
    h = arena.cpu().numpy()
    expect = np.full_like(h, poison)
    for o_, (st, out, u), s_, l_, c_ in zip(offs, host, status.tolist(), out_len.tolist(), used.tolist()):
        assert (s_, l_, c_) == (st, len(out), u)
        expect[o_:o_ + len(out)] = np.frombuffer(out, dtype=np.uint8)
    assert np.array_equal(h, expect)


def test_checksum_failures():
    data = synth.silesia_mix(7 << 20, (7 << 20) + 700_000).tobytes()
    f = o.frame_compress(data, o.make_settings(block_size=64 << 10, block_checksums=True))[1]
    bad = bytearray(f); bad[len(bad) // 2] ^= 0x40
    csum = bytearray(f); csum[-1] ^= 1
    (g1, g2) = run([bytes(bad), bytes(csum)])
    e1 = o.frame_decompress(bytes(bad))
    assert g1 == e1 and g1[0] == 19 and len(g1[1]) > 0 and data.startswith(g1[1])
    assert g2 == o.frame_decompress(bytes(csum)) and g2[0] == 20 and g2[1] == data


def test_linked_frames_with_dictionary_and_issue15():
    d = synth.repeat256(65536).tobytes()
    datas = [synth.repeat256(65536 * (1 + i % 5) + 17 * i).tobytes()[i:] for i in range(24)]
    frames = [o.frame_compress(x, o.make_settings(block_size=64 << 10, independent_blocks=False, dictionary=d, dictionary_id=5))[1] for x in datas]
    got = run(frames, dictionary=d)
    assert [(st, out) for st, out, _ in got] == [(0, x) for x in datas]
    assert [u for _, _, u in got] == [len(f) for f in frames]
    data = open(os.path.join(GOLD, "issue15_input.bin"), "rb").read()
    f15 = framed.CompressionSettings().independent_blocks(False).block_size(64 * 1024).compress(data)
    assert run([f15]) == [(0, data, len(f15))]


def test_memory_budget_passes_and_refusal():
    data = [synth.silesia_mix((100 + k) << 20, ((100 + k) << 20) + 900_000).tobytes() for k in range(9)]
    frames = [o.frame_compress(x, o.make_settings(block_size=64 << 10, independent_blocks=bool(k % 2)))[1] for k, x in enumerate(data)]
    big = o.frame_compress(synth.silesia_mix(0, 40 << 20).tobytes(), o.make_settings(block_size=1 << 20))[1]
    allf = frames + [big] + frames[:2]
    caps = [2 << 20] * 9 + [48 << 20] + [2 << 20] * 2
    try:
        ffi.lib().lzf_frame_set_memory_budget(64 << 20)
        got = run(allf, caps=caps)
        host = framed.decompress_frames(allf, caps=caps, with_consumed=True)
    finally:
        ffi.lib().lzf_frame_set_memory_budget(0)
    assert got == host
    assert [g[:2] for g in got[:9]] == [(0, x) for x in data] and [g[:2] for g in got[10:]] == [(0, x) for x in data[:2]]
    assert got[9] == (ffi.E_NO_MEMORY, b"", 0)
    assert run([big], caps=[48 << 20])[0][0] == 0


def test_headline_class_4mib_blocks_aliased():
    """3 200 blocks of 4 MiB in one call: 48 distinct default-settings frames of four blocks, aliased over 800 frame slots, one
    tenth of the slots distinct damaged copies."""
    rng = np.random.default_rng(5)
    bases = [synth.silesia_mix((k * 16) << 20, ((k * 16) + 16) << 20).tobytes() for k in range(8)]
    plains = [b[r * 777_001:] + b[:r * 777_001] for b in bases for r in range(6)]          # 48 distinct plaintexts
    frames = framed.CompressionSettings().compress_many(plains)
    d_plain = [dev(p) for p in plains]
    d_frames = [dev(f) for f in frames]
    slots, damaged = [], {}
    for s in range(800):
        k = s % 48
        if s % 10 == 9:
            b = mutate(rng, frames[k])
            damaged[s] = b
            slots.append(dev(b))
        else:
            slots.append(d_frames[k])
    bounds = dict(zip(damaged, device.frame_decompress_bound([slots[s] for s in damaged])))
    caps = [max(16 << 20, int(bounds.get(s, 0))) for s in range(800)]        # out_cap >= out_bound: the reference's results
    outs = [torch.empty(c, dtype=torch.uint8, device=DEV) for c in caps]
    status, out_len, used = device.frame_decompress_many(slots, outs)
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    torch.cuda.synchronize()
    assert launch.startswith("bitmap-fed"), launch
    st, ol, us = status.tolist(), out_len.tolist(), used.tolist()
    for s in range(800):
        k = s % 48
        if s in damaged:
            erc, eout, eused = o.frame_decompress(damaged[s])
            assert (st[s], ol[s], us[s]) == (erc, len(eout), eused), s
            assert bytes(outs[s][:ol[s]].cpu().numpy().tobytes()) == eout
        else:
            assert (st[s], ol[s], us[s]) == (0, 16 << 20, len(frames[k])), s
            assert torch.equal(outs[s], d_plain[k]), s


def test_stream_order_side_stream():
    data = [synth.silesia_mix((20 + 2 * k) << 20, ((20 + 2 * k) << 20) + 1_500_000).tobytes() for k in range(6)]
    frames = framed.CompressionSettings().block_size(64 << 10).compress_many(data)
    srcs = [dev(f) for f in frames]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        dsts = [torch.empty_like(s) for s in srcs]
        for d_, s_ in zip(dsts, srcs):
            d_.copy_(s_, non_blocking=True)
        outs = [torch.empty(len(x), dtype=torch.uint8, device=DEV) for x in data]
        status, out_len, used = device.frame_decompress_many(dsts, outs, stream=side)
    side.synchronize()
    assert status.tolist() == [0] * len(data) and out_len.tolist() == [len(x) for x in data]
    assert used.tolist() == [len(f) for f in frames]
    assert [bytes(t.cpu().numpy().tobytes()) for t in outs] == data
