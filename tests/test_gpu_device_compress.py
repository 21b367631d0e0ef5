"""GPU tests (-m gpu) of lzf_frame_compress_device_many (include/lzfear_frame.h, "frames in device memory"): inputs in HBM
compressed into LZ4 frames in HBM.  Every case holds the device call's status, out_len and bytes to lzf_frame_compress_many on host
copies of the same inputs (the host driver), and where the frame is one the oracle can write, to the oracle's bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_ffi as o
import vectors
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi, framed, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
POISON = 0xA5


def dev(b):
    b = bytes(b)
    if not b:
        return torch.empty(0, dtype=torch.uint8, device=DEV)
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(DEV)


def gsettings(independent_blocks=True, block_checksums=False, content_checksum=True, block_size=4 << 20, dictionary=None,
              dictionary_id=None):
    g = framed.CompressionSettings().independent_blocks(independent_blocks).block_checksums(block_checksums)
    g.content_checksum(content_checksum).block_size(block_size)
    if dictionary is not None:
        g.dictionary(dictionary_id or 0, dictionary)
        if dictionary_id is None:
            g.dictionary_id_nonsense_override(None)
    return g


def host_many(g, datas, caps=None, content_size=None):
    """lzf_frame_compress_many on host buffers: [(status, frame bytes)]."""
    datas = [bytes(d) for d in datas]
    n = len(datas)
    s = g._struct(content_size)
    L = ffi.lib()
    if caps is None:
        caps = [L.lzf_frame_compress_bound(C.byref(s), len(d)) for d in datas]
    outs = [C.create_string_buffer(max(c, 1)) for c in caps]
    olen, st = (C.c_size_t * n)(), (C.c_int * n)()
    ffi.check(L.lzf_frame_compress_many(C.byref(s), n, (C.c_char_p * n)(*datas), (C.c_size_t * n)(*[len(d) for d in datas]),
                                        (C.c_void_p * n)(*[C.addressof(x) for x in outs]), (C.c_size_t * n)(*caps), olen, st))
    return [(st[f], C.string_at(outs[f], olen[f])) for f in range(n)]


def device_struct(g, content_size=None):
    s = g._struct(content_size)
    s.dictionary, s.dictionary_len = None, 0
    return s


def bounds(g, lens, content_size=None):
    s = device_struct(g, content_size)
    return [ffi.lib().lzf_frame_compress_bound(C.byref(s), n) for n in lens]


def device_many(g, ins, caps=None, content_size=None, stream=None):
    """lzf_frame_compress_device_many over CUDA tensors into poisoned outputs: (status list, out_len list, outs)."""
    if caps is None:
        caps = bounds(g, [t.numel() for t in ins], content_size)
    outs = [torch.full((c,), POISON, dtype=torch.uint8, device=DEV) for c in caps]
    d_dict = dev(g._dictionary) if g._dictionary else None
    status, out_len = device.frame_compress_many(device_struct(g, content_size), ins, outs, dictionary=d_dict, stream=stream)
    torch.cuda.synchronize()
    return status.tolist(), out_len.tolist(), outs


def check_against_host(g, datas, caps=None, content_size=None, oracle=None):
    """The device call on device copies of `datas` equals the host driver on `datas` (and the oracle's frames when given)."""
    st, ol, outs = device_many(g, [dev(d) for d in datas], caps=caps, content_size=content_size)
    host = host_many(g, datas, caps=caps, content_size=content_size)
    for f, (hs, hb) in enumerate(host):
        assert (st[f], ol[f]) == (hs, len(hb)), f
        h = outs[f].cpu().numpy()
        assert h[:ol[f]].tobytes() == hb, f
        assert (h[ol[f]:] == POISON).all(), f
        if oracle is not None and hs == 0:
            rc, want = o.frame_compress(datas[f], o.make_settings(content_size=content_size, **oracle))
            assert rc == 0 and hb == want, f
    return st, ol, outs


@pytest.mark.parametrize("bits", range(32))
def test_flag_matrix_exact_frame_bytes(bits):
    """The flag matrix of test_gpu_frame.py's test_flag_matrix_exact_frame_bytes on its 700 000-byte input."""
    data = synth.silesia_mix(0, 700_000).tobytes()
    kw = dict(content_checksum=not (bits & 1), independent_blocks=not (bits & 2), block_size=(256 << 10) if bits & 4 else (64 << 10))
    if bits & 8:
        kw["dictionary"] = bytes([1, 3, 3, 7])
    size = len(data) if bits & 16 else None
    st, ol, outs = check_against_host(gsettings(**kw), [data], content_size=size, oracle=kw)
    assert st == [0]
    got = outs[0][:ol[0]]
    assert framed.decompress_frame(got.cpu().numpy().tobytes(), dictionary=kw.get("dictionary", b"")) == data


def _mixed_inputs():
    mix = synth.silesia_mix(30 << 20, (30 << 20) + 3_000_000).tobytes()
    rnd = vectors.rng_bytes(11, 1_200_000)
    partial = b"".join(mix[k * 65536:(k + 1) * 65536] if k % 2 else rnd[k * 65536:(k + 1) * 65536] for k in range(12)) + rnd[:5000]
    return [b"", mix[:17], vectors.rng_bytes(9, 150_000), partial, mix[:1_300_001], synth.repeat256(5 * 65536 + 1234).tobytes(),
            rnd[:300_000] + mix[:2_400_000]]


@pytest.mark.parametrize("bsum", [False, True])
@pytest.mark.parametrize("bs", [64 << 10, 256 << 10, 1 << 20, 4 << 20])
def test_mixed_frames_one_call(bs, bsum):
    """Empty, 17 bytes, random (every block stored), some blocks stored, repeat256 and text in one call."""
    datas = _mixed_inputs()
    kw = dict(block_size=bs, block_checksums=bsum)
    st, ol, _ = check_against_host(gsettings(**kw), datas, oracle=kw)
    launch = ffi.lib().lzf_last_compress_launch().decode()
    assert st == [0] * len(datas)
    assert ol[2] > 150_000                               # stored blocks: larger than the input
    if bs == 4 << 20:
        assert launch == "lzf_compress_team_kernel", launch


@pytest.mark.parametrize("indep", [True, False])
def test_frames_of_65_blocks_cross_the_assembly_round(indep):
    """65 blocks of 64 KiB per frame, block checksums on: the assembly kernel places 64 blocks per round, so block 64's length
    word goes behind the first round's total (the carry of the wave scan).  Text, and text with the last block stored (random
    bytes: its span differs from its neighbours'), in one call."""
    mix = synth.silesia_mix(9 << 20, (9 << 20) + 65 * 65536).tobytes()
    datas = [mix, mix[:64 * 65536] + vectors.rng_bytes(65, 65536)]
    kw = dict(block_size=64 << 10, block_checksums=True, independent_blocks=indep)
    st, ol, outs = check_against_host(gsettings(**kw), datas, oracle=kw)
    assert st == [0, 0]
    for d, n, t in zip(datas, ol, outs):
        assert framed.decompress_frame(t[:n].cpu().numpy().tobytes()) == d


def test_dictionaries():
    """A 70 000-byte dictionary with an id for independent and linked blocks, linked streams of 1, 2 and 17 blocks in one call,
    and a 4-byte dictionary."""
    d = synth.gen_text_zipf(3, 70000).tobytes()
    mix = synth.silesia_mix(50 << 20, (50 << 20) + 1_200_000).tobytes()
    datas = [mix[:50_000], mix[:100_000], mix[5:17 * 65536 - 1000], b"", mix[:65536], synth.repeat256(3 * 65536).tobytes()]
    for indep in (True, False):
        for bsum in (False, True):
            kw = dict(block_size=64 << 10, independent_blocks=indep, block_checksums=bsum, dictionary=d, dictionary_id=77)
            st, ol, outs = check_against_host(gsettings(**kw), datas, oracle=kw)
            assert st == [0] * len(datas)
            for x, t, n in zip(datas, outs, ol):
                assert framed.decompress_frame(t[:n].cpu().numpy().tobytes(), dictionary=d) == x
    for indep in (True, False):
        kw = dict(block_size=64 << 10, independent_blocks=indep, dictionary=b"\x01\x03\x03\x07")
        st, _, _ = check_against_host(gsettings(**kw), datas, oracle=kw)
        assert st == [0] * len(datas)


INVALID_BLOCK_SIZE, PANIC = 27, 28          # LZF_F_INVALID_BLOCK_SIZE, LZF_F_PANIC


@pytest.mark.parametrize("bs, want", [(100_000, INVALID_BLOCK_SIZE), (128 << 10, INVALID_BLOCK_SIZE), (16 << 20, PANIC)])
def test_bad_block_size(bs, want):
    """Every frame gets the host driver's status, out_len 0 and an untouched output."""
    datas = [b"", b"abc", synth.silesia_mix(0, 300_000).tobytes()]
    g = gsettings(block_size=bs)
    caps = [4096, 4096, 400_000]
    st, ol, outs = device_many(g, [dev(x) for x in datas], caps=caps)
    host = host_many(g, datas, caps=caps)
    assert [h[0] for h in host] == [want] * 3
    assert st == [want] * 3 and ol == [0] * 3
    for t in outs:
        assert (t.cpu().numpy() == POISON).all()


def test_capacity_and_red_zones():
    """Outputs carved from one poisoned arena at varying low address bits, 4 KiB apart, capacities the bound and the bound - 1:
    nothing outside [0, out_len) is written, nothing at all for an LZF_OUT_CAPACITY frame.  Inputs with two different poisons
    behind in_len give the same results."""
    base = _mixed_inputs()
    datas = base + base
    results = []
    for poison_in in (0x00, 0xFF):
        for ki, kw in enumerate((dict(block_size=64 << 10, block_checksums=True), dict(block_size=64 << 10, independent_blocks=False))):
            rng = np.random.default_rng(5 + ki)                   # (the same arena layout for both input poisons)
            g = gsettings(**kw)
            b = bounds(g, [len(x) for x in datas])
            caps = [c if i < len(base) else c - 1 for i, c in enumerate(b)]
            pos, offs = 0, []
            for c in caps:
                pos += 4096 + int(rng.integers(0, 64))
                offs.append(pos)
                pos += c
            arena = torch.full((pos + 4096,), POISON, dtype=torch.uint8, device=DEV)
            outs = [arena[a:a + c] for a, c in zip(offs, caps)]
            ins = []
            for x in datas:                                   # the input, then poison up to the end of its allocation
                t = torch.full((len(x) + 4096,), poison_in, dtype=torch.uint8, device=DEV)
                if x:
                    t[:len(x)] = dev(x)
                ins.append(t[:len(x)])
            status, out_len = device.frame_compress_many(device_struct(g), ins, outs)
            torch.cuda.synchronize()
            st, ol = status.tolist(), out_len.tolist()
            host = host_many(g, datas, caps=caps)
            h = arena.cpu().numpy()
            expect = np.full_like(h, POISON)
            for a, (hs, hb), s_, l_ in zip(offs, host, st, ol):
                assert (s_, l_) == (hs, len(hb))
                expect[a:a + len(hb)] = np.frombuffer(hb, dtype=np.uint8)
            assert np.array_equal(h, expect)
            assert st[:len(base)] == [0] * len(base) and st[len(base):] == [ffi.OUT_CAPACITY] * len(base)
            results.append((st, ol, h))
    for a, b in zip(results[:2], results[2:]):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_large_call_aliased_4mib_blocks():
    """3 104 blocks of 4 MiB in one call (194 frames of 16 blocks aliased from 2 distinct inputs): the compact kernel's class;
    every frame equals the host frame of its source."""
    srcs = [synth.silesia_mix(k << 26, (k + 1) << 26).tobytes() for k in range(2)]
    d_src = [dev(x) for x in srcs]
    g = gsettings()
    host = host_many(g, srcs)
    ins = [d_src[s % 2] for s in range(194)]
    caps = bounds(g, [t.numel() for t in ins])
    outs = [torch.empty(c, dtype=torch.uint8, device=DEV) for c in caps]
    status, out_len = device.frame_compress_many(device_struct(g), ins, outs)
    launch = ffi.lib().lzf_last_compress_launch().decode()
    torch.cuda.synchronize()
    assert launch == "lzf_compress_compact_kernel", launch
    ref = [dev(hb) for _, hb in host]
    st, ol = status.tolist(), out_len.tolist()
    for s in range(194):
        assert (st[s], ol[s]) == (0, len(host[s % 2][1])), s
        assert torch.equal(outs[s][:ol[s]], ref[s % 2]), s


def test_memory_budget_passes():
    """A budget that makes every frame a pass of its own gives the results of the call without one."""
    data = [synth.silesia_mix((100 + k) << 20, ((100 + k) << 20) + 900_000).tobytes() for k in range(5)]
    d = synth.gen_text_zipf(4, 70000).tobytes()
    for kw in (dict(block_size=64 << 10, block_checksums=True), dict(block_size=64 << 10, independent_blocks=False, dictionary=d),
               dict(block_size=256 << 10, dictionary=d, dictionary_id=3)):
        g = gsettings(**kw)
        ins = [dev(x) for x in data]
        one = device_many(g, ins)
        try:
            ffi.lib().lzf_frame_set_memory_budget(1 << 20)
            many = device_many(g, ins)
        finally:
            ffi.lib().lzf_frame_set_memory_budget(0)
        assert one[0] == many[0] == [0] * 5 and one[1] == many[1]
        for a, b in zip(one[2], many[2]):
            assert torch.equal(a, b)
        host = host_many(g, data)
        assert [bytes(t[:n].cpu().numpy().tobytes()) for t, n in zip(one[2], one[1])] == [hb for _, hb in host]


def test_stream_order_and_host_memory():
    """Inputs produced by a kernel on a side stream, the call queued behind it with no synchronisation, the host arrays given
    to the call overwritten as soon as it returns: the results are right once the stream has finished, and lzf_frame_stats
    has not moved."""
    data = [synth.silesia_mix((20 + 2 * k) << 20, ((20 + 2 * k) << 20) + 1_500_000).tobytes() for k in range(6)]
    srcs = [dev(x) for x in data]
    g = gsettings(block_size=64 << 10, block_checksums=True)
    host = host_many(g, data)
    caps = bounds(g, [len(x) for x in data])
    torch.cuda.synchronize()
    stats = ffi.frame_stats()
    side = torch.cuda.Stream(device=DEV)
    n = len(data)
    with torch.cuda.stream(side):
        ins = [torch.empty_like(s_) for s_ in srcs]
        for d_, s_ in zip(ins, srcs):
            d_.copy_(s_, non_blocking=True)
        outs = [torch.empty(c, dtype=torch.uint8, device=DEV) for c in caps]
        status = torch.empty(n, dtype=torch.int32, device=DEV)
        out_len = torch.empty(n, dtype=torch.int64, device=DEV)
        s = device_struct(g)
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ins])
        lens = (C.c_size_t * n)(*[t.numel() for t in ins])
        optr = (C.c_void_p * n)(*[t.data_ptr() for t in outs])
        ocap = (C.c_size_t * n)(*caps)
        rc = ffi.lib().lzf_frame_compress_device_many(C.byref(s), n, ptrs, lens, None, 0, optr, ocap, out_len.data_ptr(),
                                                      status.data_ptr(), side.cuda_stream)
        for arr in (ptrs, optr):
            for i in range(n):
                arr[i] = 0
        for arr in (lens, ocap):
            for i in range(n):
                arr[i] = 1
        C.memset(C.byref(s), 0xFF, C.sizeof(s))
    assert rc == 0
    side.synchronize()
    assert status.tolist() == [0] * n and out_len.tolist() == [len(hb) for _, hb in host]
    assert [bytes(t[:len(hb)].cpu().numpy().tobytes()) for t, (_, hb) in zip(outs, host)] == [hb for _, hb in host]
    assert ffi.frame_stats() == stats


def test_round_trip_on_the_device():
    """lzf_frame_decompress_device_many decodes the device frames back to the inputs without a host copy of the frames."""
    datas = _mixed_inputs()
    ins = [dev(x) for x in datas]
    for g in (gsettings(block_size=64 << 10, block_checksums=True), gsettings(block_size=64 << 10, independent_blocks=False),
              gsettings(block_size=1 << 20)):
        frames = g.compress_many_device(ins)
        assert all(f.is_cuda for f in frames)
        got = framed.decompress_frames_device(frames, caps=[max(len(x), 1) for x in datas])
        for (st, out, used), x, f, t in zip(got, datas, frames, ins):
            assert st == 0 and used == f.numel()
            assert torch.equal(out, t)
