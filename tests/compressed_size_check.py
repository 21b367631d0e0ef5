"""The compressed-size calls on the GPU, group by group; tests/test_gpu_compressed_size.py runs every group as a script in a child
process of its own (`python compressed_size_check.py GROUP`).  The cases and their expectations are tests/compressed_size_cases.py's,
pinned to the oracle on the CPU.  All comparisons are exact integers, statuses and bytes; every group prints the number of cases it
compared and the test asserts it.

    raw      lzf_compressed_size_batch with out = NULL == the expectation == lzf_compress_batch on fresh copies of the tables;
             the caller's tables afterwards == the compress call's == the expectation; read-only tables unchanged
    redzone  the same call with `out` pointing into a poisoned buffer between red zones, the bytes behind every input 0x00, then
             0xFF: not one byte of the buffer changes, the answers do not depend on the poison
    host     lzf_compressed_size_batch_host: the same answers and tables
    frame    lzf_frame_compressed_size_device == lzf_frame_compress_device_many's (status, out_len) == the oracle frame's length
    stream   lzf_frame_compress_stream_size_device == lzf_frame_compress_stream_device's (status, out_len)
    exact    compress_many_device / compress_streams_device with exact=True: the bytes of exact=False in storage of exactly that size
    launch   lzf_last_compress_launch reads the same before and after a size call"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import compressed_size_cases as cc  # noqa: E402
import oracle_ffi as o  # noqa: E402
import redzone  # noqa: E402
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import device, ffi, framed  # noqa: E402

DEV = torch.device("cuda", 0)
POISON = redzone.OUT_POISON


def dev(b):
    b = bytes(b)
    if not b:
        return torch.empty(0, dtype=torch.uint8, device=DEV)
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(DEV)


def run_case(c, call_fn, out_mode, in_poison=0x00):
    """Every call of the case through call_fn(d_jobs, d_res, n, kinds).  out_mode: "null" (out = NULL), "poison" (out inside a poisoned
    buffer that must come back untouched) or "real" (room for the output: the compress call).  Returns per call
    ([(status, out_len)], {slot: table bytes after the call})."""
    tables = {k: dev(v["init"]) for k, v in c["tables"].items()}
    for t in tables.values():
        assert t.data_ptr() % 8 == 0
    rng = np.random.default_rng(5)
    per_call = []
    for ci, call in enumerate(c["calls"]):
        for slot, add in c["adds"][ci].items():
            ffi.check(ffi.lib().lzf_table_offset(tables[slot].data_ptr(), c["tables"][slot]["kind"], add, None))
        n = len(call)
        lows = [j["in_low"] for j in call]
        explicit = any(v is not None for v in lows)
        offs, total, arena = redzone._place([len(j["input"]) for j in call], lows, rng, DEV, explicit)
        h_in = np.full(total, in_poison, dtype=np.uint8)
        for off, j in zip(offs, call):
            h_in[off:off + len(j["input"])] = np.frombuffer(j["input"], dtype=np.uint8)
        d_in = redzone._upload(h_in, arena, DEV)
        jobs = np.zeros(n, dtype=device.CJOB)
        jobs["input"] = np.uint64(d_in.data_ptr()) + np.array(offs, dtype=np.uint64)
        if explicit:
            assert [int(a) & 15 for a in jobs["input"]] == [v & 15 for v in lows]
        jobs["input_len"] = [len(j["input"]) for j in call]
        jobs["cursor"] = [j["cursor"] for j in call]
        jobs["table_kind"] = [j["kind"] for j in call]
        jobs["table"] = [tables[j["slot"]].data_ptr() if j["slot"] is not None else 0 for j in call]
        jobs["flags"] = [ffi.CJOB_TABLE_READONLY if j["readonly"] else 0 for j in call]
        bounds = [cc.bound(len(j["input"]) - min(j["cursor"], len(j["input"]))) for j in call]
        d_out = None
        if out_mode == "real":                                   # UINT64_MAX cannot be a buffer: the bound, which compress2 never exceeds
            caps = [b if j["cap"] is None else min(j["cap"], b) for j, b in zip(call, bounds)]
            starts = np.concatenate([[0], np.cumsum([(cp + 255) // 256 * 256 for cp in caps])]).astype(np.uint64)
            d_out = torch.empty(int(starts[-1]) + 256, dtype=torch.uint8, device=DEV)
            jobs["out"] = np.uint64(d_out.data_ptr()) + starts[:-1]
            jobs["out_cap"] = caps
        else:
            jobs["out_cap"] = [cc.UINT64_MAX if j["cap"] is None else j["cap"] for j in call]
            if out_mode == "poison":
                d_out = torch.full((2 * redzone.ZONE + 64 * n,), POISON, dtype=torch.uint8, device=DEV)
                jobs["out"] = np.uint64(d_out.data_ptr() + redzone.ZONE) + np.arange(n, dtype=np.uint64) * np.uint64(61)
        d_jobs = device.to_device(jobs, DEV)
        d_res = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
        call_fn(d_jobs, d_res, n, cc.call_kinds(c, call))
        torch.cuda.synchronize()
        res = device.results_to_host(d_res, n)
        if out_mode == "poison":
            assert bool((d_out == POISON).all()), f"{c['name']}: the size call wrote into `out`"
        assert np.array_equal(d_in.cpu().numpy(), h_in), f"{c['name']}: the input arena was written to"
        per_call.append(([(int(s), int(n_)) for s, n_ in zip(res["status"], res["out_len"])],
                         {k: t.cpu().numpy().tobytes() for k, t in tables.items()}))
    return per_call


def compare(c, got, want, what, tables=True):
    for ci, ((res, tabs), (wres, wtabs)) in enumerate(zip(got, want)):
        for ji, (a, b) in enumerate(zip(res, wres)):
            assert a == b, f"{c['name']}, call {ci}, job {ji}: {what}: (status, out_len) {a} != {b}"
        if tables:
            for k in tabs:
                assert tabs[k] == wtabs[k], f"{c['name']}, call {ci}: {what}: table {k!r} differs"


def expected(c):
    return [(res, tabs) for res, tabs, _ in cc.expectations(c["name"])]


def group_raw():
    n = 0
    for c in cc.cases():
        size = run_case(c, device.compressed_size_batch, "null")
        comp = run_case(c, device.compress_batch, "real")
        compare(c, size, expected(c), "size call against the oracle")
        compare(c, size, comp, "size call against lzf_compress_batch")
        for k, v in c["tables"].items():
            if all(j["readonly"] for call in c["calls"] for j in call if j["slot"] == k):
                assert size[-1][1][k] == v["init"], f"{c['name']}: read-only table {k!r} changed"
        n += 1
    return n


def group_redzone():
    n = 0
    for c in cc.cases():
        a = run_case(c, device.compressed_size_batch, "poison", in_poison=0x00)
        b = run_case(c, device.compressed_size_batch, "poison", in_poison=0xFF)
        compare(c, a, expected(c), "poisoned out, input poison 0x00")
        compare(c, b, expected(c), "poisoned out, input poison 0xFF")
        n += 1
    return n


def group_host():
    n = 0
    for c in cc.cases():
        def host_tables():
            t = {}
            for k, v in c["tables"].items():
                t[k] = (ffi.U32Table if v["kind"] == cc.U32 else ffi.U16Table)()
                C.memmove(C.addressof(t[k]), v["init"], len(v["init"]))
            return t
        tabs, ctabs = host_tables(), host_tables()
        for ci, (call, (wres, wtabs)) in enumerate(zip(c["calls"], expected(c))):
            for slot, add in c["adds"][ci].items():
                tabs[slot].offset += add; ctabs[slot].offset += add
            items = [dict(input=j["input"], cursor=j["cursor"], kind=j["kind"], out_cap=j["cap"], table=tabs[j["slot"]] if j["slot"] else None,
                          readonly=j["readonly"]) for j in call]
            got = ffi.compressed_sizes_host(items)
            # (the host call has no table_kinds word, hence no promise to break: such a job is held to the host compress call instead)
            citems = [dict(it, table=ctabs[j["slot"]] if j["slot"] else None, out_cap=cc.bound(len(j["input"])) if j["cap"] is None else j["cap"])
                      for it, j in zip(items, call)]
            comp = ffi.compress_blocks_host(citems)
            for ji, (g, w, (crc, cout)) in enumerate(zip(got, wres, comp)):
                if (ci, ji) in c["contract"]:
                    assert g == (crc, len(cout)) and crc == ffi.OK, (c["name"], ci, ji, g)
                else:
                    assert g == w, f"{c['name']}, call {ci}, job {ji}: host size call {g} != {w}"
                    assert g[0] == crc and (crc != ffi.OK or g[1] == len(cout)), (c["name"], ci, ji, g, crc)
            for k in tabs:
                assert bytes(tabs[k]) == bytes(ctabs[k]), f"{c['name']}, call {ci}: host table {k!r} differs from the compress call's"
                if not c["contract"]:
                    assert bytes(tabs[k]) == wtabs[k], f"{c['name']}, call {ci}: host table {k!r} differs from the oracle's"
        n += 1
    return n


def gsettings(independent_blocks=True, block_checksums=False, content_checksum=True, block_size=4 << 20, dictionary=None):
    g = framed.CompressionSettings().independent_blocks(independent_blocks).block_checksums(block_checksums)
    g.content_checksum(content_checksum).block_size(block_size)
    if dictionary is not None:
        g.dictionary(0, dictionary)
        g.dictionary_id_nonsense_override(None)
    return g


def device_struct(g, content_size=None):
    s = g._struct(content_size)
    s.dictionary, s.dictionary_len = None, 0
    return s


def frame_both(g, ins, content_size=None):
    """(size call, compress call) as lists of (status, out_len)"""
    s = device_struct(g, content_size)
    d_dict = dev(g._dictionary) if g._dictionary else None
    st, ol = device.frame_compressed_size(s, ins, dictionary=d_dict)
    torch.cuda.synchronize()
    size = list(zip(st.tolist(), ol.tolist()))
    caps = [ffi.lib().lzf_frame_compress_bound(C.byref(s), t.numel()) for t in ins]
    outs = [torch.empty(max(cp, 1), dtype=torch.uint8, device=DEV)[:cp] for cp in caps]
    st, ol = device.frame_compress_many(s, ins, outs, dictionary=d_dict)
    torch.cuda.synchronize()
    return size, list(zip(st.tolist(), ol.tolist()))


def group_frame():
    datas = cc.frame_inputs()
    ins = [dev(d) for d in datas]
    n = 0
    for kw, with_size in cc.flag_combos():
        size, comp = frame_both(gsettings(**kw), ins, content_size=12345 if with_size else None)
        want = [(0, cc.oracle_frame_len(kw, d, with_size)) for d in datas]
        assert size == want, (kw, with_size, size, want)
        assert size == comp, (kw, with_size, size, comp)
        n += len(datas)
    # a content checksum is 4 bytes of the answer, whatever its value
    on, _ = frame_both(gsettings(block_size=cc.FRAME_BS, content_checksum=True), ins)
    off, _ = frame_both(gsettings(block_size=cc.FRAME_BS, content_checksum=False), ins)
    assert [a[1] - b[1] for a, b in zip(on, off)] == [4] * len(ins)
    # a bad block size fails every frame, as in the compress call
    for bs, code in ((12345, o.F_INVALID_BLOCK_SIZE), (1 << 24, o.F_PANIC)):
        size, comp = frame_both(gsettings(block_size=bs), ins)
        assert size == comp == [(code, 0)] * len(ins), (bs, size, comp)
        n += len(ins)
    return n


def stream_both(g, frame_bytes, ins, with_size):
    s = device_struct(g, 0 if with_size else None)
    d_dict = dev(g._dictionary) if g._dictionary else None
    st, ol = device.stream_compressed_size(s, frame_bytes, ins, dictionary=d_dict)
    torch.cuda.synchronize()
    size = list(zip(st.tolist(), ol.tolist()))
    caps = [ffi.lib().lzf_frame_compress_stream_bound(C.byref(s), frame_bytes, t.numel()) for t in ins]
    outs = [torch.empty(cp, dtype=torch.uint8, device=DEV) for cp in caps]
    st, ol = device.stream_compress(s, frame_bytes, ins, outs, dictionary=d_dict)
    torch.cuda.synchronize()
    return size, list(zip(st.tolist(), ol.tolist())), outs


def group_stream():
    datas = cc.stream_inputs()
    assert [len(d) for d in datas] == [0, 1, 65536, 200001, 1 << 20]
    ins = [dev(d) for d in datas]
    n = 0
    for fb in cc.STREAM_FRAME_BYTES:
        for kw, with_size in ((dict(block_size=cc.FRAME_BS), False), (dict(block_size=cc.FRAME_BS, block_checksums=True), True),
                              (dict(block_size=cc.FRAME_BS, independent_blocks=False, dictionary=cc.FRAME_DICT), False)):
            size, comp, outs = stream_both(gsettings(**kw), fb, ins, with_size)
            assert size == comp and all(s == 0 for s, _ in size), (fb, kw, size, comp)
            # ... which is the sum of the oracle's frames over the pieces
            for d, (_, ln) in zip(datas, size):
                pieces = [d[a:a + fb] for a in range(0, len(d), fb)] or [b""]
                assert ln == sum(cc.oracle_frame_len(kw, p, with_size) for p in pieces), (fb, kw, len(d), ln)
            n += len(datas)
    return n


def group_exact():
    datas = cc.frame_inputs() + [cc.stream_inputs()[3]]
    ins = [dev(d) for d in datas]
    n = 0
    for kw in (dict(block_size=cc.FRAME_BS), dict(block_size=cc.FRAME_BS, independent_blocks=False, dictionary=cc.FRAME_DICT, block_checksums=True)):
        g = gsettings(**kw)
        plain = g.compress_many_device(ins)
        exact = g.compress_many_device(ins, exact=True)
        sizes = g.compressed_sizes_device(ins)
        for d, a, b, sz in zip(datas, plain, exact, sizes):
            assert b.numel() == a.numel() == sz == cc.oracle_frame_len(kw, d, False)
            assert b.untyped_storage().nbytes() == b.numel() and a.untyped_storage().nbytes() >= a.numel()
            assert torch.equal(a, b)
            n += 1
        for fb in cc.STREAM_FRAME_BYTES:
            plain = g.compress_streams_device(ins, fb)
            exact = g.compress_streams_device(ins, fb, exact=True)
            for a, b in zip(plain, exact):
                assert b.numel() == a.numel() and b.untyped_storage().nbytes() == b.numel() and torch.equal(a, b)
                n += 1
    return n


def group_launch():
    c = next(x for x in cc.cases() if x["cls"] == "mixed")
    small = dict(c, calls=[c["calls"][0][:40]])

    def launch():
        return ffi.lib().lzf_last_compress_launch().decode()
    run_case(small, device.compress_batch, "real")
    before = launch()
    assert "lzf_compress" in before
    run_case(small, device.compressed_size_batch, "null")
    assert launch() == before, (before, launch())
    run_case(small, device.compress_batch, "real")
    assert launch() == before, (before, launch())
    return 1


GROUPS = dict(raw=group_raw, redzone=group_redzone, host=group_host, frame=group_frame, stream=group_stream, exact=group_exact, launch=group_launch)
# the number of cases each group compares (tests/test_gpu_compressed_size.py asserts it: nothing skipped, nothing filtered out)
COUNTS = dict(raw=13, redzone=13, host=13, frame=170, stream=30, exact=36, launch=1)

if __name__ == "__main__":
    name = sys.argv[1]
    print(f"{name} ok: {GROUPS[name]()} cases")
