"""Timing of lzf_frame_compress_device_many (inputs in HBM in, LZ4 frames in HBM out).  Never writes the bench.py line.

One process, a warm-up, HIP events around the call, the median of --runs runs (every run printed).  Cases:
  a  240 frames x 51 blocks of 4 MiB (silesia stand-in, --distinct inputs aliased), content_checksum(false), next to
     lzf_compress_batch on the same 12 240 blocks
  b  the same frames with default settings (content checksums)
  c  4 096 linked streams of 1 MiB in 64 KiB blocks behind a 64 KiB dictionary (bench.py's config5 shape), next to the host
     driver lzf_frame_compress_many on the same data
Every case checks its output once: the frames decode on the device (lzf_frame_decompress_device_many) to their inputs, and each
distinct input's frame equals the host driver's frame.

  python tools/device_compress_bench.py [--cases abc] [--runs 5] [--frames 240] [--blocks 51] [--distinct 2]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import device, ffi, framed, synth  # noqa: E402

DEV = torch.device("cuda", 0)
GiB = float(1 << 30)


def timed(fn, runs):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), ts


def host_frames(g, datas):
    """lzf_frame_compress_many (the host driver) on host buffers."""
    n = len(datas)
    s = g._struct(None)
    L = ffi.lib()
    caps = [L.lzf_frame_compress_bound(C.byref(s), len(d)) for d in datas]
    outs = [C.create_string_buffer(c) for c in caps]
    olen, st = (C.c_size_t * n)(), (C.c_int * n)()
    args = (C.byref(s), n, (C.c_char_p * n)(*datas), (C.c_size_t * n)(*[len(d) for d in datas]),
            (C.c_void_p * n)(*[C.addressof(x) for x in outs]), (C.c_size_t * n)(*caps), olen, st)
    return args, outs, olen, st


def run_host(g, datas):
    args, outs, olen, st = host_frames(g, datas)
    ffi.check(ffi.lib().lzf_frame_compress_many(*args))
    assert list(st) == [0] * len(datas)
    return [C.string_at(outs[f], olen[f]) for f in range(len(datas))]


def device_call(g, ins, dictionary=None):
    """(call, outs, result dict) for lzf_frame_compress_device_many over `ins` into outputs of the bound."""
    s = g._struct(None)
    s.dictionary, s.dictionary_len = None, 0
    caps = [ffi.lib().lzf_frame_compress_bound(C.byref(s), t.numel()) for t in ins]
    outs = [torch.empty(c, dtype=torch.uint8, device=DEV) for c in caps]
    res = {}

    def call():
        res["r"] = device.frame_compress_many(s, ins, outs, dictionary=dictionary)
        res["launch"] = ffi.lib().lzf_last_compress_launch().decode()
    return call, outs, res


def check(g, ins, outs, res, distinct, host, dictionary=None):
    """status / out_len of every frame, every frame equal to its source's host frame, the distinct frames decoded on the device."""
    st, ol = res["r"]
    torch.cuda.synchronize()
    st, ol = st.tolist(), ol.tolist()
    assert st == [0] * len(ins)
    ref = [torch.frombuffer(bytearray(h), dtype=torch.uint8).to(DEV) for h in host]
    for f in range(len(ins)):
        assert ol[f] == len(host[f % distinct]) and torch.equal(outs[f][:ol[f]], ref[f % distinct]), f
    dec = framed.decompress_frames_device([outs[f][:ol[f]] for f in range(distinct)], dictionary=dictionary,
                                          caps=[ins[f].numel() for f in range(distinct)])
    for f, (s_, t, _) in enumerate(dec):
        assert s_ == 0 and torch.equal(t, ins[f]), f
    return sum(ol)


def frames_case(args, content_checksum):
    bs = 4 << 20
    n = min(args.blocks * bs, synth.SILESIA_TOTAL)      # bench.py's unit: one silesia_mix copy, 51 blocks of 4 MiB (the last one short)
    plains = [synth.silesia_mix(0, n, copy=k).tobytes() for k in range(args.distinct)]
    d_plain = [torch.frombuffer(bytearray(p), dtype=torch.uint8).to(DEV) for p in plains]
    ins = [d_plain[f % args.distinct] for f in range(args.frames)]
    g = framed.CompressionSettings().content_checksum(content_checksum)
    call, outs, res = device_call(g, ins)
    med, ts = timed(call, args.runs)
    total = sum(t.numel() for t in ins)
    host = run_host(g, plains)
    out_bytes = check(g, ins, outs, res, args.distinct, host)
    out = dict(ms=med, runs=ts, gib_s=total / GiB / (med / 1e3), blocks=args.frames * ((n + bs - 1) // bs), bytes=total, out_bytes=out_bytes,
               launch=res["launch"])
    del outs, res
    return out, ins


def raw_case(args, ins):
    """The same blocks through one lzf_compress_batch (fresh tables, out_cap = block length, as the frame layer's jobs)."""
    bs = 4 << 20
    per = (ins[0].numel() + bs - 1) // bs
    nj = len(ins) * per
    jobs = np.zeros(nj, dtype=device.CJOB)
    out = torch.empty(len(ins) * ins[0].numel(), dtype=torch.uint8, device=DEV)
    j = 0
    for f, t in enumerate(ins):
        for k in range(per):
            n = min(bs, t.numel() - k * bs)
            jobs[j]["input"] = t.data_ptr() + k * bs; jobs[j]["input_len"] = n
            jobs[j]["out"] = out.data_ptr() + f * t.numel() + k * bs; jobs[j]["out_cap"] = n
            j += 1
    jobs["table_kind"] = ffi.TABLE_U32
    d_jobs = device.to_device(jobs, DEV)
    d_res = torch.zeros(nj * 16, dtype=torch.uint8, device=DEV)
    med, ts = timed(lambda: device.compress_batch(d_jobs, d_res, nj, kinds=ffi.KINDS_U32 | ffi.KINDS_U32_FRESH_ONLY), args.runs)
    r = device.results_to_host(d_res, nj)
    assert np.isin(r["status"], [0, ffi.OUTPUT_FULL]).all()
    total = sum(t.numel() for t in ins)
    return dict(ms=med, runs=ts, gib_s=total / GiB / (med / 1e3), blocks=nj, launch=ffi.lib().lzf_last_compress_launch().decode())


def linked_case(args):
    """4 096 linked streams of 1 MiB (16 distinct inputs aliased), 64 KiB blocks, a 64 KiB dictionary; device call against host driver."""
    S, SL, distinct = args.streams, 1 << 20, 16
    plains = [synth.silesia_mix(k * SL, (k + 1) * SL).tobytes() for k in range(distinct)]
    dct = synth.silesia_mix(100 << 20, (100 << 20) + 65536).tobytes()
    g = framed.CompressionSettings().independent_blocks(False).block_size(64 << 10).dictionary(1, dct)
    d_plain = [torch.frombuffer(bytearray(p), dtype=torch.uint8).to(DEV) for p in plains]
    d_dict = torch.frombuffer(bytearray(dct), dtype=torch.uint8).to(DEV)
    ins = [d_plain[s % distinct] for s in range(S)]
    call, outs, res = device_call(g, ins, dictionary=d_dict)
    med, ts = timed(call, args.runs)
    host = run_host(g, plains)
    check(g, ins, outs, res, distinct, host, dictionary=d_dict)
    hargs, houts, _, hst = host_frames(g, [plains[s % distinct] for s in range(S)])      # (houts: the buffers hargs points at)
    L = ffi.lib()
    ffi.check(L.lzf_frame_compress_many(*hargs))                   # (warm-up)
    hts = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        ffi.check(L.lzf_frame_compress_many(*hargs))
        hts.append((time.perf_counter() - t0) * 1e3)
    assert list(hst) == [0] * S
    del houts
    total = S * SL
    return dict(ms=med, runs=ts, gib_s=total / GiB / (med / 1e3), host_ms=statistics.median(hts), host_runs=hts,
                host_gib_s=total / GiB / (statistics.median(hts) / 1e3), launch=res["launch"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--blocks", type=int, default=51)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--streams", type=int, default=4096)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    r2 = lambda v: [round(t, 2) for t in v]
    if "a" in args.cases:
        a, ins = frames_case(args, False)
        print(f"(a) device frames, no content checksum: {a['blocks']} blocks, {a['bytes'] / GiB:.1f} GiB in, {a['out_bytes'] / GiB:.1f} GiB of frames, "
              f"median {a['ms']:.2f} ms, {a['gib_s']:.1f} GiB/s  [{a['launch']}]  runs {r2(a['runs'])}", flush=True)
        torch.cuda.empty_cache()
        raw = raw_case(args, ins)
        print(f"(a) raw lzf_compress_batch, same blocks: {raw['blocks']} blocks, median {raw['ms']:.2f} ms, {raw['gib_s']:.1f} GiB/s  [{raw['launch']}]  "
              f"runs {r2(raw['runs'])}", flush=True)
        print(f"(a) ratio device frames / raw: {a['gib_s'] / raw['gib_s']:.3f}", flush=True)
        del ins
        torch.cuda.empty_cache()
    if "b" in args.cases:
        b, _ = frames_case(args, True)
        print(f"(b) device frames, default settings (content checksums): median {b['ms']:.2f} ms, {b['gib_s']:.1f} GiB/s  runs {r2(b['runs'])}", flush=True)
        torch.cuda.empty_cache()
    if "c" in args.cases:
        c = linked_case(args)
        print(f"(c) {args.streams} linked streams of 1 MiB, 64 KiB blocks, 64 KiB dictionary: device median {c['ms']:.2f} ms, {c['gib_s']:.2f} GiB/s  "
              f"[{c['launch']}]  runs {r2(c['runs'])}", flush=True)
        print(f"(c) host driver lzf_frame_compress_many, same data: median {c['host_ms']:.2f} ms, {c['host_gib_s']:.2f} GiB/s  runs {r2(c['host_runs'])}", flush=True)
        print(f"(c) ratio device / host driver: {c['gib_s'] / c['host_gib_s']:.3f}", flush=True)


if __name__ == "__main__":
    main()
