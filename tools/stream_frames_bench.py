"""Timing of the streams of back-to-back frames in device memory (lzf_frame_decompress_stream_device /
lzf_frame_compress_stream_device).  Never writes the bench.py line.

One process, a warm-up, HIP events around the call, the median of --runs runs; where two calls are compared they alternate.
  a  a 1 GiB payload (silesia_mix tiled), default settings: written as ONE frame and decoded with
     lzf_frame_decompress_device_many (the yardstick: one content checksum chain), against the same payload written as a
     stream of 4 MiB and of 32 MiB frames and decoded with lzf_frame_decompress_stream_device
  b  240 streams of 51 four-MiB frames, content_checksum(false): the stream call against lzf_frame_decompress_device_many on
     the same frames with their addresses from the host
  c  the stream scan alone (lzf_frame_stream_bound_device) on one 1 GiB stream of single-block 64 KiB frames
  w  the write side: lzf_frame_compress_stream_device against lzf_frame_compress_device_many over the same pieces
  t  one decode of the 4 MiB-frame stream of (a), for a kernel trace: --save FILE writes the stream (run it first, untraced),
     --load FILE decodes it (under the tracer: only the decode's kernels are in the trace)
Streams are aliased: --distinct distinct ones serve the slots.

  python tools/stream_frames_bench.py [--cases abcw] [--runs 5] [--streams 240] [--distinct 2]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import device, ffi, framed, synth  # noqa: E402

DEV = torch.device("cuda", 0)
GiB = float(1 << 30)
MiB = 1 << 20


def up(b):
    return torch.from_numpy(np.ascontiguousarray(b)).to(DEV)


def timed_alternating(fns, runs):
    """Median ms of every fn, the fns called in turn: run k of each before run k + 1 of any."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [(statistics.median(t), [round(x, 2) for x in t]) for t in ts]


def payload_1gib():
    n = 1 << 30
    parts, k = [], 0
    while n:
        m = min(n, synth.SILESIA_TOTAL)
        parts.append(synth.silesia_mix(0, m, copy=k))
        n -= m; k += 1
    return up(np.concatenate(parts))


def frame_starts(stream, frame_lens_known=None):
    """Start offsets of the frames of a stream (a CUDA tensor), walked on the host."""
    h = stream.cpu().numpy()
    starts, pos = [], 0
    while pos < len(h):
        starts.append(pos)
        flg = int(h[pos + 4])
        r = pos + 7 + (8 if flg & 0x08 else 0) + (4 if flg & 0x01 else 0)
        while True:
            bl = int.from_bytes(h[r:r + 4].tobytes(), "little"); r += 4
            if bl == 0:
                break
            r += (bl & 0x7FFFFFFF) + (4 if flg & 0x10 else 0)
        pos = r + (4 if flg & 0x04 else 0)
    return starts + [len(h)]


def case_a(args):
    plain = payload_1gib()
    g = framed.CompressionSettings()
    (one,) = g.compress_many_device([plain])
    out = torch.empty(plain.numel(), dtype=torch.uint8, device=DEV)
    res = {}
    fns = [lambda: res.__setitem__("one", device.frame_decompress_many([one], [out]))]
    streams = {}
    for fb in (4 * MiB, 32 * MiB):
        (streams[fb],) = g.compress_streams_device([plain], fb)
        fns.append(lambda fb=fb: res.__setitem__(fb, device.stream_decompress([streams[fb]], [out])))
    meds = timed_alternating(fns, args.runs)
    torch.cuda.synchronize()
    assert res["one"][0].tolist() == [0] and res["one"][1].tolist() == [plain.numel()]
    print(f"(a) one frame of 1 GiB, default settings, lzf_frame_decompress_device_many: median {meds[0][0]:.2f} ms, "
          f"{1.0 / (meds[0][0] / 1e3):.2f} GiB/s  runs {meds[0][1]}", flush=True)
    for (fb, s), m in zip(streams.items(), meds[1:]):
        out.zero_()
        st, ol, co, nf = device.stream_decompress([s], [out])
        torch.cuda.synchronize()
        assert (st.tolist(), ol.tolist(), co.tolist()) == ([0], [plain.numel()], [s.numel()]) and torch.equal(out, plain)
        print(f"(a) stream of {nf.tolist()[0]} frames of {fb // MiB} MiB, lzf_frame_decompress_stream_device: median {m[0]:.2f} ms, "
              f"{1.0 / (m[0] / 1e3):.2f} GiB/s, {meds[0][0] / m[0]:.1f} x the one frame  runs {m[1]}", flush=True)
    return streams[4 * MiB]


def case_b(args):
    n = synth.SILESIA_TOTAL
    g = framed.CompressionSettings().content_checksum(False)
    plains = [up(synth.silesia_mix(0, n, copy=k)) for k in range(args.distinct)]
    streams = g.compress_streams_device(plains, 4 * MiB)
    starts = [frame_starts(s) for s in streams]
    slots = [streams[s % args.distinct] for s in range(args.streams)]
    outs = [torch.empty(n, dtype=torch.uint8, device=DEV) for _ in range(args.streams)]
    f_in, f_out = [], []
    for s in range(args.streams):
        st = starts[s % args.distinct]
        for k in range(len(st) - 1):
            f_in.append(slots[s][st[k]:st[k + 1]]); f_out.append(outs[s][k * 4 * MiB:min((k + 1) * 4 * MiB, n)])
    res = {}
    (ms_s, runs_s), (ms_f, runs_f) = timed_alternating(
        [lambda: res.__setitem__("s", device.stream_decompress(slots, outs)),
         lambda: res.__setitem__("f", device.frame_decompress_many(f_in, f_out))], args.runs)
    (ms_scan, runs_scan), = timed_alternating([lambda: device.stream_decompress_bound(slots)], args.runs)
    torch.cuda.synchronize()
    assert res["s"][0].tolist() == [0] * args.streams and res["s"][1].tolist() == [n] * args.streams
    assert res["f"][0].tolist() == [0] * len(f_in)
    for s in range(min(args.streams, args.distinct)):
        assert torch.equal(outs[s], plains[s])
    total = args.streams * n
    print(f"(b) {args.streams} streams of {len(starts[0]) - 1} frames of 4 MiB, no content checksum: stream call median {ms_s:.2f} ms "
          f"({total / GiB / (ms_s / 1e3):.1f} GiB/s), per-frame call with host addresses {ms_f:.2f} ms ({total / GiB / (ms_f / 1e3):.1f} GiB/s), "
          f"ratio stream / per-frame time {ms_s / ms_f:.3f}", flush=True)
    print(f"    runs stream {runs_s}  per-frame {runs_f}", flush=True)
    print(f"(b) lzf_frame_stream_bound_device on the same streams (stream scan twice + per-frame summary, three waits): median {ms_scan:.2f} ms "
          f"= {100 * ms_scan / ms_s:.1f} % of the stream call  runs {runs_scan}", flush=True)


def case_c(args):
    one = framed.CompressionSettings().block_size(64 << 10).content_checksum(False).compress(synth.silesia_mix(0, 65536).tobytes())
    nf = (1 << 30) // len(one)
    d = up(np.frombuffer(one * nf, dtype=np.uint8))
    res = {}
    (ms, runs), (ms_f, runs_f) = timed_alternating([lambda: res.__setitem__("b", device.stream_decompress_bound([d])),
                                                    lambda: device.frame_decompress_bound([d[:len(one)]])], args.runs)
    assert res["b"][0] == nf * 65536
    print(f"(c) lzf_frame_stream_bound_device on one stream of {nf} single-block frames of 64 KiB ({d.numel() / GiB:.2f} GiB): median {ms:.2f} ms "
          f"= {ms * 1e3 / nf:.3f} us per frame for two stream walks and the per-frame scan  runs {runs}  (one such frame alone: {ms_f:.3f} ms)", flush=True)


def case_w(args):
    n = synth.SILESIA_TOTAL
    g = framed.CompressionSettings()
    s = g._struct(None)
    plains = [up(synth.silesia_mix(0, n, copy=k)) for k in range(args.distinct)]
    slots = [plains[k % args.distinct] for k in range(args.wstreams)]
    fb = 4 * MiB
    L = ffi.lib()
    outs = [torch.empty(L.lzf_frame_compress_stream_bound(C.byref(s), fb, n), dtype=torch.uint8, device=DEV) for _ in slots]
    pieces, pouts = [], []
    for k, p in enumerate(slots):
        for at in range(0, n, fb):
            x = p[at:at + fb]
            pieces.append(x); pouts.append(torch.empty(L.lzf_frame_compress_bound(C.byref(s), x.numel()), dtype=torch.uint8, device=DEV))
    res = {}
    (ms_s, runs_s), (ms_f, runs_f) = timed_alternating(
        [lambda: res.__setitem__("s", device.stream_compress(s, fb, slots, outs)),
         lambda: res.__setitem__("f", device.frame_compress_many(s, pieces, pouts))], args.runs)
    torch.cuda.synchronize()
    assert res["s"][0].tolist() == [0] * len(slots) and res["f"][0].tolist() == [0] * len(pieces)
    per = len(pieces) // len(slots)
    lens = res["f"][1].tolist()
    for k in range(min(len(slots), args.distinct)):
        cat = torch.cat([pouts[k * per + i][:lens[k * per + i]] for i in range(per)])
        assert torch.equal(outs[k][:res["s"][1].tolist()[k]], cat)
    total = len(slots) * n
    print(f"(w) {len(slots)} inputs of {n / MiB:.0f} MiB as streams of {per} frames of 4 MiB, default settings: stream call median {ms_s:.2f} ms "
          f"({total / GiB / (ms_s / 1e3):.1f} GiB/s), lzf_frame_compress_device_many over the {len(pieces)} pieces {ms_f:.2f} ms "
          f"({total / GiB / (ms_f / 1e3):.1f} GiB/s), ratio {ms_s / ms_f:.3f}, added {ms_s - ms_f:+.2f} ms", flush=True)
    print(f"    runs stream {runs_s}  per-frame {runs_f}", flush=True)


def case_t(args):
    if args.save:
        plain = payload_1gib()
        (s,) = framed.CompressionSettings().compress_streams_device([plain], 4 * MiB)
        np.save(args.save, s.cpu().numpy())
        print(f"(t) stream of {s.numel()} bytes written to {args.save}", flush=True)
        return
    s = up(np.load(args.load))
    out = torch.empty(1 << 30, dtype=torch.uint8, device=DEV)
    for _ in range(2):
        st, ol, co, nf = device.stream_decompress([s], [out])
        torch.cuda.synchronize()
    assert st.tolist() == [0] and ol.tolist() == [1 << 30]
    print(f"(t) decoded {nf.tolist()[0]} frames twice", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abcw")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--streams", type=int, default=240)
    ap.add_argument("--wstreams", type=int, default=48, help="case w: inputs per call")
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--save", default=None)
    ap.add_argument("--load", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    for c, fn in (("a", case_a), ("b", case_b), ("c", case_c), ("w", case_w), ("t", case_t)):
        if c in args.cases:
            fn(args)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
