"""Timing of the exact sizes and the frame index of streams in device memory (lzf_frame_stream_decompressed_size_device) against
the decode of the same streams (lzf_frame_decompress_stream_device), and of a range read.  Never writes the bench.py line.

One process, a warm-up of every call, then the calls alternate: run k of each before run k + 1 of any.  Wall time (perf_counter,
the device idle before and after), the median of --runs runs.  The streams are those of tools/stream_frames_bench.py.
  a  4 streams x 256 frames of 4 MiB (a 1 GiB payload, silesia_mix tiled, default settings; the 4 slots alias one stream unless
     --distinct says otherwise): count + size + index, size only, and the decode
  b  one stream of ~100 000 frames of ~10 KB content (one 1 GiB payload cut every 10 240 bytes): the same three calls
  r  a range read of 64 MiB out of the 1 GiB stream of (a): framed.read_stream_range_device against the whole decode, and the
     bytes it decoded

  python tools/stream_index_bench.py [--cases abr] [--runs 5] [--streams 4] [--distinct 1]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import device, framed  # noqa: E402
from stream_frames_bench import DEV, GiB, MiB, payload_1gib  # noqa: E402


def wall_alternating(fns, runs):
    """Median wall ms of every fn, the fns called in turn; the device is idle when a call starts and when its time is taken."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(t), [round(x, 2) for x in t]) for t in ts]


def three_calls(label, slots, plain_bytes, runs):
    outs = [torch.empty(plain_bytes, dtype=torch.uint8, device=DEV) for _ in slots]
    res = {}
    meds = wall_alternating([lambda: res.__setitem__("i", device.stream_index(slots)),
                             lambda: res.__setitem__("s", device.stream_decompressed_size(slots)),
                             lambda: res.__setitem__("d", device.stream_decompress(slots, outs))], runs)
    torch.cuda.synchronize()
    st, ol, co, nf, nl, entries = res["i"]
    dst, dol, dco, dnf = res["d"]
    assert st.tolist() == dst.tolist() == [0] * len(slots) and ol.tolist() == dol.tolist() == [plain_bytes] * len(slots)
    assert co.tolist() == dco.tolist() and nf.tolist() == dnf.tolist() == nl.tolist()
    assert [x.tolist() for x in res["s"][:4]] == [st.tolist(), ol.tolist(), co.tolist(), nf.tolist()]
    total = len(slots) * plain_bytes
    (mi, ri), (ms, rs), (md, rd) = meds
    print(f"({label}) {len(slots)} stream(s) of {nf.tolist()[0]} frames, {total / GiB:.2f} GiB decoded, {sum(s.numel() for s in slots) / GiB:.2f} GiB compressed", flush=True)
    print(f"    count + size + index (lzf_frame_stream_count_device, lzf_frame_stream_decompressed_size_device): median {mi:.2f} ms  runs {ri}", flush=True)
    print(f"    size only (no index, no count):                                                              median {ms:.2f} ms  runs {rs}", flush=True)
    print(f"    decode (lzf_frame_decompress_stream_device):                                                  median {md:.2f} ms  runs {rd}", flush=True)
    print(f"    size + index / decode = {mi / md:.3f}, size only / decode = {ms / md:.3f}", flush=True)


def case_a(args, plain):
    g = framed.CompressionSettings()
    streams = g.compress_streams_device([plain] + [plain.roll(k * 4097) for k in range(1, args.distinct)], 4 * MiB)
    three_calls("a", [streams[k % len(streams)] for k in range(args.streams)], plain.numel(), args.runs)
    return streams[0]


def case_b(args, plain):
    (s,) = framed.CompressionSettings().block_size(64 << 10).compress_streams_device([plain], 10240)
    three_calls("b", [s], plain.numel(), args.runs)


def case_r(args, plain, s):
    (index,) = framed.stream_index_device([s])
    assert index.status == 0 and index.out_len == plain.numel()
    a = 3 * (1 << 28) + 12345                         # 768 MiB and a bit: inside a frame at both ends
    b = a + 64 * MiB
    res, seen = {}, []
    real = device.stream_decompress
    device.stream_decompress = lambda streams, *x, **kw: (seen.append(sum(t.numel() for t in streams)), real(streams, *x, **kw))[1]
    try:
        (mr, rr), (mw, rw) = wall_alternating([lambda: res.__setitem__("r", framed.read_stream_range_device(s, index, a, b)),
                                               lambda: res.__setitem__("w", framed.decompress_streams_device([s], caps=[plain.numel()]))], args.runs)
    finally:
        device.stream_decompress = real
    assert torch.equal(res["r"], plain[a:b]) and torch.equal(res["w"][0][1], plain)
    first, count = framed.locate_frames(index, a, b)
    decoded = int(index.frames["out_len"][first:first + count].sum())
    print(f"(r) bytes [{a}, {b}) = 64 MiB of a 1 GiB stream of {len(index.frames)} frames of 4 MiB: read_stream_range_device median {mr:.2f} ms  runs {rr}", flush=True)
    print(f"    it decoded frames [{first}, {first + count}): {decoded} bytes ({decoded / MiB:.0f} MiB) from {min(seen)} compressed bytes of {s.numel()}", flush=True)
    print(f"    the whole stream with decompress_streams_device (caps given: no bound call): median {mw:.2f} ms  runs {rw};  range / whole = {mr / mw:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abr")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--distinct", type=int, default=1)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    plain = payload_1gib()
    s = case_a(args, plain) if "a" in args.cases else None
    torch.cuda.empty_cache()
    if "b" in args.cases:
        case_b(args, plain)
        torch.cuda.empty_cache()
    if "r" in args.cases:
        if s is None:
            (s,) = framed.CompressionSettings().compress_streams_device([plain], 4 * MiB)
        case_r(args, plain, s)


if __name__ == "__main__":
    main()
