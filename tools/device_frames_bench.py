"""Timing of lzf_frame_decompress_device_many (frames in HBM in, decoded bytes in HBM out).  Never writes the bench.py line.

One process, a warm-up, HIP events around the call, the median of --runs runs.  Cases:
  a  240 frames x 51 blocks of 4 MiB, content_checksum(false), next to lzf_decompress_batch on the same blocks
  b  the same frames with default settings (content checksums)
  c  one 1 GiB frame of 64 KiB blocks: the scan alone (lzf_frame_decompress_bound_device)
Frames are aliased: --distinct distinct frames serve the 240 slots (the plaintext would not fit a test box's host otherwise).

  python tools/device_frames_bench.py [--cases abc] [--runs 5] [--frames 240] [--blocks 51] [--distinct 2]
"""
import argparse
import os
import statistics
import struct
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


def frames_case(args, content_checksum):
    bs = 4 << 20
    n = min(args.blocks * bs, synth.SILESIA_TOTAL)      # bench.py's unit: one silesia_mix copy, 51 blocks of 4 MiB (the last one short)
    plains = [synth.silesia_mix(0, n, copy=k).tobytes() for k in range(args.distinct)]
    g = framed.CompressionSettings().content_checksum(content_checksum)
    frames = g.compress_many(plains)
    d_frames = [torch.frombuffer(bytearray(f), dtype=torch.uint8).to(DEV) for f in frames]
    slots = [d_frames[s % args.distinct] for s in range(args.frames)]
    outs = [torch.empty(len(plains[s % args.distinct]), dtype=torch.uint8, device=DEV) for s in range(args.frames)]
    total = sum(o.numel() for o in outs)
    res = {}

    def call():
        res["r"] = device.frame_decompress_many(slots, outs)
    med, ts = timed(call, args.runs)
    st, ol, _ = res["r"]
    torch.cuda.synchronize()
    assert st.tolist() == [0] * args.frames and ol.tolist() == [o.numel() for o in outs]
    for s in range(min(args.frames, args.distinct)):
        assert torch.equal(outs[s], torch.frombuffer(bytearray(plains[s]), dtype=torch.uint8).to(DEV))
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    out = dict(ms=med, runs=ts, gib_s=total / GiB / (med / 1e3), blocks=args.frames * args.blocks, bytes=total, launch=launch)
    return out, frames, slots


def raw_case(args, frames):
    """The same blocks through lzf_decompress_batch: one job per block of every slot, outputs of 4 MiB + input each."""
    blocks = []
    for f in frames:                                  # walk the frame (independent, no block checksums)
        flg = f[4]
        r = 7 + (8 if flg & 0x08 else 0) + (4 if flg & 0x01 else 0)
        while True:
            bl = struct.unpack_from("<I", f, r)[0]; r += 4
            if bl == 0:
                break
            if not bl & 0x80000000:                   # (stored blocks are a copy, not a decode: left out here)
                blocks.append(f[r:r + bl])
            r += bl & 0x7FFFFFFF
    per = len(blocks) // len(frames)              # (the frames are copies of the same stream: the same block count each)
    d_blocks = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(DEV) for b in blocks]
    n = args.frames * per
    bs = 4 << 20
    jobs = np.zeros(n, dtype=device.DJOB)
    slot = bs + max(len(b) for b in blocks) + 256
    out = torch.empty(n * slot, dtype=torch.uint8, device=DEV)
    for j in range(n):
        b = d_blocks[(j // per) % len(frames) * per + j % per]
        jobs[j]["input"] = b.data_ptr(); jobs[j]["input_len"] = b.numel()
        jobs[j]["out"] = out.data_ptr() + j * slot; jobs[j]["out_cap"] = slot; jobs[j]["output_limit"] = bs
    d_jobs = device.to_device(jobs, DEV)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    max_in = max(len(b) for b in blocks)
    med, ts = timed(lambda: device.decompress_batch(d_jobs, d_res, n, max_input_len=max_in), args.runs)
    r = device.results_to_host(d_res, n)
    assert (r["status"] == 0).all()
    return dict(ms=med, runs=ts, gib_s=float(r["out_len"].sum()) / GiB / (med / 1e3), blocks=n, launch=ffi.lib().lzf_last_decompress_launch().decode())


def scan_case(args):
    """One 1 GiB frame of 64 KiB blocks (one compressed block repeated): lzf_frame_decompress_bound_device."""
    one = framed.CompressionSettings().block_size(64 << 10).content_checksum(False).compress(synth.silesia_mix(0, 65536).tobytes())
    blk = one[7:-4]                                   # length word + payload of the single block
    nb = (1 << 30) // 65536
    frame = one[:7] + blk * nb + bytes(4)
    d = torch.frombuffer(bytearray(frame), dtype=torch.uint8).to(DEV)
    res = {}
    med, ts = timed(lambda: res.__setitem__("b", device.frame_decompress_bound([d])), args.runs)
    assert res["b"][0] == nb * 65536
    return dict(ms=med, runs=ts, blocks=nb, us_per_block=med * 1e3 / nb, frame_bytes=len(frame))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--blocks", type=int, default=51)
    ap.add_argument("--distinct", type=int, default=2)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if "a" in args.cases:
        a, frames, _ = frames_case(args, False)
        print(f"(a) device frames, no content checksum: {a['blocks']} blocks, median {a['ms']:.2f} ms, {a['gib_s']:.1f} GiB/s  [{a['launch']}]  runs {[round(t, 2) for t in a['runs']]}", flush=True)
        torch.cuda.empty_cache()
        raw = raw_case(args, frames)
        print(f"(a) raw lzf_decompress_batch, same blocks: {raw['blocks']} blocks, median {raw['ms']:.2f} ms, {raw['gib_s']:.1f} GiB/s  [{raw['launch']}]  runs {[round(t, 2) for t in raw['runs']]}", flush=True)
        print(f"(a) ratio device frames / raw: {a['gib_s'] / raw['gib_s']:.3f}", flush=True)
        del frames
        torch.cuda.empty_cache()
    if "b" in args.cases:
        b, _, _ = frames_case(args, True)
        print(f"(b) device frames, default settings (content checksums): median {b['ms']:.2f} ms, {b['gib_s']:.1f} GiB/s  runs {[round(t, 2) for t in b['runs']]}", flush=True)
        torch.cuda.empty_cache()
    if "c" in args.cases:
        c = scan_case(args)
        print(f"(c) scan of one 1 GiB frame of {c['blocks']} blocks of 64 KiB: median {c['ms']:.2f} ms ({c['us_per_block']:.3f} us per block)  runs {[round(t, 2) for t in c['runs']]}", flush=True)


if __name__ == "__main__":
    main()
