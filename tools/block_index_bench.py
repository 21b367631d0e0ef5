"""Timing of the block index of a frame in device memory (lzf_frame_block_index_device) against the size query it extends
(lzf_frame_decompressed_size_device), and of the decode of runs of blocks (lzf_frame_decompress_blocks_device) against the decode
of the whole frame (lzf_frame_decompress_device_many).  Never writes the bench.py line.

One process, a warm-up of every call, then the calls alternate: run k of each before run k + 1 of any.  Wall time (perf_counter,
the device idle before and after); per call the median, the smallest and the largest of --runs runs, so that a difference
between two calls can be held against the spread of either.  The frame: 1 GiB (64 MiB of silesia_mix, tiled 16 times: blocks
are independent, so every block compresses as it would in an untiled payload) in independent 4 MiB blocks, 256 of them.
  a  no content checksum: count + index, index alone (the entries' room given), the size query
  b  the same frame: runs of 1, 16 and all 256 blocks into a tensor of the run's length, against the whole-frame decode into a
     tensor of the frame's length
  c  the frame written with a content checksum: the whole-frame decode (which verifies it: one serial XXH32 chain) against the
     whole-frame run and a run of 16 blocks (which do not)

  python tools/block_index_bench.py [--cases abc] [--runs 7]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import device, framed, synth  # noqa: E402

DEV = torch.device("cuda", 0)
MiB = 1 << 20


def wall_alternating(fns, runs):
    """Wall ms of every fn, the fns called in turn; the device is idle when a call starts and when its time is taken."""
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
    return ts


def line(label, t):
    print(f"    {label:<74} median {statistics.median(t):8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  runs {[round(x, 3) for x in t]}", flush=True)


def case_a(frame, runs):
    found = device.frame_block_count([frame])
    room = [torch.empty(found[0] * device.FBLOCK.itemsize, dtype=torch.uint8, device=DEV)]
    res = {}
    ts = wall_alternating([lambda: res.__setitem__("s", device.frame_decompressed_size([frame])),
                           lambda: res.__setitem__("i", device.frame_block_index_raw([frame], index=room)),
                           lambda: res.__setitem__("c", device.frame_block_index([frame]))], runs)
    assert [x.tolist() for x in res["s"]] == [x.tolist() for x in res["i"][:3]] and res["i"][3].tolist() == found
    print(f"(a) one frame of {found[0]} blocks, {frame.numel() / MiB:.1f} MiB compressed, {res['s'][1].item() / MiB:.0f} MiB decoded", flush=True)
    line("size query (lzf_frame_decompressed_size_device)", ts[0])
    line("index, room given (lzf_frame_block_index_device)", ts[1])
    line("count + index (lzf_frame_block_count_device, then the index)", ts[2])
    d = statistics.median(ts[1]) - statistics.median(ts[0])
    print(f"    index - size query = {d * 1e3:+.0f} us (medians); the size query's own spread: {(max(ts[0]) - min(ts[0])) * 1e3:.0f} us", flush=True)


def case_runs(label, frame, plain, runs, counts=(1, 16, 256)):
    (g,) = framed.block_index_device([frame])
    assert g.status == 0 and g.out_len == plain.numel()
    n = len(g.blocks)
    whole = torch.empty(plain.numel(), dtype=torch.uint8, device=DEV)
    fns, outs, spans, res = [], [], [], {}
    for c in counts:
        a = (n - c) // 2
        run = g.blocks[a:a + c]
        out = torch.empty(int(run["out_len"].sum()), dtype=torch.uint8, device=DEV)
        outs.append(out); spans.append((int(run[0]["out_off"]), out.numel()))
        fns.append(lambda run=run, out=out, c=c: res.__setitem__(c, device.frame_decompress_blocks([frame], [run], [out])))
    fns.append(lambda: res.__setitem__("w", device.frame_decompress_many([frame], [whole])))
    ts = wall_alternating(fns, runs)
    for c, out, (at, m) in zip(counts, outs, spans):
        assert res[c][0].item() == 0 and res[c][1].item() == m and torch.equal(out, plain[at:at + m])
    assert res["w"][0].item() == 0 and torch.equal(whole, plain)
    print(f"({label}) one frame of {n} blocks, {frame.numel() / MiB:.1f} MiB compressed", flush=True)
    for c, t, (at, m) in zip(counts, ts, spans):
        line(f"run of {c} block(s), {m / MiB:.0f} MiB (lzf_frame_decompress_blocks_device)", t)
    line("the whole frame (lzf_frame_decompress_device_many, out_cap = the frame's length)", ts[-1])
    print(f"    whole-frame run / whole-frame decode = {statistics.median(ts[len(counts) - 1]) / statistics.median(ts[-1]):.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    tile = torch.from_numpy(synth.silesia_mix(0, 64 * MiB).copy()).to(DEV)
    plain = tile.repeat(16)
    print(f"payload: {plain.numel() / MiB:.0f} MiB", flush=True)
    g = framed.CompressionSettings().content_checksum(False)
    if "a" in args.cases or "b" in args.cases:
        (frame,) = g.compress_many_device([plain])
        if "a" in args.cases:
            case_a(frame, args.runs)
        if "b" in args.cases:
            case_runs("b", frame, plain, args.runs)
        del frame
        torch.cuda.empty_cache()
    if "c" in args.cases:
        (frame,) = framed.CompressionSettings().compress_many_device([plain])
        case_runs("c: content checksum", frame, plain, args.runs, counts=(16, 256))


if __name__ == "__main__":
    main()
