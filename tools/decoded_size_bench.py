"""Timing of the decoded-size query next to the decode it spares.  Never writes the bench.py line.

One process on one MI355X, HIP events around every call, the calls of a pair alternating.  Cases:
  1  lzf_decompressed_size_batch against lzf_decompress_batch over bench.py's blocks (--copies 240: 12 240 blocks of 4 MiB, the
     compressed ones), --pairs pairs after a warm-up of both; the size kernel's compressed GB/s against the 8 TB/s HBM figure
  2  the same pair over the first 20 / 4 / 1 copies (980 / 196 / 49 blocks: the README's small-call rows)
  3  --frames frames of ~10 KB of text with default settings (4 MiB blocks): lzf_frame_decompressed_size_device wall time, and
     the bytes decompress_frames_device allocates with exact=False (the bound; computed, not allocated) and exact=True
Under `rocprofv3 --kernel-trace --stats -- python tools/decoded_size_bench.py --cases 1` the same process gives the size kernel's
time next to the decode's parse and seam kernels.

  python tools/decoded_size_bench.py [--cases 123] [--pairs 5] [--copies 240] [--distinct 12] [--frames 100000]
"""
import argparse
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
BS = 4 << 20
HBM_GBS = 8000.0


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench_blocks(copies, distinct):
    """bench.py's source (silesia_mix copies, rotated and XOR-ed beyond the distinct ones) compressed on the device: the job
    array of the compressed blocks, as bench.py builds it."""
    import bench
    bases = bench.make_distinct_copies(max(1, min(distinct, copies)))
    total = bases[0].size
    nb1 = (total + BS - 1) // BS
    nblk = nb1 * copies
    d_bases = [torch.from_numpy(b).to(DEV) for b in bases]
    nd = len(d_bases)
    src = torch.zeros(nblk * BS, dtype=torch.uint8, device=DEV)
    lens = np.full(nblk, BS, dtype=np.uint64)
    for k in range(copies):
        b = d_bases[k % nd]
        gen = k // nd
        dst = src[k * nb1 * BS:k * nb1 * BS + total]
        if gen == 0:
            dst.copy_(b)
        else:
            shift = (gen * 1000003 + (k % nd) * 65537) % total
            c = (gen * 37 + (gen >> 3) + 1) & 0xFF
            torch.bitwise_xor(torch.roll(b, shift), c, out=dst)
        lens[k * nb1 + nb1 - 1] = total - (nb1 - 1) * BS
    del d_bases
    comp = torch.empty(nblk * BS, dtype=torch.uint8, device=DEV)
    cj = np.zeros(nblk, dtype=device.CJOB)
    cj["input"] = np.uint64(src.data_ptr()) + np.arange(nblk, dtype=np.uint64) * np.uint64(BS)
    cj["input_len"] = lens
    cj["out"] = np.uint64(comp.data_ptr()) + np.arange(nblk, dtype=np.uint64) * np.uint64(BS)
    cj["out_cap"] = lens
    cj["table_kind"] = ffi.TABLE_U32
    d_cres = torch.zeros(nblk * 16, dtype=torch.uint8, device=DEV)
    device.compress_batch(device.to_device(cj, DEV), d_cres, nblk, ffi.KINDS_U32 | ffi.KINDS_U32_FRESH_ONLY)
    torch.cuda.synchronize()
    del src
    torch.cuda.empty_cache()
    cres = device.results_to_host(d_cres, nblk)
    ok = cres["status"] == ffi.OK
    kidx = np.nonzero(ok)[0]
    clen = cres["out_len"].astype(np.uint64)
    dec = torch.empty(nblk * BS, dtype=torch.uint8, device=DEV)
    dj = np.zeros(len(kidx), dtype=device.DJOB)
    dj["input"] = np.uint64(comp.data_ptr()) + kidx.astype(np.uint64) * np.uint64(BS)
    dj["input_len"] = clen[kidx]
    dj["out"] = np.uint64(dec.data_ptr()) + kidx.astype(np.uint64) * np.uint64(BS)
    dj["out_cap"] = lens[kidx]
    dj["output_limit"] = BS
    return dict(jobs=device.to_device(dj, DEV), n=len(kidx), lens=lens[kidx], clen=clen[kidx], per_copy=max(1, len(kidx) // copies),
                nblk=nblk, keep=(comp, dec))


def pair_case(B, n, pairs, label):
    d_rs = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    d_rd = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)

    def size():
        device.decompressed_size_batch(B["jobs"], d_rs, n)

    def decode():
        device.decompress_batch(B["jobs"], d_rd, n)
    for _ in range(2):                                         # warm-up of both
        event_ms(size); event_ms(decode)
    ts, td = [], []
    for _ in range(pairs):
        ts.append(event_ms(size)); td.append(event_ms(decode))
    rs, rd = device.results_to_host(d_rs, n), device.results_to_host(d_rd, n)
    assert (rs["status"] == 0).all() and (rd["status"] == 0).all()
    assert np.array_equal(rs["out_len"], B["lens"][:n]) and np.array_equal(rd["out_len"], B["lens"][:n])
    cbytes, ubytes = float(B["clen"][:n].sum()), float(B["lens"][:n].sum())
    ms, md = statistics.median(ts), statistics.median(td)
    print(f"({label}) {n} blocks, {cbytes / 1e9:.3f} GB compressed, {ubytes / 2**30:.2f} GiB decoded  [{ffi.lib().lzf_last_decompress_launch().decode()}]")
    print(f"    size   ms {[round(t, 3) for t in ts]}  median {ms:.3f}")
    print(f"    decode ms {[round(t, 3) for t in td]}  median {md:.3f}")
    print(f"    every size run shorter than every decode run: {max(ts) < min(td)}   median ratio size / decode {ms / md:.3f}")
    print(f"    size kernel: {cbytes / 1e9 / (ms / 1e3):.1f} GB/s of compressed input = {cbytes / 1e9 / (ms / 1e3) / HBM_GBS:.4f} of {HBM_GBS:.0f} GB/s HBM"
          f"   (decode: {ubytes / 2**30 / (md / 1e3):.1f} GiB/s of output)", flush=True)
    kc = rs["reserved"].astype(np.float64)
    print(f"    size jobs, kilo-cycles per job: mean {kc.mean():.0f}  max {kc.max():.0f}", flush=True)
    return max(ts) < min(td)


def frames_case(n_frames):
    text = synth.gen_text_zipf(11, 64 << 20).tobytes()
    distinct = 4000                                            # distinct shards; the frame slots alias them
    plains = [text[k * 16_001: k * 16_001 + 9_000 + (k * 37) % 2_000] for k in range(distinct)]
    shards = framed.CompressionSettings().compress_many(plains)
    d_sh = [torch.frombuffer(bytearray(f), dtype=torch.uint8).to(DEV) for f in shards]
    slots = [d_sh[s % distinct] for s in range(n_frames)]
    torch.cuda.synchronize()
    walls = []
    for _ in range(4):
        t0 = time.perf_counter()
        st, ol, co = device.frame_decompressed_size(slots)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    assert (st == 0).all().item() and ol.tolist() == [len(plains[s % distinct]) for s in range(n_frames)]
    bound = 0
    for a in range(0, n_frames, 20000):
        bound += sum(device.frame_decompress_bound(slots[a:a + 20000]))
    t0 = time.perf_counter()
    res = framed.decompress_frames_device(slots, exact=True)
    wall_exact = (time.perf_counter() - t0) * 1e3
    exact = sum(t.untyped_storage().nbytes() for _, t, _ in res)
    assert all(s == 0 for s, _, _ in res)
    print(f"(3) {n_frames} frames of ~10 KB ({sum(map(len, shards)) / distinct:.0f} B compressed on average, 4 MiB blocks)")
    print(f"    lzf_frame_decompressed_size_device wall ms {[round(w, 1) for w in walls]} (first call: warm-up)  median of the rest {statistics.median(walls[1:]):.1f}")
    print(f"    output bytes allocated: exact=False (lzf_frame_decompress_bound_device, summed, not allocated here) {bound}  = {bound / 2**30:.1f} GiB")
    print(f"                            exact=True  {exact}  = {exact / 2**30:.3f} GiB   ({bound / exact:.0f} x less)")
    print(f"    decompress_frames_device(exact=True) wall {wall_exact:.1f} ms (size query + decode + host lists)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="123")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--copies", type=int, default=240)
    ap.add_argument("--distinct", type=int, default=12)
    ap.add_argument("--frames", type=int, default=100000)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ok = True
    if "1" in args.cases or "2" in args.cases:
        B = bench_blocks(args.copies, args.distinct)
        if "1" in args.cases:
            ok = pair_case(B, B["n"], args.pairs, "1") and ok
        if "2" in args.cases:
            for c_n in (20, 4, 1):
                m = min(B["n"], B["per_copy"] * c_n)
                if m < B["n"]:
                    pair_case(B, m, args.pairs, f"2: first {c_n} copies")
        del B
        torch.cuda.empty_cache()
    if "3" in args.cases:
        frames_case(args.frames)
    if not ok:
        print("FAILED: a size run was not shorter than every decode run")
        sys.exit(1)


if __name__ == "__main__":
    main()
