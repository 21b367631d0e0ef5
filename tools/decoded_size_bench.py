"""Timing of the decoded-size query next to the decode it spares.  Never writes the bench.py line.

One process on one MI355X, HIP events around every call, the calls of a pair alternating.  Cases:
  1  lzf_decompressed_size_batch against lzf_decompress_batch over bench.py's blocks (--copies 240: 12 240 blocks of 4 MiB, the
     compressed ones), --pairs pairs after a warm-up of both; the size kernel's compressed GB/s against the 8 TB/s HBM figure
  2  the same pair over the first 20 / 4 / 1 copies (980 / 196 / 49 blocks: the README's small-call rows)
  3  --frames frames of ~10 KB of text with default settings (4 MiB blocks): lzf_frame_decompressed_size_device wall time, and
     the bytes decompress_frames_device allocates with exact=False (the bound; computed, not allocated) and exact=True
  4  the latency class against the parent commit's library: the size call and the decode call at --counts blocks of the bench's
     (49,196,980,2048,4096,11769), one "SWEEP" line per count with every call's time.  One process measures ONE library — the one
     LZF_LIB_PATH names, this tree's otherwise; `--ab PARENT_LIB --runs 5` starts such processes in turns, this tree's library and
     the parent's (built from a `git worktree` of the parent commit), and prints per count every run of both and whether every run of
     this tree's is shorter than every run of the parent's
  5  the class's smallest input: 256 blocks of 16, 64 and 256 KiB (text cut to size), the size call through the product's rule
     (the class from 64 KiB on) — `--ab` alternates it with the parent's library, which has the one-wave kernel alone, and
     `--class0 ANALYSIS_LIB` adds processes of the analysis library with LZF_SIZE_SEG_MIN_IN=0: the class at every size
  6  a call the class cannot help: 4 096 blocks of ~500 bytes, with no bound of the inputs (max_input_len unknown: the class's front
     runs over jobs that are all below its window, its scratch sized for 4 MiB blocks) and with the caller's bound (one-wave kernel alone)
Under `rocprofv3 --kernel-trace --stats -- python tools/decoded_size_bench.py --cases 1` the same process gives the size kernel's
time next to the decode's parse and seam kernels.

  python tools/decoded_size_bench.py [--cases 123] [--pairs 5] [--copies 240] [--distinct 12] [--frames 100000]
  python tools/decoded_size_bench.py --cases 45 --ab /path/to/parent/liblzfear_hip.so [--runs 5] [--counts 49,196,980,2048,4096,11769]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import device, ffi, framed, synth  # noqa: E402

import ctypes  # noqa: E402


class _OlderLibrary(ctypes.CDLL):
    """--ab loads the parent commit's library by LZF_LIB_PATH; it has no lzf_last_size_launch, which ffi.lib() declares."""

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name != "lzf_last_size_launch":
                raise

            def absent():
                return b"(a library without lzf_last_size_launch)"
            setattr(self, name, absent)
            return absent


def _load_library():
    loader, ctypes.CDLL = ctypes.CDLL, _OlderLibrary               # (only while ffi.lib() loads and declares the library)
    try:
        ffi.lib()
    finally:
        ctypes.CDLL = loader


_load_library()

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


def size_launch():
    return ffi.lib().lzf_last_size_launch().decode()


def sweep_case(B, counts, pairs):
    """One SWEEP line per count: every timed size and decode call of this process's library."""
    for n in counts:
        n = min(n, B["n"])
        d_rs = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
        d_rd = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)

        def size():
            device.decompressed_size_batch(B["jobs"], d_rs, n)

        def decode():
            device.decompress_batch(B["jobs"], d_rd, n)
        for _ in range(2):
            event_ms(size); event_ms(decode)
        ts, td = [], []
        for _ in range(pairs):
            ts.append(event_ms(size)); td.append(event_ms(decode))
        rs = device.results_to_host(d_rs, n)
        assert (rs["status"] == 0).all() and np.array_equal(rs["out_len"], B["lens"][:n])
        print("SWEEP " + json.dumps(dict(n=n, size_ms=[round(t, 3) for t in ts], decode_ms=[round(t, 3) for t in td], launch=size_launch())), flush=True)


def min_in_case(pairs):
    """256 blocks of 16 / 64 / 256 KiB: one MINSWEEP line each."""
    text = synth.gen_text_zipf(23, 256 * (256 << 10)).tobytes()
    for kib in (16, 64, 256):
        bs = kib << 10
        plains = [text[k * bs:(k + 1) * bs] for k in range(256)]
        comp = ffi.compress_blocks_host([dict(input=p, out_cap=len(p)) for p in plains])
        assert all(rc == 0 for rc, _ in comp)
        blobs = [c for _, c in comp]
        offs = np.cumsum([0] + [len(b) + 64 for b in blobs])
        h = np.zeros(int(offs[-1]), dtype=np.uint8)
        for b, a in zip(blobs, offs):
            h[a:a + len(b)] = np.frombuffer(b, dtype=np.uint8)
        d_in = torch.from_numpy(h).to(DEV)
        j = np.zeros(256, dtype=device.DJOB)
        j["input"] = np.uint64(d_in.data_ptr()) + offs[:-1].astype(np.uint64)
        j["input_len"] = [len(b) for b in blobs]
        j["output_limit"] = bs
        d_j = device.to_device(j, DEV)
        d_rs = torch.zeros(256 * 16, dtype=torch.uint8, device=DEV)
        bound = max(len(b) for b in blobs)

        def size():
            device.decompressed_size_batch(d_j, d_rs, 256, max_input_len=bound)
        for _ in range(2):
            event_ms(size)
        ts = [event_ms(size) for _ in range(pairs)]
        rs = device.results_to_host(d_rs, 256)
        assert (rs["status"] == 0).all() and (rs["out_len"] == bs).all()
        print("MINSWEEP " + json.dumps(dict(block_kib=kib, max_input=bound, min_input=min(len(b) for b in blobs), size_ms=[round(t, 3) for t in ts], launch=size_launch())), flush=True)


def tiny_case(pairs):
    """4 096 blocks of ~500 bytes: one TINY line for the call without a bound of its inputs, one for the call with it."""
    text = synth.gen_text_zipf(29, 4096 * 500).tobytes()
    comp = ffi.compress_blocks_host([dict(input=text[k * 500:(k + 1) * 500], out_cap=500) for k in range(4096)])
    blobs = [c if rc == 0 else b"\x00" for rc, c in comp]
    offs = np.cumsum([0] + [len(b) + 16 for b in blobs])
    h = np.zeros(int(offs[-1]), dtype=np.uint8)
    for b, a in zip(blobs, offs):
        h[a:a + len(b)] = np.frombuffer(b, dtype=np.uint8)
    d_in = torch.from_numpy(h).to(DEV)
    j = np.zeros(4096, dtype=device.DJOB)
    j["input"] = np.uint64(d_in.data_ptr()) + offs[:-1].astype(np.uint64)
    j["input_len"] = [len(b) for b in blobs]
    j["output_limit"] = 500
    d_j = device.to_device(j, DEV)
    d_rs = torch.zeros(4096 * 16, dtype=torch.uint8, device=DEV)
    for label, bound in (("unknown", None), ("bound", max(len(b) for b in blobs))):
        def size():
            device.decompressed_size_batch(d_j, d_rs, 4096, max_input_len=bound)
        first = event_ms(size)                                     # (the first call allocates the scratch from the device)
        event_ms(size)
        ts = [event_ms(size) for _ in range(pairs)]
        assert (device.results_to_host(d_rs, 4096)["status"] == 0).all()
        print("TINY " + json.dumps(dict(block_kib=label, first_ms=round(first, 3), size_ms=[round(t, 3) for t in ts], launch=size_launch())), flush=True)


def ab_driver(args):
    """Processes of this tree's library and the parent's in turns; every SWEEP / MINSWEEP line collected, the verdict per count."""
    mine = os.environ.get("LZF_LIB_PATH") or ffi.lib_path()
    rows = {}
    for run in range(args.runs):
        for who, lib, extra in [("new", mine, {}), ("parent", args.ab, {})] + ([("class0", args.class0, {"LZF_SIZE_SEG_MIN_IN": "0"})] if args.class0 else []):
            cmd = [sys.executable, os.path.abspath(__file__), "--cases", args.cases, "--pairs", str(args.pairs), "--copies", str(args.copies),
                   "--distinct", str(args.distinct), "--counts", args.counts]
            r = subprocess.run(cmd, env=dict(os.environ, LZF_LIB_PATH=lib, **extra), capture_output=True, text=True, timeout=args.run_timeout)
            if r.returncode != 0:
                print(r.stdout[-2000:] + r.stderr[-3000:])
                sys.exit(f"run {run} of {who} failed ({r.returncode}): nothing more is started")
            for ln in r.stdout.splitlines():
                if ln.startswith(("SWEEP ", "MINSWEEP ", "TINY ")):
                    kind, d = ln.split(" ", 1)
                    d = json.loads(d)
                    key = (kind, d.get("n", d.get("block_kib")))
                    rows.setdefault(key, {}).setdefault(who, []).append(d)
            print(f"run {run} {who}: done", flush=True)
    for (kind, k), by in sorted(rows.items(), key=lambda kv: (kv[0][0], str(kv[0][1]).zfill(8))):
        new = [t for d in by["new"] for t in d["size_ms"]]; par = [t for d in by["parent"] for t in d["size_ms"]]
        print(f"{kind} {k}: [{by['new'][0]['launch']}]")
        for who in by:
            print(f"    {who:6s} size ms per run: {[d['size_ms'] for d in by[who]]}" + (f"   first call of each process: {[d['first_ms'] for d in by[who]]}" if kind == "TINY" else ""))
        if "class0" in by:
            c0 = [t for d in by["class0"] for t in d["size_ms"]]
            print(f"    class0 (analysis library, LZF_SIZE_SEG_MIN_IN=0) [{by['class0'][0]['launch']}] median {statistics.median(c0):.3f}  every run shorter than every run of parent: {max(c0) < min(par)}")
        if kind == "SWEEP":
            print(f"    decode ms per run (new): {[d['decode_ms'] for d in by['new']]}")
            print(f"    decode ms per run (parent): {[d['decode_ms'] for d in by['parent']]}")
            dec = [t for d in by["new"] for t in d["decode_ms"]]
            print(f"    size (new) median {statistics.median(new):.3f}  decode median {statistics.median(dec):.3f}  every size call shorter than every decode call: {max(new) < min(dec)}")
        print(f"    new median {statistics.median(new):.3f}  parent median {statistics.median(par):.3f}  every run of new shorter than every run of parent: {max(new) < min(par)}", flush=True)


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
    ap.add_argument("--counts", default="49,196,980,2048,4096,11769")
    ap.add_argument("--ab", default=None, help="the parent commit's liblzfear_hip.so: alternate processes of the two libraries")
    ap.add_argument("--class0", default=None, help="the analysis library: with --ab, a third kind of process with LZF_SIZE_SEG_MIN_IN=0")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--run-timeout", type=int, default=600)
    args = ap.parse_args()
    if args.ab:
        return ab_driver(args)
    torch.cuda.set_device(0)
    ok = True
    if "5" in args.cases:
        min_in_case(args.pairs)
    if "6" in args.cases:
        tiny_case(args.pairs)
    if any(c in args.cases for c in "124"):
        B = bench_blocks(args.copies, args.distinct)
        if "4" in args.cases:
            sweep_case(B, [int(x) for x in args.counts.split(",")], args.pairs)
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
