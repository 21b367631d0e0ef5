"""Timing of lzf_frame_head_device next to what a caller does without it: lzf_frame_decompress_device_many of the whole frames into
scratch, then lzf_copy_ranges of the heads.  Never writes the bench.py line.

Rows (silesia_mix, the bench's corpus, framed by the CPU oracle with its default settings: a content checksum, no block checksums):
  f980        980 frames of one 4 MiB block (49 distinct frames, 20 copies), at a sweep of targets: 64 bytes, 4 KiB, and on to the
              crossover, the smallest target of the sweep at which decoding whole and slicing is not slower
  f49x20      49 frames of 20 x 4 MiB independent blocks (7 distinct frames, 7 copies), at 64 bytes
  linked16    one linked-block frame of 16 x 4 MiB, at 64 bytes and at 4 MiB + 64: the second reaches into the second block
  small30000  30 000 frames of one 64 KiB block (3 136 distinct frames), at 256 bytes

The inputs are made once; then one child process per run, row and side, each under its own time limit, in turns: `head` with this
tree's library, `baseline` with the library --parent-lib names (the parent commit's: what a caller has today; absent: this
tree's).  A run is a warm-up call and the median of --calls calls, wall clock around the call, which ends with the device
synchronised.  The frames alias their distinct copies; every frame has an output of its own on both sides (the baseline's
scratch for the whole frames is kept from call to call), and the heads are checked once against the plain bytes.

  python tools/frame_head_bench.py [--parent-lib PATH] [--runs 2] [--calls 5] [--rows f980,f49x20,linked16,small30000] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BS, SMALL = 4 << 20, 64 << 10
N_DISTINCT = 49
SWEEP = (64, 4096, 65536, 262144, 524288, 786432, 1 << 20, 2 << 20, 4 << 20)
# row -> (frames, distinct frames, plain bytes per frame, plain bytes between the starts of two distinct frames, targets)
ROWS = dict(f980=(980, 49, BS, BS, SWEEP), f49x20=(49, 7, 20 * BS, 4 * BS, (64,)), linked16=(1, 1, 16 * BS, 0, (64, BS + 64)),
            small30000=(30000, N_DISTINCT * BS // SMALL, SMALL, SMALL, (256,)))


def make_inputs(path):
    import numpy as np
    import xxhash
    import oracle_ffi as o
    import rust_lz_fear_amd  # noqa: F401
    from rust_lz_fear_amd import synth
    plain = synth.silesia_mix(0, N_DISTINCT * BS).tobytes()
    arrs = dict(plain=np.frombuffer(plain, np.uint8))

    def put(row, frames):
        arrs[row] = np.frombuffer(b"".join(frames), np.uint8)
        arrs[row + "_len"] = np.array([len(f) for f in frames], dtype=np.int64)

    def framed(data, bs, **kw):
        rc, f = o.frame_compress(data, o.make_settings(block_size=bs, **kw))
        assert rc == 0
        return f
    one = [framed(plain[k:k + BS], BS) for k in range(0, len(plain), BS)]
    put("f980", one)
    # 20 blocks a frame: header, the length words and payloads of 20 one-block frames, EndMark, content checksum
    many = []
    for d in range(7):
        body = b"".join(f[7:-8] for f in one[4 * d:4 * d + 20])
        many.append(one[0][:7] + body + b"\x00" * 4 + struct.pack("<I", xxhash.xxh32(plain[4 * d * BS:(4 * d + 20) * BS]).intdigest()))
    put("f49x20", many)
    put("linked16", [framed(plain[:16 * BS], BS, independent_blocks=False)])
    put("small30000", [framed(plain[k:k + SMALL], SMALL) for k in range(0, len(plain), SMALL)])
    np.savez(path, **arrs)


def _timed(fn, calls):
    import torch
    fn()                                               # warm-up
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=statistics.median(ts), calls=[round(t, 3) for t in ts])


def child(path, row, calls, side):
    import numpy as np
    import torch
    import rust_lz_fear_amd  # noqa: F401
    from rust_lz_fear_amd import device, ffi
    torch.cuda.set_device(0)
    DEV = torch.device("cuda", 0)
    lib = ffi.lib()
    z = np.load(path)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    n, distinct, size, stride, targets = ROWS[row]
    d_plain, d_frames, f_len = dev(z["plain"]), dev(z[row]), z[row + "_len"]
    assert len(f_len) == distinct
    f_off = np.concatenate([[0], np.cumsum(f_len)[:-1]]).astype(np.int64)
    which = np.arange(n) % distinct
    st = torch.cuda.current_stream().cuda_stream
    in_ptrs = (C.c_void_p * n)(*[d_frames.data_ptr() + int(f_off[k]) for k in which])
    in_lens = (C.c_size_t * n)(*[int(f_len[k]) for k in which])
    d_status = torch.zeros(n, dtype=torch.int32, device=DEV)
    d_len = torch.zeros(n, dtype=torch.int64, device=DEV)
    d_used = torch.zeros(n, dtype=torch.int64, device=DEV)
    whole = torch.empty((n, size), dtype=torch.uint8, device=DEV) if side == "baseline" else None
    out = {}
    for t in targets:
        heads = torch.zeros((n, t), dtype=torch.uint8, device=DEV)
        want = torch.stack([d_plain[int(k) * stride:int(k) * stride + t] for k in range(distinct)])[torch.from_numpy(which).to(DEV)]
        head_ptrs = [heads.data_ptr() + f * t for f in range(n)]
        if side == "head":
            outs, tgs = (C.c_void_p * n)(*head_ptrs), (C.c_size_t * n)(*[t] * n)
            run = lambda: ffi.check(lib.lzf_frame_head_device(n, in_ptrs, in_lens, None, 0, outs, tgs, d_len.data_ptr(), d_status.data_ptr(), st))      # noqa: E731
        else:
            whole_ptrs = [whole.data_ptr() + f * size for f in range(n)]
            outs, caps = (C.c_void_p * n)(*whole_ptrs), (C.c_size_t * n)(*[size] * n)
            src, dst = dev(np.array(whole_ptrs, dtype=np.int64)), dev(np.array(head_ptrs, dtype=np.int64))
            lens = dev(np.full(n, t, dtype=np.int64))

            def run():
                ffi.check(lib.lzf_frame_decompress_device_many(n, in_ptrs, in_lens, None, 0, outs, caps, d_len.data_ptr(), d_used.data_ptr(), d_status.data_ptr(), st))
                device.copy_ranges(src, dst, lens, n, t)
        out[str(t)] = _timed(run, calls)
        assert bool((d_status == 0).all()) and bool((d_len == (t if side == "head" else size)).all()), (row, t)
        assert torch.equal(heads, want), (row, t, side)
        del heads, want
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblzfear_hip.so of the parent commit for the baseline (absent: this tree's library)")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--out", default=None, help="append the table to this file")
    ap.add_argument("--limit", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--side", default="head", help=argparse.SUPPRESS)
    args = ap.parse_args()
    rows = [r for r in args.rows.split(",") if r]
    assert all(r in ROWS for r in rows), rows
    if args.child:
        return child(args.child, rows[0], args.calls, args.side)
    from rust_lz_fear_amd import build
    sides = [("head", build.LIB_PATH), ("baseline", os.path.abspath(args.parent_lib) if args.parent_lib else build.LIB_PATH)]
    got = {name: {row: [] for row in rows} for name, _ in sides}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "inputs.npz")
        make_inputs(path)
        print("inputs made", flush=True)
        for run in range(args.runs):
            for row in rows:
                for name, lib in sides:                          # in turns: a drift of the machine falls on both alike
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--side", name, "--rows", row, "--calls", str(args.calls)],
                                       env=dict(os.environ, LZF_LIB_PATH=lib), capture_output=True, text=True, timeout=args.limit)
                    if r.returncode != 0:                        # (nothing more is started on the device after a child that failed)
                        sys.exit(f"{row} {name} run {run}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-3000:]}")
                    got[name][row].append(json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:]))
                    print(f"run {run} {row} {name} done", flush=True)
    lines = [f"ms per call, median of {args.calls} calls per run behind a warm-up, {args.runs} runs per side in turns, one child process per run, row and side; "
             f"baseline (decode the frames whole + copy the heads) library: {'the parent commit' if args.parent_lib else 'this tree'}"]
    for row in rows:
        cross = None
        for t in ROWS[row][4]:
            med = {}
            for name in ("head", "baseline"):
                ms = [g[str(t)]["ms"] for g in got[name][row]]
                med[name] = statistics.median(ms)
                lines.append(f"{row:10s} target {t:8d} {name:8s} runs {' / '.join(f'{m:9.3f}' for m in ms)}   median {med[name]:9.3f}   spread {max(ms) - min(ms):7.3f}")
            verdict = "" if med["head"] < med["baseline"] else "   (the frame head call is NOT quicker here)"
            lines.append(f"{row:10s} target {t:8d} baseline over head: {med['baseline'] / med['head']:.2f} x{verdict}")
            if cross is None and med["baseline"] <= med["head"]:
                cross = t
        if len(ROWS[row][4]) > 2:
            lines.append(f"{row:10s} crossover: " + (f"decode-whole-then-slice is not slower from a target of {cross} bytes on" if cross else "none in the sweep: the frame head call is quicker at every target"))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
