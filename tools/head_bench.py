"""Timing of lzf_decompress_head_batch next to what a caller does without it: lzf_decompress_batch_sized of the whole blocks into
scratch, then lzf_copy_ranges of the heads.  Never writes the bench.py line.

Rows (silesia_mix, the bench's corpus, compressed by the CPU oracle), each at a sweep of targets:
  big980     980 raw 4 MiB blocks (49 distinct blocks, 20 copies)
  big49      the 49 blocks alone: a call that leaves the chip mostly empty
  small30000 30 000 blocks of 64 KiB (the same 196 MiB cut small, about ten copies), at 256 bytes

The inputs are made once; then one child process per run and side, in turns: `head` with this tree's library, `baseline` with the
library --parent-lib names (the parent commit's: what a caller has today; absent: this tree's).  A run is a warm-up call and the
median of --calls calls, wall clock around the call, which ends with the device synchronised.  Both sides write the heads into a
[n, target] tensor kept from call to call (the baseline's scratch for the whole blocks is kept too) and check it once against the
plain bytes.  The crossover of a row is the smallest target of the sweep at which the baseline is not slower.

  python tools/head_bench.py [--parent-lib PATH] [--runs 3] [--calls 5] [--rows big980,big49,small30000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BS, SMALL = 4 << 20, 64 << 10
N_DISTINCT = 49
SWEEP = (64, 4096, 16384, 65536, 262144, 393216, 524288, 786432, 1 << 20, 4 << 20)
ROWS = dict(big980=(980, BS, SWEEP), big49=(49, BS, SWEEP), small30000=(30000, SMALL, (256,)))


def make_inputs(path):
    import numpy as np
    import oracle_ffi as o
    import rust_lz_fear_amd  # noqa: F401
    from rust_lz_fear_amd import synth
    plain = synth.silesia_mix(0, N_DISTINCT * BS).tobytes()
    arrs = dict(plain=np.frombuffer(plain, np.uint8))
    for tag, bs in (("big", BS), ("small", SMALL)):
        comps = [o.compress2(plain[k:k + bs])[1] for k in range(0, len(plain), bs)]
        arrs[tag] = np.frombuffer(b"".join(comps), np.uint8)
        arrs[tag + "_len"] = np.array([len(c) for c in comps], dtype=np.int64)
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


def child(path, rows, calls, side):
    import numpy as np
    import torch
    import rust_lz_fear_amd  # noqa: F401
    from rust_lz_fear_amd import device
    torch.cuda.set_device(0)
    DEV = torch.device("cuda", 0)
    z = np.load(path)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    d_plain = dev(z["plain"])
    out = {}
    for row in rows:
        n, bs, targets = ROWS[row]
        tag = "big" if bs == BS else "small"
        d_comp, comp_len = dev(z[tag]), z[tag + "_len"]
        comp_off = np.concatenate([[0], np.cumsum(comp_len)[:-1]]).astype(np.uint64)
        distinct = len(comp_len)
        which = np.arange(n) % distinct
        bound = int(comp_len.max())
        d_res = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
        j = np.zeros(n, dtype=device.DJOB)
        j["input"] = np.uint64(d_comp.data_ptr()) + comp_off[which]
        j["input_len"] = comp_len[which]
        j["output_limit"] = bs
        whole = torch.empty((n, bs), dtype=torch.uint8, device=DEV) if side == "baseline" else None
        out[row] = {}
        for t in targets:
            heads = torch.zeros((n, t), dtype=torch.uint8, device=DEV)
            want = d_plain.view(distinct, bs)[torch.from_numpy(which).to(DEV), :t]
            arange = np.arange(n, dtype=np.uint64)
            if side == "head":
                j["out"] = np.uint64(heads.data_ptr()) + arange * np.uint64(t)
                j["out_cap"] = t
                d_j = device.to_device(j, DEV)
                run = lambda: device.decompress_head_batch(d_j, d_res, n)      # noqa: E731
            else:
                j["out"] = np.uint64(whole.data_ptr()) + arange * np.uint64(bs)
                j["out_cap"] = bs
                d_j = device.to_device(j, DEV)
                src = dev(j["out"].astype(np.int64))
                dst = dev((np.uint64(heads.data_ptr()) + arange * np.uint64(t)).astype(np.int64))
                lens = dev(np.full(n, t, dtype=np.int64))

                def run():
                    device.decompress_batch(d_j, d_res, n, max_input_len=bound)
                    device.copy_ranges(src, dst, lens, n, t)
            out[row][str(t)] = _timed(run, calls)
            res = device.results_to_host(d_res, n)
            assert (res["status"] == 0).all() and (res["out_len"] == (t if side == "head" else bs)).all(), (row, t)
            assert torch.equal(heads, want), (row, t, side)
            del heads, want
        del whole, d_comp
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblzfear_hip.so of the parent commit for the baseline (absent: this tree's library)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--out", default=None, help="append the table to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--side", default="head", help=argparse.SUPPRESS)
    args = ap.parse_args()
    rows = [r for r in args.rows.split(",") if r]
    assert all(r in ROWS for r in rows), rows
    if args.child:
        return child(args.child, rows, args.calls, args.side)
    from rust_lz_fear_amd import build
    sides = [("head", build.LIB_PATH), ("baseline", os.path.abspath(args.parent_lib) if args.parent_lib else build.LIB_PATH)]
    got = {name: [] for name, _ in sides}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "inputs.npz")
        make_inputs(path)
        for run in range(args.runs):
            for name, lib in sides:                              # in turns: a drift of the machine falls on both alike
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--side", name, "--rows", args.rows, "--calls", str(args.calls)],
                                   env=dict(os.environ, LZF_LIB_PATH=lib), capture_output=True, text=True, timeout=600)
                if r.returncode != 0:                            # (nothing more is started on the device after a child that failed)
                    sys.exit(f"{name} run {run}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-3000:]}")
                got[name].append(json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:]))
                print(f"run {run} {name} done", flush=True)
    lines = [f"ms per call, median of {args.calls} calls per run behind a warm-up, {args.runs} runs per side in turns, one child process per run; "
             f"baseline (decode whole + copy the heads) library: {'the parent commit' if args.parent_lib else 'this tree'}"]
    for row in rows:
        cross = None
        for t in ROWS[row][2]:
            med = {}
            for name in ("head", "baseline"):
                ms = [g[row][str(t)]["ms"] for g in got[name]]
                med[name] = statistics.median(ms)
                lines.append(f"{row:10s} target {t:8d} {name:8s} runs {' / '.join(f'{m:9.3f}' for m in ms)}   median {med[name]:9.3f}   spread {max(ms) - min(ms):7.3f}")
            lines.append(f"{row:10s} target {t:8d} baseline over head: {med['baseline'] / med['head']:.2f} x")
            if cross is None and med["baseline"] <= med["head"]:
                cross = t
        if len(ROWS[row][2]) > 1:
            lines.append(f"{row:10s} crossover: " + (f"decode-whole-then-slice is not slower from a target of {cross} bytes on" if cross else "none in the sweep: the head call is quicker at every target"))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
