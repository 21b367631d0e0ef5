"""Timing of the verify calls next to what a caller does without them: decode into fresh output, then torch.equal.  Never writes
the bench.py line.

Rows (4 MiB blocks of silesia_mix, compressed by the CPU oracle):
  raw980     980 raw jobs (49 distinct blocks, 20 copies): lzf_decompress_verify_batch against lzf_decompress_batch + torch.equal
  raw49      the 49 blocks alone: a call that leaves the chip mostly empty
             both through the product (the latency class in front) and, as `one-wave only`, through the analysis library with
             LZF_VERIFY_SEG=off
  linked1 / linked16   tools/seg_history_bench.py's frames — 1 and 16 linked-block frames of sixteen blocks, content checksum off —
             lzf_frame_verify_device against framed.decompress_frames_device + torch.equal
  indep64    one independent-blocks frame of 64 blocks WITH a content checksum (the verify call hashes the expected bytes)

The inputs are made once; then one child process per run and side, in turns: `verify` with this tree's library, `baseline` with the
library --parent-lib names (the parent commit's: what a caller has today; absent: this tree's).  A run is a warm-up call and the
median of --calls calls, wall clock around the call, which ends with the device synchronised.  The baseline is timed twice: with its
output allocated inside the window (torch.empty behind torch.cuda.empty_cache(): a fresh allocation from the device) and into
outputs kept from call to call.  Every child checks its answers once: all LZF_OK with the right lengths / all outputs equal.

  python tools/verify_bench.py [--parent-lib PATH] [--runs 3] [--calls 5] [--rows raw980,raw49,linked1,linked16,indep64] [--out FILE]
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

BS = 4 << 20
ROWS = ("raw980", "raw49", "linked1", "linked16", "indep64")
N_DISTINCT = 49


def make_inputs(path):
    import numpy as np
    import oracle_ffi as o
    import rust_lz_fear_amd  # noqa: F401
    from rust_lz_fear_amd import synth
    plain = synth.silesia_mix(0, N_DISTINCT * BS).tobytes()
    comps = [o.compress2(plain[k * BS:(k + 1) * BS])[1] for k in range(N_DISTINCT)]
    arrs = dict(plain=np.frombuffer(plain, np.uint8), comp=np.frombuffer(b"".join(comps), np.uint8),
                comp_len=np.array([len(c) for c in comps], dtype=np.int64))
    for k in range(2):
        p = plain[k * 16 * BS:(k + 1) * 16 * BS]
        arrs[f"linked{k}"] = np.frombuffer(o.frame_compress(p, o.make_settings(block_size=BS, independent_blocks=False, content_checksum=False))[1], np.uint8)
    big = plain + plain[:15 * BS]
    arrs["indep"] = np.frombuffer(o.frame_compress(big, o.make_settings(block_size=BS, content_checksum=True))[1], np.uint8)
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
    from rust_lz_fear_amd import device, ffi, framed
    torch.cuda.set_device(0)
    DEV = torch.device("cuda", 0)
    z = np.load(path)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    d_plain, d_comp = dev(z["plain"]), dev(z["comp"])
    comp_len = z["comp_len"]
    comp_off = np.concatenate([[0], np.cumsum(comp_len)[:-1]]).astype(np.uint64)
    out = {}
    for row in rows:
        if row.startswith("raw"):
            n = int(row[3:])
            which = np.arange(n) % N_DISTINCT
            j = np.zeros(n, dtype=device.DJOB)
            j["input"] = np.uint64(d_comp.data_ptr()) + comp_off[which]
            j["input_len"] = comp_len[which]
            j["out_cap"] = BS
            j["output_limit"] = BS
            d_res = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
            bound = int(comp_len.max())
            if side != "baseline":
                j["out"] = np.uint64(d_plain.data_ptr()) + which.astype(np.uint64) * np.uint64(BS)
                d_j = device.to_device(j, DEV)
                run = lambda: device.decompress_verify_batch(d_j, d_res, n, max_input_len=bound)      # noqa: E731
                out[row] = dict(verify=_timed(run, calls), launch=device.last_verify_launch())
                res = device.results_to_host(d_res, n)
                assert (res["status"] == 0).all() and (res["out_len"] == BS).all(), row
            else:
                want = d_plain.view(N_DISTINCT, BS)[torch.from_numpy(which).to(DEV)] if n != N_DISTINCT else d_plain.view(N_DISTINCT, BS)
                keep = {}

                def decode(fresh):
                    if fresh:
                        keep.clear()
                        torch.cuda.empty_cache()
                    if "o" not in keep:
                        keep["o"] = torch.empty((n, BS), dtype=torch.uint8, device=DEV)
                        j["out"] = np.uint64(keep["o"].data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(BS)
                        keep["j"] = device.to_device(j, DEV)
                    device.decompress_batch(keep["j"], d_res, n, max_input_len=bound)
                    keep["ok"] = torch.equal(keep["o"], want)
                r_alloc = _timed(lambda: decode(True), calls)
                assert keep["ok"]
                r_kept = _timed(lambda: decode(False), calls)
                assert keep["ok"]
                out[row] = dict(decode_alloc=r_alloc, decode_kept=r_kept, launch=ffi.lib().lzf_last_decompress_launch().decode())
                keep.clear(); del want
        elif side == "onewave":
            continue
        else:
            if row == "indep64":
                frames, want = [dev(z["indep"])], [torch.cat([d_plain, d_plain[:15 * BS]])]
            else:
                n = int(row[6:])
                fr = [dev(z["linked0"]), dev(z["linked1"])]
                frames, want = [fr[s % 2] for s in range(n)], [d_plain[(s % 2) * 16 * BS:(s % 2 + 1) * 16 * BS] for s in range(n)]
            caps = [int(w.numel()) for w in want]
            if side == "verify":
                got = {}

                def run():
                    got["r"] = framed.verify_frames_device(frames, want)
                out[row] = dict(verify=_timed(run, calls), launch=device.last_verify_launch())
                assert got["r"] == [(0, c) for c in caps], (row, got["r"][:3])
            else:
                got = {}

                def decode(fresh):
                    if fresh:
                        got.clear()
                        torch.cuda.empty_cache()
                    res = framed.decompress_frames_device(frames, caps=caps)
                    got["ok"] = all(st == 0 and torch.equal(t, w) for (st, t, _), w in zip(res, want))
                r_alloc = _timed(lambda: decode(True), calls)
                assert got["ok"]
                out[row] = dict(decode_alloc=r_alloc, launch=ffi.lib().lzf_last_decompress_launch().decode())
            del frames, want
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
    ap.add_argument("--side", default="verify", help=argparse.SUPPRESS)
    args = ap.parse_args()
    rows = [r for r in args.rows.split(",") if r]
    assert all(r in ROWS for r in rows), rows
    if args.child:
        return child(args.child, rows, args.calls, args.side)
    from rust_lz_fear_amd import build
    # onewave: the analysis library with the latency class switched off — the one-wave kernel alone, on the raw rows
    sides = [("verify", build.LIB_PATH), ("onewave", build.build_analysis_library()),
             ("baseline", os.path.abspath(args.parent_lib) if args.parent_lib else build.LIB_PATH)]
    got = {name: [] for name, _ in sides}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "inputs.npz")
        make_inputs(path)
        for run in range(args.runs):
            for name, lib in sides:                              # in turns: a drift of the machine falls on both alike
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--side", name, "--rows", args.rows, "--calls", str(args.calls)],
                                   env=dict(os.environ, LZF_LIB_PATH=lib, **({"LZF_VERIFY_SEG": "off"} if name == "onewave" else {})), capture_output=True, text=True, timeout=900)
                if r.returncode != 0:                            # (nothing more is started on the device after a child that failed)
                    sys.exit(f"{name} run {run}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-3000:]}")
                got[name].append(json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:]))
                print(f"run {run} {name} done", flush=True)
    lines = [f"ms per call, median of {args.calls} calls per run behind a warm-up, {args.runs} runs per side in turns, one child process per run; "
             f"baseline library: {'the parent commit' if args.parent_lib else 'this tree'}"]
    for row in rows:
        med = {}
        for name, key, label in (("verify", "verify", "verify"), ("onewave", "verify", "one-wave only"), ("baseline", "decode_alloc", "decode_alloc"), ("baseline", "decode_kept", "decode_kept")):
            if row not in got[name][0] or key not in got[name][0][row]:
                continue
            ms = [g[row][key]["ms"] for g in got[name]]
            med[label] = statistics.median(ms)
            key = label
            lines.append(f"{row:9s} {key:13s} runs {' / '.join(f'{m:9.3f}' for m in ms)}   median {med[key]:9.3f}   spread {max(ms) - min(ms):7.3f}   [{got[name][0][row]['launch']}]")
        lines.append(f"{row:9s} decode + equal over verify: fresh output {med['decode_alloc'] / med['verify']:.2f} x" +
                     (f", kept output {med['decode_kept'] / med['verify']:.2f} x" if "decode_kept" in med else ""))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
