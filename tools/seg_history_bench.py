"""Timing of framed.decompress_frames_device on frames whose blocks have HISTORY: linked-block frames (every block continues the stream so
far: lock-step launches of block k of every stream, each job with existing output) and an independent-blocks frame behind a dictionary
(every job with a prefix).  Never writes the bench.py line.

Inputs (4 MiB blocks of silesia_mix, content checksum off so that its serial chain is not what is measured):
  linked1 / linked16 / linked256   1, 16 and 256 linked-block frames of sixteen blocks each (--distinct distinct frames serve the slots)
  dict64                           one independent-blocks frame of 64 blocks behind a 64 KiB dictionary

The frames are made once; then one child process per run and library, the libraries in turns (LZF_LIB_PATH: this tree's library and, with
--parent-lib, the parent commit's), --runs runs each.  A run is a warm-up call and the median of --calls calls, wall clock around the call
(it ends with the stream synchronised); the output is compared with the plaintext once per run.

  python tools/seg_history_bench.py [--parent-lib PATH] [--runs 3] [--calls 5] [--rows linked1,linked16,linked256,dict64] [--out FILE] [--inputs FILE.npz]
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
ROWS = {"linked1": 1, "linked16": 16, "linked256": 256, "dict64": 1}


def make_inputs(path, distinct):
    """Frames (the CPU oracle's: what the reference writes) and plaintexts into one .npz (the children only decode)."""
    import numpy as np
    import oracle_ffi as o
    import rust_lz_fear_amd  # noqa: F401
    from rust_lz_fear_amd import synth
    n = 16 * BS
    plains = [synth.silesia_mix(k * n, (k + 1) * n).tobytes() for k in range(distinct)]
    linked = [o.frame_compress(p, o.make_settings(block_size=BS, independent_blocks=False, content_checksum=False))[1] for p in plains]
    dct = synth.gen_text_zipf(3, 65536).tobytes()
    big = b"".join(synth.silesia_mix(0, min(64 * BS - k * synth.SILESIA_TOTAL, synth.SILESIA_TOTAL), copy=k).tobytes()
                   for k in range((64 * BS + synth.SILESIA_TOTAL - 1) // synth.SILESIA_TOTAL))
    assert len(big) == 64 * BS
    dfr = o.frame_compress(big, o.make_settings(block_size=BS, content_checksum=False, dictionary=dct, dictionary_id=7))[1]
    arrs = {f"plain{k}": np.frombuffer(p, np.uint8) for k, p in enumerate(plains)}
    arrs.update({f"linked{k}": np.frombuffer(f, np.uint8) for k, f in enumerate(linked)})
    arrs.update(dict=np.frombuffer(dct, np.uint8), dplain=np.frombuffer(big, np.uint8), dframe=np.frombuffer(dfr, np.uint8))
    np.savez(path, **arrs)


def child(path, rows, calls):
    import numpy as np
    import torch
    import rust_lz_fear_amd  # noqa: F401
    from rust_lz_fear_amd import ffi, framed
    torch.cuda.set_device(0)
    z = np.load(path)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    distinct = sum(1 for k in z.files if k.startswith("linked"))
    d_linked = [dev(z[f"linked{k}"]) for k in range(distinct)]
    d_plain = [dev(z[f"plain{k}"]) for k in range(distinct)]
    out = {}
    for row in rows:
        if row == "dict64":
            frames, dct, caps, want = [dev(z["dframe"])], dev(z["dict"]), [int(z["dplain"].size)], [dev(z["dplain"])]
        else:
            n = ROWS[row]
            frames, dct, caps, want = [d_linked[s % distinct] for s in range(n)], None, [16 * BS] * n, [d_plain[s % distinct] for s in range(n)]
        res = framed.decompress_frames_device(frames, dictionary=dct, caps=caps)          # warm-up, and the check
        launch = ffi.lib().lzf_last_decompress_launch().decode()
        for (st, t, _), w in list(zip(res, want))[:max(distinct, 1)]:
            assert st == 0 and torch.equal(t, w), row
        assert all(st == 0 and t.numel() == c for (st, t, _), c in zip(res, caps)), row
        del res
        ts = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = framed.decompress_frames_device(frames, dictionary=dct, caps=caps)
            ts.append((time.perf_counter() - t0) * 1e3)
            del res
        out[row] = dict(ms=statistics.median(ts), calls=[round(t, 2) for t in ts], launch=launch)
        del frames, want
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblzfear_hip.so of the parent commit (absent: this tree's library only)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--rows", default="linked1,linked16,linked256,dict64")
    ap.add_argument("--out", default=None, help="append the table to this file")
    ap.add_argument("--inputs", default=None, help="keep the frames in this .npz (made when it is missing) instead of a temporary file: a profiler can run "
                                                   "one child on it, `... --child FILE --rows linked16`")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    rows = [r for r in args.rows.split(",") if r]
    assert all(r in ROWS for r in rows), rows
    if args.child:
        return child(args.child, rows, args.calls)
    from rust_lz_fear_amd import build
    libs = [("this", build.LIB_PATH)] + ([("parent", os.path.abspath(args.parent_lib))] if args.parent_lib else [])
    lines = []
    with tempfile.TemporaryDirectory() as td:
        path = args.inputs or os.path.join(td, "inputs.npz")
        if not os.path.exists(path):
            make_inputs(path, args.distinct)
        got = {name: [] for name, _ in libs}
        for run in range(args.runs):
            for name, lib in libs:                               # in turns: a drift of the machine falls on both alike
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--rows", args.rows, "--calls", str(args.calls)],
                                   env=dict(os.environ, LZF_LIB_PATH=lib), capture_output=True, text=True, timeout=900)
                if r.returncode != 0:                            # (nothing more is started on the device after a child that failed)
                    sys.exit(f"{name} run {run}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-3000:]}")
                res = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
                got[name].append(res)
                print(f"run {run} {name}: " + "  ".join(f"{k} {v['ms']:.2f} ms" for k, v in res.items()), flush=True)
    lines.append(f"ms per call of framed.decompress_frames_device, median of {args.calls} calls per run, {args.runs} runs per library in turns")
    for row in rows:
        for name, _ in libs:
            ms = [g[row]["ms"] for g in got[name]]
            lines.append(f"{row:10s} {name:7s} runs {' / '.join(f'{m:8.2f}' for m in ms)}   median {statistics.median(ms):8.2f}   spread {max(ms) - min(ms):6.2f}   [{got[name][0][row]['launch']}]")
        if len(libs) == 2:
            a, b = statistics.median(g[row]["ms"] for g in got["this"]), statistics.median(g[row]["ms"] for g in got["parent"])
            lines.append(f"{row:10s} parent / this = {b / a:.3f}")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
