"""Timing of the resumable decode (lzf_frame_resume_device, lzf_xxh32_update_batch) next to what the parent commit offers:
lzf_frame_decompress_device_many of the whole frames and lzf_xxh32_batch.  Never writes the bench.py line.

Rows (silesia_mix, the bench's corpus, framed by the CPU oracle; workloads of profiles/frame_head.txt):
  xxh          the device XXH32 chain: 1, 16 and 256 states over 4 MiB updates (lzf_xxh32_update_batch, this tree), next to
               lzf_xxh32_batch on the same bytes (both sides): GB/s per chain
  f49x20       49 frames of 20 x 4 MiB independent blocks (7 distinct frames, 7 copies), a content checksum each: through the
               cursor in pieces of 1, 4 and 16 blocks per call, against the whole-frame call
  linked16     one linked-block frame of 16 x 4 MiB: the same pieces, against the whole-frame call
  budget       the linked frame (64 MiB of content) under lzf_frame_set_memory_budget(32 MiB): the whole-frame call reports
               LZF_E_NO_MEMORY, the cursor decodes it in pieces of one block; the time and the peak use of the device's default
               memory pool.  The tool restores the budget.

The inputs are made once; then one child process per side, each under its own time limit: `this` with this tree's library,
`parent` with the library --parent-lib names (the parent commit's; absent: the comparison columns are left out and say so).  A
measurement is one warm-up run and --runs timed runs, wall clock (time.perf_counter) around the run, which starts and ends with the
device synchronised, on the process's current stream (torch's default stream); the median is reported with the least and the
largest run beside it: that spread is the measurement's, and a difference inside it is none.  A piecewise run is every call from
fresh cursors to the last frame's DONE, with the read-back of the phases that a caller needs to know when to stop.

  python tools/frame_resume_bench.py [--parent-lib PATH] [--runs 5] [--out FILE]
"""
import argparse
import ctypes as C
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
PIECES = (1, 4, 16)
CHAINS = (1, 16, 256)


def make_inputs(path):
    import numpy as np
    import oracle_ffi as o
    import rust_lz_fear_amd  # noqa: F401
    from rust_lz_fear_amd import synth
    plain = synth.silesia_mix(0, 28 * BS).tobytes()

    def framed(data, **kw):
        rc, f = o.frame_compress(data, o.make_settings(block_size=BS, **kw))
        assert rc == 0
        return np.frombuffer(f, np.uint8)
    arrs = {f"f{k}": framed(plain[k * 4 * BS:k * 4 * BS + 20 * BS]) for k in range(3)}     # (three distinct frames of 20 blocks here: the copies alias them)
    arrs["linked"] = framed(plain[:16 * BS], independent_blocks=False)
    np.savez(path, **arrs)


def timed(fn, runs):
    import torch
    fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=statistics.median(ts), lo=min(ts), hi=max(ts))


def pool_high(reset=False):
    """Peak bytes in use of the device's default memory pool (hipMemPoolAttrUsedMemHigh); None where the runtime does not say."""
    try:
        hip = C.CDLL("libamdhip64.so")
        pool, v = C.c_void_p(), C.c_uint64(0)
        if hip.hipDeviceGetDefaultMemPool(C.byref(pool), 0) != 0:
            return None
        if reset:
            return 0 if hip.hipMemPoolSetAttribute(pool, 8, C.byref(v)) == 0 else None
        return int(v.value) if hip.hipMemPoolGetAttribute(pool, 8, C.byref(v)) == 0 else None
    except OSError:
        return None


def child(side, inputs, runs):
    import numpy as np
    import torch
    import rust_lz_fear_amd  # noqa: F401
    from rust_lz_fear_amd import device, ffi
    dev = torch.device("cuda", 0)
    lib = ffi.lib()
    z = np.load(inputs)
    rows = []

    def emit(**kw):
        rows.append(dict(side=side, **kw))
        print(json.dumps(rows[-1]), flush=True)

    # ---- the XXH32 chain
    data = torch.randint(0, 256, (max(CHAINS) * BS,), dtype=torch.uint8, device=dev)
    for n in CHAINS:
        ptrs = torch.tensor([data.data_ptr() + i * BS for i in range(n)], dtype=torch.int64, device=dev)
        lens = torch.full((n,), BS, dtype=torch.int64, device=dev)
        out = torch.empty(n, dtype=torch.int32, device=dev)
        r = timed(lambda: device.xxh32_batch(ptrs, lens, out, n), runs)
        emit(row="xxh", call="lzf_xxh32_batch", chains=n, gbps=BS / r["ms"] / 1e6, gbps_lo=BS / r["hi"] / 1e6, gbps_hi=BS / r["lo"] / 1e6, **r)
        want = out.clone()
        if side == "this":
            st0 = ffi.Xxh32State()
            lib.lzf_xxh32_reset(C.byref(st0), 0)
            fresh = torch.from_numpy(np.tile(np.frombuffer(bytes(st0), np.uint8), n).copy()).to(dev)
            states = fresh.clone()
            r = timed(lambda: device.xxh32_update_batch(states, ptrs, lens, n), runs)
            emit(row="xxh", call="lzf_xxh32_update_batch", chains=n, gbps=BS / r["ms"] / 1e6, gbps_lo=BS / r["hi"] / 1e6, gbps_hi=BS / r["lo"] / 1e6, **r)
            states.copy_(fresh)
            device.xxh32_update_batch(states, ptrs, lens, n)
            device.xxh32_digest_batch(states, out, n)
            assert torch.equal(out, want), "the state chain's digest differs from lzf_xxh32_batch"
    del data

    # ---- piecewise against whole
    def whole(frames, outs):
        st, ol, co = device.frame_decompress_many(frames, outs)
        return st, ol

    def pieces(frames, bufs, k):
        cursors = device.new_frame_cursors(len(frames), dev)
        calls = 0
        while True:
            st, ol, co, ph = device.frame_resume(frames, None, cursors, bufs)
            calls += 1
            ph = ph.cpu().tolist()
            assert not any(st.cpu().tolist()), "a piece failed"
            if all(p == ffi.RESUME_DONE for p in ph):
                return calls

    distinct = [torch.from_numpy(z[f"f{k}"].copy()).to(dev) for k in range(3)]
    linked = torch.from_numpy(z["linked"].copy()).to(dev)
    for row, frames, nb in (("f49x20", [distinct[i % 3] for i in range(49)], 20), ("linked16", [linked], 16)):
        outs = [torch.empty(nb * BS, dtype=torch.uint8, device=dev) for _ in frames]
        st, ol = whole(frames, outs)
        assert not st.cpu().any() and int(ol.cpu()[0]) == nb * BS
        emit(row=row, call="whole", **timed(lambda: whole(frames, outs), runs))
        if side == "this":
            for k in PIECES:
                bufs = [o[:k * BS] for o in outs]
                calls = pieces(frames, bufs, k)
                emit(row=row, call=f"pieces of {k}", calls=calls, **timed(lambda: pieces(frames, bufs, k), runs))
        del outs

    # ---- one frame larger than the memory budget
    out = torch.empty(16 * BS, dtype=torch.uint8, device=dev)
    lib.lzf_frame_set_memory_budget(32 << 20)
    try:
        st, ol = whole([linked], [out])
        emit(row="budget", call="whole", status=int(st.cpu()[0]), out_len=int(ol.cpu()[0]))
        if side == "this":
            torch.cuda.synchronize()
            pool_high(reset=True)
            r = timed(lambda: pieces([linked], [out[:BS]], 1), runs)
            emit(row="budget", call="pieces of 1", pool_high=pool_high(), **r)
    finally:
        lib.lzf_frame_set_memory_budget(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--child")
    ap.add_argument("--inputs")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.inputs, a.runs)
    with tempfile.TemporaryDirectory() as tmp:
        inputs = os.path.join(tmp, "inputs.npz")
        make_inputs(inputs)
        rows = []
        for side, libpath in (("this", None), ("parent", a.parent_lib)):
            if side == "parent" and not libpath:
                continue
            env = dict(os.environ)
            if libpath:
                env["LZF_LIB_PATH"] = os.path.abspath(libpath)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, "--inputs", inputs, "--runs", str(a.runs)],
                               env=env, capture_output=True, text=True, timeout=420)
            sys.stderr.write(p.stderr[-2000:])
            if p.returncode != 0:
                raise SystemExit(f"the {side} side ended with {p.returncode}")
            rows += [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    text = report(rows, a)
    print(text)
    if a.out:
        open(a.out, "w").write(text)


def report(rows, a):
    def get(side, row, call, **kw):
        for r in rows:
            if (r["side"], r["row"], r["call"]) == (side, row, call) and all(r.get(k) == v for k, v in kw.items()):
                return r
        return None

    def ms(r):
        return f"{r['ms']:8.2f} ms ({r['lo']:.2f} .. {r['hi']:.2f})" if r else "not measured"
    base = "parent" if any(r["side"] == "parent" for r in rows) else "this"
    L = [f"tools/frame_resume_bench.py --runs {a.runs}: median of {a.runs} runs behind one warm-up, (least .. largest) beside it; wall clock",
         "(time.perf_counter) around the run, device synchronised before and after, torch's current stream.",
         f"Comparison side: {'the parent commit library' if base == 'parent' else 'THIS tree (no --parent-lib given): no parent numbers'}.", "",
         "The device XXH32 chain, 4 MiB per chain, GB/s per chain (least .. largest):"]
    for n in CHAINS:
        u, b, t = get("this", "xxh", "lzf_xxh32_update_batch", chains=n), get(base, "xxh", "lzf_xxh32_batch", chains=n), get("this", "xxh", "lzf_xxh32_batch", chains=n)
        f = lambda r: f"{r['gbps']:.3f} ({r['gbps_lo']:.3f} .. {r['gbps_hi']:.3f})" if r else "not measured"
        L.append(f"  {n:4d} chains   lzf_xxh32_update_batch {f(u)}   lzf_xxh32_batch [{base}] {f(b)}   lzf_xxh32_batch [this] {f(t)}")
    for row, what in (("f49x20", "49 frames of 20 x 4 MiB independent blocks"), ("linked16", "one linked-block frame of 16 x 4 MiB")):
        w = get(base, row, "whole")
        L += ["", f"{what}: lzf_frame_decompress_device_many [{base}] {ms(w)}   [this] {ms(get('this', row, 'whole'))}"]
        for k in PIECES:
            r = get("this", row, f"pieces of {k}")
            ratio = f"{r['ms'] / w['ms']:.2f} x the whole call; within its spread: {'yes' if r['lo'] <= w['hi'] else 'no'}" if r and w else ""
            L.append(f"  pieces of {k:2d} blocks  {r['calls'] if r else '?':>3} calls  {ms(r)}   {ratio}")
    w, r = get("this", "budget", "whole"), get("this", "budget", "pieces of 1")
    L += ["", "The linked frame (64 MiB of content) under a memory budget of 32 MiB:",
          f"  lzf_frame_decompress_device_many: status {w['status'] if w else '?'} (LZF_E_NO_MEMORY is -4), out_len {w['out_len'] if w else '?'}",
          f"  through the cursor, pieces of one block: {ms(r)}; peak use of the default memory pool: " +
          (f"{r['pool_high'] / (1 << 20):.1f} MiB" if r and r.get("pool_high") is not None else "not measured (the runtime did not report it)")]
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    main()
