"""Timing of the streaming frame writer (lzf_frame_append_device) next to lzf_frame_compress_device_many on the same inputs.
Never writes the bench.py line.

Rows (silesia_mix, the bench's corpus; the default settings: independent blocks, a content checksum, 4 MiB blocks):
  f49x20       49 inputs of 20 x 4 MiB (3 distinct ranges of the corpus, the copies alias them): through write cursors in pieces
               of 1, 4 and 16 blocks per call and in ONE call with FINISH, against the whole call
  linked16     one linked-block input of 16 x 4 MiB: the same pieces, against the whole call
  budget       the linked input (64 MiB; input plus bound: 128 MiB) under lzf_frame_set_memory_budget(32 MiB), fed block by block
               through ONE reused input buffer of 4 MiB (a device copy refills it in stream order): the time and the peak use of
               the device's default memory pool, next to the whole call's under the same budget.  The tool restores the budget.

One child process per side, each under its own time limit: `this` with this tree's library, `parent` (whole calls only) with
the library --parent-lib names; absent, the whole call of THIS tree is the comparison: the compress driver's launches are the
parent's, unchanged.  A measurement is one warm-up run and --runs timed runs, wall clock (time.perf_counter) around the run,
which starts and ends with the device synchronised, on torch's current stream; the median is reported with the least and the
largest run beside it: a difference inside that spread is none.  A piecewise run is every call from fresh (zeroed) cursors to the
call with FINISH; nothing is read back between the calls (every piece goes to a slot of its own of the bound's size).

  python tools/frame_append_bench.py [--parent-lib PATH] [--runs 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BS = 4 << 20
PIECES = (1, 4, 16)


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


def child(side, runs):
    import torch
    import rust_lz_fear_amd  # noqa: F401
    from rust_lz_fear_amd import device, ffi, synth
    dev = torch.device("cuda", 0)
    lib = ffi.lib()
    plain = torch.from_numpy(synth.silesia_mix(0, 28 * BS).copy()).to(dev)

    def emit(**kw):
        print(json.dumps(dict(side=side, **kw)), flush=True)

    def settings(linked):
        s = ffi.Settings()
        lib.lzf_settings_default(C.byref(s))
        s.independent_blocks = 0 if linked else 1
        return s

    def bound(s, n):
        return int(lib.lzf_frame_compress_bound(C.byref(s), n))

    def appended(s, ins, nb, k, slots, cursors):
        """Every call from zeroed cursors to FINISH, k blocks per call; piece i of frame f goes to slots[i][f]."""
        cursors.zero_()
        for i, p in enumerate(range(0, nb, k)):
            last = p + k >= nb
            device.frame_append(s, [t[p * BS:(p + k) * BS] for t in ins], [ffi.APPEND_FINISH if last else 0] * len(ins), cursors, slots[i])

    for row, linked, ins, nb in (("f49x20", False, [plain[(f % 3) * 4 * BS:(f % 3) * 4 * BS + 20 * BS] for f in range(49)], 20),
                                 ("linked16", True, [plain[:16 * BS]], 16)):
        s = settings(linked)
        outs = [torch.empty(bound(s, nb * BS), dtype=torch.uint8, device=dev) for _ in ins]
        st, ol = device.frame_compress_many(s, ins, outs)
        assert not st.cpu().any()
        want = outs[0][:int(ol.cpu()[0])].clone()
        emit(row=row, call="whole", **timed(lambda: device.frame_compress_many(s, ins, outs), runs))
        if side != "this":
            continue
        cursors = device.new_frame_write_cursors(len(ins), dev)
        for k in PIECES + (nb,):
            calls = (nb + k - 1) // k
            slots = [[torch.empty(bound(s, k * BS), dtype=torch.uint8, device=dev) for _ in ins] for _ in range(calls)]
            # once with the results read back: the concatenation of frame 0's pieces is the whole call's frame
            cursors.zero_()
            got = []
            for i, p in enumerate(range(0, nb, k)):
                st, ol, tk, ph = device.frame_append(s, [t[p * BS:(p + k) * BS] for t in ins], [ffi.APPEND_FINISH if p + k >= nb else 0] * len(ins), cursors, slots[i])
                assert not st.cpu().any()
                got.append(slots[i][0][:int(ol.cpu()[0])].clone())
            assert torch.equal(torch.cat(got), want) and all(p == ffi.APPEND_DONE for p in ph.cpu().tolist()), "the pieces are not the whole call's frame"
            emit(row=row, call="one call with FINISH" if k == nb else f"pieces of {k}", calls=calls, **timed(lambda: appended(s, ins, nb, k, slots, cursors), runs))
            del slots
        del outs

    if side != "this":
        return
    # ---- one frame whose input plus bound is over the memory budget, through one reused input buffer
    s = settings(True)
    nb = 16
    src = plain[:nb * BS]
    out = torch.empty(bound(s, nb * BS), dtype=torch.uint8, device=dev)
    buf = torch.empty(BS, dtype=torch.uint8, device=dev)
    slots = [[torch.empty(bound(s, BS), dtype=torch.uint8, device=dev)] for _ in range(nb)]
    cursors = device.new_frame_write_cursors(1, dev)

    def fed():
        cursors.zero_()
        for i in range(nb):
            buf.copy_(src[i * BS:(i + 1) * BS])             # (stream order: the call before is done with the buffer)
            device.frame_append(s, [buf], [ffi.APPEND_FINISH if i == nb - 1 else 0], cursors, slots[i])

    lib.lzf_frame_set_memory_budget(32 << 20)
    try:
        torch.cuda.synchronize()
        pool_high(reset=True)
        r = timed(lambda: device.frame_compress_many(s, [src], [out]), runs)
        emit(row="budget", call="whole", pool_high=pool_high(), **r)
        st, ol = device.frame_compress_many(s, [src], [out])
        want = out[:int(ol.cpu()[0])].clone()
        torch.cuda.synchronize()
        pool_high(reset=True)
        r = timed(fed, runs)
        emit(row="budget", call="fed block by block", pool_high=pool_high(), **r)
        fed()
        lens = []
        cursors.zero_()
        for i in range(nb):
            buf.copy_(src[i * BS:(i + 1) * BS])
            st, ol, tk, ph = device.frame_append(s, [buf], [ffi.APPEND_FINISH if i == nb - 1 else 0], cursors, slots[i])
            lens.append(int(ol.cpu()[0]))
        assert torch.equal(torch.cat([slots[i][0][:lens[i]] for i in range(nb)]), want), "the fed frame is not the whole call's"
    finally:
        lib.lzf_frame_set_memory_budget(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.runs)
    rows = []
    for side, libpath in (("this", None), ("parent", a.parent_lib)):
        if side == "parent" and not libpath:
            continue
        env = dict(os.environ)
        if libpath:
            env["LZF_LIB_PATH"] = os.path.abspath(libpath)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, "--runs", str(a.runs)], env=env, capture_output=True, text=True, timeout=540)
        sys.stderr.write(p.stderr[-2000:])
        rows += [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode != 0:
            print(report(rows, a))
            raise SystemExit(f"the {side} side ended with {p.returncode}")
    text = report(rows, a)
    print(text)
    if a.out:
        open(a.out, "w").write(text)


def report(rows, a):
    def get(side, row, call):
        for r in rows:
            if (r["side"], r["row"], r["call"]) == (side, row, call):
                return r
        return None

    def ms(r):
        return f"{r['ms']:8.2f} ms ({r['lo']:.2f} .. {r['hi']:.2f})" if r else "not measured"

    def mib(r):
        return f"{r['pool_high'] / (1 << 20):.1f} MiB" if r and r.get("pool_high") is not None else "not measured (the runtime did not report it)"
    base = "parent" if any(r["side"] == "parent" for r in rows) else "this"
    L = [f"tools/frame_append_bench.py --runs {a.runs}: median of {a.runs} runs behind one warm-up, (least .. largest) beside it; wall clock",
         "(time.perf_counter) around the run, device synchronised before and after, torch's current stream.",
         f"Comparison side: {'the parent commit library' if base == 'parent' else 'the whole call of THIS tree (no --parent-lib given; its launches are unchanged from the parent commit)'}."]
    for row, what in (("f49x20", "49 inputs of 20 x 4 MiB, independent blocks, content checksum"), ("linked16", "one linked-block input of 16 x 4 MiB")):
        w = get(base, row, "whole")
        L += ["", f"{what}: lzf_frame_compress_device_many [{base}] {ms(w)}" + (f"   [this] {ms(get('this', row, 'whole'))}" if base != "this" else "")]
        for call in [f"pieces of {k}" for k in PIECES] + ["one call with FINISH"]:
            r = get("this", row, call)
            if r is None and call != "one call with FINISH":
                continue                    # (pieces as long as the input: that is the one call)
            ratio = f"{r['ms'] / w['ms']:.2f} x the whole call; within its spread: {'yes' if r['lo'] <= w['hi'] and w['lo'] <= r['hi'] else 'no'}" if r and w else ""
            L.append(f"  lzf_frame_append_device, {call:22s} {r['calls'] if r else '?':>3} calls  {ms(r)}   {ratio}")
    w, r = get("this", "budget", "whole"), get("this", "budget", "fed block by block")
    L += ["", "The linked input (64 MiB; input plus bound 128 MiB) under a memory budget of 32 MiB:",
          f"  lzf_frame_compress_device_many (input and bound resident, a pass of its own over the budget): {ms(w)}; peak use of the default memory pool: {mib(w)}",
          f"  lzf_frame_append_device through ONE reused 4 MiB input buffer, a block per call, 16 calls: {ms(r)}; peak use of the default memory pool: {mib(r)}",
          "", "Not timed: offers below one block (NEED_INPUT calls), capacities that leave blocks behind (MORE), dictionaries, many cursors fed at",
          "different rates, and a producer that is slower than the writer."]
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    main()
