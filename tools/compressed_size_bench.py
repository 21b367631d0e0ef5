"""Timing of the compressed-size calls next to the compress calls they spare.  Never writes the bench.py line.

One process on one MI355X, HIP events around every call.  Three workloads:
  a  --blocks independent 4 MiB blocks of silesia_mix (4 608), the raw call: lzf_compressed_size_batch against lzf_compress_batch
  b  one default-settings frame of --frame-mib MiB (1 024), content checksum on: lzf_frame_compressed_size_device against
     lzf_frame_compress_device_many — the size call runs no content chain
  c  --streams linked streams of 1 MiB (4 096; 64 KiB blocks) behind a 64 KiB dictionary, the same pair
For each workload the median of --runs (7) alternating runs of
     the size call of this build | the compress call of the PARENT commit's library (--parent-lib: the yardstick) | the compress
     call of this build
after one warm-up of each.  Both libraries live in this process, each behind a ctypes handle of its own (local symbol scope), and
work on the same inputs.  The size call's (status, out_len) are held to this build's compress call before anything is timed.

  python tools/compressed_size_bench.py --parent-lib /path/to/parent/liblzfear_hip.so [--workloads abc] [--runs 7]
                                        [--blocks 4608] [--frame-mib 1024] [--streams 4096]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import build, device, ffi, synth  # noqa: E402

DEV = torch.device("cuda", 0)
BS = 4 << 20
KINDS = ffi.KINDS_U32 | ffi.KINDS_U32_FRESH_ONLY


def load(path, sizes):
    """A library behind its own handle, with the argument types of the calls this tool makes (the parent's has no size calls)."""
    L = C.CDLL(path)
    batch = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.lzf_compress_batch.argtypes = batch
    L.lzf_settings_default.argtypes = [C.POINTER(ffi.Settings)]
    L.lzf_frame_compress_bound.restype = C.c_size_t
    L.lzf_frame_compress_bound.argtypes = [C.POINTER(ffi.Settings), C.c_size_t]
    L.lzf_frame_compress_device_many.argtypes = [C.POINTER(ffi.Settings), C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p,
                                                 C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_void_p]
    if sizes:
        L.lzf_compressed_size_batch.argtypes = batch
        L.lzf_frame_compressed_size_device.argtypes = [C.POINTER(ffi.Settings), C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p,
                                                       C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def ok(rc):
    assert rc == 0, rc


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def tiled_source(nbytes):
    """silesia_mix's first 48 MiB, tiled on the device: every copy beyond the first rotated and XOR-ed, as bench.py does"""
    base = torch.from_numpy(synth.silesia_mix(0, 12 * BS).copy()).to(DEV)
    src = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    for k, a in enumerate(range(0, nbytes, base.numel())):
        n = min(base.numel(), nbytes - a)
        if k == 0:
            src[a:a + n].copy_(base[:n])
        else:
            src[a:a + n].copy_(torch.bitwise_xor(torch.roll(base, (k * 1000003) % base.numel()), (k * 37 + 1) & 0xFF)[:n])
    return src


def alternate(runs, calls):
    """calls: {name: fn}.  One warm-up of each, then `runs` rounds in the given order; {name: [ms]}"""
    for fn in calls.values():
        event_ms(fn)
    out = {k: [] for k in calls}
    for _ in range(runs):
        for k, fn in calls.items():
            out[k].append(event_ms(fn))
    return out


def report(tag, what, times, nbytes):
    line = {"workload": tag, "what": what, "input_bytes": nbytes}
    for k, v in times.items():
        line[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "runs_ms": [round(x, 3) for x in v]}
    p, s = line["compress_parent"], line["size"]
    line["size_over_parent_compress"] = round(s["median_ms"] / p["median_ms"], 4)
    line["size_not_slower_than_parent_beyond_its_spread"] = s["median_ms"] <= p["max_ms"]
    print("SIZEBENCH " + json.dumps(line), flush=True)
    return line


def workload_a(this, parent, n_blocks, runs):
    src = tiled_source(n_blocks * BS)
    out = torch.empty(n_blocks * BS, dtype=torch.uint8, device=DEV)
    j = np.zeros(n_blocks, dtype=device.CJOB)
    j["input"] = np.uint64(src.data_ptr()) + np.arange(n_blocks, dtype=np.uint64) * np.uint64(BS)
    j["input_len"] = BS
    j["out"] = np.uint64(out.data_ptr()) + np.arange(n_blocks, dtype=np.uint64) * np.uint64(BS)
    j["out_cap"] = BS
    j["table_kind"] = ffi.TABLE_U32
    d_jobs = device.to_device(j, DEV)
    res = [torch.zeros(n_blocks * 16, dtype=torch.uint8, device=DEV) for _ in range(3)]
    st = torch.cuda.current_stream().cuda_stream
    calls = {"size": lambda: ok(this.lzf_compressed_size_batch(d_jobs.data_ptr(), res[0].data_ptr(), n_blocks, KINDS, st)),
             "compress_parent": lambda: ok(parent.lzf_compress_batch(d_jobs.data_ptr(), res[1].data_ptr(), n_blocks, KINDS, st)),
             "compress_this": lambda: ok(this.lzf_compress_batch(d_jobs.data_ptr(), res[2].data_ptr(), n_blocks, KINDS, st))}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    r = [device.results_to_host(x, n_blocks) for x in res]
    for other in r[1:]:
        assert np.array_equal(r[0]["status"], other["status"]) and np.array_equal(r[0]["out_len"], other["out_len"]), "the size call differs from a compress call"
    line = report("a", f"{n_blocks} independent 4 MiB blocks, raw call", alternate(runs, calls), n_blocks * BS)
    line["compressed_bytes"] = int(r[0]["out_len"][r[0]["status"] == 0].sum())
    return line


def frames_pair(this, parent, s, ins, d_dict, runs, tag, what):
    n = len(ins)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ins])
    lens = (C.c_size_t * n)(*[t.numel() for t in ins])
    caps_l = [this.lzf_frame_compress_bound(C.byref(s), t.numel()) for t in ins]
    slab = torch.empty(sum(caps_l), dtype=torch.uint8, device=DEV)
    offs = np.concatenate([[0], np.cumsum(caps_l)])
    optr = (C.c_void_p * n)(*[slab.data_ptr() + int(o) for o in offs[:-1]])
    caps = (C.c_size_t * n)(*caps_l)
    status = [torch.empty(n, dtype=torch.int32, device=DEV) for _ in range(3)]
    out_len = [torch.empty(n, dtype=torch.int64, device=DEV) for _ in range(3)]
    dptr, dlen = (d_dict.data_ptr(), d_dict.numel()) if d_dict is not None else (None, 0)
    st = torch.cuda.current_stream().cuda_stream
    calls = {"size": lambda: ok(this.lzf_frame_compressed_size_device(C.byref(s), n, ptrs, lens, dptr, dlen, out_len[0].data_ptr(), status[0].data_ptr(), st)),
             "compress_parent": lambda: ok(parent.lzf_frame_compress_device_many(C.byref(s), n, ptrs, lens, dptr, dlen, optr, caps, out_len[1].data_ptr(),
                                                                                 status[1].data_ptr(), st)),
             "compress_this": lambda: ok(this.lzf_frame_compress_device_many(C.byref(s), n, ptrs, lens, dptr, dlen, optr, caps, out_len[2].data_ptr(),
                                                                             status[2].data_ptr(), st))}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    for k in (1, 2):
        assert torch.equal(status[0], status[k]) and torch.equal(out_len[0], out_len[k]), "the size call differs from a compress call"
    assert int(status[0].abs().sum()) == 0
    line = report(tag, what, alternate(runs, calls), sum(t.numel() for t in ins))
    line["compressed_bytes"] = int(out_len[0].sum())
    return line


def workload_b(this, parent, mib, runs):
    s = ffi.Settings()
    this.lzf_settings_default(C.byref(s))
    assert s.content_checksum == 1 and s.block_size == BS
    src = tiled_source(mib << 20)
    return frames_pair(this, parent, s, [src], None, runs, "b", f"one default-settings frame of {mib} MiB, content checksum on")


def workload_c(this, parent, n_streams, runs):
    s = ffi.Settings()
    this.lzf_settings_default(C.byref(s))
    s.independent_blocks, s.block_size, s.content_checksum = 0, 65536, 0
    src = tiled_source((n_streams << 20) + 65536)
    d_dict = src[:65536]
    ins = [src[65536 + (k << 20):65536 + ((k + 1) << 20)] for k in range(n_streams)]
    return frames_pair(this, parent, s, ins, d_dict, runs, "c", f"{n_streams} linked streams of 1 MiB (64 KiB blocks) behind a 64 KiB dictionary")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="liblzfear_hip.so built from the parent commit: its compress calls are the yardstick")
    ap.add_argument("--workloads", default="abc")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--blocks", type=int, default=4608)
    ap.add_argument("--frame-mib", type=int, default=1024)
    ap.add_argument("--streams", type=int, default=4096)
    args = ap.parse_args()
    this, parent = load(build.LIB_PATH, True), load(args.parent_lib, False)
    assert not hasattr(parent, "lzf_compressed_size_batch"), "--parent-lib has the size call: not the parent commit's library"
    print(f"this build: {build.LIB_PATH}\nparent:     {args.parent_lib}\n{torch.cuda.get_device_name(0)}, {args.runs} alternating runs per call", flush=True)
    for w in args.workloads:
        {"a": lambda: workload_a(this, parent, args.blocks, args.runs), "b": lambda: workload_b(this, parent, args.frame_mib, args.runs),
         "c": lambda: workload_c(this, parent, args.streams, args.runs)}[w]()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
