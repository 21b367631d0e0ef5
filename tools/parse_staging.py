"""Where a wave of lzf_seg_parse_kernel spends its cycles, by section, at the benchmark's shape (the stand-in's blocks, `copies` times,
through the product dispatch: the bitmap-fed path from 3 073 jobs on).  Needs a library built with -DLZF_DBG_PARSE_TIME, e.g.
    python -c "from rust_lz_fear_amd import build as b; print(b.build_library(defines=['LZF_DBG_PARSE_TIME']))"
usage: LZF_LIB_PATH=<that library> python tools/parse_staging.py [copies=240] [reps=3]"""
import ctypes as C, os, sys
import numpy as np, torch
sys.path.insert(0, os.getcwd())
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi, synth
copies = int(sys.argv[1]) if len(sys.argv) > 1 else 240
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
BS = 4 << 20
d_in = torch.from_numpy(synth.silesia_mix()).cuda()
blocks = device.BlockSet(d_in, BS); n = blocks.n
d_out = torch.empty(n * BS, dtype=torch.uint8, device='cuda'); d_res = torch.zeros(n * 16, dtype=torch.uint8, device='cuda')
device.compress_batch(device.to_device(blocks.compress_jobs(d_out, BS), 'cuda'), d_res, n); torch.cuda.synchronize()
res = device.results_to_host(d_res, n).copy()
ok = np.nonzero(res['status'] == 0)[0]
idx = np.tile(ok, copies); m = len(idx)
dj = np.zeros(m, dtype=device.DJOB); d_dec = torch.empty(m * BS, dtype=torch.uint8, device='cuda')
dj['input'] = d_out.data_ptr() + idx.astype(np.uint64) * BS; dj['input_len'] = res['out_len'][idx]
dj['out'] = d_dec.data_ptr() + np.arange(m, dtype=np.uint64) * BS; dj['out_cap'] = BS; dj['output_limit'] = BS
d_dj = device.to_device(dj, 'cuda'); d_res2 = torch.zeros(m * 16, dtype=torch.uint8, device='cuda')
fn = ffi.lib().lzf_debug_parse_timers
fn.argtypes = [C.POINTER(C.c_uint64), C.c_int]
t = (C.c_uint64 * 10)()
device.decompress_batch(d_dj, d_res2, m); torch.cuda.synchronize()          # warm-up
assert fn(None, 1) == 0
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ev[0].record()
for _ in range(reps):
    device.decompress_batch(d_dj, d_res2, m)
ev[1].record(); torch.cuda.synchronize()
assert fn(t, 1) == 0
assert (device.results_to_host(d_res2, m)['status'] == 0).all()
sec, chunks, wgs = np.array(t[:4], dtype=np.float64), int(t[4]), int(t[5])
print(f"{ffi.lib().lzf_last_decompress_launch().decode()}")
print(f"{m} jobs, {reps} calls (with timers: {ev[0].elapsed_time(ev[1]) / reps:.1f} ms per call), {chunks // reps} chunks and {wgs // reps} workgroups with a chunk per call, {chunks / max(wgs, 1):.2f} chunks per workgroup")
print("mean cycles per chunk (clock64 of the wave):")
for name, v in zip(("staging", "pass 0", "fixed-point passes", "write-out"), sec):
    print(f"  {name:20s} {v / chunks:9.0f}  {100.0 * v / sec.sum():5.1f} %")
print(f"  {'sum':20s} {sec.sum() / chunks:9.0f}")
# the plain-hop loop: hops of the wave (one per half of a trip), and what a hop costs if the whole section is charged to them
print("hops of the wave in the plain-hop loop, per chunk, and cycles of the section per hop:")
for name, v, hops in (("pass 0 (mode 0)", sec[1], int(t[6])), ("fixed-point passes (mode 1)", sec[2], int(t[7]))):
    print(f"  {name:28s} {hops / chunks:8.1f} hops  {v / max(hops, 1):7.1f} cycles per hop")
# the saved walks of the fixed point: a lookup is a lane whose entry changed; a hit takes a displaced walk back instead of walking (tools/parse_memo_model.c)
print(f"lookups of the saved walks per chunk {int(t[8]) / chunks:8.1f}, of which hit {int(t[9]) / chunks:8.1f}  ({100.0 * int(t[9]) / max(int(t[8]), 1):.1f} %)")
