"""The saved walks of lzf_seg_parse_kernel's fixed point (lz4_seg_front.hip, kParseMemo) on the device, against the host model of
tests/parse_memo_cases.py, whose reach tests/test_parse_memo_cases_cpu.py proves: an entry that comes back after one pass and after two
others, restored walks that had merged / left the region / never entered it / gone through the general routine, a hit and then a miss,
hits in the lowest lane that can have one and in lane 63, and two chunks in which a lane meets the same chunk-relative entry over other
bytes.  All blocks go in one launch.  For every block the device's bit map (lzf_debug_seg, upto = 2) equals the model's word for word,
its chunk exits equal the model's, and the fed front's estimate (lzf_debug_order, no byte share) is the model's count of owned marks —
for the product loop, for its C++ twin (-DLZF_SEG_NOASM), and with one workgroup per job, which then walks both chunks of the two-chunk
block with the same registers.  The timing build's lookups and hits over the launch equal the model's sums.  The blocks decode
through the forced fed path and through the segmented pipeline to the oracle's bytes.  The children (one per library / path) run side
by side, each under a time limit, and none is left behind."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import oracle_ffi as o  # noqa: E402
import parse_hop_cases as P  # noqa: E402
import parse_memo_cases as M  # noqa: E402
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import ffi  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = M.all_cases()
NAMES = [n for n, _ in CASES]
TILES = 524288                        # LZF_SEG_GRID's second value: the tile kernels' default (not under test)
PATHS = {"fed": (dict(LZF_DECOMPRESS_KERNEL="fed", LZF_FED_MIN_IN="1", LZF_FED_PIECES="1"), "bitmap-fed"),
         "seg": (dict(LZF_DECOMPRESS_KERNEL="seg"), "segmented")}
MAPS = ["asm", "twin", "one", "timing"]


@pytest.fixture(scope="module")
def model():
    """Per block: (rows, exits, owned marks, lookups, hits) with one saved walk, as the kernel is built."""
    return [M.expected(b, 1) for _, b in CASES]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from rust_lz_fear_amd import build
    d = tmp_path_factory.mktemp("parse_memo")
    blocks = [b for _, b in CASES]
    exp = [o.decompress_raw(b, limit=M.LIMIT, cap=M.LIMIT + len(b) + 64) for b in blocks]
    assert all(e[0] == 0 for e in exp)
    corpus = d / "corpus.pkl"
    corpus.write_bytes(pickle.dumps((blocks, exp)))
    analysis = build.build_analysis_library()
    libs = {"asm": (analysis, {}), "twin": (build.build_library(defines=build.PARSE_TWIN_BUILD), {}),
            "one": (analysis, {"LZF_SEG_GRID": f"1,{TILES}"}),                 # (the library gives every job at least one workgroup)
            "timing": (build.build_library(defines=build.PARSE_TIME_BUILD), {})}
    procs = {}
    for key, (lib, env) in libs.items():
        e = dict(os.environ, LZF_LIB_PATH=lib, PARSE_STAGING_CORPUS=str(corpus), **env)
        procs["map_" + key] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "maps", str(d / f"maps_{key}.pkl")], env=e,
                                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    for key, (env, prefix) in PATHS.items():
        e = dict(os.environ, LZF_LIB_PATH=analysis, PARSE_STAGING_CORPUS=str(corpus), **env)
        procs["dec_" + key] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "decode", prefix, str(d / f"dec_{key}.pkl")], env=e,
                                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = {}
    try:
        for key, p in procs.items():
            text, _ = p.communicate(timeout=120)
            out[key] = (p.returncode, text)
    finally:                                             # whatever happened to one child, none is left with the GPU open
        for p in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
    res = {"exp": exp, "out": out}
    for key in list(out):
        f = d / f"{key.replace('map_', 'maps_')}.pkl"
        if out[key][0] == 0:
            res[key] = pickle.loads(f.read_bytes())
    return res


def _need(runs, key):
    rc, text = runs["out"][key]
    assert rc == 0 and ("parse memo ok" in text or "parse hop ok" in text), text[-4000:]
    return runs[key]


@pytest.mark.parametrize("lib", MAPS)
@pytest.mark.parametrize("case", range(len(CASES)), ids=NAMES)
def test_map_exits_and_estimate_are_the_models(runs, model, case, lib):
    got = _need(runs, "map_" + lib)
    rows, exits, est, _, _ = model[case]
    blk = CASES[case][1]
    nch = P.nch(len(blk))
    diff = np.argwhere(got["bits"][case][:nch] != rows)
    assert diff.size == 0, f"chunk {int(diff[0][0])} word {int(diff[0][1])}: {int(got['bits'][case][tuple(diff[0])]):#x}, the model has {int(rows[tuple(diff[0])]):#x}"
    assert (got["xexit"][case][:nch] == exits).all(), (got["xexit"][case][:nch], exits)
    assert int(got["est"][case]) == est


def test_lookups_and_hits_are_the_models(runs, model):
    got = _need(runs, "map_timing")["counters"]
    assert got is not None
    assert (int(got[8]), int(got[9])) == (sum(m[3] for m in model), sum(m[4] for m in model))
    assert int(got[9]) > 0 and int(got[4]) == sum(P.nch(len(b)) for _, b in CASES)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("case", range(len(CASES)), ids=NAMES)
def test_decodes_like_the_oracle(runs, case, path):
    rc, out = _need(runs, "dec_" + path)[case]
    erc, eout = runs["exp"][case]
    assert rc == erc and len(out) == len(eout) and out == eout


# ---------------------------------------------------------------------------------------------------------------- the children
def child_maps(out_path):
    import torch
    from rust_lz_fear_amd import device
    with open(os.environ["PARSE_STAGING_CORPUS"], "rb") as f:
        blocks, _ = pickle.load(f)
    n = len(blocks)
    offs = np.cumsum([0] + [(len(b) + 255) // 256 * 256 + 16 for b in blocks])
    h_in = np.zeros(int(offs[-1]) + 64, np.uint8)
    for b, a in zip(blocks, offs):
        h_in[a:a + len(b)] = np.frombuffer(b, np.uint8)
    d_in = torch.from_numpy(h_in).cuda()
    d_out = torch.zeros(n * 4096, dtype=torch.uint8, device="cuda")                 # (stage 2 writes no output)
    dj = np.zeros(n, dtype=device.DJOB)
    dj["input"] = np.uint64(d_in.data_ptr()) + offs[:n].astype(np.uint64)
    dj["input_len"] = [len(b) for b in blocks]
    dj["out"] = np.uint64(d_out.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(4096)
    dj["out_cap"] = 4096
    dj["output_limit"] = M.LIMIT
    d_dj = device.to_device(dj, "cuda")
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    lib = ffi.lib()
    fn = lib.lzf_debug_seg
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 7 + [C.c_uint64, C.c_void_p]
    geom = np.zeros(4, np.uint32)
    ffi.check(fn(d_dj.data_ptr(), d_res.data_ptr(), n, 1, 1, None, None, None, None, None, None, None, 0, geom.ctypes.data))
    maxch, cw = int(geom[0]), int(geom[2])
    assert cw == M.CHUNK // 32 and maxch >= max(P.nch(len(b)) for b in blocks)
    timers = getattr(lib, "lzf_debug_parse_timers", None)
    counters = None
    if timers is not None:
        timers.restype = C.c_int
        timers.argtypes = [C.POINTER(C.c_uint64), C.c_int]
        ffi.check(timers(None, 1))
    bits = np.zeros((n, maxch, cw), np.uint32)
    xexit = np.zeros((n, maxch), np.uint32)
    ffi.check(fn(d_dj.data_ptr(), d_res.data_ptr(), n, 1, 2, None, bits.ctypes.data, xexit.ctypes.data, None, None, None, None, 0, geom.ctypes.data))
    if timers is not None:
        t = (C.c_uint64 * 10)()
        ffi.check(timers(t, 1))
        counters = [int(v) for v in t]
    # the fed front (plan + parse with fed = 1): est[j] = the marks the job's chunks own, with len_shift 32 no share of the bytes on top
    order = lib.lzf_debug_order
    order.restype = C.c_int
    order.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    est = np.zeros(n, np.uint32); perm = np.zeros(n, np.uint32)
    ffi.check(order(4, d_dj.data_ptr(), n, None, 1, 32, est.ctypes.data, perm.ctypes.data, None, None))
    with open(out_path, "wb") as f:
        pickle.dump(dict(bits=[bits[i] for i in range(n)], xexit=[xexit[i] for i in range(n)], est=est, counters=counters), f)
    print("parse memo ok: maps of", n, "jobs")


if __name__ == "__main__":
    if sys.argv[1] == "maps":
        child_maps(sys.argv[2])
    else:
        import test_gpu_parse_hop as T                 # its child decodes every job and keeps status and bytes
        T.child_decode(*sys.argv[2:])
