"""lzf_seg_parse_kernel stages a chunk's 16 KiB with ONE round trip of sixteen 16-byte loads per lane: no branch around a load, a lane
whose 16 bytes end behind the chunk's `avail` loads the last whole 16 bytes in front of it and stores zeros (lz4_seg_front.hip).
The shapes here are the smallest at which that can go wrong: inputs of one chunk, of two, with a ragged tail of 1 / 15 bytes behind
the last whole 16, and with a short last chunk — kSegChunk and kSegChunk + kSegStride each - 1, + 0, + 1, and three and seven whole
chunks + 0, 1, 15, 16, 17 bytes.  Every length runs with one workgroup per job (LZF_SEG_GRID: it loops over all the job's chunks, the
short last one behind full ones), with two, and with the default of one chunk per workgroup, through the forced fed path (whole jobs
and three pieces) and through the segmented pipeline; statuses, out_len and bytes are the oracle's.  The bit map (lzf_debug_seg,
upto = 2) is the same word for word under the three grids — it must not depend on which workgroup staged a chunk, or after which
other chunk — and the red-zone harness runs the set with inputs at address residues 0, 1 and 15 (analysis library throughout)."""
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
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import ffi  # noqa: E402
from test_gpu_fed_decode_once import _block, _walk  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK, STRIDE = 16384, 14336          # kSegChunk, kSegStride (lzf_dispatch.h)
TILES = 524288                        # LZF_SEG_GRID's second value: the tile kernels' default on 256 CUs (not under test)
LENGTHS = ([CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + STRIDE - 1, CHUNK + STRIDE, CHUNK + STRIDE + 1] +
           [CHUNK + (k - 1) * STRIDE + d for k in (3, 7) for d in (0, 1, 15, 16, 17)])
LIMIT = 1 << 22
GRIDS = ["one", "two", "default"]
PATHS = {"fed": dict(LZF_DECOMPRESS_KERNEL="fed", LZF_FED_MIN_IN="1", LZF_FED_PIECES="1"),
         "fed3": dict(LZF_DECOMPRESS_KERNEL="fed", LZF_FED_MIN_IN="1", LZF_FED_PIECES="3"),
         "seg": dict(LZF_DECOMPRESS_KERNEL="seg")}


def _nch(n):
    return 1 if n <= CHUNK else 1 + (n - CHUNK + STRIDE - 1) // STRIDE


def _seq_size(L, M):
    return 1 + (0 if L < 15 else 1 + (L - 15) // 255) + L + 2 + (0 if M - 4 < 15 else 1 + (M - 19) // 255)


def _block_of(length, seed):
    """A valid block of exactly `length` compressed bytes: short sequences, now and then a literal or match length with a 0xFF
    extension byte (the general routine) or a literal run over several regions; the last literals make up the length."""
    rng = np.random.default_rng(seed)
    seqs, n = [(8, 4)], _seq_size(8, 4)
    while True:
        r = int(rng.integers(0, 100))
        L, M = ((15 + 255 + int(rng.integers(0, 40)), 4 + int(rng.integers(0, 10))) if r < 3 else
                (int(rng.integers(0, 6)), 19 + 255 + int(rng.integers(0, 300))) if r < 6 else
                (600 + int(rng.integers(0, 200)), 5) if r < 7 else
                (int(rng.integers(0, 15)), 4 + int(rng.integers(0, 15))))
        if n + _seq_size(L, M) > length - 40:
            break
        seqs.append((L, M)); n += _seq_size(L, M)
    rest = length - n                                  # token + length bytes + t literals
    t = next(t for t in range(rest, 0, -1) if 1 + (0 if t < 15 else 1 + (t - 15) // 255) + t == rest)
    blk = _block(seqs, tail=bytes((seed + i) & 0xFF for i in range(t)))
    assert len(blk) == length and _walk(blk)[-1][2] == 0
    return blk


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """The blocks and what the oracle makes of them, once for every test of the module (the children read the file)."""
    blocks = [_block_of(n, 100 + i) for i, n in enumerate(LENGTHS)]
    assert [_nch(len(b)) for b in blocks] == [1, 1, 2, 2, 2, 3, 3, 4, 4, 4, 4, 7, 8, 8, 8, 8]
    exp = [o.decompress_raw(b, limit=LIMIT, cap=LIMIT + len(b) + 64) for b in blocks]
    assert all(e[0] == 0 for e in exp)
    path = tmp_path_factory.mktemp("parse_staging") / "corpus.pkl"
    path.write_bytes(pickle.dumps((blocks, exp)))
    return str(path)


def _grid_env(grid, n_jobs):
    """LZF_SEG_GRID = "parse,tiles": workgroups of a launch over all its jobs (at least one per job).  The library divides the first
    value by the jobs of the LAUNCH: "two" is two per job where the call's jobs go in one launch (the fed path, lzf_debug_seg) and at
    least two where a path launches the parse over a group of them; either way a workgroup's first chunk and the chunks it loops on to
    are both staged, which is what the setting is for."""
    return {} if grid == "default" else {"LZF_SEG_GRID": f"{1 if grid == 'one' else 2 * n_jobs},{TILES}"}


def _child(what, corpus, grid, n_jobs, *args, **env):
    from rust_lz_fear_amd import build
    e = dict(os.environ, LZF_LIB_PATH=build.build_analysis_library(), PARSE_STAGING_CORPUS=corpus, **_grid_env(grid, n_jobs), **env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what, *args], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "parse staging ok" in r.stdout, r.stdout[-2000:]
    return r.stdout


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("path", list(PATHS))
def test_every_length_decodes_like_the_oracle(corpus, path, grid):
    _child("decode", corpus, grid, len(LENGTHS), "bitmap-fed" if path.startswith("fed") else "segmented", **PATHS[path])


def test_bit_map_is_the_same_under_every_grid(corpus, tmp_path):
    """The map must not depend on how a chunk came to be staged: first chunk of a workgroup, a later one of its loop, one chunk per workgroup."""
    maps = []
    for grid in GRIDS:
        out = tmp_path / f"bits_{grid}.npy"
        _child("bitmap", corpus, grid, len(LENGTHS), str(out))
        maps.append(np.load(out))
    assert maps[0].dtype == np.uint32 and maps[0].size == sum(_nch(n) for n in LENGTHS) * (CHUNK // 32)
    assert maps[0].any()
    for grid, m in zip(GRIDS[1:], maps[1:]):
        diff = np.nonzero(m != maps[0])[0]
        assert diff.size == 0, f"grid {grid}: {diff.size} words differ from grid {GRIDS[0]}, first at word {int(diff[0])}"


@pytest.mark.parametrize("path", ["fed", "seg"])
def test_red_zones_at_input_residues(corpus, path):
    """One workgroup per job (it stages every chunk of the job in turn), every length at input & 15 = 0, 1 and 15: nothing may depend on the
    bytes behind input_len, nothing is written outside the output slots."""
    _child("redzone", corpus, "one", 3 * len(LENGTHS), **PATHS[path])


# ---------------------------------------------------------------------------------------------------------------- the children
def _load():
    with open(os.environ["PARSE_STAGING_CORPUS"], "rb") as f:
        return pickle.load(f)


def child_decode(prefix):
    blocks, exp = _load()
    items = [dict(input=b, limit=LIMIT, out_cap=LIMIT + len(b) + 64) for b in blocks]
    res = ffi.decompress_blocks_host(items)
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    assert launch.startswith(prefix), launch
    for b, (erc, eout), (rc, out) in zip(blocks, exp, res):
        assert rc == erc, (len(b), rc, erc)
        assert len(out) == len(eout) and out == eout, len(b)
    print("parse staging ok:", len(items), "jobs", launch)


def child_bitmap(out_path):
    import torch
    from rust_lz_fear_amd import device
    blocks, _ = _load()
    n = len(blocks)
    offs = np.cumsum([0] + [(len(b) + 255) // 256 * 256 + 3 for b in blocks])       # odd alignments
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
    dj["output_limit"] = LIMIT
    d_dj = device.to_device(dj, "cuda")
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    fn = ffi.lib().lzf_debug_seg
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 7 + [C.c_uint64, C.c_void_p]
    geom = np.zeros(4, np.uint32)
    ffi.check(fn(d_dj.data_ptr(), d_res.data_ptr(), n, 1, 1, None, None, None, None, None, None, None, 0, geom.ctypes.data))
    maxch, cw = int(geom[0]), int(geom[2])
    assert cw == CHUNK // 32 and maxch >= max(_nch(len(b)) for b in blocks)
    bits = np.zeros((n, maxch, cw), np.uint32)
    ffi.check(fn(d_dj.data_ptr(), d_res.data_ptr(), n, 1, 2, None, bits.ctypes.data, None, None, None, None, None, 0, geom.ctypes.data))
    np.save(out_path, np.concatenate([bits[i, :_nch(len(b))].ravel() for i, b in enumerate(blocks)]))     # (rows beyond a job's chunks are not written)
    print("parse staging ok: bit map of", n, "jobs")


def child_redzone():
    import redzone
    blocks, exp = _load()
    items, expect, low = [], [], []
    for res in (0, 1, 15):
        for b, e in zip(blocks, exp):
            items.append(dict(input=b, limit=LIMIT, out_cap=len(e[1]) + 64)); expect.append(e); low.append(res)
    redzone.check_decompress(items, expect, label="parse staging", in_low=low)
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    print("parse staging ok:", len(items), "jobs", launch)


if __name__ == "__main__":
    {"decode": child_decode, "bitmap": child_bitmap, "redzone": child_redzone}[sys.argv[1]](*sys.argv[2:])
