"""lzf_seg_parse_kernel's plain-hop loop makes two hops per trip, the second with the two position registers in each other's role, and
lets a lane leave on the vector side alone (lz4_seg_front.hip).  The handcrafted jobs of tests/parse_hop_cases.py — one chunk or
two, 60 jobs in one launch — put every exit of that loop into the first and into the second half of a trip: the stop position and fe
after 1..5 hops, the step back on a 0xFF match-length extension, literal-length extensions 0 / 254 / 255, successors one short of, on and
one beyond end_r and fe, the last two staged bytes, re-walks that merge on their 1st..4th hop or never, 64 regions with 1..6 hops side
by side.  The bit map (lzf_debug_seg, upto = 2) is compared with the true token positions of a plain Python walk, chunk 0 whole and chunk
1 from the first mark that is a true token, and word for word with the model's rows; the same jobs decode through the forced fed path
(whole and in three pieces) and the segmented pipeline to the oracle's statuses, lengths and bytes; and the analysis build whose loop is
the C++ twin (-DLZF_SEG_NOASM) gives the same map word for word.  The children (one per library / path) run side by side."""
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
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import ffi  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = P.all_cases()
NAMES = [n for n, _ in CASES]
PATHS = {"fed": (dict(LZF_DECOMPRESS_KERNEL="fed", LZF_FED_MIN_IN="1", LZF_FED_PIECES="1"), "bitmap-fed"),
         "fed3": (dict(LZF_DECOMPRESS_KERNEL="fed", LZF_FED_MIN_IN="1", LZF_FED_PIECES="3"), "bitmap-fed"),
         "seg": (dict(LZF_DECOMPRESS_KERNEL="seg"), "segmented")}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Everything the device is asked, once: the bit map from the analysis library and from its C++-loop twin, the decodes by path."""
    from rust_lz_fear_amd import build
    d = tmp_path_factory.mktemp("parse_hop")
    blocks = [b for _, b in CASES]
    exp = [o.decompress_raw(b, limit=P.LIMIT, cap=P.LIMIT + len(b) + 64) for b in blocks]
    assert all(e[0] == 0 for e in exp) and len(blocks) <= 64
    corpus = d / "corpus.pkl"
    corpus.write_bytes(pickle.dumps((blocks, exp)))
    libs = {"asm": build.build_analysis_library(), "twin": build.build_library(defines=build.PARSE_TWIN_BUILD)}
    procs = {}
    for key, lib in libs.items():
        e = dict(os.environ, LZF_LIB_PATH=lib, PARSE_STAGING_CORPUS=str(corpus))
        procs["map_" + key] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "bitmap", str(d / f"bits_{key}.npy")], env=e,
                                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    for key, (env, prefix) in PATHS.items():
        e = dict(os.environ, LZF_LIB_PATH=libs["asm"], PARSE_STAGING_CORPUS=str(corpus), **env)
        procs["dec_" + key] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "decode", prefix, str(d / f"dec_{key}.pkl")], env=e,
                                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = {}
    try:
        for key, p in procs.items():
            text, _ = p.communicate(timeout=300)
            out[key] = (p.returncode, text)
    finally:                                             # whatever happened to one child, none is left with the GPU open
        for p in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
    res = {"exp": exp, "out": out}
    offs = np.cumsum([0] + [P.nch(len(b)) for b in blocks])
    for key in libs:
        if out["map_" + key][0] == 0:
            m = np.load(d / f"bits_{key}.npy").reshape(-1, P.CHUNK // 32)
            res["map_" + key] = [m[offs[i]:offs[i + 1]] for i in range(len(blocks))]
    for key in PATHS:
        if out["dec_" + key][0] == 0:
            res["dec_" + key] = pickle.loads((d / f"dec_{key}.pkl").read_bytes())
    return res


def _need(runs, key):
    rc, text = runs["out"][key]
    assert rc == 0 and ("parse hop ok" in text or "parse staging ok" in text), text[-4000:]
    return runs[key]


@pytest.mark.parametrize("case", range(len(CASES)), ids=NAMES)
def test_bit_map_is_the_true_token_positions(runs, case):
    rows = _need(runs, "map_asm")[case]
    blk = CASES[case][1]
    d = P.compare_with_truth(blk, rows)
    assert d is None, f"the map and the plain walk differ at byte {d}"
    want = P.expected_rows(blk)                          # (the kernel's model: also the marks of chunk 1's run-in)
    diff = np.argwhere(rows != want)
    assert diff.size == 0, f"chunk {int(diff[0][0])} word {int(diff[0][1])}: {int(rows[tuple(diff[0])]):#x}, the model has {int(want[tuple(diff[0])]):#x}"


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("case", range(len(CASES)), ids=NAMES)
def test_decodes_like_the_oracle(runs, case, path):
    rc, out = _need(runs, "dec_" + path)[case]
    erc, eout = runs["exp"][case]
    assert rc == erc and len(out) == len(eout) and out == eout


def test_cpp_twin_gives_the_same_bit_maps(runs):
    a, b = _need(runs, "map_asm"), _need(runs, "map_twin")
    for (name, _), ra, rb in zip(CASES, a, b):
        diff = np.argwhere(ra != rb)
        assert diff.size == 0, f"{name}: chunk {int(diff[0][0])} word {int(diff[0][1])}"
    assert any(r.any() for r in a)


# ---------------------------------------------------------------------------------------------------------------- the children
def child_decode(prefix, out_path):
    with open(os.environ["PARSE_STAGING_CORPUS"], "rb") as f:
        blocks, exp = pickle.load(f)
    res = ffi.decompress_blocks_host([dict(input=b, limit=P.LIMIT, out_cap=len(e[1]) + 64) for b, e in zip(blocks, exp)])
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    assert launch.startswith(prefix), launch
    with open(out_path, "wb") as f:
        pickle.dump([(int(rc), bytes(out)) for rc, out in res], f)
    print("parse hop ok:", len(blocks), "jobs", launch)


if __name__ == "__main__":
    if sys.argv[1] == "bitmap":
        import test_gpu_parse_staging as T             # its child reads the map of every chunk of every job through lzf_debug_seg
        T.child_bitmap(sys.argv[2])
    else:
        child_decode(*sys.argv[2:])
