"""The windows of the bitmap-fed decompress kernel on the GPU: windows that start where the chain stands and take every bit-map word
from the chunk that owns it, the marks below the chain's position masked off (no seam stage on this path), a window the map gets
wrong walked token by token, a short last batch left for the next window (rust-lz-fear_amd/csrc/lzf_fed_window.h).  The handcrafted
blocks of tests/fed_window_cases.py — each asserts, on the CPU, the shape it is there for — go through the fed kernel forced for every
input (analysis library, LZF_DECOMPRESS_KERNEL=fed, LZF_FED_MIN_IN=1), whole jobs and every job in 3 and 16 pieces.  Statuses,
out_len and bytes are compared with the oracle (src/raw/decompress.rs); the same jobs go once through the red-zone harness with the
inputs at address residues 0, 1 and 15."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import oracle_ffi as o  # noqa: E402
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import ffi  # noqa: E402
from test_gpu_fed_decode_once import _block, _walk  # noqa: E402,F401  (the blocks' sequence encoder and token walk, shared with fed_window_cases)
import fed_window_cases as fw  # noqa: E402

pytestmark = pytest.mark.gpu

LIMIT = fw.LIMIT


def _items():
    valid, bad = fw.cases(), fw.damaged()
    items, exp, names = [], [], []
    for name, blk in valid + bad:
        cap = LIMIT + len(blk) + 64
        items.append(dict(input=blk, limit=LIMIT, out_cap=cap)); exp.append(o.decompress_raw(blk, limit=LIMIT, cap=cap)); names.append(name)
    assert all(e[0] == 0 for e in exp[:len(valid)]) and sum(e[0] != 0 for e in exp[len(valid):]) == len(bad) // 2
    # exact-fit and one-byte-short capacity of a block with carried tails and of one that is walked
    for k in (1, 6):
        blk, out = valid[k][1], exp[k][1]
        for cap in (len(out), len(out) - 1):
            items.append(dict(input=blk, limit=len(out), out_cap=cap)); exp.append(o.decompress_raw(blk, limit=len(out), cap=cap))
            names.append(f"{valid[k][0]} cap {cap}")
    return items, exp, names


def child(mode):
    items, exp, names = _items()
    if mode == "plain":
        res = ffi.decompress_blocks_host(items)
        launch = ffi.lib().lzf_last_decompress_launch().decode()
        assert launch.startswith("bitmap-fed"), launch
        for name, (erc, eout), (rc, out) in zip(names, exp, res):
            assert rc == erc, (name, rc, erc)
            if rc == 0:
                assert out == eout, name
    else:
        import redzone
        for low in (0, 1, 15):
            redzone.check_decompress(items, exp, f"fed windows, input & 15 = {low}", max_input_len=max(len(it["input"]) for it in items),
                                     in_low=[low] * len(items))
            launch = ffi.lib().lzf_last_decompress_launch().decode()
            assert launch.startswith("bitmap-fed"), launch
    print("fed windows ok:", mode, len(items), "jobs", launch)


def _run(mode, pieces):
    from rust_lz_fear_amd import build
    env = dict(os.environ, LZF_LIB_PATH=build.build_analysis_library(), LZF_DECOMPRESS_KERNEL="fed", LZF_FED_MIN_IN="1",
               LZF_FED_PIECES=pieces)
    env.pop("LZF_FED_CARRY", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", mode], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "fed windows ok" in r.stdout


@pytest.mark.parametrize("pieces", ["1", "3", "16"])
def test_fed_windows(pieces):
    """Chunks that do not fall in step, a run over a whole chunk, tails of every kind, damage behind a good window: the oracle's
    statuses and bytes."""
    _run("plain", pieces)


def test_fed_windows_in_red_zones():
    """The same jobs between poison, inputs at residues 0, 1 and 15: nothing read behind input_len matters, nothing written outside
    the output slots."""
    _run("redzone", "3")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "child":
        child(sys.argv[2])
