"""The deferred flush of the bitmap-fed decompress kernel — a batch written to `out` by the batch behind it, whole 16-byte lines only, and
drained by whatever ends the window loop or by a solo sequence — on the built cases of fed_flush_cases.py, whose reach
test_fed_flush_cases_cpu.py proves without a GPU.  Child processes load the analysis library:

  * the fed kernel ALONE through lzf_debug_fed (no pair kernel behind it) at 1 and 3 pieces: a valid case is finished by the fed kernel
    itself — done set, the oracle's out_len and bytes; a case with an error in the batch behind a good one is left undone with `out`
    holding exactly the oracle's bytes up to the good batch's end and nothing behind them; nothing written around any output slot;
  * the full forced path (LZF_DECOMPRESS_KERNEL=fed, LZF_FED_MIN_IN=1), whole jobs and every job in three pieces: the oracle's status,
    out_len and bytes;
  * the same jobs between poison with every buffer at address residues 0, 1 and 15."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import oracle_ffi as o  # noqa: E402
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import ffi  # noqa: E402
import fed_flush_cases as F  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120      # a child takes 2 .. 4 s, most of it the start of the process (the sibling fed tests' figure)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """The cases with the oracle's answers and the model's good ends, once for the module (the children read the file)."""
    cs = F.corpus()
    for c in cs:
        c["exp"] = o.decompress_raw(c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"], cap=c["cap"])
        assert c["exp"][0] == c["status"], (c["name"], c["exp"][0])
        c["good_end"] = F.model(c)[2]
    path = tmp_path_factory.mktemp("fed_flush") / "corpus.pkl"
    path.write_bytes(pickle.dumps(cs))
    return str(path)


def _child(what, corpus, **env):
    from rust_lz_fear_amd import build
    e = dict(os.environ, FED_FLUSH_CORPUS=corpus)
    for k in ("LZF_DECOMPRESS_KERNEL", "LZF_DECOMPRESS_ORDER", "LZF_FED_MIN_IN", "LZF_FED_PIECES", "LZF_FED_SLOTS", "LZF_FED_CARRY", "LZF_LIB_PATH"):
        e.pop(k, None)
    e.update(env, LZF_LIB_PATH=build.build_analysis_library(), LZF_FED_MIN_IN="1")
    t0 = time.time()
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), what], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        out, err = p.communicate(timeout=CHILD_TIMEOUT)
    finally:
        if p.poll() is None:
            p.kill(); p.communicate()
    for line in out.splitlines():
        if line.startswith("fed flush"):
            print(line)
    print(f"child {what} {env}: {time.time() - t0:.1f} s")
    assert p.returncode == 0, out[-4000:] + err[-4000:]
    assert "fed flush ok" in out, out[-2000:]


@pytest.mark.parametrize("pieces", ["1", "3"])
def test_the_fed_kernel_alone_leaves_out_as_the_oracle_has_it(corpus, pieces):
    _child("alone", corpus, LZF_FED_PIECES=pieces)


@pytest.mark.parametrize("pieces", ["1", "3"])
def test_full_path_equals_the_oracle(corpus, pieces):
    _child("full", corpus, LZF_DECOMPRESS_KERNEL="fed", LZF_FED_PIECES=pieces)


def test_in_red_zones_at_residues_0_1_15(corpus):
    _child("redzone", corpus, LZF_DECOMPRESS_KERNEL="fed", LZF_FED_PIECES="3")


# ---------------------------------------------------------------------------------------------------------------- the children
def _load():
    with open(os.environ["FED_FLUSH_CORPUS"], "rb") as f:
        return pickle.load(f)


def _items(cases):
    return [dict(input=c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"], out_cap=c["cap"]) for c in cases]


def _report(msgs):
    for m in msgs[:40]:
        print(m)
    assert not msgs, f"{len(msgs)} differences"


def child_full():
    cases = _load()
    res = ffi.decompress_blocks_host(_items(cases))
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    assert launch.startswith("bitmap-fed"), launch
    msgs = []
    for c, (rc, out) in zip(cases, res):
        erc, eout = c["exp"]
        if rc != erc:
            msgs.append(f"[{c['name']}] status {rc}, the oracle's {erc}")
        elif rc == 0 and out != eout:
            bad = [i for i in range(min(len(out), len(eout))) if out[i] != eout[i]]
            msgs.append(f"[{c['name']}] out_len {len(out)} (oracle {len(eout)}), {len(bad)} bytes differ, first at {bad[0] if bad else None}")
    _report(msgs)
    print(f"fed flush ok: full path, {len(cases)} jobs, {launch}")


def child_alone():
    import test_gpu_fed_pieces as P
    cases = _load()
    while len(cases) < P.MIN_JOBS:      # (a call of fewer jobs is not cut into pieces)
        cases = cases + [dict(c, name=c["name"] + " (again)") for c in cases[:P.MIN_JOBS - len(cases)]]
    pl = P.Placed(cases, list(range(len(cases))))
    d = pl.run(0)
    print(f"fed flush: geometry {d['geom']}, call {d['ms']:.1f} ms")
    msgs, fin, left = [], 0, 0
    for i, c in enumerate(cases):
        say = lambda text: msgs.append(f"[{c['name']}] {text}")      # noqa: E731
        s, q, out = d["st"][i], int(pl.out_off[i]), d["out"]
        erc, eout = c["exp"]
        untouched = (d["res_raw"][i] == P.SENTINEL).all()
        if not s["eligible"] or s["failed"]:
            say(f"eligible {s['eligible']}, failed {s['failed']}"); continue
        if erc == 0:
            r = d["res"][i]
            if not s["done"] or int(r["status"]) != 0 or int(r["out_len"]) != len(eout):
                say(f"not finished by the fed kernel: done {s['done']}, result {'untouched' if untouched else (int(r['status']), int(r['out_len']))} (oracle out_len {len(eout)})")
                continue
            end = len(eout)
            fin += 1
        else:
            if s["done"] or not untouched:
                say(f"a job the oracle rejects ({erc}): done {s['done']}, result {'untouched' if untouched else d['res'][i]}")
            end = c["good_end"]      # what the batches in front of the failing one produced: all of it in `out`, nothing of the failing batch
            left += 1
        if out[q:q + end].tobytes() != eout[:end]:
            bad = np.nonzero(out[q:q + end] != np.frombuffer(eout[:end], np.uint8))[0]
            say(f"output differs at {len(bad)} of the first {end} bytes, first {int(bad[0])}, last {int(bad[-1])} (existing {len(c['existing'])})")
        if (out[q + end:q + max(c["cap"], end)] != P.POISON).any():
            say(f"bytes behind position {end} were written")
        if (out[q - P.GUARD:q] != P.POISON).any():
            say("bytes in front of the output slot were written")
        if (out[q + c["cap"]:q + c["cap"] + P.GUARD] != P.POISON).any():
            say("bytes behind the output slot were written")
    _report(msgs)
    assert left >= 9 and fin + left == len(cases)
    print(f"fed flush ok: the fed kernel alone, {len(cases)} jobs: {fin} finished by it, {left} left with the good batches in out")


def child_redzone():
    import redzone
    cases = _load()
    items, exp = _items(cases), [c["exp"] for c in cases]
    for low in (0, 1, 15):
        n = len(items)
        redzone.check_decompress(items, exp, f"fed flush, every buffer & 15 = {low}", max_input_len=max(len(it["input"]) for it in items),
                                 in_low=[low] * n, prefix_low=[low] * n, out_low=[low] * n)
        launch = ffi.lib().lzf_last_decompress_launch().decode()
        assert launch.startswith("bitmap-fed"), launch
    print(f"fed flush ok: red zones, {len(items)} jobs at residues 0, 1, 15, {launch}")


if __name__ == "__main__":
    {"full": child_full, "alone": child_alone, "redzone": child_redzone}[sys.argv[1]]()
