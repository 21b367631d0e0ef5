"""The near overlapping matches that the fed kernel's wavefront moves byte by byte — without a division where the offset is a power of two
(1, 2, 4, 8: the periods that divide 8, and 16), with the two divisions for every other offset — on the built cases of
fed_periodic_cases.py, whose reach test_fed_periodic_cases_cpu.py proves without a GPU.  Child processes load the analysis library:

  * the fed kernel ALONE through lzf_debug_fed (no pair kernel behind it) at 1 and 3 pieces: every case is finished by the fed kernel
    itself — done set, the oracle's out_len and bytes, nothing written around the output slot (each case at its own output residue);
  * the full forced path (LZF_DECOMPRESS_KERNEL=fed, LZF_FED_MIN_IN=1), whole jobs and every job in three pieces: the oracle's status, out_len and bytes;
  * the same jobs between poison with every buffer at address residues 0, 1 and 15;
  * the counter build (build.FED_PERIODIC_COUNTER_BUILD): per case, the matches moved without a division equal the host model's."""
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
import fed_periodic_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120      # a child takes 2 .. 4 s, most of it the start of the process (the sibling fed tests' figure)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """The cases with the oracle's answers and the model's counts, once for the module (the children read the file)."""
    cs = K.corpus()
    for c in cs:
        c["exp"] = o.decompress_raw(c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"], cap=c["cap"])
        assert c["exp"][0] == c["status"] == 0, (c["name"], c["exp"][0])
        c["masked"] = K.masked_moves(c)
    path = tmp_path_factory.mktemp("fed_periodic") / "corpus.pkl"
    path.write_bytes(pickle.dumps(cs))
    return str(path)


def _child(what, corpus, lib=None, **env):
    from rust_lz_fear_amd import build
    e = dict(os.environ, FED_PERIODIC_CORPUS=corpus)
    for k in ("LZF_DECOMPRESS_KERNEL", "LZF_DECOMPRESS_ORDER", "LZF_FED_MIN_IN", "LZF_FED_PIECES", "LZF_FED_SLOTS", "LZF_FED_CARRY", "LZF_LIB_PATH"):
        e.pop(k, None)
    e.update(env, LZF_LIB_PATH=lib or build.build_analysis_library(), LZF_FED_MIN_IN="1")
    t0 = time.time()
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), what], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        out, err = p.communicate(timeout=CHILD_TIMEOUT)
    finally:
        if p.poll() is None:
            p.kill(); p.communicate()
    for line in out.splitlines():
        if line.startswith("fed periodic"):
            print(line)
    print(f"child {what} {env}: {time.time() - t0:.1f} s")
    assert p.returncode == 0, out[-4000:] + err[-4000:]
    assert "fed periodic ok" in out, out[-2000:]


@pytest.mark.parametrize("pieces", ["1", "3"])
def test_the_fed_kernel_itself_finishes_every_case(corpus, pieces):
    _child("alone", corpus, LZF_FED_PIECES=pieces)


@pytest.mark.parametrize("pieces", ["1", "3"])
def test_full_path_equals_the_oracle(corpus, pieces):
    _child("full", corpus, LZF_DECOMPRESS_KERNEL="fed", LZF_FED_PIECES=pieces)


def test_in_red_zones_at_residues_0_1_15(corpus):
    _child("redzone", corpus, LZF_DECOMPRESS_KERNEL="fed", LZF_FED_PIECES="3")


def test_moves_without_a_division_equal_the_models(corpus):
    from rust_lz_fear_amd import build
    _child("count", corpus, lib=build.build_library(defines=build.FED_PERIODIC_COUNTER_BUILD), LZF_FED_PIECES="1")


# ---------------------------------------------------------------------------------------------------------------- the children
def _load():
    with open(os.environ["FED_PERIODIC_CORPUS"], "rb") as f:
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
        elif out != eout:
            bad = [i for i in range(min(len(out), len(eout))) if out[i] != eout[i]]
            msgs.append(f"[{c['name']}] out_len {len(out)} (oracle {len(eout)}), {len(bad)} bytes differ, first at {bad[0] if bad else None}")
    _report(msgs)
    print(f"fed periodic ok: full path, {len(cases)} jobs, {launch}")


def _alone(cases):
    """One call of the fed kernel alone over all cases; every case finished by it with the oracle's bytes -> the host copies."""
    import test_gpu_fed_pieces as P
    which = list(range(len(cases)))
    assert len(which) >= P.MIN_JOBS
    pl = P.Placed(cases, which)
    d = pl.run(0)
    print(f"fed periodic: geometry {d['geom']}, call {d['ms']:.1f} ms")
    msgs = []
    for i, c in enumerate(cases):
        say = lambda text: msgs.append(f"[{c['name']}] {text}")      # noqa: E731
        s, q, out = d["st"][i], int(pl.out_off[i]), d["out"]
        eout = c["exp"][1]
        r = d["res"][i]
        if not s["eligible"] or s["failed"]:
            say(f"eligible {s['eligible']}, failed {s['failed']}"); continue
        if not s["done"] or int(r["status"]) != 0 or int(r["out_len"]) != len(eout):
            untouched = (d["res_raw"][i] == P.SENTINEL).all()
            say(f"not finished by the fed kernel: done {s['done']}, result {'untouched' if untouched else (int(r['status']), int(r['out_len']))} (oracle out_len {len(eout)})")
            continue
        if out[q:q + len(eout)].tobytes() != eout:
            bad = np.nonzero(out[q:q + len(eout)] != np.frombuffer(eout, np.uint8))[0]
            say(f"output differs at {len(bad)} bytes, first {int(bad[0])} (existing {len(c['existing'])})")
        if (out[q + len(eout):q + c["cap"]] != P.POISON).any():
            say("bytes behind out_len were written")
        if (out[q - P.GUARD:q] != P.POISON).any():
            say("bytes in front of the output slot were written")
        if (out[q + c["cap"]:q + c["cap"] + P.GUARD] != P.POISON).any():
            say("bytes behind the output slot were written")
    _report(msgs)
    return d


def child_alone():
    cases = _load()
    _alone(cases)
    print(f"fed periodic ok: the fed kernel alone finished all {len(cases)} jobs")


def child_count():
    cases = _load()
    d = _alone(cases)
    msgs = [f"[{c['name']}] {int(d['res'][i]['reserved'])} moves without a division, the model's {c['masked']}"
            for i, c in enumerate(cases) if int(d["res"][i]["reserved"]) != c["masked"]]
    _report(msgs)
    total = sum(c["masked"] for c in cases)
    assert total >= 300
    print(f"fed periodic ok: {total} moves without a division over {len(cases)} jobs, each job's count the model's")


def child_redzone():
    import redzone
    cases = _load()
    items, exp = _items(cases), [c["exp"] for c in cases]
    for low in (0, 1, 15):
        n = len(items)
        redzone.check_decompress(items, exp, f"fed periodic, every buffer & 15 = {low}", max_input_len=max(len(it["input"]) for it in items),
                                 in_low=[low] * n, prefix_low=[low] * n, out_low=[low] * n)
        launch = ffi.lib().lzf_last_decompress_launch().decode()
        assert launch.startswith("bitmap-fed"), launch
    print(f"fed periodic ok: red zones, {len(items)} jobs at residues 0, 1, 15, {launch}")


if __name__ == "__main__":
    {"full": child_full, "alone": child_alone, "count": child_count, "redzone": child_redzone}[sys.argv[1]]()
