"""The set-up of a batch in the bitmap-fed decompress kernel (one read for a token's offset and match-length byte, the batch's bounds
tested once, both offset errors in one compare, the exact status worked out only when something is flagged) on the built cases of
fed_setup_cases.py, whose reach test_fed_setup_cases_cpu.py proves without a GPU.  Child processes load the analysis library:

  * the full path (LZF_DECOMPRESS_KERNEL=fed, LZF_FED_MIN_IN=1; whole jobs and every job in three pieces): every case's status, out_len and
    bytes equal the oracle's;
  * the fed kernel ALONE through lzf_debug_fed (no pair kernel behind it, as tests/test_gpu_fed_pieces.py runs it): every case the oracle
    decodes is finished by the fed kernel itself — done set, the oracle's out_len and bytes — and every case the oracle rejects is left
    !done with its result untouched.  The pair kernel decodes again whatever the fed kernel gives up, so final bytes cannot show a fast
    test that flags valid batches; this can.
The pair kernel is not run on the cases: the uniform test stands under LZF_FED_DECODE only, the pair and batched kernels are instruction
for instruction what they were."""
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
import fed_setup_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120      # a child takes 2 .. 4 s, most of it the start of the process (the sibling fed tests' figure)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """The cases with the oracle's answers, once for the module (the children read the file)."""
    cs = K.corpus(lambda blk: o.decompress_raw(blk, limit=1 << 22, cap=1 << 16)[1])
    for c in cs:
        c["exp"] = o.decompress_raw(c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"], cap=c["cap"])
        assert c["exp"][0] == c["status"], (c["name"], c["exp"][0])
    path = tmp_path_factory.mktemp("fed_setup") / "corpus.pkl"
    path.write_bytes(pickle.dumps(cs))
    return str(path)


def _child(what, corpus, **env):
    from rust_lz_fear_amd import build
    e = dict(os.environ, FED_SETUP_CORPUS=corpus)
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
        if line.startswith("fed setup"):
            print(line)
    print(f"child {what} {env}: {time.time() - t0:.1f} s")
    assert p.returncode == 0, out[-4000:] + err[-4000:]
    assert "fed setup ok" in out, out[-2000:]


@pytest.mark.parametrize("pieces", ["1", "3"])
def test_full_path_equals_the_oracle(corpus, pieces):
    _child("full", corpus, LZF_DECOMPRESS_KERNEL="fed", LZF_FED_PIECES=pieces)


@pytest.mark.parametrize("pieces", ["1", "3"])
def test_the_fed_kernel_itself_finishes_what_the_oracle_decodes(corpus, pieces):
    _child("alone", corpus, LZF_FED_PIECES=pieces)


# ---------------------------------------------------------------------------------------------------------------- the children
def _load():
    with open(os.environ["FED_SETUP_CORPUS"], "rb") as f:
        return pickle.load(f)


def child_full():
    cases = _load()
    items = [dict(input=c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"], out_cap=c["cap"]) for c in cases]
    res = ffi.decompress_blocks_host(items)
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    assert launch.startswith("bitmap-fed"), launch
    msgs = []
    for c, (rc, out) in zip(cases, res):
        erc, eout = c["exp"]
        if rc != erc:
            msgs.append(f"[{c['name']}] status {rc}, the oracle's {erc}")
        elif rc == 0 and out != eout:
            msgs.append(f"[{c['name']}] out_len {len(out)} (oracle {len(eout)}){'' if len(out) != len(eout) else ', bytes differ'}")
    for m in msgs[:40]:
        print(m)
    assert not msgs, f"{len(msgs)} differences"
    print(f"fed setup ok: full path, {len(items)} jobs, {launch}")


def child_alone():
    import test_gpu_fed_pieces as P
    cases = _load()
    which = list(range(len(cases)))
    assert len(which) >= P.MIN_JOBS
    pl = P.Placed(cases, which)
    d = pl.run(0)
    print(f"fed setup: geometry {d['geom']}, call {d['ms']:.1f} ms")
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
                say(f"a valid job the fed kernel did not finish: done {s['done']}, result {'untouched' if untouched else (int(r['status']), int(r['out_len']))} (oracle out_len {len(eout)})")
                continue
            if out[q:q + len(eout)].tobytes() != eout:
                bad = np.nonzero(out[q:q + len(eout)] != np.frombuffer(eout, np.uint8))[0]
                say(f"output differs at {len(bad)} bytes, first {int(bad[0])}")
            if (out[q + len(eout):q + c["cap"]] != P.POISON).any():
                say("bytes behind out_len were written")
            fin += 1
        else:
            if s["done"] or not untouched:
                say(f"a job the oracle rejects ({erc}): done {s['done']}, result {'untouched' if untouched else d['res'][i]}")
            left += 1
        if (out[q - P.GUARD:q] != P.POISON).any():
            say("bytes in front of the output slot were written")
        if (out[q + c["cap"]:q + c["cap"] + P.GUARD] != P.POISON).any():
            say("bytes behind the output slot were written")
    for m in msgs[:40]:
        print(m)
    assert not msgs, f"{len(msgs)} differences"
    assert fin == sum(c["exp"][0] == 0 for c in cases) and left == len(cases) - fin and left >= 20
    print(f"fed setup ok: the fed kernel alone, {len(cases)} jobs: {fin} finished by it, {left} left for the pair kernel")


if __name__ == "__main__":
    {"full": child_full, "alone": child_alone}[sys.argv[1]]()
