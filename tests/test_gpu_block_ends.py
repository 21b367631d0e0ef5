"""GPU tests (-m gpu) of the way a block ENDS, in every decoder: tests/block_end_cases.py's jobs — blocks cut at every byte, the cuts
placed at the chunk, tile and window boundaries of the kernels, the dropped byte, the order of precedence at the end — whose reach
tests/test_block_end_cases_cpu.py proves on the oracle alone.  One child process per setting (tests/block_end_check.py; the analysis
library's knobs are read once per process); every child reports how many cases it compared and that number is asserted here: nothing
skipped, nothing filtered out.  Expectations are the oracle's throughout."""
import os
import pickle
import re
import subprocess
import sys
import time

import pytest

import block_end_cases as B

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = ("LZF_DECOMPRESS_KERNEL", "LZF_SEG_MIN_IN", "LZF_SEG_RING", "LZF_SEG_FORCE", "LZF_FED_MIN_IN", "LZF_FED_PIECES", "LZF_FED_SLOTS", "LZF_FED_CARRY",
         "LZF_DECOMPRESS_ORDER", "LZF_SIZE_SEG", "LZF_SIZE_SEG_MIN_IN", "LZF_SIZE_FORCE", "LZF_VERIFY_SEG", "LZF_FAKE_CU", "LZF_LIB_PATH")
FED = dict(LZF_DECOMPRESS_KERNEL="fed", LZF_FED_MIN_IN="1")
CLASS = dict(LZF_SIZE_SEG="force", LZF_SIZE_SEG_MIN_IN="0")

DECODE = {name: dict(LZF_DECOMPRESS_KERNEL=name) for name in ("wave", "staged16", "staged32", "direct4w", "paired16", "paired24", "paired48", "paired256")}
DECODE.update({"seg": dict(LZF_DECOMPRESS_KERNEL="seg", LZF_SEG_MIN_IN="0"), "fed, whole jobs": dict(FED, LZF_FED_PIECES="1"),
               "fed, 3 pieces": dict(FED, LZF_FED_PIECES="3"), "product": None})
SIZE = {"size, one-wave kernel": dict(LZF_SIZE_SEG="off"), "size, class forced": CLASS, "size, class alone": dict(CLASS, LZF_SIZE_FORCE="2")}
VERIFY = {"verify, one-wave kernel": dict(LZF_VERIFY_SEG="off"), "verify, class forced": dict(LZF_VERIFY_SEG="force", LZF_SIZE_SEG_MIN_IN="0")}
WHO = {"pipeline alone": ("who_seg", dict(LZF_DECOMPRESS_KERNEL="seg", LZF_SEG_MIN_IN="0")), "fed kernel alone, whole jobs": ("who_fed", dict(FED, LZF_FED_PIECES="1")),
       "fed kernel alone, 3 pieces": ("who_fed", dict(FED, LZF_FED_PIECES="3"))}


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """The jobs and the oracle's answers, once for the module (the children read the file)."""
    blocks, jobs = B.decode_jobs()
    vjobs = B.verify_jobs(jobs)
    assert (len(jobs), len(B.carved(jobs)), len(vjobs)) == (B.COUNTS["all"], B.COUNTS["carved"], B.COUNTS["verify"])
    path = tmp_path_factory.mktemp("block_ends") / "corpus.pkl"
    path.write_bytes(pickle.dumps((blocks, jobs, vjobs)))
    return str(path)


def _child(what, label, env, corpus, count):
    from rust_lz_fear_amd import build
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e["BLOCK_ENDS_CORPUS"] = corpus
    if env is not None:                                        # (None: the product library, no knob)
        e.update(env, LZF_LIB_PATH=build.build_analysis_library())
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(HERE, "block_end_check.py"), what, label], env=e, capture_output=True, text=True, timeout=300)
    print(f"{label}: {time.time() - t0:.1f} s")
    print("\n".join(r.stdout.strip().splitlines()[-3:]))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-4000:]
    m = re.search(r"^%s ok: (\d+) cases$" % re.escape(label), r.stdout, re.M)
    assert m and int(m.group(1)) == count, r.stdout[-2000:]


@pytest.mark.parametrize("setting", list(DECODE))
def test_every_decoder_ends_a_block_as_the_reference_does(corpus, setting):
    _child("decode", setting, DECODE[setting], corpus, B.COUNTS["all"] + B.COUNTS["carved"])


@pytest.mark.parametrize("setting", list(SIZE))
def test_the_size_call(corpus, setting):
    _child("size", setting, SIZE[setting], corpus, B.COUNTS["all"])


@pytest.mark.parametrize("setting", list(VERIFY))
def test_the_verify_call(corpus, setting):
    _child("verify", setting, VERIFY[setting], corpus, B.COUNTS["verify"])


@pytest.mark.parametrize("setting", list(WHO))
def test_who_answered(corpus, setting):
    what, env = WHO[setting]
    _child(what, setting, env, corpus, B.COUNTS["all"])
