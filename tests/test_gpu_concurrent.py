"""GPU tests (-m gpu) of concurrent callers of the product library: INTEGRATION.md promises that every entry point works on the stream
it is given and returns with its work enqueued there, and that two host threads may call at once.  Every other test of the suite has
one caller with one call in flight; here two calls meet on what the library shares between calls — the segmented pipeline's lanes and
events, the stream-ordered scratch pool, the fed kernel's census, the per-device values filled on first use, the thread-local
diagnostics, the host calls' pinned slab and workers, the frame drivers' waits on the caller's stream.

The work is done by child processes (tests/concurrent_check.py; the kinds and their oracle expectations: tests/concurrent_cases.py,
proven on the CPU by tests/test_concurrent_cases_cpu.py), one at a time, each under a time limit:

  streams     one thread, two caller streams behind a finite device-side gate; results read on the caller's stream alone
  threads     two threads with a stream each, started by a barrier; one pair's first thread fails on the host with LZF_E_INVALID
  mix         four threads: D3, C2, F1, H2
  first-call  the first D4, Z1 and V1 call of a process beside D3 calls of another thread
  census      what the fed kernel's census keeps after such a first call, against an idle process — printed, not asserted

A child that ends by a signal or at its limit fails every test behind it without another child being started.
Measurements: profiles/concurrent_callers.txt."""
import os
import subprocess
import sys
import time

import pytest

import concurrent_cases as K
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import build

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# 5 x the longest child seen on MI355X (profiles/concurrent_callers.txt), and no less than 120 s
LONGEST_CHILD_S = 11.5
LIMIT_S = max(5 * LONGEST_CHILD_S, 120.0)
STREAM_SLICE, THREAD_SLICE = 4, 9
_trouble = []


def _slices(n, size):
    return [(a, min(a + size, n)) for a in range(0, n, size)]


def _child(*args, **env):
    if _trouble:
        pytest.fail(f"not started: an earlier child ended in trouble ({_trouble[0]})")
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "concurrent_check.py"), *args], env=dict(os.environ, **env), capture_output=True,
                           text=True, timeout=LIMIT_S)
    except subprocess.TimeoutExpired as e:
        _trouble.append(f"{' '.join(args)}: no end within {LIMIT_S:.0f} s")
        pytest.fail(_trouble[0] + "\n" + str(e.stdout)[-3000:])
    if r.returncode < 0 or r.returncode in (3, 134, 139):
        _trouble.append(f"{' '.join(args)}: exit status {r.returncode}")
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-6000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "concurrent callers ok", r.stdout[-2000:]
    print("\n".join(ln for ln in lines if ln.startswith(("alone", "gate", "pair", "first", "census", "error pair", "child"))), f"[{time.time() - t0:.1f} s]")
    return lines


@pytest.mark.parametrize("lo,hi", _slices(len(K.stream_pairs()), STREAM_SLICE))
def test_two_streams_behind_a_gate(lo, hi):
    lines = _child("streams", str(lo), str(hi))
    assert sum(ln.startswith("pair ") for ln in lines) == hi - lo


@pytest.mark.parametrize("lo,hi", _slices(len(K.thread_pairs()), THREAD_SLICE))
def test_two_threads(lo, hi):
    lines = _child("threads", str(lo), str(hi))
    assert sum(ln.startswith("pair ") for ln in lines) == hi - lo + (lo == 0)
    assert lo != 0 or any(ln.startswith("error pair") for ln in lines)


def test_four_threads():
    _child("mix")


def test_first_calls_under_contention():
    lines = _child("first-call")
    assert sum(ln.startswith("first call") for ln in lines) == 3


def test_census_after_a_contended_first_call_is_reported():
    """A smaller slot count or a partial XCD mask after contention is a finding (profiles/concurrent_callers.txt), not a
    failure: both children must only run and answer."""
    lib = build.build_analysis_library()
    for what in ("idle", "contended"):
        lines = _child("census", what, LZF_LIB_PATH=lib)
        assert any(ln.startswith(f"census {what}:") for ln in lines)
