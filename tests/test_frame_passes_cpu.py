"""CPU test (no GPU) of the frame layer's one pass planner, lzf_frame_jobs::split_passes (rust-lz-fear_amd/csrc/frame_jobs.h),
compiled here with g++: the four *_many drivers cut their frames into passes of the memory budget with it.  Held to a Python
restatement of the greedy rule: groups are taken while the running sum stays within the budget, the first group of a pass is
always taken."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("passes") / "libemu_frame_passes.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(HERE, "emu", "emu_frame_passes.cpp")])
    L = C.CDLL(so)
    L.lzf_emu_split_passes.restype = C.c_uint32
    L.lzf_emu_split_passes.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32]

    def run(need, budget, group_end=None):
        n = len(need)
        arr = (C.c_uint64 * max(n, 1))(*need)
        ge = (C.c_uint32 * max(n, 1))(*group_end) if group_end is not None else None
        out = (C.c_uint32 * (2 * (n + 1)))()
        k = L.lzf_emu_split_passes(arr, n, budget, ge, out, n + 1)
        assert k <= n + 1
        return [(out[2 * i], out[2 * i + 1]) for i in range(k)]
    return run


def group_ends(sizes):
    """group_end[f] for consecutive groups of the given sizes."""
    out, at = [], 0
    for g in sizes:
        at += g
        out += [at] * g
    return out


def py_split(need, budget, group_end=None):
    """The greedy rule, restated: whole groups while the sum stays within the budget; the first group of a pass always."""
    n, passes, f0 = len(need), [], 0
    while f0 < n:
        f1, total = f0, 0
        while f1 < n:
            e = group_end[f1] if group_end is not None else f1 + 1
            add = sum(need[f1:e])
            if f1 != f0 and total + add > budget:
                break
            total += add; f1 = e
        passes.append((f0, f1))
        f0 = f1
    return passes


def check(split, need, budget, group_end=None):
    got = split(need, budget, group_end)
    assert got == py_split(need, budget, group_end), (need, budget, group_end)
    # the passes tile [0, n) in order
    at = 0
    for a, b in got:
        assert a == at and b > a
        at = b
    assert at == len(need)
    # whole groups only, and no pass of more than one group exceeds the budget
    ge = group_end if group_end is not None else list(range(1, len(need) + 1))
    for a, b in got:
        assert a == 0 or ge[a - 1] == a
        assert ge[b - 1] == b
        if ge[a] != b:
            assert sum(need[a:b]) <= budget, (need, budget, group_end, (a, b))
    return got


B = 1000
CASES = [
    ("empty", [], B, []),
    ("all zeros", [0] * 7, B, [(0, 7)]),
    ("all zeros, no budget", [0] * 7, 0, [(0, 7)]),
    ("every frame exactly at the budget", [B] * 4, B, [(0, 1), (1, 2), (2, 3), (3, 4)]),
    ("one frame over the budget first", [B + 1, 10, 10], B, [(0, 1), (1, 3)]),
    ("one frame over the budget in the middle", [10, B + 1, 10], B, [(0, 1), (1, 2), (2, 3)]),
    ("one frame over the budget last", [10, 10, B + 1], B, [(0, 2), (2, 3)]),
    ("a sum exactly on the budget", [400, 350, 250, 1], B, [(0, 3), (3, 4)]),
    ("a sum one byte over the budget", [400, 350, 251, 1], B, [(0, 2), (2, 4)]),
    ("one frame, alone and over", [5 * B], B, [(0, 1)]),
]


@pytest.mark.parametrize("name,need,budget,want", CASES, ids=[c[0] for c in CASES])
def test_split_passes_cases(split, name, need, budget, want):
    assert check(split, need, budget) == want
    # group_end == nullptr gives the passes of singleton groups
    assert check(split, need, budget, group_ends([1] * len(need))) == want


def test_split_passes_groups(split):
    """Groups of 1, 3 and 1 where the middle group alone exceeds the budget: it is a pass of its own, whole."""
    ge = group_ends([1, 3, 1])
    assert check(split, [10, 400, 400, 400, 10], B, ge) == [(0, 1), (1, 4), (4, 5)]
    assert check(split, [10, 300, 300, 300, 10], B, ge) == [(0, 5)]                 # (the same groups within the budget: one pass)
    assert check(split, [200, 300, 300, 300, 10], B, ge) == [(0, 1), (1, 5)]        # whole groups: 200 + 900 does not fit, 900 + 10 does
    assert check(split, [10, 400, 400, 400, 10], B) == [(0, 3), (3, 5)]             # without groups the same frames split inside the group


def test_split_passes_sweep(split):
    """Every list of up to 5 needs from a small alphabet, with every grouping into runs of 1-3, against the restatement."""
    import itertools
    alphabet = (0, 1, 499, 500, 501, 1000, 1001)
    checked = 0
    for n in range(0, 6):
        groupings = [g for k in range(n + 1) for g in itertools.product((1, 2, 3), repeat=k) if sum(g) == n]
        for need in itertools.product(alphabet, repeat=n):
            if n == 5 and need[0] not in (0, 500, 1001):
                continue
            check(split, list(need), B)
            for g in groupings:
                check(split, list(need), B, group_ends(g))
                checked += 1
    assert checked > 20000
