"""CPU test (no GPU) of the call kinds of the concurrent-caller tests (tests/concurrent_cases.py): every expectation the device
test (tests/test_gpu_concurrent.py) holds the library to is the oracle's, every raw batch kind reaches the class it is named for on an
MI355X geometry under the dispatch rules (the emulated plans of lzf_dispatch.h that tests/test_dispatch_cpu.py, test_size_tiles_cpu.py
and test_verify_cases_cpu.py drive), the launch strings are the header's, and two seeds of a kind are two different calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import concurrent_cases as K
import oracle_ffi as o

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-lz-fear_amd", "csrc")
CU, LDS = 256, 163840                        # MI355X
ANY = 0xFFFFFFFFFFFFFFFF
SEEDS = (0, 1)
ALL = [(k, s) for k in K.KINDS for s in SEEDS]


def _ids(v):
    return f"{v[0]}-seed{v[1]}" if isinstance(v, tuple) else None


def _oracle_decode(case, j):
    return o.decompress_raw(case["inputs"][j["inp"]], prefix=j["prefix"], existing=j["existing"], limit=j["limit"],
                            cap=j["limit"] + len(case["inputs"][j["inp"]]) + 64)


# ------------------------------------------------------------------------------------------------------------- 1. expectations
@pytest.mark.parametrize("ks", [(k, s) for k in ("D1", "D2", "D3", "D4") for s in SEEDS], ids=_ids)
def test_decode_expectations(ks):
    case = K.build(*ks)
    seen = {}
    for j, (st, p) in zip(case["jobs"], case["expect"]):
        key = (j["inp"], j["prefix"], j["existing"], j["limit"])
        if key not in seen:                                       # (D4: thousands of jobs over half a dozen inputs)
            seen[key] = _oracle_decode(case, j)
        assert seen[key] == (st, case["plains"][p])
        assert j["cap"] >= j["limit"] + len(case["inputs"][j["inp"]]) and j["limit"] == len(case["plains"][p])
    if ks[0] in ("D1", "D2"):
        hist = [j for j in case["jobs"] if j["prefix"]]
        assert len(hist) == 2 and all(j["existing"] for j in hist)
        for j in hist:                                            # the block really refers to its history: without it, another answer
            assert o.decompress_raw(case["inputs"][j["inp"]], limit=j["limit"])[0] != 0


@pytest.mark.parametrize("ks", [(k, s) for k in ("Z1", "Z2", "V1", "V2") for s in SEEDS], ids=_ids)
def test_size_and_verify_expectations(ks):
    case = K.build(*ks)
    seen = {}
    for k, (j, (st, ln)) in enumerate(zip(case["jobs"], case["expect"])):
        if j["inp"] not in seen:                                  # (V1: hundreds of jobs over 16 blocks)
            seen[j["inp"]] = _oracle_decode(case, j)
        rc, out = seen[j["inp"]]
        assert j == case["jobs"][j["inp"]]
        if case["family"] == "size":
            assert (rc, len(out) if rc == 0 else None) == (st, ln), k
            continue
        want, ex = case["outs"][j["inp"]], len(j["existing"])
        assert j["cap"] == len(want) and want[:ex] == j["existing"]
        if rc != 0:
            assert (st, ln) == (rc, None), k                      # a malformed block is malformed first
        elif out == want:
            assert (st, ln) == (0, len(out)), k
        else:
            assert len(out) == len(want) and st == K.MISMATCH, k
            first = next(p for p in range(ex, len(out)) if out[p] != want[p])
            assert ln == first == ex + K.mismatch_at(len(out) - ex, ks[1]), k
    assert {st for st, _ in case["expect"]} >= {0, 1, 2, 3, 4}
    if case["family"] == "verify":
        assert [st for st, _ in case["expect"][:len(case["inputs"])]].count(K.MISMATCH) == 1


@pytest.mark.parametrize("ks", [(k, s) for k in ("C1", "C2", "C3", "C4") for s in SEEDS], ids=_ids)
def test_compress_expectations(ks):
    case = K.build(*ks)
    seen = set()
    for k, (j, (st, c), tab) in enumerate(zip(case["jobs"], case["expect"], case["tables_after"])):
        key = (id(j["input"]), j["cap"], st, c if c is None or isinstance(c, int) else id(c))
        if j["table"] is None and key in seen:                    # (C2: thousands of jobs over a few hundred blocks)
            continue
        seen.add(key)
        t = o.new_table(j["kind"])
        if j["table"] is not None:
            memoryview(t).cast("B")[:] = j["table"]
        rc, out = o.compress2(j["input"], cursor=j["cursor"], kind=j["kind"], table=t, cap=min(j["cap"], 1 << 20))
        assert rc == st, k
        if case["family"] == "csize":
            assert c == (len(out) if rc == 0 else None), k
        elif rc == 0:
            assert out == c, k
            # what it compresses to decodes to the input behind the cursor, with what lies in front of the cursor as the prefix
            assert o.decompress_raw(c, prefix=j["input"][:j["cursor"]], limit=len(j["input"])) == (0, j["input"][j["cursor"]:]), k
        assert (tab is None) == (j["table"] is None)
        if tab is not None:
            assert tab == bytes(memoryview(t).cast("B")) and tab != j["table"], k
    if ks[0] == "C3":
        kinds = [j["kind"] for j in case["jobs"]]
        assert kinds.count(K.TABLE_U32) == 4 and kinds.count(K.TABLE_U16) == len(kinds) - 4
        assert all(len(j["input"]) <= 65535 for j in case["jobs"] if j["kind"] == K.TABLE_U16)
        assert all(j["table"] is not None and j["cursor"] > 0 for j in case["jobs"] if j["kind"] == K.TABLE_U32)
    if ks[0] == "C4":
        assert [st for st, _ in case["expect"]].count(o.OUTPUT_FULL) == 2 and case["expect"][1][0] == case["expect"][9][0] == o.OUTPUT_FULL
        assert [j["input"] for j in case["jobs"]] == [j["input"] for j in K.build("C2", ks[1])["jobs"]]
    if ks[0] == "C1":
        assert all(64 * K.KIB <= len(j["input"]) <= 256 * K.KIB + 64 for j in case["jobs"])


@pytest.mark.parametrize("seed", SEEDS)
def test_helper_expectations(seed):
    a1 = K.build("A1", seed)
    short, long_ = a1["calls"]
    assert len(short["lens"]) > 8192 and int(short["lens"].max()) < 1024 and int(long_["lens"].min()) >= 1024 and int(long_["lens"].max()) == 300 * K.KIB
    for c in a1["calls"]:
        for a, n, h in list(zip(c["offs"].tolist(), c["lens"].tolist(), c["hashes"].tolist()))[::17]:
            assert o.xxh32(c["arena"][a:a + n].tobytes()) == h
    a2 = K.build("A2", seed)
    want = K.copy_expect(a2, 0xA5)
    ends = np.sort(a2["do"] + a2["lens"])
    assert (np.sort(a2["do"])[1:] >= ends[:-1]).all(), "destinations overlap"
    assert int((want != 0xA5).sum()) > int(a2["lens"].sum()) * 0.9 and int(a2["lens"].max()) == a2["max_len"]
    a3 = K.build("A3", seed)
    shifts = [K.trim_expect(r)[1] for r in a3["rows"]]
    assert 0 in shifts and any(shifts) and all(s % 16 == 0 for s in shifts)
    for r, s in zip(a3["rows"], shifts):
        t, _ = K.trim_expect(r)
        assert (s == 0) == (r["out_existing_len"] < 1 << 30 or r["out_existing_len"] > r["out_cap"])
        assert t["out_existing_len"] == r["out_existing_len"] - s and (s == 0 or 65536 <= t["out_existing_len"] < 65536 + 16)
    assert any(r["out_existing_len"] > r["out_cap"] for r in a3["rows"])
    assert {st for st, _ in a3["results"]} >= {0, 1, 2, 3, 4}


@pytest.mark.parametrize("ks", [(k, s) for k in K.FRAME_KINDS + K.HOST_KINDS for s in SEEDS], ids=_ids)
def test_frame_and_host_expectations(ks):
    case = K.build(*ks)
    if ks[0] == "H1":
        for d, (rc, c) in zip(case["plains"], case["comp"]):
            assert rc == 0 and o.decompress_raw(c, limit=len(d)) == (0, d)
        return
    for d, f in zip(case["plains"], case["frames"]):
        assert abs(len(d) - K.FRAME_BYTES) < 65536 and f[5] >> 4 == 4                  # BD: 64 KiB blocks
    if ks[0] == "H2":
        for d, f in zip(case["plains"], case["frames"]):
            assert o.frame_decompress(f, cap=len(d) + 65536)[:2] == (0, d)
        return
    dec = case["decoded"]
    assert [st for st, _, _ in dec].count(0) == len(dec) - 1 and dec[3][0] != 0         # one damaged
    for k, (d, f, (st, b, used)) in enumerate(zip(case["plains"], case["frames"], dec)):
        assert o.frame_decompress(f, cap=len(d) + 65536) == (st, b, used)
        assert st != 0 or (b == d and used == len(f))
        assert bool(f[4] & 0x20) == (k != 1) and bool(f[4] & 0x04) == (k == 2)           # FLG: independent blocks, content checksum
    if ks[0] == "F2":
        for d, (rc, f) in zip(case["plains"], case["expect"]):
            assert rc == 0 and o.frame_decompress(f, cap=len(d) + 65536)[:2] == (0, d)
    if ks[0] == "F4":
        assert [st for st, _ in case["expect"]].count(K.MISMATCH) == 1
        assert case["wanted"][0] != case["plains"][0] and case["wanted"][1:] == case["plains"][1:]


# ------------------------------------------------------------------------------------------------------------- 2. class reached
def _gxx(tmp, name):
    so = str(tmp / f"lib{name}.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(HERE, "emu", name + ".cpp")])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("concurrent_plans")
    D, S, V = _gxx(tmp, "emu_dispatch"), _gxx(tmp, "emu_size_dispatch"), _gxx(tmp, "emu_verify_dispatch")
    u32p = C.POINTER(C.c_uint32)
    D.lzf_emu_decompress_plan.restype = None
    D.lzf_emu_decompress_plan.argtypes = [C.c_uint32, C.c_uint32, u32p, C.c_uint32, C.c_uint64, u32p, C.POINTER(C.c_char_p)]
    D.lzf_emu_compress_plan.restype = C.c_char_p
    D.lzf_emu_compress_plan.argtypes = [C.c_uint32, C.c_uint32, u32p, C.c_uint32, C.c_uint32, u32p]
    S.lzf_emu_size_plan.restype = None
    S.lzf_emu_size_plan.argtypes = [C.c_uint32, C.c_uint32, u32p, C.c_uint32, C.c_uint64, u32p, C.POINTER(C.c_char_p)]
    V.lzf_emu_verify_plan.restype = None
    V.lzf_emu_verify_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, u32p, C.POINTER(C.c_char_p)]

    D.lzf_emu_seg_layout.restype = None
    D.lzf_emu_seg_layout.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
    D.lzf_emu_fed_layout.restype = None
    D.lzf_emu_fed_layout.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
    S.lzf_emu_size_layout.restype = None
    S.lzf_emu_size_layout.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
    V.lzf_emu_verify_layout.restype = None
    V.lzf_emu_verify_layout.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]

    class Plans:
        @staticmethod
        def seg_total(n, max_in):
            out = (C.c_uint64 * 16)(); D.lzf_emu_seg_layout(n, max_in, out)
            return out[15]

        @staticmethod
        def fed_total(n, max_in):
            out = (C.c_uint64 * 9)(); D.lzf_emu_fed_layout(n, max_in, out)
            return out[8]

        @staticmethod
        def size_total(n, max_in):
            out = (C.c_uint64 * 10)(); S.lzf_emu_size_layout(n, max_in, out)
            return out[9]

        @staticmethod
        def verify_total(n, max_in):
            out = (C.c_uint64 * 6)(); V.lzf_emu_verify_layout(n, max_in, out)
            return out[3]

        @staticmethod
        def decompress(n, max_in):
            out = (C.c_uint32 * 12)(); strs = (C.c_char_p * 3)()
            D.lzf_emu_decompress_plan(CU, LDS, None, n, max_in, out, strs)
            return dict(try_seg=bool(out[1]), groups=list(out[5:5 + out[4]]), try_fed=bool(out[9]), s_seg=strs[0].decode(), s_fed=strs[1].decode(), s_last=strs[2].decode())

        @staticmethod
        def compress(n, kinds):
            out = (C.c_uint32 * 6)()
            s = D.lzf_emu_compress_plan(CU, LDS, None, n, kinds, out)
            return dict(compact=bool(out[1]), team=bool(out[2]), fresh_only=bool(out[3]), launch=s.decode())

        @staticmethod
        def size(n, max_in):
            out = (C.c_uint32 * 4)(); strs = (C.c_char_p * 2)()
            S.lzf_emu_size_plan(CU, LDS, (C.c_uint32 * 3)(0xFFFFFFFF, 0xFFFFFFFF, 0), n, max_in, out, strs)
            return dict(try_seg=bool(out[0]), seg=strs[0].decode(), wave=strs[1].decode())

        @staticmethod
        def verify(n, max_in):
            out = (C.c_uint32 * 3)(); strs = (C.c_char_p * 2)()
            V.lzf_emu_verify_plan(CU, LDS, 0, n, max_in, out, strs)
            return dict(try_seg=bool(out[0]), seg=strs[0].decode(), wave=strs[1].decode())
    return Plans


def _bound(case):
    return ANY if case["max_input_len"] is None else case["max_input_len"]


def _in_lens(case):
    return [len(case["inputs"][j["inp"]]) for j in case["jobs"]]


@pytest.mark.parametrize("seed", SEEDS)
def test_decode_kinds_reach_their_classes(plans, seed):
    d1, d2, d3, d4 = (K.build(k, seed) for k in ("D1", "D2", "D3", "D4"))
    p = plans.decompress(len(d1["jobs"]), _bound(d1))
    assert not p["try_seg"] and not p["try_fed"] and p["s_last"] == K.launch_of("D1", seed)[1]
    assert max(_in_lens(d1)) <= K.D1_BOUND and all(2 * K.KIB <= len(d) - len(j["existing"]) <= 40 * K.KIB for d, j in zip(d1["plains"], d1["jobs"]))
    p = plans.decompress(len(d2["jobs"]), _bound(d2))
    assert p["try_seg"] and p["groups"] == [len(d2["jobs"])] and p["s_seg"] == K.launch_of("D2", seed)[1]
    p = plans.decompress(len(d3["jobs"]), _bound(d3))
    assert p["try_seg"] and len(p["groups"]) == 4 and sum(p["groups"]) == len(d3["jobs"]) >= 32 and p["s_seg"] == K.launch_of("D3", seed)[1]
    for c in (d2, d3):
        assert min(_in_lens(c)) >= K.MIN_SEG_IN                    # every block is inside the pipeline's window
    p = plans.decompress(len(d4["jobs"]), _bound(d4))
    assert len(d4["jobs"]) > 3072 and p["try_fed"] and not p["try_seg"] and p["s_fed"] == K.launch_of("D4", seed)[1]
    assert all(K.MIN_SEG_IN < n <= 128 * K.KIB for n in _in_lens(d4)) and max(_in_lens(d4)) <= K.D4_BOUND and 6 <= len(d4["inputs"]) <= 7
    assert {j["cap"] for j in d4["jobs"]} == {d4["uniform_cap"]}
    assert max(_in_lens(d3)) <= K.D3_BOUND == d3["max_input_len"]
    # what the calls ask the pool for, as the gate's allowance takes it: the emulated layouts' totals (areas aligned to 256 bytes)
    for c, layout in ((d2, plans.seg_total), (d3, plans.seg_total), (d4, plans.fed_total)):
        want, got = layout(len(c["jobs"]), _bound(c)), K.pool_request(c["kind"], seed)
        assert got <= want <= got + 256 * 16, (c["kind"], got, want)
    assert K.pool_request("D3", seed) < 1 << 30 and K.pool_request("C2", seed) == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_size_and_verify_kinds_reach_their_classes(plans, seed):
    for kind, plan in (("Z1", plans.size), ("V1", plans.verify)):
        c = K.build(kind, seed)
        p = plan(len(c["jobs"]), _bound(c))
        assert p["try_seg"] and p["seg"] == K.launch_of(kind, seed)[1]
        want, got = (plans.size_total if kind == "Z1" else plans.verify_total)(len(c["jobs"]), _bound(c)), K.pool_request(kind, seed)
        assert got <= want <= got + 256 * 16 and got <= 3 << 30, (kind, got, want)      # (kSizeMaxScratch)
        valid = [n for n, (st, _) in zip(_in_lens(c), c["expect"]) if st in (0, K.MISMATCH)]
        assert min(valid) >= K.MIN_SEG_IN and sum(len(x) >= K.MIN_SEG_IN for x in c["inputs"]) >= len(c["inputs"]) - 1     # (the cut block may be shorter)
    for kind, plan in (("Z2", plans.size), ("V2", plans.verify)):
        c = K.build(kind, seed)
        p = plan(len(c["jobs"]), _bound(c))
        assert not p["try_seg"] and p["wave"] == K.launch_of(kind, seed)[1] and max(_in_lens(c)) <= K.D1_BOUND


@pytest.mark.parametrize("seed", SEEDS)
def test_compress_kinds_reach_their_classes(plans, seed):
    c1, c2, c3 = (K.build(k, seed) for k in ("C1", "C2", "C3"))
    p = plans.compress(len(c1["jobs"]), c1["kinds"])
    assert p["team"] and p["fresh_only"] and p["launch"] == K.launch_of("C1", seed)[1]
    p = plans.compress(len(c2["jobs"]), c2["kinds"])
    assert len(c2["jobs"]) > CU and p["compact"] and not p["team"] and p["launch"] == K.launch_of("C2", seed)[1]
    p = plans.compress(len(c3["jobs"]), c3["kinds"])
    assert c3["kinds"] == K.U32 | K.U16 and p["team"] and not p["fresh_only"] and p["launch"] == K.launch_of("C3", seed)[1]


# ------------------------------------------------------------------------------------------------------------- 3. launch strings
def test_launch_strings_are_the_headers():
    with open(os.path.join(CSRC, "lzf_dispatch.h")) as f:
        literals = set(re.findall(r'"((?:[^"\\]|\\.)*)"', f.read()))
    for kind in K.LAUNCH:
        for seed in SEEDS:
            which, s = K.launch_of(kind, seed)
            assert s in literals and which in ("decompress", "size", "verify", "compress"), (kind, s)
    assert K.launch_of("C4", 0) is None
    assert set(K.LAUNCH) == set(K.ASYNC_KINDS) - {"C4", "A1", "A2", "A3"}


# ------------------------------------------------------------------------------------------------------------- 4. seeds differ
@pytest.mark.parametrize("kind", K.KINDS)
def test_two_seeds_are_two_different_calls(kind):
    a, b = K.build(kind, 0), K.build(kind, 1)
    assert K.job_count(a) == K.count(kind, 0) != K.count(kind, 1) == K.job_count(b)
    ja, jb = K.job_bytes(a), K.job_bytes(b)
    n = min(len(ja), len(jb))
    assert sum(x != y for x, y in zip(ja, jb)) * 2 >= n, kind


def test_pairs():
    sp, tp = K.stream_pairs(), K.thread_pairs()
    assert len(set(sp)) == len(sp) and len(set(tp)) == len(tp)
    for k in K.ASYNC_KINDS:
        assert ((k, 0), (k, 1)) in sp
        assert k == "D3" or ((k, 0), ("D3", 1)) in sp
        assert k == "D4" or ((k, 0), ("D4", 1)) in sp or (("D4", 0), (k, 1)) in sp
    assert (("D3", 0), ("D3", 1)) in sp and (("D3", 1), ("D3", 0)) in sp
    for k in K.KINDS:
        for other in (k, "D3", "F1", "H2"):
            assert ((k, 0), (other, 1)) in tp or ((other, 0), (k, 1)) in tp, (k, other)
    assert all(a[0] in K.ASYNC_KINDS and b[0] in K.ASYNC_KINDS for a, b in sp)
    assert set(K.LONG) <= set(K.KINDS) and [k for k, _ in K.THREAD_MIX] == ["D3", "C2", "F1", "H2"]
