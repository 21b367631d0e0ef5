"""The census and the models of tests/launch_order_cases.py, without a GPU: every named edge of the launch-order stage is reached by a case;
the models agree with an independent statement where there is one (the fed estimate of an in-step block is the block's sequence count, the
sampled estimate of a block whose windows start on tokens follows from its token list alone); the sort's contract rejects a reversed order,
a duplicated index and an order made with 8 classes, and accepts any shuffle inside a class.  tests/test_gpu_launch_order.py then asks the
device."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import launch_order_cases as Lc  # noqa: E402
import oracle_ffi as o  # noqa: E402
import seg_stage_cases as S  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------ the census
def test_sort_cases_reach_their_edges():
    got = Lc.census_sort()
    assert got == Lc.SORT_EDGES, (sorted(Lc.SORT_EDGES - got), sorted(got - Lc.SORT_EDGES))
    assert Lc.outlier_classes() == 1              # (recorded in DESIGN.md: behind one outlier of 4e9 a thousand small jobs are one class)


def test_cost_cases_reach_their_edges():
    got = Lc.census_cost()
    assert got == Lc.COST_EDGES, (sorted(Lc.COST_EDGES - got), sorted(got - Lc.COST_EDGES))
    cases = Lc.cost_cases()
    assert 28 <= len(cases) <= 34
    assert all(c["input_len"] <= 65536 for c in cases) and sum(c["input_len"] >= 15 * 1024 for c in cases) >= 27


def test_fed_cases_reach_their_edges():
    got = Lc.census_fed()
    assert got == Lc.FED_EDGES, (sorted(Lc.FED_EDGES - got), sorted(got - Lc.FED_EDGES))
    cases = Lc.fed_cases()
    assert 36 <= len(cases) <= 44
    assert sum(c["input_len"] for c in cases) <= S.CORPUS_INPUT_MAX
    assert all(c["input_len"] <= (1 << 20) for c in cases)


def test_probe_cases_reach_their_edges():
    got = Lc.census_probes()
    assert got == Lc.PROBE_EDGES, (sorted(Lc.PROBE_EDGES - got), sorted(got - Lc.PROBE_EDGES))


def test_built_blocks_are_valid():
    for c in Lc.cost_cases() + Lc.fed_cases():
        if c["input"]:
            rc, out = o.decompress_raw(c["input"])
            assert rc == 0 and len(out) > 0, c["name"]


# ------------------------------------------------------------------------------------- the models against independent statements
def test_fed_estimate_of_an_in_step_block_is_its_sequence_count():
    n_in_step = n_out = 0
    for c in Lc.fed_cases():
        for min_in in (0, Lc.FED_MIN_IN):
            est, seqs = Lc.fed_est(c, min_in, 32)
            if not Lc.fed_eligible(c, min_in):
                assert seqs is None and est == c["input_len"] >> 4, c["name"]
                assert Lc.fed_est(c, min_in, 2)[0] == (c["input_len"] >> 4) + (c["input_len"] >> 2)
                continue
            walked = len(S._walk(c["input"]))
            if seqs is not None:
                assert est == seqs == walked, (c["name"], est, seqs, walked)
                assert Lc.fed_est(c, min_in, 2)[0] == walked + (c["input_len"] >> 2)
                n_in_step += 1
            else:
                assert est != walked or "three-phase" in c["name"], c["name"]      # (out of step: some chunk counts marks off the chain)
                n_out += 1
    assert n_in_step >= 40 and n_out >= 2, (n_in_step, n_out)


def test_sampled_estimate_on_token_boundaries_is_a_direct_count():
    seen = 0
    for c in Lc.cost_cases():
        if "windows start on tokens" in c["reaches"]:
            for shift in Lc.LEN_SHIFTS:
                assert Lc.cost_est(c["input"], shift) == Lc.direct_count_est(c["input"], shift), (c["name"], shift)
            seen += 1
    assert seen == 3


def test_cost_est_short_path_and_byte_share():
    blk = Lc.cost_cases()[0]["input"]
    assert len(blk) == Lc.SAMPLED_FROM - 1
    for shift in Lc.LEN_SHIFTS:
        assert Lc.cost_est(blk, shift) == len(blk) >> 4                       # no byte share on the short path
        assert Lc.cost_est(None, shift, length=40000) == 2500
        assert Lc.cost_est(b"", shift) == 0
    big = Lc.cost_cases()[1]["input"]
    base = Lc.cost_est(big, 32)
    assert Lc.cost_est(big, 31) == base and Lc.cost_est(big, 0) == base + len(big) and Lc.cost_est(big, 2) == base + (len(big) >> 2)
    # a wrong window stride is another estimate: windows every len // 3 bytes are not those every (len - 5152) // 3
    sampled = [c["input"] for c in Lc.cost_cases() if c["input"] and c["input_len"] >= Lc.SAMPLED_FROM]
    moved = sum(1 for c in sampled if _est_with_stride(c, len(c) // 3) != Lc.cost_est(c, 32))
    assert moved >= len(sampled) // 2, (moved, len(sampled))
    assert all(_est_with_stride(c, (len(c) - Lc.WIN) // 3) == Lc.cost_est(c, 32) for c in sampled)


def _est_with_stride(c, t):
    wins = [Lc.window_walk(c[w * t:w * t + Lc.WIN], Lc.K_SKIP if w else 0) for w in range(3)]
    cnt, span = sum(w[0] for w in wins), sum(w[1] for w in wins)
    return len(c) * cnt // span


def test_probe_model_mirrors_the_kernel_on_a_worked_example():
    # piece 4096, parts 16, payload 262 144 + 16: piece k starts at ((payload - 4096) * (2k + 1) / 32) & ~15
    jobs = [dict(input=1000, input_len=262144 + 16 + 9, cursor=9)]
    pj = Lc.probe_jobs(jobs, 4096, 16)
    assert pj["input_len"].tolist() == [4096] * 16 and (pj["out_cap"] == Lc.U64).all() and not pj["cursor"].any() and not pj["out"].any()
    assert int(pj["input"][0]) == 1009 + ((258064 * 1 // 32) & ~15) and int(pj["input"][15]) == 1009 + ((258064 * 31 // 32) & ~15)
    est = Lc.cost_estimates(jobs, np.full(16, 10, np.uint32), 4096, 16)
    assert est.dtype == np.float32 and est[0] == np.float32(160) * (np.float32(262160) / np.float32(65536))
    assert Lc.cost_estimates([dict(input=0, input_len=1000, cursor=0)], np.zeros(1, np.uint32), 65536, 1)[0] == np.float32(1000) * np.float32(0.1)


# ------------------------------------------------------------------------------------------------------- the sort's contract
def _estimates():
    for n in (63, 1025, 4097):
        for kind in Lc.SORT_KINDS:
            yield n, kind, Lc.sort_estimates(kind, n)


def test_order_ok_accepts_the_modelled_sort_and_any_shuffle_inside_a_class():
    rng = np.random.default_rng(1)
    for n, kind, e in _estimates():
        assert Lc.order_fault(e, Lc.model_sort(e)) is None, (n, kind)
        for _ in range(3):
            assert Lc.order_fault(e, Lc.model_sort(e, rng=rng)) is None, (n, kind)
    jobs, reserved = Lc.cost_sort_jobs(Lc.sort_estimates("distinct 0..n-1", 2049), 3)
    ce = Lc.cost_estimates(jobs, reserved, Lc.COST_PIECE, 3)
    assert Lc.order_ok(ce, Lc.model_sort(ce, rng=rng))


def test_order_ok_rejects_a_reversed_order():
    for n, kind, e in _estimates():
        if kind in ("all zero", "all equal"):
            assert Lc.order_ok(e, Lc.model_sort(e, ascending=True))            # (nothing to tell apart)
        else:
            assert not Lc.order_ok(e, Lc.model_sort(e, ascending=True)), (n, kind)
            assert not Lc.order_ok(e, Lc.model_sort(e)[::-1]), (n, kind)


def test_order_ok_rejects_a_duplicated_index_and_a_wrong_length():
    e = Lc.sort_estimates("distinct 0..n-1", 1025)
    perm = Lc.model_sort(e)
    bad = perm.copy(); bad[7] = bad[8]
    assert "permutation" in Lc.order_fault(e, bad)
    assert "permutation" in Lc.order_fault(np.zeros(4), [0, 1, 2, 4])
    assert "permutation" in Lc.order_fault(np.zeros(4), [0, 1, 1, 3])          # (all estimates 0: the permutation is still required)
    assert Lc.order_fault(e, perm[:-1]) is not None
    assert Lc.order_ok(np.zeros(4), [3, 1, 0, 2])


def test_order_ok_rejects_an_order_made_with_8_classes():
    for n, kind, e in _estimates():
        if kind in ("distinct 0..n-1", "around 2^24 and up to 2^32-1") and n >= 1025:
            coarse = Lc.model_sort(e, classes=8, rng=np.random.default_rng(n))
            assert not Lc.order_ok(e, coarse), (n, kind)
            assert Lc.order_ok(e, coarse, classes=8)                           # (it is a sort of 8 classes: the rule scales with the class count)


def test_order_ok_rejects_a_scale_that_folds_the_jobs_into_two_classes():
    e = Lc.sort_estimates("distinct 0..n-1", 2049)
    two = np.lexsort((np.arange(len(e)), (e < e.max() // 2).astype(int)))
    assert not Lc.order_ok(e, two)
