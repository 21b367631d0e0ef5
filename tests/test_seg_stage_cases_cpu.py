"""The census of tests/seg_stage_cases.py: a condition, not a measurement.  Every named edge of the segmented decompress pipeline's stages —
both sides of every threshold — is reached by at least one case, for each ring (32, 64, 128 KiB) and each output residue (0, 9); every case
is what the oracle says it is; the model's stitched token map is the true token set.  No GPU: the reach of the cases is proven here, before
tests/test_gpu_seg_stages.py asks the device."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle_ffi as o  # noqa: E402
import seg_stage_cases as S  # noqa: E402


@pytest.fixture(scope="module")
def corpus():
    return S.all_cases(), S.models()


def test_corpus_stays_small(corpus):
    cases, _ = corpus
    total = sum(len(c["input"]) for c in cases)
    assert total <= S.CORPUS_INPUT_MAX, total
    assert all(len(c["input"]) <= (1 << 20) for c in cases)
    assert sum(c["status"] == S.OK for c in cases) >= 20 and sum(c["status"] != S.OK for c in cases) == 6


def test_every_case_is_what_the_oracle_says(corpus):
    cases, _ = corpus
    for c in cases:
        rc, out = o.decompress_raw(c["input"], limit=c["limit"], cap=c["out_cap"])
        assert rc == c["status"], (c["name"], o.STATUS_NAMES[rc], o.STATUS_NAMES[c["status"]])
        if rc == S.OK:
            assert out == c["output"], c["name"]


def test_stitched_token_map_is_the_true_token_set(corpus):
    cases, models = corpus
    for c, m in zip(cases, models):
        if c["status"] != S.OK:
            continue
        walked = [(p, L, M) for p, L, M, _ in S._walk(c["input"])]
        assert [(t[0], t[1], t[2]) for t in m.toks] == walked, c["name"]
        truth = np.zeros(m.n, bool)
        truth[[t[0] for t in m.toks]] = True
        assert not m.seam.failed and m.gives_up is None, c["name"]
        diff = np.nonzero(m.seam.stitched() != truth)[0]
        assert diff.size == 0, (c["name"], int(diff[0]))
        assert m.layout.outb == len(c["output"]) and m.layout.ntok % 64 == 0, c["name"]
        assert (m.layout.tile_n <= S.TILE_TOK_MAX).all(), c["name"]


def test_damaged_cases_are_given_up_where_they_say(corpus):
    cases, models = corpus
    seen = set()
    for c, m in zip(cases, models):
        if c["status"] != S.OK:
            assert m.gives_up == c["gives_up"], (c["name"], m.gives_up)
            seen.add((c["gives_up"], c["status"]))
    assert seen == {("seam", S.UNEXPECTED_END), ("tilesum", S.UNEXPECTED_END), ("records", S.ZERO_OFFSET), ("records", S.INVALID_OFFSET),
                    ("records", S.MEMORY_LIMIT_EXCEEDED), ("scan", S.OUT_CAPACITY)}


def test_cases_reach_the_edge_they_are_named_for(corpus):
    cases, models = corpus
    for c, m in zip(cases, models):
        if c.get("reaches"):
            got = S.census_free(c, m)
            assert set(c["reaches"]) <= got, (c["name"], sorted(set(c["reaches"]) - got))


def test_every_ring_free_edge_is_reached(corpus):
    cases, models = corpus
    got = set()
    for c, m in zip(cases, models):
        got |= S.census_free(c, m)
    assert got >= S.free_edges(), sorted(S.free_edges() - got)
    assert got <= S.free_edges(), sorted(got - S.free_edges())


@pytest.mark.parametrize("rb", S.RESIDUES)
@pytest.mark.parametrize("R", S.RINGS)
def test_every_ring_edge_is_reached(corpus, R, rb):
    _, models = corpus
    got = set()
    for m in models:
        got |= S.census_ring(m, R, rb)
    assert got >= S.ring_edges(), sorted(S.ring_edges() - got)
    assert got <= S.ring_edges(), sorted(got - S.ring_edges())


def test_model_levels_and_records_are_consistent(corpus):
    """What the model says of itself: bounds in order, sub-batches numbered 0, 1, 2 ... within a batch, no sub-batch but a giant over the span."""
    _, models = corpus
    for m in models:
        ly = m.layout
        if ly is None or m.gives_up:
            continue
        assert (ly.lvl_lo <= ly.lvl_hi).all() and ly.lvl_hi.max() <= 64
        for R in S.RINGS:
            r = ly.records(R, 9)
            sub = r["sub"].reshape(-1, 64)
            assert (sub[:, 0] == 0).all() and (np.diff(sub, axis=1) >= 0).all() and (np.diff(sub, axis=1) <= 1).all()
            act = ly.act
            assert ((r["oe"] - r["sob"])[act & ~r["giant"]] <= R // 8).all()
            assert ((ly.endp - r["sob"])[r["giant"]] > R // 8).all()


@pytest.mark.parametrize("seed", S.SEEDS)
def test_a_rule_moved_by_one_changes_a_record(corpus, seed):
    """The reach of the corpus, the other way round: the model with one threshold of the records stage moved by one (the sub-batch span, a
    class length, a ring index that wraps, the oldest byte the ring holds, overlapping, the two ends of a dependency range) gives another
    sub-batch, class, flag byte or level for some record of the corpus, under every ring and residue — the word-for-word comparison on the device
    cannot pass a kernel that has the rule off by one."""
    cases, models = corpus
    plain = [m.layout for m in models if m.layout is not None and m.gives_up is None]
    if seed in ("end < s0", "mo <= e0"):                       # (the levels: worked out again; the others only change records())
        seeded = [S.Layout(ly.n, ly.toks, seed=seed) for ly in plain]
    else:
        seeded = [copy.copy(ly) for ly in plain]
        for ly in seeded:
            ly.seed = seed
    for R in S.RINGS:
        for rb in S.RESIDUES:
            changed = 0
            for a, b in zip(plain, seeded):
                ra, rb_ = a.records(R, rb), b.records(R, rb)
                changed += int(((ra["sub"] != rb_["sub"]) | (ra["cls"] != rb_["cls"]) | (ra["fl"] != rb_["fl"]) | (a.lvl_lo != b.lvl_lo)).sum())
            assert changed, (seed, R, rb)
