"""The census of tests/seg_history_cases.py: a condition, not a measurement.  Every named edge of the segmented decompress pipeline's handling
of existing output and prefixes is reached by a case, for each ring (32, 64, 128 KiB) and output residue (0, 9); every case is what the oracle
says it is (status and bytes, with prefix=, existing=, limit=, cap=); the model's layout adds up to the oracle's output; a job without history
gets from the history model the records the history-free model gives it, word for word.  No GPU: the reach of the cases is proven here, before
tests/test_gpu_seg_history.py asks the device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle_ffi as o  # noqa: E402
import seg_history_cases as H  # noqa: E402
import seg_stage_cases as S  # noqa: E402


@pytest.fixture(scope="module")
def corpus():
    return H.all_cases(), H.models()


def test_corpus_stays_small(corpus):
    cases, _ = corpus
    assert sum(len(c["input"]) for c in cases) <= (1 << 20)
    assert sum(len(c["existing"]) + len(c["prefix"]) for c in cases) <= (6 << 20)
    assert sum(c["status"] == S.OK for c in cases) >= 40 and sum(c["status"] != S.OK for c in cases) == 6


def test_every_case_is_what_the_oracle_says(corpus):
    cases, models = corpus
    for c, m in zip(cases, models):
        rc, out = o.decompress_raw(c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"], cap=c["out_cap"])
        assert rc == c["status"], (c["name"], o.STATUS_NAMES[rc], o.STATUS_NAMES[c["status"]])
        if rc == S.OK:
            assert out == c["output"], c["name"]
            assert out[:m.E] == c["existing"] and m.layout.outb == len(out) and m.gives_up is None, c["name"]
            assert int(m.layout.tile_out[0]) == m.E, c["name"]


def test_the_limit_comes_before_the_offset(corpus):
    """decompress.rs:72-74 before :83-89: the same damaged block with room under the limit is an offset error."""
    cases, _ = corpus
    c = next(c for c in cases if "the limit comes first" in c["name"])
    rc, _ = o.decompress_raw(c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"] + 1, cap=c["out_cap"])
    assert rc == S.INVALID_OFFSET and c["status"] == S.MEMORY_LIMIT_EXCEEDED


def test_a_prefix_behind_65535_bytes_is_ignored(corpus):
    """off = 65 535 at mo = E >= 65 535 decodes the same with and without the prefix; one byte more of reach would be needed to see it."""
    cases, _ = corpus
    hit = [c for c in cases if "out of reach" in c["name"]]
    assert len(hit) == 2
    for c in hit:
        rc, out = o.decompress_raw(c["input"], prefix=b"", existing=c["existing"], limit=c["limit"], cap=c["out_cap"])
        assert rc == S.OK and out == c["output"], c["name"]


def test_damaged_cases_are_given_up_where_they_say(corpus):
    cases, models = corpus
    seen = set()
    for c, m in zip(cases, models):
        if c["status"] != S.OK:
            assert m.gives_up == c["gives_up"], (c["name"], m.gives_up)
            seen.add((c["gives_up"], c["status"]))
        else:
            assert m.gives_up is None, c["name"]
    assert seen == {("records", S.MEMORY_LIMIT_EXCEEDED), ("records", S.INVALID_OFFSET), ("records", S.ZERO_OFFSET), ("scan", S.OUT_CAPACITY)}


def test_every_ring_free_edge_is_reached(corpus):
    cases, models = corpus
    got = set()
    for c, m in zip(cases, models):
        got |= H.census_free(c, m)
    got.discard("-")
    assert got >= H.free_edges(), sorted(H.free_edges() - got)
    assert got <= H.free_edges(), sorted(got - H.free_edges())


@pytest.mark.parametrize("rb", S.RESIDUES)
@pytest.mark.parametrize("R", S.RINGS)
def test_every_ring_edge_is_reached(corpus, R, rb):
    cases, models = corpus
    got = set()
    for c, m in zip(cases, models):
        got |= H.census_ring(c, m, R, rb)
    assert got >= H.ring_edges(R), sorted(H.ring_edges(R) - got)
    assert got <= H.ring_edges(R), sorted(got - H.ring_edges(R))


def test_history_at_three_rings_is_older_than_the_ring(corpus):
    """E = 3 R: at the block's first sub-batch the ring keeps R - 3 R / 8 - 64 bytes of the history; a source further back is class 7."""
    cases, models = corpus
    for R in S.RINGS[:2]:
        c, m = next((c, m) for c, m in zip(cases, models) if c.get("E_named") == 3 * R)
        for rb in S.RESIDUES:
            r = m.layout.records(R, rb)
            first = (r["sub"][:64] == 0) & m.layout.act[:64] & (m.layout.M[:64] > 0)
            assert (r["cls"][:64][first] == 7).any(), (R, rb)


def test_model_records_are_consistent(corpus):
    _, models = corpus
    for m in models:
        ly = m.layout
        assert (ly.lvl_lo <= ly.lvl_hi).all() and ly.lvl_hi.max() <= 64
        assert (ly.lvl_lo[ly.pre] == 1).all()
        for R in S.RINGS:
            r = ly.records(R, 9)
            sub = r["sub"].reshape(-1, 64)
            assert (sub[:, 0] == 0).all() and (np.diff(sub, axis=1) >= 0).all() and (np.diff(sub, axis=1) <= 1).all()
            assert ((r["oe"] - r["sob"])[ly.act & ~r["giant"]] <= R // 8).all()
            assert (r["cls"][ly.strad] == 8).all() and (r["giant"][ly.strad]).all()
            assert (r["cls"][ly.pre & ~ly.strad & ~r["giant"]] == 13).all()
            assert (r["fl"][np.isin(r["cls"], (7, 8, 13))] == 0).all()


def test_history_free_jobs_keep_their_records():
    """The history model over the history-free corpus (E = 0, P = 0; and with a prefix no offset asks for) gives seg_stage_cases' records and
    levels, word for word."""
    for c, m in zip(S.all_cases(), S.models()):
        if m.layout is None or m.gives_up:
            continue
        for P in (0, 1000):
            h = H.HLayout(m.n, m.toks, 0, P)
            assert not h.pre.any()
            assert (h.lvl_lo == m.layout.lvl_lo).all() and (h.lvl_hi == m.layout.lvl_hi).all() and (h.tile_out == m.layout.tile_out).all(), c["name"]
            for R in S.RINGS:
                a, b = h.records(R, 9), m.layout.records(R, 9)
                for k in ("sub", "cls", "fl", "w0", "w1", "w2_low", "w3"):
                    assert (a[k] == b[k]).all(), (c["name"], R, k)
