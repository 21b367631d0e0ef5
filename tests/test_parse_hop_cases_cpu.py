"""The census of tests/parse_hop_cases.py: a condition, not a measurement.  Every case is a valid block (the oracle decodes it), the
model's rows of every chunk are the true token positions (chunk 1 from where its chain is on the true one), and every named edge of the
parse kernel's plain-hop loop — each exit, in the first and in the second half of a trip — is reached by at least one case.  No GPU:
tests/test_gpu_parse_hop.py asks the device for the same rows."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle_ffi as o  # noqa: E402
import parse_hop_cases as P  # noqa: E402


@pytest.fixture(scope="module")
def cases():
    return P.all_cases()


def test_jobs_are_one_or_two_chunks_and_few(cases):
    assert len(cases) <= 64 and len({n for n, _ in cases}) == len(cases)
    assert all(len(b) <= P.CHUNK or P.STRIDE < len(b) <= P.CHUNK + 1024 for _, b in cases), [len(b) for _, b in cases]
    assert any(P.nch(len(b)) == 2 for _, b in cases)


def test_every_case_decodes_and_its_walk_is_the_oracles(cases):
    for name, b in cases:
        rc, out = o.decompress_raw(b, limit=P.LIMIT, cap=P.LIMIT + len(b) + 64)
        assert rc == 0, (name, o.STATUS_NAMES[rc])
        toks = P.true_tokens(b)
        assert toks == sorted(set(toks)) and toks[0] == 0, name
        # the walk's last token is the last literals, and they end the block: what the oracle consumed
        last = toks[-1]; L = b[last] >> 4; q = last + 1
        if L == 15:
            while b[q] == 255:
                L += 255; q += 1
            L += b[q]; q += 1
        assert q + L == len(b) and (b[last] & 15) == 0, name


def test_model_rows_are_the_true_tokens(cases):
    for name, b in cases:
        assert P.compare_with_truth(b, P.expected_rows(b)) is None, name


def test_every_named_edge_is_reached(cases):
    got = set()
    for _, b in cases:
        got |= P.census(b)
    assert got >= set(P.EDGES), sorted(set(P.EDGES) - got)


def test_cases_reach_the_edge_they_are_named_for(cases):
    built = P.built_for()
    assert set(built) == {name for name, _ in cases}
    assert {e for edges in built.values() for e in edges} == set(P.EDGES)      # every edge has a case built for it
    for name, b in cases:
        got = P.census(b)
        assert set(built[name]) <= got, (name, sorted(set(built[name]) - got))
