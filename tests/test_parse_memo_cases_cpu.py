"""tests/parse_memo_cases.py without a GPU: every named edge of the saved walks is reached, by the block chosen for it; the model with one
and with two saved walks gives the maps, exits and owned marks of the model without any, word for word (the fixed point is unique: a
saved walk may only shorten the way to it); the model without saved walks is parse_hop_cases.Chunk; every block decodes with the oracle
and its chunk-0 map is the true token positions; and each defect the kernel could have — slots kept over a chunk boundary, a hit that
brings back the row without the merge position, the exit without the walked entry, a miss that leaves row B — changes a map or the
lookups of at least one block, so the device comparison of tests/test_gpu_parse_memo.py can see it."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import oracle_ffi as o  # noqa: E402
import parse_hop_cases as P  # noqa: E402
import parse_memo_cases as M  # noqa: E402

BLOCKS = M.all_cases()
NAMES = [n for n, _ in BLOCKS]


@pytest.fixture(scope="module")
def reached():
    return [M.census(b) for _, b in BLOCKS]


def test_blocks_are_small():
    assert all(P.nch(len(b)) <= 3 and len(b) <= 3 * M.CHUNK for _, b in BLOCKS)
    assert any(P.nch(len(b)) == 2 for _, b in BLOCKS)


@pytest.mark.parametrize("case", range(len(BLOCKS)), ids=NAMES)
def test_case_reaches_the_edges_it_was_chosen_for(reached, case):
    missing = [M.EDGES[k] for k in M.CASES[case][2] if M.EDGES[k] not in reached[case]]
    assert not missing, missing


def test_every_named_edge_is_reached(reached):
    missing = [e for e in M.EDGES if not any(e in r for r in reached)]
    assert not missing, missing


@pytest.mark.parametrize("case", range(len(BLOCKS)), ids=NAMES)
def test_saved_walks_change_no_word(case):
    blk = BLOCKS[case][1]
    rows0, exit0, est0, looks0, hits0 = M.expected(blk, 0)
    assert hits0 == 0
    for h in range(rows0.shape[0]):                      # depth 0 is the model the hop tests hold the device to
        c = P.Chunk(blk, h)
        assert (np.packbits(c.bits, bitorder="little").view(np.uint32) == rows0[h]).all() and c.exit == exit0[h]
    for depth in (1, 2):
        rows, exits, est, looks, hits = M.expected(blk, depth)
        assert (rows == rows0).all() and (exits == exit0).all() and est == est0
        assert looks == looks0                                      # (every pass starts from the same exits)


@pytest.mark.parametrize("case", range(len(BLOCKS)), ids=NAMES)
def test_block_decodes_and_chunk_0_is_the_true_chain(case):
    blk = BLOCKS[case][1]
    rc, out = o.decompress_raw(blk, limit=M.LIMIT, cap=M.LIMIT + len(blk) + 64)
    assert rc == 0 and len(out) > 65536
    assert P.compare_with_truth(blk, M.expected(blk, 1)[0]) is None


@pytest.mark.parametrize("defect", ["no reset", "row without mpos", "X without walked", "row B not cleared"])
def test_each_defect_shows_in_some_block(defect):
    seen = []
    for name, blk in BLOCKS:
        good, bad = M.expected(blk, 1), M.expected(blk, 1, defect)
        if (good[0] != bad[0]).any() or (good[1] != bad[1]).any() or good[3:] != bad[3:]:
            seen.append(name)
    assert seen, defect
