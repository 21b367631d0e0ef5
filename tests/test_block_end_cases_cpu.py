"""The census of tests/block_end_cases.py on the oracle alone (no GPU): the cases reach what they are built for.  Every front's sweep
holds each of the ends 2 .. 7 at least four times, every boundary has each of them within two bytes, classify() — the reference's walk —
agrees with the oracle's status on every cut, the dropped-byte and precedence lists have the statuses their names say, and the case file's copies of the
kernels' geometry are the headers' numbers."""
import pytest

import block_end_cases as B
import seg_stage_cases as S
import verify_cases as V


@pytest.fixture(scope="module")
def corpus():
    blocks, jobs = B.decode_jobs()
    return blocks, jobs


def test_the_boundaries_are_the_headers():
    h = B.header_constants()
    assert h == dict(FED_ROUND=B.FED_ROUND, FED_STAGE=B.FED_STAGE, SEG_TILE=B.SEG_TILE, TILE_STAGE=B.TILE_STAGE, SEG_CHUNK=B.SEG_CHUNK,
                     SEG_STRIDE=B.SEG_STRIDE, REGIONS=B.REGIONS)
    assert B.WAVE * 16 == B.FED_ROUND and V.CHUNK == B.WAVE * 48 and V.TILE == B.SEG_TILE == S.TILE and S.CHUNK == B.SEG_CHUNK and S.STRIDE == B.SEG_STRIDE
    assert S.TILE_STAGE == B.TILE_STAGE
    # every boundary has the front that puts the tail's first token 40 bytes in front of it, and the one that puts it between
    # the literals and the offset of the tail's five-byte sequence
    for name, b in B.BOUNDARIES[1:]:
        fronts = [f for f, (_, bb) in B.FRONTS if bb == b]
        assert fronts == [b - B.BACK, b - B.MICRO_OFFSET_AT]
        blk = B.block_of(fronts[1])
        assert B.classify(blk[:b]) == 4 and B.classify(blk[:b + 1]) == 5 and blk[b - 2] >> 4 == 1
        assert B.classify(B.block_of(fronts[0])[:b - B.BACK]) == 7


def test_the_tail_holds_every_token_form():
    toks = V.walk(B.TAIL)
    assert len(toks) == len(B.TAIL_SEQS) and toks[-1][3] == 0
    L, M = [t[2] for t in toks], [t[3] for t in toks]
    length_bytes = lambda v: 0 if v < 15 else (v - 15) // 255 + 1       # noqa: E731
    assert {length_bytes(x) for x in L} == {0, 1, 2, 3} and {length_bytes(m - 4) for m in M[:-1]} == {0, 1, 2, 3}
    assert 0 in L and 4 in M and any(x >= 15 and m >= 19 for x, m in zip(L, M))
    assert any(t[4] == 1 and t[3] > 1 for t in toks)                    # an overlapping match at offset 1
    assert any(15 <= x < 15 + 255 and (x - 15) % 255 == 0 for x in L)   # a length byte of 0 behind nibble 15


def test_census(corpus):
    _, jobs = corpus
    per_front, near = B.census(jobs)
    assert sorted(per_front) == sorted(f for f, _ in B.FRONTS)
    for front, n in per_front.items():
        assert all(n[e] >= 4 for e in range(2, 8)), (front, n)
    assert sum(n[1] for n in per_front.values()) == 1 and per_front[0][1] == 1
    assert sorted(near) == [b for _, b in B.BOUNDARIES[1:]]
    for b, n in near.items():
        assert all(n[e] >= 1 for e in range(2, 8)), (b, n)
    print("cuts per front and end class:")
    for front, n in sorted(per_front.items()):
        print(f"  front {front:6d}: {n}")
    print("cuts within 2 bytes of a boundary, per end class:")
    for b, n in sorted(near.items()):
        print(f"  boundary {b:6d}: {n}")


def test_classify_agrees_with_the_oracle_on_every_cut(corpus):
    _, jobs = corpus
    for j in jobs:
        if "want" in j:
            continue
        rc = j["exp"][0]
        assert rc == (0 if j["end"] in B.OK_ENDS else B.UNEXPECTED_END), (j["name"], j["end"], rc)
        assert j["end"] == B.classify(j["blk"][:j["k"]])
        if rc == 0:
            assert j["cap"] == len(j["exp"][1])
    # the cuts of one block decode to prefixes of one another: an Ok cut's bytes are the head of the whole block's
    by_block = {}
    for j in jobs:
        if "front" in j and j["exp"][0] == 0:
            by_block.setdefault(j["block"], []).append(j["exp"][1])
    for outs in by_block.values():
        whole = max(outs, key=len)
        assert all(whole.startswith(x) for x in outs)


def test_the_lists_have_the_statuses_their_names_say(corpus):
    _, jobs = corpus
    listed = [j for j in jobs if "want" in j]
    assert len(listed) == 3 * len(B.DROPPED) + 36
    for j in listed:
        assert (j["exp"][0], j["end"]) == j["want"], (j["name"], j["exp"][0], j["end"], j["want"])
    dropped = [j for j in listed if j["name"].startswith("dropped")]
    for j in dropped:                                      # read as a token the byte would give another result: the same block without it decodes alike
        assert j["exp"] == B.o.decompress_raw(j["blk"][:-1], limit=j["limit"]) and B.classify(j["blk"][:-1]) == 4
    assert {j["blk"][-1] for j in dropped} == set(B.DROPPED)
    short = [j for j in listed if "out_cap and limit below" in j["name"]]
    assert len(short) == 4 and all(j["cap"] < 40 + len(j["exp"][1]) and j["limit"] == j["cap"] for j in short)
    kinds = {j["want"] for j in listed}
    assert kinds == {(0, 5), (1, 3), (1, 6), (2, 7), (3, 7), (4, 7)}
    assert sum(bool(j["prefix"]) and bool(j["existing"]) for j in listed) == 18


def test_counts_and_the_verify_jobs(corpus):
    _, jobs = corpus
    assert B.counts() == dict(all=B.COUNTS["all"], carved=B.COUNTS["carved"]) and len(jobs) == B.COUNTS["all"] and len(B.carved(jobs)) == B.COUNTS["carved"]
    assert B.COUNTS["all"] <= 20000 and sum(max(j["cap"], len(j["exp"][1])) for j in jobs) < 1 << 30          # the caps of one call
    v = B.verify_jobs(jobs)
    assert len(v) == B.COUNTS["verify"] <= 20000
    assert [i for i, at, _ in v if at is None] == list(range(len(jobs)))                                       # every job once with its expected bytes ...
    ok = [i for i, j in enumerate(jobs) if j["exp"][0] == 0 and len(j["exp"][1]) > len(j["existing"])]
    assert [i for i, at, _ in v if at is not None] == ok                                                        # ... every Ok job with output once more, flipped
    for i, at, e in v:
        rc, dec = jobs[i]["exp"]
        assert e == ((rc, None) if rc else (0, len(dec)) if at is None else (B.MISMATCH, at))


def test_the_pipeline_model_gives_up_exactly_the_error_ends(corpus):
    """seg_stage_cases.Model on the jobs without history (block_end_check.py's who_seg holds the device's `done` to it): it gives up
    nowhere on the ends 1, 4, 5 and 7, and in the tile sums (or in a seam walk) on the ends 2, 3 and 6."""
    _, jobs = corpus
    for j in jobs[::7]:
        if j["prefix"] or j["existing"]:
            continue
        g = S.Model(dict(input=j["blk"][:j["k"]], limit=j["limit"], out_cap=j["cap"])).gives_up
        want = (None,) if j["exp"][0] == 0 else ("seam", "tilesum") if j["exp"][0] == 1 else ("records",)      # (a seam walk may meet the end first)
        assert g in want, (j["name"], g)
