"""The built cases of fed_flush_cases.py reach the edges they were built for — by the host model of the fed kernel's windows, batches,
pieces and pending range, which is held here to the models the repository already has: fed_setup_cases.layout (windows and batches), the
emulator of the window loop run piece by piece (fed_piece_cases.emulate_pieces: where every piece parks) and the oracle (statuses, bytes)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle_ffi as o  # noqa: E402
import fed_flush_cases as F  # noqa: E402
import fed_periodic_cases as K  # noqa: E402
import fed_piece_cases as P  # noqa: E402
import fed_setup_cases as S  # noqa: E402

CORPUS = F.corpus()


def test_sizes_stay_small():
    large = [c for c in CORPUS if F.E_WALK in c["wants"]]      # the walk-mode retry needs more than a parse chunk of input: one case
    assert len(large) == 1 and len(large[0]["input"]) <= 32 * 1024 and large[0]["cap"] <= 40 * 1024
    for c in CORPUS:
        assert c in large or (len(c["input"]) <= 5 * 1024 and c["cap"] <= 16384), c["name"]
    assert len(CORPUS) <= 64


def test_no_far_source_reaches_the_two_batches_before_its_own():
    """What the case module calls unreachable, by the kernel's own ring (lzf_decompress_fed_kernel<4096, ...>: kSpanMax = RING / 3)."""
    ring = 4096
    assert (K.RING, K.SPAN_MAX, K.NEAR_HIST) == (ring, ring // 3, ring - ring // 3)
    assert 2 * K.SPAN_MAX < K.NEAR_HIST          # two batches span less than the distance to the newest far source
    assert K.SPAN_MAX + 16 <= K.NEAR_HIST        # the kernel's static_assert: the pending range lies in the intact history
    for c in CORPUS:                             # ... and by the model: no far source of any case starts at or above the batch two before
        bs = [e for e in F.model(c)[0] if e["kind"] == "batch"]
        for b, e in enumerate(bs):
            for t in e["toks"]:
                if t["cls"] == K.FAR and b >= 2 and bs[b - 1]["nb"] >= 1 and bs[b - 2]["nb"] >= 1:      # (a solo sequence is larger than a batch)
                    assert t["mo"] - t["off"] + t["M"] <= bs[b - 2]["ob0"], (c["name"], b, t["lane"])


def test_every_case_reaches_its_edges_and_every_edge_is_reached():
    reached = set()
    for c in CORPUS:
        got = F.census(c)
        assert c["wants"] <= got, (c["name"], c["wants"] - got)
        reached |= got
    assert set(F.edges()) <= reached, set(F.edges()) - reached


def test_the_oracle_agrees_with_the_models_status_and_bytes():
    for c in CORPUS:
        rc, out = o.decompress_raw(c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"], cap=c["cap"])
        ev, status, good_end = F.model(c)
        assert rc == c["status"] == status, (c["name"], rc, status)
        if rc == 0:
            assert out == K.decode(c) and len(out) == good_end, c["name"]
        else:
            assert len(c["existing"]) < good_end <= len(out), (c["name"], good_end, len(out))      # the oracle has written the good batches


def test_batches_equal_the_layout_model():
    for c in CORPUS:
        if c["status"] != 0:
            continue
        mine = [e for e in F.model(c)[0] if e["kind"] == "batch"]
        recs = S.layout(c["input"], len(c["existing"]))
        theirs = {}
        for t in recs:
            theirs.setdefault(t["batch"], []).append(t)
        assert len(mine) == len(theirs), c["name"]
        for e, (k, ts) in zip(mine, sorted(theirs.items())):
            assert (e["nb"], e["ob0"], e["win"], e["first"], len(e["toks"])) == (ts[0]["nb"], ts[0]["lo"], ts[0]["win"], ts[0]["first"], len(ts)), (c["name"], k)


def test_pieces_park_where_the_emulator_parks():
    for c in CORPUS:
        if c["status"] != 0:
            continue
        m = P.emulate_pieces(c["input"], 3, prefix_len=len(c["prefix"]), existing_len=len(c["existing"]), limit=c["limit"], cap=c["cap"])
        parks = [e for e in F.model(c, 3)[0] if e["kind"] == "park"]
        emu = [(p, r["expect"], r["o"]) for p, r in enumerate(m.rec) if r["what"] in (P.PARKED, P.PARKED_AT_ONCE)]
        assert [(e["piece"], e["expect"], e["o"]) for e in parks] == emu, (c["name"], parks, emu)


def test_flush_lines_writes_whole_lines_once():
    for rb in range(16):
        for a in range(40):
            for n in range(70):
                e = F.flush_lines(a, a + n, rb)
                assert a <= e <= a + n and (e == a or (e + rb) % 16 == 0)
                assert a + n - e < 16 or (e == a and n < 16)
