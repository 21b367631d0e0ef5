"""The built cases of fed_setup_cases.py without a GPU: every named edge of the fed kernel's batch set-up is reached by a case, the oracle
gives each case the status it is named for, and the host model of windows and batches that places the edges agrees with the emulator of
the window loop (tests/emu/emu_fed_window.cpp) on every block it can walk."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle_ffi as o  # noqa: E402
import fed_setup_cases as K  # noqa: E402
import fed_window_cases as fw  # noqa: E402

_cs = None


def corpus():
    global _cs
    if _cs is None:
        _cs = K.corpus(lambda blk: o.decompress_raw(blk, limit=1 << 22, cap=1 << 16)[1])
        for c in _cs:
            c["exp"] = o.decompress_raw(c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"], cap=c["cap"])
    return _cs


def test_every_edge_is_reached():
    missing = [e for e in K.edges() if e not in K.reach(corpus())]
    assert not missing, missing
    assert len(corpus()) <= 160 and sum(len(c["input"]) for c in corpus()) < 512 << 10


def test_the_oracle_gives_each_case_its_status():
    wrong = [(c["name"], c["status"], c["exp"][0]) for c in corpus() if c["exp"][0] != c["status"]]
    assert not wrong, wrong
    assert {c["status"] for c in corpus()} >= {K.OK, K.UNEXPECTED_END, K.MEMORY_LIMIT_EXCEEDED, K.ZERO_OFFSET, K.INVALID_OFFSET, K.OUT_CAPACITY}


def test_the_sweep_covers_every_class_of_staged_position():
    for rq in K.RQ_SWEEP:
        for kind in K.M_KINDS:
            hits = [c for c in corpus() if f"offset at staged position {rq}, {kind}" in c["wants"]]
            assert hits, (rq, kind)
            for c in hits:      # where the model puts the token, the block has the bytes the name says
                r = [t for t in K.layout(c["input"]) if t["rq"] == rq and t["M"] == K.M_KINDS[kind] and t["batch"] == 1]
                assert len(r) == 1 and r[0]["cstart"] == 0 and r[0]["nb"] == 44
                assert K.staged_class(rq) == ("four bytes fit" if rq <= K.STAGED - 4 else "two fit, four do not" if rq <= K.STAGED - 2 else
                                              "straddles the staged bytes" if rq == K.STAGED - 1 else "past the staged bytes")
                if r[0]["M"] >= 19:
                    assert c["input"][r[0]["q"] + 2] == min(r[0]["M"] - 19, 255)


def test_the_model_agrees_with_the_emulator():
    """Windows (their starts, the batches left for the next one) and the number of batches, over every block whose chain is whole."""
    seen = 0
    for c in corpus():
        if c["status"] == K.UNEXPECTED_END:      # (its last token cannot be walked)
            continue
        lay = K.layout(c["input"], len(c["existing"]))
        rc, stats, log = fw.emulate(c["input"])
        assert rc == 0 and stats["walked_windows"] == 0, (c["name"], rc, stats)
        assert stats["batches"] == len({t["batch"] for t in lay}), (c["name"], stats)
        starts = [pos for kind, pos in log if kind == 0]
        mine = []
        for t in lay:
            if not mine or mine[-1][0] != t["win"]:
                mine.append((t["win"], t["cstart"]))
        assert starts == [s for _, s in mine], c["name"]
        seen += 1
    assert seen == len(corpus()) - 1
