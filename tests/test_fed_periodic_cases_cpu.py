"""The built cases of fed_periodic_cases.py without a GPU: every named edge of the fed kernel's periodic-match classes is reached by a case
(a host model of the class rule says which match is moved without a division), every case reaches the
edges it is named for, the oracle decodes every case to the bytes of a plain decoder over the token walk, and the model of windows and
batches that places the edges agrees with the emulator of the window loop (tests/emu/emu_fed_window.cpp)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle_ffi as o  # noqa: E402
import fed_periodic_cases as K  # noqa: E402
import fed_window_cases as fw  # noqa: E402

_cs = None


def corpus():
    global _cs
    if _cs is None:
        _cs = K.corpus()
        for c in _cs:
            c["exp"] = o.decompress_raw(c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"], cap=c["cap"])
            c["got"] = K.census(c)
    return _cs


def test_every_edge_is_reached_and_every_case_reaches_its_own():
    reached = set()
    for c in corpus():
        assert c["wants"] <= c["got"], (c["name"], sorted(c["wants"] - c["got"]))
        reached |= c["got"]
    missing = [e for e in K.edges() if e not in reached]
    assert not missing, missing
    # small: inputs of about 2 KiB at the most, outputs (existing bytes included) of about 6 KiB
    assert max(len(c["input"]) for c in corpus()) <= 2100 and max(len(c["exp"][1]) for c in corpus()) <= 6600 and len(corpus()) <= 260


def test_the_oracle_decodes_every_case_to_the_plain_decoders_bytes():
    for c in corpus():
        assert c["exp"][0] == K.S.OK == c["status"], (c["name"], c["exp"][0])
        assert c["exp"][1] == K.decode(c), c["name"]


def test_every_class_occurs_and_the_grid_is_classified_as_the_rule_says():
    seen = {}
    for c in corpus():
        for t in K.tokens(c):
            seen[t["cls"]] = seen.get(t["cls"], 0) + 1
    for cls in (K.OWN, K.MASK, K.BYTE_LOOP, K.COOP_PLAIN, K.PREFIX, K.SOLO_SEQ, K.NONE):
        assert seen.get(cls, 0) > 0, (cls, seen)
    assert K.STRADDLING not in seen          # (not reachable with an overlapping match inside a batch: the module's docstring)
    for c in corpus():
        if c["kind"] not in ("grid", "other"):
            continue
        t = K.tokens(c)[0]
        M, off = t["M"], t["off"]
        want = K.OWN if M <= off and M <= K.SHORT else K.COOP_PLAIN if M <= off else K.MASK if off in K.PERIODS + (16,) else K.BYTE_LOOP
        assert t["cls"] == want and t["lane"] == 0, (c["name"], t["cls"], want)
    assert sum(K.masked_moves(c) for c in corpus()) >= 300


def test_the_model_agrees_with_the_emulator():
    """Windows (their starts) and the number of batches, over every case."""
    for c in corpus():
        lay = K.tokens(c)
        rc, stats, log = fw.emulate(c["input"])
        assert rc == 0 and stats["walked_windows"] == 0, (c["name"], rc, stats)
        assert stats["batches"] == len({t["batch"] for t in lay}), (c["name"], stats)
        starts = [pos for kind, pos in log if kind == 0]
        mine = []
        for t in lay:
            if not mine or mine[-1][0] != t["win"]:
                mine.append((t["win"], t["cstart"]))
        assert starts == [s for _, s in mine], c["name"]
