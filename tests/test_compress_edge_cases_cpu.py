"""The corpus of tests/compress_edge_cases.py reaches every candidate rule of raw::compress2 in the reference — proven here, without a
GPU, from the oracle's trace (lzfo_compress2_trace): the census conditions are assertions, the traced oracle is the plain oracle, a
distance rule that is off by one in either direction would change the bytes of these inputs, and the team kernel's source under the
lock-step emulator agrees with the oracle on a subset (one job per class, the distance class at every epoch phase).  The GPU side is
tests/test_gpu_compress_edges.py."""
import ctypes as C

import pytest

import compress_edge_cases as ec
import emu_ffi
import oracle_ffi as o


def test_traced_oracle_is_the_plain_oracle():
    """Status, bytes and the table after the call, every job (chains: after every call)."""
    jobs = ec.corpus()
    plain = ec.run_oracle(jobs, trace=False)
    for j, t, p in zip(jobs, ec.traced(), plain):
        assert (t["rc"], t["out"]) == (p["rc"], p["out"]), (j["cls"], j["name"])
        assert t["table"] == p["table"], (j["cls"], j["name"], "table")
        assert t["rc"] == o.OK, (j["cls"], j["name"], t["rc"])


def test_trace_counts_what_it_cannot_hold():
    j = ec.of_class(ec.corpus(), "block end")[0]
    rc, out, ev = o.compress2_trace(j["input"])
    assert len(ev) > 4
    buf = (o.TraceEvent * 4)()
    n, ne = C.c_size_t(0), C.c_size_t(0)
    ob = C.create_string_buffer(ec.bound(len(j["input"])))
    t = o.new_table()
    rc2 = o.lib().lzfo_compress2_trace(j["input"], len(j["input"]), 0, o.TABLE_U32, C.addressof(t), ob, len(ob), C.byref(n), buf, 4, C.byref(ne))
    assert (rc2, ob.raw[:n.value], ne.value) == (rc, out, len(ev))
    assert [(e.type, e.pos, e.candidate) for e in buf] == [(e["type"], e["pos"], e["candidate"]) for e in o.events_as_dicts(ev[:4])]


def test_census_every_class_reaches_its_rule():
    jobs = ec.corpus()
    cen = ec.census(jobs, ec.traced())
    print(ec.report(cen))
    for cls in ec.CLASSES:
        assert cen[cls]["jobs"] > 0, cls
        assert not cen[cls]["missing"], (cls, cen[cls]["missing"][:10])
    # the grid of the distance class is whole: 3 epochs x 14 phases x 4 distances less the one with no room for the source
    grid = {(j["par"]["e"], j["par"]["ph"], j["par"]["D"]) for j in ec.of_class(jobs, "distance") if j["cursor"] == 0}
    assert len(grid) == 167
    assert {(j["cursor"], j["par"]["ph"]) for j in ec.of_class(jobs, "distance") if j["cursor"]} == {(c, ph) for c in (1, 4096) for ph in (0, 1, 65535)}
    assert cen["backtrack"]["counts"]["over-read variants kept"] >= 8
    zero_runs = [j for j in ec.of_class(jobs, "backtrack") if j["par"]["stop"] == "candidate 0"]
    assert cen["backtrack"]["counts"]["stopped at candidate 0, backtrack >= 1 (second zero run)"] == len(zero_runs) == 56
    assert sum(j["kind"] == o.TABLE_U16 for j in jobs) > 1000


# -------------------------------------------------------------------------------------------------- a wrong distance rule changes bytes
def _predict(j, events, bound):
    """The sequences a walk with `cursor - candidate <= bound` in the place of mod.rs:201 emits, as far as the oracle's trace decides
    them: the oracle's own up to the first probe whose verdict flips, then the flipped one (a refused repeat that is now a match: its
    sequence; a match that is now refused: None).  Not a compressor: what follows a flipped verdict is not predicted."""
    d, seqs = j["input"], []
    for e in ec.dicts(events):
        dist = e["pos"] - e["candidate"]
        if e["type"] == o.EV_MATCH:
            if dist > bound:
                return seqs + [None]
            seqs.append((e["pos"] - e["backtrack"] - e["literal_start"], dist, e["matching_bytes"] + e["backtrack"]))
        elif e["type"] == o.EV_REFUSED and not e["flags"] & o.REFUSED_FIRST_POSITION and dist <= bound:
            bt = 0
            while bt < e["pos"] - e["literal_start"] and bt < e["candidate"] and d[e["pos"] - 1 - bt] == d[e["candidate"] - 1 - bt]:
                bt += 1
            return seqs + [(e["pos"] - bt - e["literal_start"], dist, e["matching_bytes"] + bt)]
    return seqs


def test_a_distance_rule_off_by_one_changes_the_sequences():
    """With the bound at 0xFFFE every D = 65535 input, with 0x10000 every D = 65536 input parses differently from the oracle (and the
    inputs on the right side of either bound do not): a kernel off by one in either direction fails on them."""
    jobs = ec.corpus()
    n = {}
    for j, r in zip(jobs, ec.traced()):
        if j["cls"] != "distance":
            continue
        ev, D, c = r["events"], j["par"]["D"], j["par"]["c"]
        # up to the plant (what a flipped verdict there changes is the point), and only the probes either bound can flip: the text's own
        # matches, thousands per job, are the same under all three bounds
        ev = ev[(ev["type"] != o.EV_SHORT_INSERT) & (ev["pos"] <= c) & (ev["pos"] - ev["candidate"] >= 0xFFFE)]
        seqs = ec.sequences(j, ev)[0]
        assert _predict(j, ev, 0xFFFF) == seqs, j["name"]
        low, high = _predict(j, ev, 0xFFFE), _predict(j, ev, 0x10000)
        assert (low != seqs) == (D == 65535), (j["name"], "bound 0xFFFE")
        assert (high != seqs) == (D == 65536), (j["name"], "bound 0x10000")
        if D == 65535:
            assert low[-1] is None and len(low) == len(seqs), j["name"]
        if D == 65536:
            assert high[-1] == (0, 65536, 24) and len(high) == len(seqs) + 1, j["name"]
        if D in (65535, 65536):
            n[D] = n.get(D, 0) + 1
    # cursor 0: 42 (epoch, phase) pairs each; cursor 1: 9 and 8 (the source of e1 ph0 D65536 would lie in front of the cursor); cursor 4096: 7 each
    assert n == {65535: 42 + 9 + 7, 65536: 42 + 8 + 7}, n


# ----------------------------------------------------------------------------------------------------- the team kernel's source, emulated
def _emulate(jobs):
    """Jobs through emu_ffi.compress_batch (fresh tables in one batch; a chain call by call on a caller-owned table) against the
    oracle: status, bytes, and a chain's table after every call."""
    want = ec.run_oracle(jobs, trace=False)
    fresh = [(j, w) for j, w in zip(jobs, want) if j["chain"] is None]
    if fresh:
        res, _ = emu_ffi.compress_batch([j["input"] for j, _ in fresh], cursors=[j["cursor"] for j, _ in fresh], caps=[j["cap"] for j, _ in fresh])
        for (j, w), (rc, out) in zip(fresh, res):
            assert (rc, out) == (w["rc"], w["out"]), (j["cls"], j["name"])
    tables = {}
    for j, w in zip(jobs, want):
        if j["chain"] is None:
            continue
        t = tables.setdefault(j["chain"], o.new_table())
        t.offset += j["offset_add"]
        (rc, out), = emu_ffi.compress_batch([j["input"]], cursors=[j["cursor"]], caps=[j["cap"]], tables=[t], writable=True, alone=0)[0]
        assert (rc, out) == (w["rc"], w["out"]), (j["cls"], j["name"])
        assert bytes(t) == w["table"], (j["cls"], j["name"], "table after the call")


def test_emulated_team_kernel_one_job_per_class():
    jobs = ec.corpus()
    pick = []
    for cls in ec.CLASSES:
        if cls in ("distance", "u16"):              # (distance: the test below; the team kernel takes no U16 table)
            continue
        mine = ec.of_class(jobs, cls)
        if cls in ("stale slot", "first position"):
            ch = [j["chain"] for j in mine if j["chain"]][0]
            pick += [j for j in mine if j["chain"] == ch]
        if cls == "first position":
            pick += [j for j in mine if j["chain"] is None][:1]
        if cls == "empty slot":
            pick += [j for j in mine if j["par"]["X"] == 65535][:1]
        if cls == "backtrack":
            pick += [[j for j in mine if j["par"]["stop"] == s][0] for s in ("literal_start", "candidate 0", "over-read")]
        if cls == "skip schedule":
            pick += [j for j in mine if j["par"]["p"] in (100, 101, 300, 301, 302, 900, 903)]
        if cls == "lsic":
            pick += [j for j in mine if j["par"]["v"] in (15, 270, 1035)]
        if cls == "block end":
            pick += [j for j in mine if j["par"]["n"] == 65536 - 12 and j["kind"] == o.TABLE_U32 and j["par"]["what"] in ("text", "final 11", "probe len - 12")][:1]
            pick += [dict(j, input=j["input"][-20000:], name=j["name"] + ", last 20000 bytes") for j in mine
                     if j["par"]["n"] == 65536 - 12 and j["kind"] == o.TABLE_U32 and j["par"]["what"] in ("final 11", "probe len - 12")]
    assert {j["cls"] for j in pick} == set(ec.CLASSES) - {"distance", "u16"}
    assert sum(len(j["input"]) > 60000 for j in pick) <= 2      # (with the 28 distance jobs below: 30 large jobs under the emulator at most)
    _emulate(pick)


@pytest.mark.parametrize("D", [65535, 65536])
def test_emulated_team_kernel_distance_at_every_phase(D):
    """Epoch 2, every phase: 14 jobs of about 130 KB."""
    pick = [j for j in ec.of_class(ec.corpus(), "distance") if j["par"]["e"] == 2 and j["par"]["D"] == D and j["cursor"] == 0]
    assert sorted(j["par"]["ph"] for j in pick) == sorted(ec.PHASES)
    _emulate(pick)
