"""The census of tests/copy_stage_cases.py: a condition, not a measurement.  For every geometry of the batched kernels' copy stage (paired48,
paired24, staged16, fed) and every output residue (0, 1, 15) the built blocks reach every named edge of the stage — both sides of every
threshold — with bytes that tell a wrong copy apart; every case is what the oracle says it is, status and bytes; the model's batches for the fed
geometry are the window emulator's.  No GPU: the reach of the cases is proven here, before tests/test_gpu_copy_stage.py asks the device."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import oracle_ffi as o  # noqa: E402
import rust_lz_fear_amd  # noqa: E402,F401
import copy_stage_cases as K  # noqa: E402

GEOMS = tuple(K.GEOMS)


@pytest.fixture(scope="module", params=[(g, rb) for g in GEOMS for rb in K.RESIDUES], ids=lambda p: f"{p[0]}-rb{p[1]}")
def reach(request):
    g, rb = request.param
    return (K.GEOMS[g], rb) + K.reach(g, rb)


def test_constants_hold_together():
    """The literals of the geometries against each other (a constant changed by one breaks a relation here, or an edge below)."""
    assert (K.KSHORT, K.KFARSHORT) == (64, 32)
    for g in K.GEOMS.values():
        assert g.ring == 4096 and g.span == g.ring // 3 and g.hist == g.ring - g.span
        assert g.kcb == g.cover + (64 if g.rule == "chunk" else 128) and 64 < g.tokcap < g.cover
    assert [K.GEOMS[n].cover for n in GEOMS] == [64 * 48, 64 * 24, 64 * 16, 32 * 32]
    # the two edges the fed geometry cannot have: an own share (64 bytes at most) of a batch's token (it starts in the window's 1 024 bytes, with at
    # most 7 bytes of token and lengths in front of its literals) ends at 1 023 + 7 + 64 < kCB
    fed = K.GEOMS["fed"]
    assert fed.cover - 1 + 7 + K.KSHORT < fed.kcb
    assert K.edges(fed) == K.edges(K.GEOMS["paired48"]) - {"literals: own share ends at kCB", "literals: own share ends one byte beyond kCB"}
    for n in GEOMS[:3]:
        assert K.edges(K.GEOMS[n]) == K.edges(K.GEOMS["paired48"])


def test_every_named_edge_is_reached(reach):
    g, rb, cases, models, got = reach
    want = K.edges(g)
    assert got >= want, f"{g.name} rb {rb}: not reached: {sorted(want - got)}"
    assert got <= want, sorted(got - want)


@pytest.mark.parametrize("mut", K.MUTANTS)
def test_a_rule_moved_by_one_changes_the_counts(reach, mut):
    """The reach of the blocks, the other way round: with one comparison of the match classification (.inc:225-233, :344) or one threshold moved
    by one, the model's batches or rounds differ for some valid block — so the equalities test_gpu_copy_stage.py asserts on the device cannot hold
    for a kernel that has the rule off by one."""
    g, rb, cases, models, got = reach
    changed = [c["name"] for c, m in zip(cases, models) if c["status"] == K.OK and
               (lambda x: (x.nbatch, x.rounds) != (m.nbatch, m.rounds))(K.model(c["input"], g, rb, len(c["prefix"]), len(c["existing"]), c["limit"], c["cap"], mut=mut))]
    assert changed, f"{g.name} rb {rb}: no block's counts notice '{mut}'"


def test_every_case_owns_an_edge(reach):
    """No case is there for nothing: each reaches an edge no other case reaches, so a removed case fails the census, which names that edge."""
    g, rb, cases, models, got = reach
    per = [K.census(c, g, rb, m) for c, m in zip(cases, models)]
    for i, c in enumerate(cases):
        rest = set().union(*(p for k, p in enumerate(per) if k != i))
        assert per[i] - rest, f"{g.name} rb {rb}: '{c['name']}' owns no edge"


def test_the_oracle_agrees_with_builder_and_model(reach):
    g, rb, cases, models, got = reach
    for c, m in zip(cases, models):
        rc, out = o.decompress_raw(c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"], cap=c["cap"])
        assert rc == c["status"] == m.status, (c["name"], o.STATUS_NAMES[rc], o.STATUS_NAMES[c["status"]], o.STATUS_NAMES[m.status])
        if rc == K.OK:
            assert out == c["output"], c["name"]


@pytest.mark.parametrize("rb", K.RESIDUES)
def test_fed_batches_are_the_emulators(rb):
    import fed_window_cases as fw
    cases, models, _ = K.reach("fed", rb)
    n = 0
    for c, m in zip(cases, models):
        if c["status"] != K.OK:
            continue
        rc, st, _ = fw.emulate(c["input"], want_log=False)
        assert rc == 0 and st["batches"] == m.nbatch, (c["name"], st["batches"], m.nbatch)
        assert st["solo"] == sum(b["solo"] for b in m.batches) and st["tokens"] == len(m.toks), c["name"]
        n += 1
    assert n >= 20


@pytest.mark.parametrize("rb", K.RESIDUES)
def test_a_job_the_fed_kernel_hands_back_cannot_pass_for_finished(rb):
    """The counter build the fed batch equality is read from lets the pair kernel <4096,24,384>, which decodes every job the fed kernel gives up,
    write its ROUND count where the fed kernel writes its batch count (its batch count would not do: the two kernels cut the same batches for
    most blocks).  For every valid block of the fed geometry the two differ, so the equality on the device holds only for a job the fed kernel
    finished."""
    from rust_lz_fear_amd.build import COUNTER_BUILDS
    assert set(COUNTER_BUILDS[0]) == {"LZF_DBG_ROUNDS=1", "LZF_DBG_FED_COUNT=0"}
    cases, models, _ = K.reach("fed", rb)
    same = []
    for c, m in zip(cases, models):
        if c["status"] == K.OK:
            p = K.run_model(c, K.GEOMS["paired24"], rb)
            assert p.status == K.OK
            if m.nbatch == p.rounds:
                same.append(f"'{c['name']}': {p.rounds} rounds in the pair kernel, {m.nbatch} batches in the fed kernel")
    assert not same, f"rb {rb}: " + "; ".join(same)


def test_sizes_stay_small(reach):
    g, rb, cases, models, got = reach
    assert len(cases) * len(K.RESIDUES) <= K.JOBS_MAX          # a GPU child sends every case at every residue in one call
    for c in cases:
        assert len(c["input"]) < K.INPUT_MAX and len(c["output"]) < K.OUTPUT_MAX, (c["name"], len(c["input"]), len(c["output"]))
