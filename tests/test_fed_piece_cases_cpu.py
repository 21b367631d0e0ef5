"""CPU tests (no GPU) of the piece hand-over of the bitmap-fed decompress kernel: the piece rules of rust-lz-fear_amd/csrc/lzf_fed_window.h (where a
piece ends, which group serves a job, ticket -> (piece, rank)) through the functions the kernel itself compiles, and the built cases of
tests/fed_piece_cases.py against the emulator of the kernel's window loop run piece by piece (tests/emu/emu_fed_window.cpp): every case reaches the
edge it was built for, the corpus reaches every named edge, and the emulator's guarantees hold per piece — progress, every true token taken exactly
once and in order, a parked `o` that is the output of the tokens below the parked `expect`, no work behind the piece that ends a job.  The rule of
the expiry path (a hand-over wait that runs out) is stated in the emulator and tested here: it is not provoked on a GPU."""
import pytest

import fed_piece_cases as K
from fed_piece_cases import ROUND


@pytest.fixture(scope="module")
def corpus():
    return K.corpus()


def test_every_case_reaches_its_edge_and_the_corpus_every_edge(corpus):
    got = K.reach()                       # (asserts every case's own edges)
    missing = K.edges() - set(got)
    assert not missing, sorted(missing)
    # the edges the GPU tests rely on are reached at a piece count they run
    for e in K.edges():
        assert any(p in K.PIECES for _, p in got[e]), e
    assert {r for c in corpus for r in [K.rounds_of(len(c["input"]))]} >= {1, 2, 3, 4, 5, 6, 12, 16, 32, 33, 48}
    for e in sorted(got):
        print(f"{len(got[e]):4d}  {e}")


def test_piece_end_against_the_rule_spelled_out():
    """Every piece but the last is ceil(rounds / pieces) whole rounds; the piece that reaches the last round ends at len, and so do those behind it."""
    for n in list(range(1, 40)) + [1023, 1024, 1025, 2047, 2048, 2049, 5 * ROUND, 5 * ROUND + 1, 48 * ROUND, 48 * ROUND + 1, (4 << 20) - 1, 4 << 20, (4 << 20) + 1]:
        rounds = -(-n // ROUND)
        for pieces in (1, 2, 3, 16, rounds + 1, 64, 4096):
            per = -(-rounds // pieces)
            ends = [K.piece_end(n, pieces, p) for p in range(pieces)]
            assert ends == [min((p + 1) * per * ROUND, n) if (p + 1) * per < rounds else n for p in range(pieces)], (n, pieces)
            assert ends[-1] == n and ends == sorted(ends) and all(e == n or e % ROUND == 0 for e in ends)


@pytest.mark.parametrize("mask", [0xFF, 0x0F, 0x01, 0xA5])
def test_ticket_map(mask):
    """The kernel's ticket loop over the functions of the header: every (job, piece) pair is handed to exactly one group exactly once, a job's
    pieces stay in one group, and piece p - 1 of a job is drawn n_g tickets before its piece p."""
    L = K._lib()
    xccs = [i for i in range(32) if mask >> i & 1]
    ng = len(xccs)
    for n in list(range(1, 71)) + [255, 256, 257, 1000, 12240]:
        for pieces in (1, 2, 3, 16):
            seen = {}
            for xcc in xccs:
                g = bin(mask & ((1 << xcc) - 1)).count("1")          # the kernel: popc(mask & ((1 << xcc) - 1))
                n_g = L.lzf_emu_fedw_group_jobs(n, g, ng)
                assert n_g == len(range(g, n, ng))
                for tk in range(n_g * pieces):
                    piece = L.lzf_emu_fedw_ticket_piece(tk, n_g)
                    k = L.lzf_emu_fedw_ticket_rank(tk, piece, n_g, g, ng)
                    assert piece < pieces and k < n and k % ng == g, (n, pieces, g, tk, piece, k)
                    assert (k, piece) not in seen, (n, pieces, g, tk)
                    seen[(k, piece)] = (g, tk)
            assert len(seen) == n * pieces
            for (k, piece), (g, tk) in seen.items():
                if piece:
                    g0, tk0 = seen[(k, piece - 1)]
                    assert g0 == g and tk - tk0 == L.lzf_emu_fedw_group_jobs(n, g, ng)


def test_per_piece_guarantees(corpus):
    """What the model says per piece, held against the token walk: the pieces' tokens add up to the chain, the parked state is consistent, a job
    that ends in piece p has no work behind it, and the whole job in one piece is the emulator's single-piece answer."""
    for c in corpus:
        toks = K.tokens(c["input"])
        n = len(c["input"])
        ex = len(c["existing"])
        for pieces in sorted({1, 2, 3, 16, K.rounds_of(n) + 1}):
            m = K.model(c, pieces)
            assert m.rc == 0, (c["name"], pieces, m.rc)          # progress, order, overrun below a window (the emulator's return codes)
            valid = c["exp"][0] == 0
            assert bool(m.done) == valid, (c["name"], pieces)
            assert m.end_piece is not None
            for p, r in enumerate(m.rec):
                if p > m.end_piece:
                    assert r["what"] == K.PASS and r["listed"] == r["walked"] == r["batches"] == r["tokens"] == 0
                elif p < m.end_piece:
                    assert r["what"] in (K.PARKED, K.PARKED_AT_ONCE)
                    E = K.piece_end(n, pieces, p)
                    assert E <= r["expect"] < n and r["expect"] < E + ROUND + max(t[4] - t[0] for t in toks)
                    below = [t for t in toks if t[0] < r["expect"]]
                    assert r["o"] == ex + sum(t[1] + t[2] for t in below) and sum(x["tokens"] for x in m.rec[:p + 1]) == len(below)
                    if r["what"] == K.PARKED_AT_ONCE:
                        assert (r["expect"], r["listed"], r["batches"], r["tokens"]) == (r["took"], 0, 0, 0)
                    else:
                        assert r["batches"] >= 1 and r["listed"] >= 1 and r["batches"] >= r["listed"] - r["walked"]
            if valid:
                assert K.decode_below(c, n) == c["exp"][1], c["name"]            # (the plain decoder the GPU test takes parked bytes from)
                assert m.taken == len(toks) == m.stats["tokens"] and m.rec[m.end_piece]["what"] == K.FINISHED
                assert m.flag == (K.ENDED if pieces > 1 else 0)
            else:
                assert m.rec[m.end_piece]["what"] in (K.WALK_FAILED, K.STATUS)
            if pieces == 1 and valid:
                rc, st, _ = K.fw.emulate(c["input"], want_log=False)
                assert rc == 0 and st == m.stats


def test_expired_wait_rule(corpus):
    """The expiry path's rule: the piece whose wait runs out skips, every piece behind it expires too, the job stays !done and its flag is what
    the last piece that ran left — not kFedEnded, so nothing marks the job as dealt with and the pair kernel takes it."""
    tried = 0
    for c in corpus:
        if c["exp"][0] != 0:
            continue
        for pieces in K.PIECES:
            ref = K.model(c, pieces)
            for x in range(1, pieces):
                m = K.model(c, pieces, expire=x)
                assert m.rc == 0
                if ref.end_piece < x:                   # the job had ended before: the ticket passes, nothing expires
                    assert m == ref
                    continue
                tried += 1
                assert not m.done and m.end_piece is None and m.flag == x
                assert m.rec[:x] == ref.rec[:x]
                assert all(r["what"] == K.EXPIRED and r["batches"] == 0 and (r["expect"], r["o"]) == (m.rec[x - 1]["expect"], m.rec[x - 1]["o"]) for r in m.rec[x:])
    assert tried >= 100
