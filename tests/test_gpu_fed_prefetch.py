"""The round edges of the bitmap-fed decompress kernel where a guess about the NEXT round would matter.  The kernel stages one round
(1 024 compressed bytes + 128 for the bodies of its last tokens) at a time (lz4_decompress_feed_phase.inc, F0); builds that asked
for the following round while the current one was copied were measured and not kept (profiles/fed_residency_prefetch.txt), and
these cases are what any such build has to pass.  Handcrafted raw blocks: literal runs that jump over the round that would have
been predicted, input lengths on both sides of the last round that lies in the input with all of its 1 152 staged bytes, a piece
boundary directly behind a whole round, damage in the round behind a good one (the kernel gives the job up to the pair kernel
there) — with the fed kernel forced for every input (analysis library, LZF_DECOMPRESS_KERNEL=fed, LZF_FED_MIN_IN=1), whole jobs
and every job in 3 and 16 pieces.  Statuses, out_len and bytes are compared with the oracle (src/raw/decompress.rs); the same set
goes through the red-zone harness with the inputs at address residues 0, 1 and 15: a result that depends on bytes behind input_len
fails."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import oracle_ffi as o  # noqa: E402
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import ffi  # noqa: E402
from test_gpu_fed_decode_once import ROUND, STAGED, _block, _walk  # noqa: E402

pytestmark = pytest.mark.gpu

LIMIT = 1 << 22


def _pad(nbytes):
    """Sequences without literal-run or match-length extension bytes that encode to exactly nbytes (0, 3, 4 or >= 6)."""
    b = nbytes % 3                      # 4-byte sequences (one literal); the rest 3-byte ones (no literal)
    assert nbytes >= 4 * b, nbytes
    return [(1, 4 + (i % 11)) for i in range(b)] + [(0, 4 + (i % 7)) for i in range((nbytes - 4 * b) // 3)]


def _fill(nbytes):
    """Sequences that encode to exactly nbytes (>= 40): 16-byte ones (64 tokens per round) and a few short ones behind them."""
    bulk = (nbytes - 11 - 12) // 16
    seqs = [(8, 4)] + [(13, 4 + (i % 5)) for i in range(bulk)]
    return seqs + _pad(nbytes - 11 - 16 * bulk)


def _sized(n):
    """A valid block of exactly n compressed bytes (the last literals are 6 bytes)."""
    blk = _block(_fill(n - 7), tail=b"ending")
    assert len(blk) == n, (len(blk), n)
    return blk


def _cases():
    """(name, block bytes) of valid blocks; each asserts the shape it is there for."""
    cases = []
    # a literal run of r rounds in a token that starts at offset d of round 2: the rounds behind round 2 hold no token (a prediction
    # of "round 3" is wrong unless r = 1 and d < 1 023), the chain goes on r rounds later
    for r in (1, 2, 3):
        for d in (0, 1, ROUND - 1):
            head = _fill(2 * ROUND + d)
            blk = _block(head + [(r * ROUND, 9)] + _fill(3 * ROUND + 100), tail=b"ending")
            toks = _walk(blk)
            p, L, _, _ = toks[len(head)]
            assert p == 2 * ROUND + d and L == r * ROUND
            nxt = toks[len(head) + 1][0]
            assert nxt // ROUND >= 2 + r and not any(2 < t[0] // ROUND < nxt // ROUND for t in toks)
            cases.append((f"literal run of {r} rounds from round offset {d}", blk))
    # input lengths around k rounds: the last whole round on both sides of "all of its staged bytes are input"
    for k in (1, 2, 17):
        for d in (-129, -128, -127, -1, 0, 1, 127, 128, 129):
            cases.append((f"input of {k} rounds {d:+d} bytes", _sized(k * ROUND + d)))
    assert STAGED - ROUND == 128
    # a piece boundary directly behind a whole round: 5 rounds in 3 pieces (2 + 2 + 1), 33 rounds in 16 (3 each; 11 pieces used)
    for rounds in (5, 33):
        for d in (0, -10):
            blk = _sized(rounds * ROUND + d)
            assert (len(blk) + ROUND - 1) // ROUND == rounds
            cases.append((f"{rounds} rounds {d:+d} bytes", blk))
    return cases


def _damaged():
    """A token byte changed in the round BEHIND a good one: once so that the reference rejects the block, once so that the block
    stays valid and decodes to something else."""
    out = []
    for rounds, r in ((8, 3), (8, 7), (33, 17)):
        blk = _sized(rounds * ROUND + 300)
        good = o.decompress_raw(blk, limit=LIMIT, cap=LIMIT)
        assert good[0] == 0
        p = next(t[0] for t in _walk(blk) if t[0] >= r * ROUND)          # the first token of round r
        assert p // ROUND == r
        bad = other = None
        for v in range(256):
            if v == blk[p]:
                continue
            b = bytes(blk[:p]) + bytes([v]) + bytes(blk[p + 1:])
            e = o.decompress_raw(b, limit=LIMIT, cap=LIMIT)
            if e[0] != 0 and bad is None:
                bad = b
            if e[0] == 0 and e[1] != good[1] and other is None:
                other = b
        assert bad is not None and other is not None, (rounds, r)
        out.append((f"{rounds} rounds, token of round {r} changed: invalid", bad))
        out.append((f"{rounds} rounds, token of round {r} changed: still valid", other))
    return out


def _items():
    items, exp, names = [], [], []
    for name, blk in _cases() + _damaged():
        cap = LIMIT + len(blk) + 64
        items.append(dict(input=blk, limit=LIMIT, out_cap=cap)); exp.append(o.decompress_raw(blk, limit=LIMIT, cap=cap)); names.append(name)
    n_valid = len(_cases())
    assert all(e[0] == 0 for e in exp[:n_valid]) and sum(e[0] != 0 for e in exp[n_valid:]) == 3
    return items, exp, names


def child(mode):
    items, exp, names = _items()
    if mode == "plain":
        res = ffi.decompress_blocks_host(items)
        launch = ffi.lib().lzf_last_decompress_launch().decode()
        assert launch.startswith("bitmap-fed"), launch
        for name, (erc, eout), (rc, out) in zip(names, exp, res):
            assert rc == erc, (name, rc, erc)
            if rc == 0:
                assert out == eout, name
    else:
        import redzone
        for low in (0, 1, 15):
            redzone.check_decompress(items, exp, f"prefetch edges, input & 15 = {low}", max_input_len=max(len(it["input"]) for it in items),
                                     in_low=[low] * len(items))
            launch = ffi.lib().lzf_last_decompress_launch().decode()
            assert launch.startswith("bitmap-fed"), launch
    print("fed prefetch ok:", mode, len(items), "jobs", launch)


def _run(mode, pieces):
    from rust_lz_fear_amd import build
    env = dict(os.environ, LZF_LIB_PATH=build.build_analysis_library(), LZF_DECOMPRESS_KERNEL="fed", LZF_FED_MIN_IN="1",
               LZF_FED_PIECES=pieces)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", mode], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "fed prefetch ok" in r.stdout


@pytest.mark.parametrize("pieces", ["1", "3", "16"])
def test_fed_prefetch_edges(pieces):
    """Skipped rounds, the last prefetchable round, piece boundaries and damage behind a good round: the oracle's statuses and bytes."""
    _run("plain", pieces)


@pytest.mark.parametrize("pieces", ["1", "3", "16"])
def test_fed_prefetch_edges_in_red_zones(pieces):
    """The same jobs between poison: nothing read behind input_len matters, nothing written outside the output slots."""
    _run("redzone", pieces)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "child":
        child(sys.argv[2])
