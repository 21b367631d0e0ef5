"""The bitmap-fed decompress kernel decodes each listed token once, in its copy stage, and checks the chain's links batch by batch
(lz4_decompress_batch_phase.inc, LZF_FED_DECODE).  Handcrafted raw blocks put the batch and round edges of that set-up where they
matter — a batch cut at exactly 64 tokens, a round whose last token is lane 63, 0xFF length runs at the first and last lane of a
batch, damage in a later batch of a round after earlier batches were copied, a literal run over whole rounds, a token body past the
staged bytes — with the fed kernel forced for every input (analysis library, LZF_DECOMPRESS_KERNEL=fed, LZF_FED_MIN_IN=1), whole
jobs and every job in three pieces.  One product-dispatch batch beyond the pair kernel's residency takes the fed path on its own.
Statuses, out_len and bytes are compared with the oracle (src/raw/decompress.rs)."""
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
from rust_lz_fear_amd import ffi, synth  # noqa: E402

pytestmark = pytest.mark.gpu

ROUND = 1024          # compressed bytes one round of lzf_decompress_fed_kernel<4096, 32, 352> lists (32 x W)
STAGED = ROUND + 128  # bytes of a round staged in LDS
SPAN_MAX = 4096 // 3  # output bytes one batch may produce
BS = 4 << 20


# raw blocks, sequence by sequence: the builder lives in seg_stage_cases.py (test_gpu_parse_staging.py takes _block / _walk from here)
from seg_stage_cases import _lsic, _seq, _block, _walk  # noqa: E402,F401


def _batches(blk):
    """The fed kernel's batches over a valid block: (round, first token index in the round, nb_try, nb, token list of the round).
    A round lists the tokens that start in it; a batch is up to 64 of them, cut where the output passes SPAN_MAX (nb 0: one solo
    sequence)."""
    toks = _walk(blk)
    by_round = {}
    for t in toks:
        by_round.setdefault(t[0] // ROUND, []).append(t)
    out = []
    for r in sorted(by_round):
        lst = by_round[r]; tidx = 0
        while tidx < len(lst):
            nb_try = min(64, len(lst) - tidx)
            incl = np.cumsum([min(L + M, 1 << 25) for _, L, M, _ in lst[tidx:tidx + nb_try]])
            over = np.nonzero(incl > SPAN_MAX)[0]
            nb = min(int(over[0]) if len(over) else 64, nb_try)
            out.append((r, tidx, nb_try, nb, lst))
            tidx += max(nb, 1)
    return out


def _lane_of(blk, pos):
    """(round, batch number in the round, lane) of the token at `pos`."""
    k = {}
    for r, tidx, nb_try, nb, lst in _batches(blk):
        k[r] = k.get(r, -1) + 1
        for j, t in enumerate(lst[tidx:tidx + max(nb, 1)]):
            if t[0] == pos:
                return r, k[r], j
    raise AssertionError(f"no token at {pos}")


def _cases():
    """(name, block bytes) — each valid block asserts the shape it is there for."""
    cases = []
    # dense tokens (3 bytes, 4..6 output bytes): 341 per round, batches of exactly 64 whose last token's successor is the next
    # batch's first
    dense = _block([(8, 4)] + [(0, 4 + (i % 3)) for i in range(1500)])
    assert any(nb == 64 and tidx + 64 < len(lst) for _, tidx, _, nb, lst in _batches(dense))
    cases.append(("dense", dense))
    # 16-byte sequences (13 literals, 4..8 match bytes): 64 tokens fill a round exactly, the round's last token is lane 63
    r64 = _block([(13, 4 + (i % 5)) for i in range(64 * 6)])
    assert _walk(r64)[64][0] == ROUND
    assert all(nb == 64 and tidx == 0 and len(lst) == 64 for r, tidx, _, nb, lst in _batches(r64) if r < 5)
    cases.append(("round of 64", r64))
    # 8-byte sequences: 128 tokens per round, its last token lane 63 of its second batch
    r128 = _block([(5, 4 + (i % 4)) for i in range(128 * 5)])
    assert all(nb == 64 and len(lst) == 128 for r, _, _, nb, lst in _batches(r128) if r < 4)
    cases.append(("round of 128", r128))
    # 0xFF runs (literal length 15 + 255 + x, match length 19 + 255 + x) at the first lane of batches, and at lane 63 of a batch
    # of 64 (63 short tokens before it)
    seqs = []
    for i in range(900):
        k = i % 64
        seqs.append((15 + 255 + 7, 4) if k == 0 and (i // 64) % 2 == 0 else (2, 19 + 255 + 9) if k == 0 else
                    (1, 19 + 255 + 3) if k == 63 and (i // 64) % 2 == 0 else (15 + 255 + 1, 5) if k == 63 else (0, 4))
    runs = _block(seqs)
    edge = _block([(4, 4)] + [(0, 4)] * 62 + [(15 + 255 + 2, 4)] + [(0, 4)] * 200 + [(2, 19 + 255)] + [(0, 5)] * 300)
    assert _lane_of(edge, _walk(edge)[63][0]) == (0, 0, 63)
    lanes = {_lane_of(b, p)[2] for b in (runs, edge) for p, L, M, _ in _walk(b) if L >= 270 or M >= 274}
    assert {0, 63} <= lanes, lanes
    cases += [("0xFF runs at batch edges", runs), ("0xFF run at lane 63", edge)]
    # one literal run over several whole rounds, then short tokens again (a solo sequence, rounds the chain jumps over)
    longlit = _block([(20, 6)] * 50 + [(5 * ROUND + 77, 30)] + [(3, 5)] * 400 + [(4000, 4)] + [(1, 4)] * 200)
    assert max(L for _, L, _, _ in _walk(longlit)) > 3 * ROUND
    cases.append(("literals over whole rounds", longlit))
    # token bodies that end beyond the staged bytes: a token 8 bytes before a round's end whose match-length byte (and literals)
    # lie past ROUND + 128 (3- and 4-byte sequences move it there)
    seqs = [(9, 4)] * 100
    d = (ROUND - 8 - (len(_block(seqs, tail=b"")) - 1)) % ROUND       # (less the last literals token)
    d += ROUND if d < 8 else 0
    seqs += [(1, 4)] * (d % 3) + [(0, 4)] * ((d - 4 * (d % 3)) // 3)
    body = _block(seqs + [(140, 40), (0, 4)] * 3 + [(200, 300)] + [(1, 4)] * 400)
    assert _walk(body)[len(seqs)][0] % ROUND == ROUND - 8
    far = [t for t in _walk(body) if t[3] is not None and t[3] - t[0] // ROUND * ROUND >= STAGED]
    assert far, "no match-length byte beyond the staged bytes"
    cases.append(("body past the staged bytes", body))
    return cases


def _damaged(cases):
    """Damage in the second or a later batch of a round (earlier batches of the round already copied) and truncations."""
    out = []
    for name, blk in cases:
        bt = _batches(blk)
        later = [(r, tidx, nb, lst) for r, tidx, _, nb, lst in bt if tidx > 0 and nb > 4]
        if not later:
            continue
        r, tidx, nb, lst = later[len(later) // 2]
        p, L, M, _ = lst[tidx + nb // 2]
        q = p + 1 + (0 if L < 15 else 1 + (L - 15) // 255) + L          # the match offset of that token
        if M:
            b = bytearray(blk); b[q] = 0; b[q + 1] = 0
            out.append((name + ": zero offset", bytes(b)))
            b = bytearray(blk); b[q] = 0xFF; b[q + 1] = 0xFF
            out.append((name + ": offset beyond the output", bytes(b)))
        b = bytearray(blk); b[p] = 0xF0 | (b[p] & 15); b[p + 1:p + 2] = b"\xff\xff\xff\x40"
        out.append((name + ": long literal run inserted", bytes(b)))
        b = bytearray(blk); b[p] ^= 0x5A
        out.append((name + ": token byte flipped", bytes(b)))
        out.append((name + ": truncated inside the batch", blk[:p + 2]))
        out.append((name + ": truncated after a token byte", blk[:p + 1]))
    return out


def child():
    cases = _cases()
    items, exp, names = [], [], []
    for name, blk in cases + _damaged(cases):
        e = o.decompress_raw(blk, limit=1 << 22, cap=(1 << 22) + len(blk) + 64)
        items.append(dict(input=blk, limit=1 << 22, out_cap=(1 << 22) + len(blk) + 64)); exp.append(e); names.append(name)
        if e[0] == 0:      # exact-fit and short output capacity
            for cap in (len(e[1]), len(e[1]) - 1):
                items.append(dict(input=blk, limit=len(e[1]), out_cap=max(cap, 0)))
                exp.append(o.decompress_raw(blk, limit=len(e[1]), cap=max(cap, 0))); names.append(f"{name} cap {cap}")
    assert sum(e[0] == 0 for e in exp) >= len(cases) and len({e[0] for e in exp}) >= 3
    res = ffi.decompress_blocks_host(items)
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    assert launch.startswith("bitmap-fed"), launch
    for name, (erc, eout), (rc, out) in zip(names, exp, res):
        assert rc == erc, (name, rc, erc)
        if rc == 0:
            assert out == eout, name
    print("fed decode ok:", len(items), "jobs", launch)


@pytest.mark.parametrize("pieces", ["1", "3"])
def test_fed_kernel_batch_and_round_edges(pieces):
    """The handcrafted blocks through the forced fed kernel: whole jobs and every job in three pieces (each piece picks up the
    chain carry of the piece before it)."""
    from rust_lz_fear_amd import build
    env = dict(os.environ, LZF_LIB_PATH=build.build_analysis_library(), LZF_DECOMPRESS_KERNEL="fed", LZF_FED_MIN_IN="1",
               LZF_FED_PIECES=pieces)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "fed decode ok" in r.stdout


def _damage(rng, c):
    b = bytearray(c)
    kind = int(rng.integers(0, 3))
    if kind == 0:
        for _ in range(int(rng.integers(1, 6))):
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
    elif kind == 1:
        del b[int(rng.integers(1, len(b))):]
    else:
        i = int(rng.integers(len(b) // 3, len(b)))
        b[i:] = bytes(rng.integers(0, 256, len(b) - i, dtype=np.uint8))
    return bytes(b)


def test_product_dispatch_beyond_the_pair_kernel_residency():
    """3 400 jobs of 4 MiB (beyond the pair kernel's 12 blocks per CU on 256 CUs): the product dispatch takes the bitmap-fed path.
    Inputs alias 40 distinct compressed blocks; a tenth of the jobs are damaged or truncated.  Statuses and out_len equal the
    oracle's, the bytes of every Ok job too."""
    import torch
    from rust_lz_fear_amd import device
    rng = np.random.default_rng(3400)
    n_jobs, n_good, n_bad = 3400, 32, 8
    raws = [synth.silesia_mix(k * BS, (k + 1) * BS).tobytes() for k in range(n_good)]
    comps = [o.compress2(d)[1] for d in raws]
    bads = [_damage(rng, comps[k % n_good]) for k in range(n_bad)]
    exp_bad = [o.decompress_raw(m, limit=BS, cap=BS) for m in bads]
    assert len({e[0] for e in exp_bad}) >= 2
    inputs = comps + bads
    offs = np.cumsum([0] + [len(c) + 64 for c in inputs])
    h_in = np.zeros(int(offs[-1]), dtype=np.uint8)
    for c, a in zip(inputs, offs):
        h_in[a:a + len(c)] = np.frombuffer(c, dtype=np.uint8)
    d_in = torch.from_numpy(h_in).cuda()
    which = np.array([n_good + (i // 10) % n_bad if i % 10 == 3 else i % n_good for i in range(n_jobs)])
    d_out = torch.empty(n_jobs * BS, dtype=torch.uint8, device="cuda")
    dj = np.zeros(n_jobs, dtype=device.DJOB)
    dj["input"] = d_in.data_ptr() + offs[which].astype(np.uint64)
    dj["input_len"] = [len(inputs[k]) for k in which]
    dj["out"] = d_out.data_ptr() + np.arange(n_jobs, dtype=np.uint64) * BS
    dj["out_cap"] = BS
    dj["output_limit"] = BS
    d_res = torch.zeros(n_jobs * 16, dtype=torch.uint8, device="cuda")
    device.decompress_batch(device.to_device(dj, "cuda"), d_res, n_jobs)
    torch.cuda.synchronize()
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    assert launch.startswith("bitmap-fed"), launch
    res = device.results_to_host(d_res, n_jobs)
    outv = d_out.view(n_jobs, BS)
    for k in range(n_good + n_bad):
        idx = np.nonzero(which == k)[0]
        erc, eout = (0, raws[k]) if k < n_good else exp_bad[k - n_good]
        assert (res["status"][idx] == erc).all(), (k, set(res["status"][idx].tolist()), erc)
        if erc == 0:
            assert (res["out_len"][idx] == len(eout)).all(), k
            ref = torch.from_numpy(np.frombuffer(eout, dtype=np.uint8).copy()).cuda()
            for i in range(0, len(idx), 32):
                sel = torch.from_numpy(idx[i:i + 32]).cuda()
                assert bool((outv.index_select(0, sel)[:, :len(eout)] == ref).all()), k


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child()
