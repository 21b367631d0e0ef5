"""Handcrafted raw blocks for the windows of the bitmap-fed decompress kernel (test infrastructure; used by
tests/test_fed_window_cpu.py on the CPU and tests/test_gpu_fed_windows.py on the GPU).

The kernel lists the tokens of a window of 1 024 compressed bytes from the bit map of the segmented parse, masks the marks below the
chain's own position, walks a window the map gets wrong token by token, and leaves a short last batch of a window for the next one
(rust-lz-fear_amd/csrc/lzf_fed_window.h).  Every block here puts one of those rules where it matters and asserts, on the CPU, the
shape it is there for: the assertions use the token walk of the block and the emulator of the window loop
(tests/emu/emu_fed_window.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from test_gpu_fed_decode_once import ROUND, SPAN_MAX, STAGED, _seq, _walk

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK, OVERLAP = 16384, 2048
STRIDE = CHUNK - OVERLAP
CARRY = 32            # kFedwCarry
LIMIT = 1 << 22

_emu = None


def emu_lib():
    """tests/emu/emu_fed_window.cpp compiled with g++ (rebuilt when it or the window header is newer)."""
    global _emu
    if _emu is None:
        src = os.path.join(HERE, "emu", "emu_fed_window.cpp")
        hdr = os.path.join(os.path.dirname(HERE), "rust-lz-fear_amd", "csrc", "lzf_fed_window.h")
        so = os.path.join(HERE, "emu", "libemu_fed_window.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so, src])
        L = C.CDLL(so)
        L.lzf_emu_fed_window.restype = C.c_int
        L.lzf_emu_fed_window.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
        _emu = L
    return _emu


STAT_NAMES = ("batches", "map_windows", "walked_windows", "sequences", "under32", "carried", "solo", "tokens")


def emulate(blk, fixed=False, carry=CARRY, drop_chunk=-1, want_log=True):
    """The window loop over one block: (return code, stats dict, log [(kind, position)]) — kind 0 a window listed from the map,
    1 a window walked, 2 a batch left for the next window (position of its first token)."""
    st = (C.c_uint64 * 8)()
    cap = len(blk) // 8 + 64 if want_log else 0
    log = (C.c_uint32 * (2 * cap))() if cap else None
    n = C.c_uint32(0)
    rc = emu_lib().lzf_emu_fed_window(bytes(blk), len(blk), 1 if fixed else 0, carry, drop_chunk, st, log, cap, C.byref(n))
    assert n.value <= cap or not want_log
    pairs = [(log[2 * i], log[2 * i + 1]) for i in range(n.value)] if want_log else []
    return rc, dict(zip(STAT_NAMES, [int(v) for v in st])), pairs


# ------------------------------------------------------------------------------------------------------------ building blocks
def build(seqs, tail=b"ending"):
    """seqs: (literals, M) — literals an int (that many random bytes) or bytes — -> a valid block + the last literals."""
    rng = np.random.default_rng(len(seqs) * 7 + 1)
    out_len, blk = 0, bytearray()
    for lit, M in seqs:
        if isinstance(lit, int):
            lit = bytes(rng.integers(0, 256, lit, dtype=np.uint8))
        out_len += len(lit)
        assert out_len >= 1, "a match needs output before it"
        off = int(rng.integers(1, min(out_len, 3000) + 1))
        blk += _seq(lit, off, M)
        out_len += M
    blk += _seq(tail, None, 0)
    return bytes(blk)


def enc_len(L, M):
    return 1 + (0 if L < 15 else 1 + (L - 15) // 255) + L + 2 + (0 if M - 4 < 15 else 1 + (M - 19) // 255)


def pad(nbytes):
    """Short sequences without extension bytes that encode to exactly nbytes (0, 3, 4 or >= 6)."""
    b = nbytes % 3
    assert nbytes >= 4 * b, nbytes
    return [(1, 4 + (i % 11)) for i in range(b)] + [(0, 4 + (i % 7)) for i in range((nbytes - 4 * b) // 3)]


def fill(nbytes):
    """Sequences that encode to exactly nbytes (>= 40): 16-byte ones and a few short ones behind them."""
    bulk = (nbytes - 11 - 12) // 16
    seqs = [(8, 4)] + [(13, 4 + (i % 5)) for i in range(bulk)]
    return seqs + pad(nbytes - 11 - 16 * bulk)


def stretch(n_tok):
    """n_tok sequences (64 < n_tok <= 128) that encode to exactly 1 KiB."""
    lo = ROUND // n_tok
    n_hi = ROUND - lo * n_tok
    sizes = [lo + 1] * n_hi + [lo] * (n_tok - n_hi)
    assert sum(sizes) == ROUND and lo >= 4
    return [(s - 3, 4 + (i % 6)) for i, s in enumerate(sizes)]


def token_like(n):
    """n literal bytes that read as three-byte tokens (00 xx xx: no literals, a match of four) from every third byte."""
    rng = np.random.default_rng(n)
    b = bytearray(rng.integers(1, 256, n + 3, dtype=np.uint8))
    b[0::3] = bytes(len(b[0::3]))
    return bytes(b[:n])


def false_walk(blk, start, stop):
    """The positions a token walk from `start` steps on below `stop` (the walk of a chunk's parse: it starts at an arbitrary byte)."""
    pos, p, n = [], start, len(blk)
    while p < stop and p < n:
        pos.append(p)
        t = blk[p]; q = p + 1; L = t >> 4
        if L == 15:
            while q < n:
                b = blk[q]; q += 1; L += b
                if b != 255:
                    break
        q += L + 2
        if (t & 15) == 15:
            while q < n:
                b = blk[q]; q += 1
                if b != 255:
                    break
        p = q
    return pos


# ------------------------------------------------------------------------------------------------------------------ the cases
def not_in_step(chunk, rem):
    """A literal run of token-like bytes from in front of chunk `chunk`'s first byte to behind the end of its overlap with the chunk
    before it; the run ends `rem` (1 or 2) mod 3 from the chunk's first byte.  The chunk's own parse walks the run's triples and meets
    no true token inside the overlap, so where the chain enters the chunk's share of the map its marks are not the chain's."""
    c0 = chunk * STRIDE
    head = fill(c0 - 200)
    at = len(build(head, tail=b"")) - 1                       # where the run's token starts
    assert at == c0 - 200
    L = 200 + OVERLAP + 300
    while True:                                                 # (the number of length bytes moves with L)
        lit_start = at + 1 + (1 + (L - 15) // 255)
        if (lit_start + L - c0) % 3 == rem:
            break
        L += 1
    lit = bytearray(np.random.default_rng(chunk).integers(1, 256, L, dtype=np.uint8))
    k = c0 - lit_start
    lit[k:] = token_like(L - k)                                 # a triple starts on the chunk's first byte
    blk = build(head + [(bytes(lit), 7)] + fill(6 * ROUND + 77) + stretch(70) * 3 + fill(3000))
    end = lit_start + L
    assert lit_start < c0 and end > c0 + OVERLAP and (end - c0) % 3 == rem
    true = {t[0] for t in _walk(blk)}
    fw = false_walk(blk, c0, end)
    assert fw[:3] == [c0, c0 + 3, c0 + 6] and not (set(fw) & true), "the chunk's walk meets the chain inside the run"
    return blk, end


def cases():
    """[(name, block)] of valid blocks, 30-50 KiB compressed unless the case needs another size."""
    out = []
    # ---- a chunk that does not fall in step (chunks 1 and 2, both residues of the run's end)
    for chunk in (1, 2):
        for rem in (1, 2):
            blk, end = not_in_step(chunk, rem)
            rc, st, log = emulate(blk)
            assert rc == 0, rc
            if rem == 2:       # the walk leaves the run one byte behind the chain's token: the map is wrong about the window behind the run
                assert st["walked_windows"] >= 1 and any(k == 1 and p <= end < p + ROUND + 64 for k, p in log), (chunk, rem, st)
            out.append((f"chunk {chunk} not in step, run ends {rem} mod 3", blk))
    # ---- a literal run longer than a whole chunk: the chain jumps over chunk 1's share of the map
    blk = build(fill(9000) + [(CHUNK + 7000, 12)] + fill(12000))
    big = max(_walk(blk), key=lambda t: t[1])
    assert big[0] < CHUNK and big[0] + big[1] > STRIDE + OVERLAP + STRIDE
    assert not any(STRIDE + OVERLAP <= t[0] < 2 * STRIDE + OVERLAP for t in _walk(blk)), "a token in chunk 1's share"
    out.append(("literal run over a whole chunk", blk))
    # ---- tails: 1 KiB stretches of 64 + k tokens
    for k in (1, 31, 32, 33, 63):
        blk = build(stretch(64 + k) * 32 + fill(2000))
        toks = _walk(blk)
        for r in range(32):
            assert sum(1 for t in toks if t[0] // ROUND == r) == 64 + k
        rc, st, log = emulate(blk)
        rc_f, st_f, _ = emulate(blk, fixed=True)
        assert rc == 0 and rc_f == 0
        assert st_f["batches"] >= 64 and st["batches"] < st_f["batches"], (k, st, st_f)
        if k <= CARRY:
            assert st["carried"] >= 8, (k, st)
        out.append((f"stretches of 64 + {k} tokens", blk))
    # ---- a tail cut by the span limit: 61 output bytes per 5-byte sequence, 22 of them fill a batch's 1 365 bytes
    blk = build(fill(1000) + [(1, 60)] * 6000 + fill(1500))
    assert enc_len(1, 60) == 5 and 23 * 61 > SPAN_MAX > 22 * 61
    rc, st, _ = emulate(blk)
    assert rc == 0 and st["sequences"] / st["batches"] < 24
    out.append(("batches cut by the span limit", blk))
    # ---- windows of fewer than 64 tokens in all (long literals): one batch per window, nothing to carry
    blk = build([(40, 4 + (i % 9)) for i in range(800)])
    assert enc_len(40, 4) == 44
    rc, st, _ = emulate(blk)
    assert rc == 0 and st["carried"] == 0 and st["batches"] == st["map_windows"]
    out.append(("windows of fewer than 64 tokens", blk))
    # ---- a tail at the end of the input: the one window of a block of under 1 KiB holds 64 + 5 tokens and reaches the input's end, so
    # the tail is not carried (no later window would take it)
    blk = build([(12, 4)] * 64 + [(9, 5)] * 4, tail=b"e")
    rc, st, log = emulate(blk)
    assert rc == 0 and len(blk) < ROUND and len(_walk(blk)) == 69 and log == [(0, 0)] and st["batches"] == 2
    out.append(("tail at the end of the input", blk))
    # (and the same tail behind 31 KiB of dense stretches, wherever the windows have drifted to by then)
    out.append(("tail at the end of a long input", build(stretch(90) * 31 + [(12, 4)] * 64 + [(9, 5)] * 4, tail=b"e")))
    # ---- a tail whose first token sits at bit 0, 1 and 31 of its bit-map word: 64 sequences of 15 bytes (d of them 16), then the tail
    for d in (0, 1, 31):
        blk = build([(13, 4)] * d + [(12, 4)] * (64 - d) + [(12, 5)] * 3 + fill(32 * ROUND))
        p64 = _walk(blk)[64][0]
        assert p64 == 960 + d and p64 % 32 == d
        rc, st, log = emulate(blk)
        assert rc == 0 and log[:3] == [(0, 0), (2, p64), (0, 960)], log[:4]
        out.append((f"tail from bit {d} of its word", blk))
    # ---- a token of a carried tail whose body reaches past the staged bytes of the window that lists it
    blk = build([(12, 4)] * 64 + [(300, 4)] + fill(31 * ROUND))
    t64 = _walk(blk)[64]
    assert t64[0] == 960 and t64[0] + t64[1] > STAGED
    rc, st, log = emulate(blk)
    assert rc == 0 and log[1] == (2, 960)
    out.append(("carried tail with a body past the staged bytes", blk))
    # ---- windows across the boundaries between the chunks' shares of the map (16 384 and 2 * 14 336 + 2 048)
    blk = build(stretch(75) * 40)
    rc, st, log = emulate(blk)
    assert rc == 0
    for edge in (CHUNK, 2 * STRIDE + OVERLAP):
        assert any(k == 0 and p < edge < p + ROUND and p % ROUND for k, p in log), edge
    out.append(("windows across the shares' boundaries", blk))
    # ---- tails directly in front of piece boundaries: 16 and 3 rounds, so that with 16 and 3 pieces every round's end is a piece's end
    for rounds in (16, 3):
        blk = build(stretch(64 + 7) * (rounds - 1) + stretch(64 + 7)[:-1] + [(stretch(64 + 7)[-1][0] - 4, 4)], tail=b"end")
        assert len(blk) == rounds * ROUND, len(blk)
        rc, st, log = emulate(blk)
        assert rc == 0 and any(k == 2 and ROUND - 128 < p < ROUND for k, p in log), log[:6]
        out.append((f"tails in front of piece boundaries, {rounds} rounds", blk))
    return out


def damaged():
    """A token byte changed in a window BEHIND a good one (and behind a carried tail): once so that the reference rejects the block,
    once so that it stays valid and decodes to something else."""
    import oracle_ffi as o
    out = []
    for n_tok, r in ((70, 5), (96, 21)):
        blk = build(stretch(n_tok) * 34 + fill(1500))
        good = o.decompress_raw(blk, limit=LIMIT, cap=LIMIT)
        assert good[0] == 0
        p = next(t[0] for t in _walk(blk) if t[0] >= r * ROUND)
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
        assert bad is not None and other is not None, (n_tok, r)
        out.append((f"{n_tok} tokens per KiB, token of round {r} changed: invalid", bad))
        out.append((f"{n_tok} tokens per KiB, token of round {r} changed: still valid", other))
    return out
