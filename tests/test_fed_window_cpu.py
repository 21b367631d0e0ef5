"""CPU tests (no GPU) of the window rules of the bitmap-fed decompress kernel (rust-lz-fear_amd/csrc/lzf_fed_window.h): where a
window starts, which chunk's row of the bit map a word comes from, and when a short last batch waits for the next window.  The
emulator of the kernel's window loop (tests/emu/emu_fed_window.cpp, g++) compiles the same header and runs over the first blocks of
the Silesia stand-in and over the handcrafted blocks of tests/fed_window_cases.py: every pass of the loop makes progress, every token
of the true chain goes into a batch exactly once and in order (the emulator returns 0 only then), and the windows that follow the
chain form fewer batches than the fixed rounds of the same emulator."""
import pytest

import oracle_ffi as o
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import synth

import fed_window_cases as fw

BS = 4 << 20


@pytest.fixture(scope="module")
def silesia_blocks():
    out = []
    for k in (0, 1, 12, 30):
        rc, c = o.compress2(synth.silesia_mix(k * BS, (k + 1) * BS).tobytes())
        assert rc == 0
        out.append(c)
    return out


@pytest.fixture(scope="module")
def handcrafted():
    return fw.cases()


def test_geometry_of_the_header():
    """The per-word chunk and word index against the ownership rule spelled out: chunk 0 owns [0, 16 384), chunk h >= 1
    [h * 14 336 + 2 048, (h + 1) * 14 336 + 2 048)."""
    L = fw.emu_lib()
    assert L is not None
    for h in range(0, 6):
        lo = 0 if h == 0 else h * fw.STRIDE + fw.OVERLAP
        hi = (h + 1) * fw.STRIDE + fw.OVERLAP
        assert lo % 32 == 0 and hi % 32 == 0
        for wpos in (lo, lo + 32, hi - 32):
            hh = 0 if wpos < fw.CHUNK else 1 + (wpos - fw.CHUNK) // fw.STRIDE
            assert hh == h, (wpos, hh, h)
            assert 0 <= (wpos - h * fw.STRIDE) >> 5 < fw.CHUNK // 32


def test_silesia_blocks_progress_and_fewer_batches(silesia_blocks):
    for c in silesia_blocks:
        rc_f, fixed, _ = fw.emulate(c, fixed=True, want_log=False)
        assert rc_f == 0 and fixed["sequences"] == fixed["tokens"] and fixed["carried"] == 0
        rc_0, chain0, _ = fw.emulate(c, carry=0, want_log=False)
        assert rc_0 == 0 and chain0["sequences"] == chain0["tokens"] and chain0["carried"] == 0
        for carry in (24, 32, 48):
            rc, st, _ = fw.emulate(c, carry=carry, want_log=False)
            assert rc == 0 and st["sequences"] == st["tokens"] == fixed["tokens"]
            assert st["batches"] < fixed["batches"], (carry, st, fixed)
            # at least one batch per window that is not done again in walk mode (as many of those as windows walked): the progress guarantee
            assert st["batches"] >= st["map_windows"]


def test_a_wrong_map_is_walked(silesia_blocks):
    """A chunk's row of the bit map cleared: its share is walked window by window, the windows behind it come from the map again."""
    c = silesia_blocks[0]
    rc, ref, _ = fw.emulate(c, want_log=False)
    for h in (0, 1, 5):
        rc, st, log = fw.emulate(c, drop_chunk=h)
        assert rc == 0 and st["sequences"] == ref["tokens"]
        lo, hi = (0 if h == 0 else h * fw.STRIDE + fw.OVERLAP), (h + 1) * fw.STRIDE + fw.OVERLAP
        walked = [p for k, p in log if k == 1]
        assert len(walked) >= 10 and all(lo - fw.ROUND <= p < hi for p in walked), (h, walked[:3], walked[-3:])
        assert st["map_windows"] > ref["map_windows"] - 40


def test_handcrafted_blocks(handcrafted):
    assert len(handcrafted) >= 20
    for name, blk in handcrafted:
        e = o.decompress_raw(blk, limit=fw.LIMIT, cap=fw.LIMIT)
        assert e[0] == 0, name
        for kw in (dict(fixed=True), dict(carry=0), dict(carry=24), dict(), dict(carry=48), dict(carry=63)):
            rc, st, _ = fw.emulate(blk, want_log=False, **kw)
            assert rc == 0 and st["sequences"] == st["tokens"], (name, kw, rc, st)


def test_damaged_blocks_end_as_the_chain_does():
    """An invalid block ends in walk mode (return 1: the kernel leaves it to the pair kernel), never without progress."""
    for name, blk in fw.damaged():
        rc, st, _ = fw.emulate(blk, want_log=False)
        valid = o.decompress_raw(blk, limit=fw.LIMIT, cap=fw.LIMIT)[0] == 0
        # (-4: the emulator could not walk the true chain — UnexpectedEnd — which is the kernel's walk-mode failure)
        assert rc in ((0,) if valid else (0, 1, -4)), (name, rc)
