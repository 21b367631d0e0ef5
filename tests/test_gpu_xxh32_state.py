"""GPU tests (-m gpu) of the resumable XXH32: lzf_xxh32_update_batch / lzf_xxh32_digest_batch on the host's 48-byte lzf_xxh32_state.
The expectation is lzf_xxh32 on the host (tests/test_frame_resume_cases_cpu.py pins the host's own update in pieces to it, and to
the oracle, on the same splits): buffers of 0..100 bytes cut at every pair of split points — every fill 0..15 on both sides of a
stripe boundary — and 70 000 bytes in three uneven pieces, all as states of ONE call per piece (mixed lengths, zero lengths among
them); states that travel host -> device -> host and device -> host -> device between the pieces."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_resume_cases as R
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def rows():
    return R.xxh_splits()


@pytest.fixture(scope="module")
def expected(rows):
    lib, by_len = ffi.lib(), {}
    for buf, _, _ in rows:
        if len(buf) not in by_len:
            by_len[len(buf)] = lib.lzf_xxh32(buf, len(buf), 0)
    return np.array([by_len[len(buf)] for buf, _, _ in rows], dtype=np.uint32)


def _fresh(n):
    st = ffi.Xxh32State()
    ffi.lib().lzf_xxh32_reset(C.byref(st), 0)
    return np.tile(np.frombuffer(bytes(st), dtype=np.uint8), n).view(device.XXH32_STATE)


def _pieces(rows, base):
    """Per piece (three of them) the device addresses and lengths of every row: the small buffers are prefixes of the big one.  A
    piece of no bytes hands in a NULL pointer: it is never read."""
    n = np.array([len(b) for b, _, _ in rows], dtype=np.int64)
    a = np.array([r[1] for r in rows], dtype=np.int64)
    b = np.array([r[2] for r in rows], dtype=np.int64)
    out = []
    for start, length in ((np.zeros_like(a), a), (a, b - a), (b, n - b)):
        out.append((np.where(length > 0, base + start, 0).astype(np.uint64), length.astype(np.uint64)))
    return out


def _update(states, ptrs, lens):
    d_ptrs, d_lens = torch.from_numpy(ptrs.view(np.int64)).to(DEV), torch.from_numpy(lens.view(np.int64)).to(DEV)
    device.xxh32_update_batch(states, d_ptrs, d_lens, len(ptrs))
    torch.cuda.synchronize()


def _digest(states, n):
    out = torch.empty(n, dtype=torch.int32, device=DEV)
    device.xxh32_digest_batch(states, out, n)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def test_every_split_as_states_of_one_call(rows, expected):
    data = torch.from_numpy(np.frombuffer(rows[-1][0], dtype=np.uint8).copy()).to(DEV)
    n = len(rows)
    states = device.to_device(_fresh(n), DEV)
    host = _fresh(n)
    for ptrs, lens in _pieces(rows, data.data_ptr()):
        before = states.cpu().numpy().view(device.XXH32_STATE)
        _update(states, ptrs, lens)
        after = states.cpu().numpy().view(device.XXH32_STATE)
        idle = lens == 0
        assert idle.any() and (~idle).any()
        assert (before[idle].view(np.uint8) == after[idle].view(np.uint8)).all(), "a zero-length update changed a state"
        host["total"] += lens
        assert (after["total"] == host["total"]).all() and (after["fill"] == host["total"] % 16).all()
    got = _digest(states, n)
    bad = np.flatnonzero(got != expected)
    assert not len(bad), (len(bad), [(len(rows[i][0]), rows[i][1], rows[i][2]) for i in bad[:8]])
    assert (states.cpu().numpy().view(device.XXH32_STATE)["total"] == host["total"]).all(), "the digest changed a state"


def test_states_travel_between_host_and_device(rows, expected):
    """host update, device update, host update + host digest; and device, host, device + device digest."""
    lib = ffi.lib()
    pick = [i for i, (buf, a, b) in enumerate(rows) if len(buf) in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 64, 100, 70000)]
    sub = [rows[i] for i in pick]
    data = torch.from_numpy(np.frombuffer(rows[-1][0], dtype=np.uint8).copy()).to(DEV)
    pieces = _pieces(sub, data.data_ptr())
    n = len(sub)

    def host_update(st, k):
        for i, (buf, a, b) in enumerate(sub):
            piece = (buf[:a], buf[a:b], buf[b:])[k]
            s = ffi.Xxh32State.from_buffer(st, 48 * i)
            lib.lzf_xxh32_update(C.byref(s), piece, len(piece))

    # host -> device -> host
    st = bytearray(_fresh(n).tobytes())
    host_update(st, 0)
    d = torch.from_numpy(np.frombuffer(bytes(st), dtype=np.uint8).copy()).to(DEV)
    _update(d, *pieces[1])
    st = bytearray(d.cpu().numpy().tobytes())
    host_update(st, 2)
    got = np.array([lib.lzf_xxh32_digest(C.byref(ffi.Xxh32State.from_buffer(st, 48 * i))) for i in range(n)], dtype=np.uint32)
    assert (got == expected[pick]).all()
    # device -> host -> device
    d = device.to_device(_fresh(n), DEV)
    _update(d, *pieces[0])
    st = bytearray(d.cpu().numpy().tobytes())
    host_update(st, 1)
    d = torch.from_numpy(np.frombuffer(bytes(st), dtype=np.uint8).copy()).to(DEV)
    _update(d, *pieces[2])
    assert (_digest(d, n) == expected[pick]).all()


def test_an_empty_call_and_a_state_of_no_bytes():
    device.xxh32_update_batch(torch.empty(0, dtype=torch.uint8, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV),
                              torch.empty(0, dtype=torch.int64, device=DEV), 0)
    assert _digest(device.to_device(_fresh(1), DEV), 1)[0] == ffi.lib().lzf_xxh32(b"", 0, 0)
