"""GPU tests (-m gpu) of lzf_frame_append_device: the streaming frame writer for inputs held in device memory.  Every call of every
frame is held to the Python model of tests/frame_append_cases.py (the bytes of the call, out_len, taken, status, phase), and the
concatenation to lzf_frame_compress_device_many and to the oracle's frame of the whole input.  Every output stands in an arena
of poison built with tests/redzone.py's layout and the cursor array between two zones of it: after a call nothing but
[0, out_len) of every output and the cursors has changed, under two poisons."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_append_cases as A
import redzone
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi, framed

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _dev(b, lead=0):
    """b in device memory, `lead` bytes behind an allocation's start: an input at any residue."""
    h = np.zeros(lead + len(b), dtype=np.uint8)
    h[lead:] = np.frombuffer(bytes(b), dtype=np.uint8)
    return torch.from_numpy(h).to(DEV)[lead:]


def settings_of(c, block_size=A.BS):
    s = ffi.Settings()
    ffi.lib().lzf_settings_default(C.byref(s))
    s.independent_blocks, s.block_checksums, s.content_checksum = int(c["indep"]), int(c["bsum"]), int(c["csum"])
    s.block_size = block_size
    s.has_content_size, s.content_size = int(c["csize"]), len(c["data"]) if c["csize"] else 0
    return s


def _key(c):
    """Frames of one call share the settings (the header's content size among them) and the dictionary."""
    return (c["indep"], c["bsum"], c["csum"], len(c["data"]) if c["csize"] else -1, c["dict"])


def _groups(cases):
    keys = []
    for c in cases:
        if _key(c) not in keys:
            keys.append(_key(c))
    return [[c for c in cases if _key(c) == k] for k in keys]


@pytest.fixture(scope="module")
def cases():
    return A.all_cases()


@pytest.fixture(scope="module")
def whole(cases):
    """lzf_frame_compress_device_many on every case's whole input: name -> the frame's bytes."""
    res = {}
    for some in _groups(cases):
        s = settings_of(some[0])
        ins = [_dev(c["data"]) for c in some]
        outs = [torch.empty(A.bound(len(c["data"])), dtype=torch.uint8, device=DEV) for c in some]
        st, ol = device.frame_compress_many(s, ins, outs, dictionary=_dev(some[0]["dict"]) if some[0]["dict"] else None)
        torch.cuda.synchronize()
        st, ol = st.cpu().tolist(), ol.cpu().tolist()
        for i, c in enumerate(some):
            assert st[i] == 0
            res[c["name"]] = outs[i][:ol[i]].cpu().numpy().tobytes()
            assert res[c["name"]] == A.oracle_frame(c), c["name"]
    return res


class Batch:
    """Frames that share settings and dictionary, each with a schedule, a cursor and a model of its own, driven call by call
    through lzf_frame_append_device."""

    def __init__(self, cases, schedules, poison=redzone.OUT_POISON, block_size=A.BS):
        assert len({_key(c) for c in cases}) == 1 and len(cases) == len(schedules)
        self.cases, self.poison, n = cases, poison, len(cases)
        self.s = settings_of(cases[0], block_size)
        self.data = [_dev(c["data"], lead=(1, 3, 0, 13, 16, 7)[f % 6]) for f, c in enumerate(cases)]
        self.dic = _dev(cases[0]["dict"], lead=5) if cases[0]["dict"] else None
        self.sched = [A.Schedule(name, len(c["data"])) for name, c in zip(schedules, cases)]
        self.models = [A.Model(c, block_size) for c in cases]
        cb = device.frame_write_cursor_bytes()
        self.guard = torch.full((2 * redzone.ZONE + n * cb,), poison, dtype=torch.uint8, device=DEV)
        self.cursors = self.guard[redzone.ZONE:redzone.ZONE + n * cb]
        self.cursors.zero_()
        self.got, self.taken, self.last = [b""] * n, [0] * n, [None] * n
        self.rng = np.random.default_rng(9)
        self.calls = 0

    def call(self, steps=None):
        """One call: every frame's next offer under its schedule (or steps[f] = (a, b, finish, cap)).  Every result against the
        model; the whole output arena against poison with the written bytes taken out; the zones around the cursors."""
        n = len(self.cases)
        steps = steps if steps is not None else [s.step() for s in self.sched]
        caps = [st[3] for st in steps]
        low = [None if f % 2 else (37 * (f + self.calls) + 1) % 256 for f in range(n)]          # every other output at a chosen, mostly odd, residue
        offs, total = redzone._layout(caps, redzone.ZONE, self.rng, low=low)
        arena = torch.full((total,), self.poison, dtype=torch.uint8, device=DEV)
        outs = [arena[o:o + cap] for o, cap in zip(offs, caps)]
        offers = [self.data[f][a:b] for f, (a, b, _, _) in enumerate(steps)]
        st, ol, tk, ph = device.frame_append(self.s, offers, [A.FINISH if x[2] else 0 for x in steps], self.cursors, outs, dictionary=self.dic)
        torch.cuda.synchronize()
        st, ol, tk, ph = st.cpu().tolist(), ol.cpu().tolist(), tk.cpu().tolist(), ph.cpu().tolist()
        h = arena.cpu().numpy()
        res = []
        for f in range(n):
            a, b, finish, cap = steps[f]
            want = self.models[f].call(self.cases[f]["data"][a:b], finish, cap)
            name = (self.cases[f]["name"], self.sched[f].name, self.calls)
            assert (ol[f], tk[f], st[f], ph[f]) == (len(want[0]), want[1], want[2], want[3]), (name, (ol[f], tk[f], st[f], ph[f]), (len(want[0]),) + want[1:4])
            got = h[offs[f]:offs[f] + ol[f]].tobytes()
            assert got == want[0], (name, "the bytes of the call")
            h[offs[f]:offs[f] + ol[f]] = self.poison
            self.got[f] += got
            self.taken[f] += tk[f]
            self.last[f] = (st[f], ph[f])
            self.sched[f].feed(tk[f], st[f], ph[f])
            res.append((got, tk[f], st[f], ph[f]))
        assert (h == self.poison).all(), "a byte outside [0, out_len) of an output changed"
        g = self.guard.cpu().numpy()
        assert (g[:redzone.ZONE] == self.poison).all() and (g[-redzone.ZONE:] == self.poison).all(), "a byte around the cursor array changed"
        self.calls += 1
        return res

    def finish(self, limit=40):
        """Until every frame is DONE, and one call more: DONE cursors called again write nothing."""
        for _ in range(limit):
            if all(m.phase == A.DONE for m in self.models):
                for r, m in zip(self.call(), self.models):
                    assert r == (b"", 0, m.status, A.DONE)
                return
            self.call()
        raise AssertionError("the frames did not end")

    def assert_whole(self, whole):
        for f, c in enumerate(self.cases):
            assert self.got[f] == whole[c["name"]] and self.taken[f] == len(c["data"]) and self.last[f] == (A.OK, A.DONE), (c["name"], self.sched[f].name)


PARTS = {"pairs": lambda c: "pair" in c["tags"], "flavours": lambda c: "flavour" in c["tags"], "special": lambda c: "stored" in c["tags"] or "carry" in c["tags"]}


@pytest.mark.parametrize("poison", [redzone.OUT_POISON, 0x5A])
@pytest.mark.parametrize("part", sorted(PARTS))
def test_every_case_under_every_schedule(cases, whole, part, poison):
    """Every case under every schedule, call by call against the model.  One call holds all frames of a settings group under ALL
    schedules at once: frames with different offers, block counts and phases side by side (linked streams of unequal length in
    lock-step), frames that have ended called again."""
    some = [c for c in cases if PARTS[part](c)]
    assert some
    for group in _groups(some):
        b = Batch([c for c in group for _ in A.SCHEDULES], [s for _ in group for s in A.SCHEDULES], poison)
        b.finish()
        b.assert_whole(whole)


def test_bad_block_size(cases):
    c = cases[3]
    for size, want in ((65537, A.INVALID_BLOCK_SIZE), (1 << 24, A.PANIC)):
        b = Batch([c], ["everything"], block_size=size)
        assert b.call()[0] == (b"", 0, want, A.DONE)
        assert b.call()[0] == (b"", 0, want, A.DONE)


def test_untouched_cursor_when_nothing_is_taken(cases, whole):
    """LZF_OUT_CAPACITY and NEED_INPUT without a whole block leave the cursor as it was, fresh or not."""
    c = next(c for c in cases if c["name"] == "linked dict 70000 len 196613")
    n = len(c["data"])
    b = Batch([c], ["everything"])
    assert b.call([(0, n, True, A.bound(A.BS) - 1)])[0] == (b"", 0, A.OUT_CAPACITY, A.MORE)
    assert b.call([(0, A.BS - 1, False, A.bound(n))])[0] == (b"", 0, A.OK, A.NEED_INPUT)
    assert not b.cursors.any(), "the fresh cursor was written"
    assert b.call([(0, A.BS + 9, False, A.bound(n))])[0][1:] == (A.BS, A.OK, A.NEED_INPUT)
    before = b.cursors.clone()
    assert b.call([(A.BS, n, True, A.bound(A.BS) - 1)])[0] == (b"", 0, A.OUT_CAPACITY, A.MORE)
    assert b.call([(A.BS, A.BS + 100, False, A.bound(n))])[0] == (b"", 0, A.OK, A.NEED_INPUT)
    assert torch.equal(before, b.cursors), "the cursor was written"
    b.finish()
    b.assert_whole(whole)


def test_small_memory_budget_goes_through_in_passes(cases, whole):
    """Four linked frames of one call under a budget that holds the scratch of two: the call goes through in passes, same results."""
    group = [c for c in cases if "pair" in c["tags"] and not c["indep"] and c["dict"] == A.dictionaries()["7"]]
    some = [c for c in group if len(c["data"]) >= A.BS]
    assert len(some) == 4 and len({_key(c) for c in some}) == 1
    ffi.lib().lzf_frame_set_memory_budget(400 << 10)
    try:
        b = Batch(some, ["one and a half blocks"] * len(some))
        b.finish()
    finally:
        ffi.lib().lzf_frame_set_memory_budget(0)
    b.assert_whole(whole)


def test_pieces_feed_the_resumable_reader_as_they_appear(cases):
    """The frame grows in device memory call by call; after every call lzf_frame_resume_device is given what is there.  The
    reader's output is the input, and it ends when the writer does."""
    for name in ("window carry", "flavour 1110"):
        c = next(c for c in cases if c["name"] == name)
        b = Batch([c], ["one and a half blocks"])
        frame = torch.zeros(A.bound(len(c["data"])), dtype=torch.uint8, device=DEV)
        rcur = device.new_frame_cursors(1, DEV)
        room = torch.empty(4 * A.BS, dtype=torch.uint8, device=DEV)
        at, back, phase = 0, b"", None
        while b.models[0].phase != A.DONE:
            piece = b.call()[0][0]
            frame[at:at + len(piece)] = _dev(piece)
            at += len(piece)
            st, ol, _, ph = device.frame_resume([frame], [at], rcur, [room], dictionary=b.dic)
            torch.cuda.synchronize()
            assert st.item() == 0
            back += room[:ol.item()].cpu().numpy().tobytes()
            phase = ph.item()
        assert back == c["data"] and phase == ffi.RESUME_DONE, name


def test_python_layer(cases, whole):
    """FrameWriterDevice and CompressionSettings.compress_pieces_device against compress_many_device."""
    c = next(c for c in cases if c["name"] == "linked dict 70000 len 196613")
    data = _dev(c["data"])
    cs = framed.CompressionSettings().independent_blocks(False).block_checksums(True).content_checksum(True).block_size(A.BS).dictionary(77, c["dict"])
    want = cs.compress_many_device([data])[0].cpu().numpy().tobytes()
    pieces = [p.cpu().numpy().tobytes() for p in cs.compress_pieces_device(data[i:i + 100000] for i in range(0, len(c["data"]), 100000))]
    assert b"".join(pieces) == want and len(pieces) == 3
    assert b"".join(p.cpu().numpy().tobytes() for p in cs.compress_pieces_device([])) == cs.compress_many_device([data[:0]])[0].cpu().numpy().tobytes()
    w = framed.FrameWriterDevice(cs)
    out = torch.empty(A.bound(2 * A.BS), dtype=torch.uint8, device=DEV)
    view, taken, status, phase = w.write(data[:1000], out)
    assert (view.numel(), taken, status, phase) == (0, 0, 0, ffi.APPEND_NEED_INPUT) and not w.finished
    got = b""
    view, taken, status, phase = w.write(data, out, finish=True)
    assert (taken, status, phase) == (2 * A.BS, 0, ffi.APPEND_MORE)
    got += view.cpu().numpy().tobytes()
    view, taken, status, phase = w.write(data[w.taken:], out, finish=True)
    got += view.cpu().numpy().tobytes()
    assert (status, phase) == (0, ffi.APPEND_DONE) and w.finished and w.taken == len(c["data"]) and got == want
    assert w.write(data, out, finish=True)[1:] == (0, 0, ffi.APPEND_DONE)
