"""GPU tests (-m gpu) of lzf_frame_resume_device: the resumable decode of frames held in device memory.  Every call of every frame
is held to the Python model of tests/frame_resume_cases.py (status, consumed, phase, the bytes of the call), and the concatenation,
the last status and the last consumed to lzf_frame_decompress_device_many on the same bytes.  Every output buffer stands in an
arena of poison built with tests/redzone.py's layout: after a call nothing but the delivered bytes has changed, under two
poisons.  Damaged inputs here are data errors that end in a status."""
import numpy as np
import pytest
import torch

import frame_resume_cases as R
import redzone
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi, framed

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _dev(b):
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).to(DEV) if len(b) else torch.empty(0, dtype=torch.uint8, device=DEV)


@pytest.fixture(scope="module")
def cases():
    return R.all_cases()


@pytest.fixture(scope="module")
def whole(cases):
    """lzf_frame_decompress_device_many on every case's bytes with room for everything: name -> (status, bytes, consumed)."""
    res = {}
    for dic in {c["dict"] for c in cases}:
        some = [c for c in cases if c["dict"] == dic]
        frames = [_dev(c["frame"]) for c in some]
        outs = [torch.empty(R.OUT_ROOM, dtype=torch.uint8, device=DEV) for _ in some]
        st, ol, co = device.frame_decompress_many(frames, outs, dictionary=_dev(dic) if dic else None)
        torch.cuda.synchronize()
        st, ol, co = st.cpu().tolist(), ol.cpu().tolist(), co.cpu().tolist()
        for i, c in enumerate(some):
            res[c["name"]] = (st[i], outs[i][:ol[i]].cpu().numpy().tobytes(), co[i])
    return res


class Batch:
    """Frames that share a dictionary, a cursor and a model each, driven call by call through lzf_frame_resume_device."""

    def __init__(self, cases, poison=redzone.OUT_POISON, frames=None):
        self.cases, self.poison = cases, poison
        self.frames = frames if frames is not None else [_dev(c["frame"]) for c in cases]
        self.dic = _dev(cases[0]["dict"]) if cases[0]["dict"] else None
        assert all(c["dict"] == cases[0]["dict"] for c in cases)
        self.cursors = device.new_frame_cursors(len(cases), DEV)
        self.models = [R.Model(c) for c in cases]
        self.got = [b""] * len(cases)
        self.last = [None] * len(cases)
        self.rng = np.random.default_rng(5)

    def call(self, caps, in_lens=None):
        """One call: frame f with room caps[f] and in_lens[f] bytes of input (None: all).  Every result against the model; the
        whole output arena against its picture before the call with the delivered bytes put in."""
        n = len(self.cases)
        in_lens = in_lens if in_lens is not None else [len(c["frame"]) for c in self.cases]
        offs, total = redzone._layout(caps, redzone.ZONE, self.rng)
        arena = torch.full((total,), self.poison, dtype=torch.uint8, device=DEV)
        outs = [arena[o:o + cap] for o, cap in zip(offs, caps)]
        st, ol, co, ph = device.frame_resume(self.frames, in_lens, self.cursors, outs, dictionary=self.dic)
        torch.cuda.synchronize()
        st, ol, co, ph = st.cpu().tolist(), ol.cpu().tolist(), co.cpu().tolist(), ph.cpu().tolist()
        h = arena.cpu().numpy()
        res = []
        for f in range(n):
            want = self.models[f].call(in_lens[f], caps[f])
            got = h[offs[f]:offs[f] + max(ol[f], 0)].tobytes()
            assert (st[f], co[f], ph[f], ol[f]) == (want[1], want[2], want[3], len(want[0])), (self.cases[f]["name"], (st[f], co[f], ph[f], ol[f]), want[1:4], len(want[0]))
            assert got == want[0], (self.cases[f]["name"], "the bytes of the call")
            h[offs[f]:offs[f] + ol[f]] = self.poison
            self.got[f] += got
            self.last[f] = (st[f], co[f], ph[f])
            res.append((got, st[f], co[f], ph[f]))
        assert (h == self.poison).all(), "a byte outside the delivered ranges changed"
        return res

    def finish(self, cap_of, limit=40):
        for _ in range(limit):
            if all(m.phase == R.DONE for m in self.models):
                return
            self.call([cap_of(c) for c in self.cases])
        raise AssertionError("the frames did not end")

    def assert_whole(self, whole):
        for f, c in enumerate(self.cases):
            st, out, consumed = whole[c["name"]]
            assert self.last[f] == (st, consumed, R.DONE) and self.got[f] == out, (c["name"], self.last[f], (st, consumed), len(self.got[f]), len(out))


def _groups(cases):
    for dic in sorted({c["dict"] for c in cases}, key=len):
        yield [c for c in cases if c["dict"] == dic]


@pytest.mark.parametrize("poison", [redzone.OUT_POISON, 0x5A])
@pytest.mark.parametrize("schedule", R.CAP_SCHEDULES + ("three bounds",))
def test_every_case_under_every_capacity_schedule(cases, whole, schedule, poison):
    """The flavour product, the stored blocks, the empty frame, the empty block in the middle and every stop rule in front of, at
    and behind a piece boundary: one call holds every frame of a dictionary (frames that have ended are called again and deliver
    nothing), until all have ended.  With room for everything one call equals the whole-frame call, consumed included."""
    for some in _groups(cases):
        b = Batch(some, poison)
        b.finish(lambda c: R.capacity(c, schedule))
        b.assert_whole(whole)
    if schedule == "everything":
        c = cases[0]
        b = Batch([c], poison)
        assert b.call([R.capacity(c, schedule)])[0][1:] == (whole[c["name"]][0], whole[c["name"]][2], R.DONE)      # in one step


def test_input_that_grows_at_every_byte(cases, whole):
    """in_len cut at every byte of a two-block frame with both checksums — every cut a frame of its own in ONE call — then the
    full length.  No cut moves the cursor past an incomplete item; the final result is the whole decode."""
    c = next(c for c in cases if "growth" in c["tags"])
    n = len(c["frame"])
    t = _dev(c["frame"])
    b = Batch([c] * n, frames=[t] * n)
    cap = R.capacity(c, "everything")
    res = b.call([cap] * n, in_lens=list(range(n)))
    assert all(r[3] == R.NEED_INPUT and r[1] == R.OK and r[2] <= cut for cut, r in enumerate(res))
    assert {r[2] for r in res} == {0} | {m.header_len for m in b.models[:1]} | {e for _, _, _, e in b.models[0].blocks}
    b.finish(lambda c: cap)
    b.assert_whole(whole)


def test_nothing_behind_the_piece_is_read(cases, whole):
    """The bytes behind the first block that does not fit are garbage during the first call and restored before the second: the
    results are those of the intact frame.  (The one place where a frame's bytes change between calls.)"""
    for name in ("linked+dict+bsum+csum", "indep+bsum+csum+csize"):
        c = next(c for c in cases if c["name"] == name)
        blocks = R.walk(c["frame"])[2]
        bad = bytearray(c["frame"])
        bad[blocks[1][3]:] = bytes([0xEE]) * (len(bad) - blocks[1][3])
        t = _dev(bytes(bad))
        b = Batch([c], frames=[t])
        cap = R.capacity(c, "one bound")
        first = b.call([cap])[0]
        assert first[3] == R.MORE and first[2] == blocks[0][3] and len(first[0]) == R.BS
        t.copy_(_dev(c["frame"]))
        b.finish(lambda c: cap)
        b.assert_whole(whole)


def test_content_checksum_fails_at_the_last_call_only(cases, whole):
    c = next(c for c in cases if c["tags"].get("stop") == "content")
    b = Batch([c])
    seen = []
    while b.models[0].phase != R.DONE:
        seen.append(b.call([R.capacity(c, "two bounds")])[0])
    assert [r[1] for r in seen[:-1]] == [R.OK] * (len(seen) - 1) and len(seen) >= 3 and seen[-1][1] == R.FRAME_CHECKSUM_FAIL
    b.assert_whole(whole)


def test_frames_in_different_phases_in_one_call(cases, whole):
    """One call holds a fresh frame, one in the middle and one that has ended."""
    some = [c for c in cases if c["name"] in ("linked+bsum+csum", "indep+csum", "one short block")]
    assert len(some) == 3
    middle, fresh, done = Batch([some[0]]), Batch([some[1]]), Batch([some[2]])
    middle.call([R.capacity(some[0], "two bounds")])
    done.finish(lambda c: R.capacity(c, "one bound"))
    both = Batch(some)
    both.frames = middle.frames + fresh.frames + done.frames
    both.cursors = torch.cat([middle.cursors, fresh.cursors, done.cursors])
    both.models, both.got, both.last = middle.models + fresh.models + done.models, middle.got + fresh.got + done.got, middle.last + fresh.last + done.last
    r = both.call([R.capacity(c, "two bounds") for c in some])
    assert [x[3] for x in r] == [R.MORE, R.MORE, R.DONE] and r[2][0] == b""
    both.finish(lambda c: R.capacity(c, "two bounds"))
    both.assert_whole(whole)


def test_capacity_below_the_first_bound(cases, whole):
    """LZF_OUT_CAPACITY with phase MORE and an untouched cursor, fresh or not; the next call with room proceeds."""
    c = next(c for c in cases if c["name"] == "linked+dict+csum")
    b = Batch([c])
    cap = R.capacity(c, "one bound")
    assert b.call([cap - 1])[0] == (b"", R.OUT_CAPACITY, 0, R.MORE)
    assert not b.cursors.any(), "the fresh cursor was written"
    assert b.call([cap])[0][1] == R.OK
    before = b.cursors.clone()
    assert b.call([100])[0][1:] == (R.OUT_CAPACITY, b.last[0][1], R.MORE)
    assert torch.equal(before, b.cursors), "the cursor was written"
    b.finish(lambda c: cap)
    b.assert_whole(whole)


def test_two_threads_on_two_streams(cases, whole):
    """The call keeps no state between calls and takes no lock beyond reading the budget: two threads, each on a stream of its
    own with frames, cursors and outputs of its own, get what one caller gets."""
    import threading
    errors = []

    def work(some):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                b = Batch(some)
                b.finish(lambda c: R.capacity(c, "two bounds"))
                b.assert_whole(whole)
        except BaseException as e:          # (reported by the test's thread)
            errors.append(repr(e)[:400])

    threads = [threading.Thread(target=work, args=(some,)) for some in _groups(cases)]
    assert len(threads) == 2
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_python_layer(cases, whole):
    """FrameCursorDevice and iter_frame_pieces_device reproduce a linked, dictionary, content-checksum frame through a buffer of
    two block bounds."""
    c = next(c for c in cases if c["name"] == "linked+dict+csum")
    st, out, consumed = whole[c["name"]]
    t, dic = _dev(c["frame"]), _dev(c["dict"])
    assert device.frame_cursor_bytes() % 256 == 0
    pieces = [p.cpu().numpy().tobytes() for p in framed.iter_frame_pieces_device(t, 2 * R.BS, dictionary=dic)]
    assert st == 0 and b"".join(pieces) == out and len(pieces) == 3
    cur = framed.FrameCursorDevice(t, dictionary=c["dict"])
    buf = torch.empty(2 * R.BS, dtype=torch.uint8, device=DEV)
    n, status, phase = cur.read_into(buf, in_len=len(c["frame"]) - 3)
    assert (n, status, phase) == (2 * R.BS, 0, ffi.RESUME_MORE) and not cur.finished
    got = buf[:n].cpu().numpy().tobytes()
    while not cur.finished:
        n, status, phase = cur.read_into(buf, in_len=len(c["frame"]) - 3)
        got += buf[:n].cpu().numpy().tobytes()
        if phase == ffi.RESUME_NEED_INPUT:
            break
    assert phase == ffi.RESUME_NEED_INPUT and status == 0 and got == out            # the content checksum word is cut off: come back with more
    assert cur.read_into(buf) == (0, 0, ffi.RESUME_DONE) and cur.finished and cur.consumed == consumed
    bad = next(c for c in cases if c["tags"].get("stop") == "content")
    with pytest.raises(framed.FrameError) as e:
        list(framed.iter_frame_pieces_device(_dev(bad["frame"]), 2 * R.BS, dictionary=bad["dict"]))
    assert e.value.code == R.FRAME_CHECKSUM_FAIL
