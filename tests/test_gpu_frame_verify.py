"""GPU tests (-m gpu) of lzf_frame_verify_device: does a frame in device memory deliver exactly the expected bytes — no decode, no
output memory.  Held to verify_cases.py's frame expectations (the oracle's frame decode, compared by numpy); a frame that does not
decode reports what lzf_frame_decompressed_size_device reports.  Damaged frames here are data errors that end in a status."""
import numpy as np
import pytest
import torch

import verify_cases as cases
import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi, framed, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def dev(b):
    b = bytes(b)
    if not b:
        return torch.empty(0, dtype=torch.uint8, device=DEV)
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(DEV)


@pytest.fixture(scope="module")
def rows():
    r = cases.frame_cases()
    cases.assert_frames_cover(r)
    return r


def test_every_frame_case_in_mixed_calls(rows):
    """One call per dictionary, the frames of every flavour and every expected-byte variant mixed (a fixed shuffle); the verdicts,
    and for the frames that do not decode the size query's status, length and consumed."""
    by_dict = {}
    for c, e in rows:
        by_dict.setdefault(c["dictionary"], []).append((c, e))
    assert len(by_dict) == 4
    for dic, some in by_dict.items():
        order = np.random.default_rng(len(dic)).permutation(len(some))
        some = [some[k] for k in order]
        frames, exp = [dev(c["frame"]) for c, _ in some], [dev(c["expected"]) for c, _ in some]
        status, at, consumed = device.frame_verify(frames, exp, dictionary=dev(dic) if dic else None)
        s_status, s_len, s_consumed = device.frame_decompressed_size(frames, dictionary_len=len(dic))
        torch.cuda.synchronize()
        got = list(zip(status.tolist(), at.tolist()))
        bad = [(c["name"], g, e) for (c, e), g in zip(some, got) if g != e]
        assert not bad, bad[:10]
        assert consumed.tolist() == s_consumed.tolist()
        for (c, e), g, ss, sl in zip(some, got, s_status.tolist(), s_len.tolist()):
            if g[0] not in (0, cases.MISMATCH, cases.F_FRAME_CHECKSUM_FAIL):
                assert g == (ss, sl), c["name"]
            else:
                assert ss == 0, c["name"]
    assert framed.verify_frames_device([], []) == []


def test_wrapper_with_a_host_dictionary_and_a_side_stream(rows):
    some = [(c, e) for c, e in rows if len(c["dictionary"]) == 100][:40]
    side = torch.cuda.Stream(device=DEV)
    frames, exp = [dev(c["frame"]) for c, _ in some], [dev(c["expected"]) for c, _ in some]
    torch.cuda.synchronize()
    got = framed.verify_frames_device(frames, exp, dictionary=some[0][0]["dictionary"], stream=side)
    assert got == [e for _, e in some]


def test_compress_many_device_with_verify_and_a_frame_corrupted_in_between():
    """compress_many_device(verify=True) on good inputs returns the frames of the plain call; with the two calls used separately,
    a frame corrupted between compress and verify is found: a payload byte (a mismatch, or a codec status), the content checksum."""
    text = synth.gen_text_zipf(51, 700000).tobytes()
    datas = [text[:200000], b"", text[200000:200001], cases._rand(52, 100000), text[300000:700000]]
    tensors = [dev(d) for d in datas]
    dic = synth.gen_text_zipf(53, 5000).tobytes()
    for st in (framed.CompressionSettings().block_size(64 << 10), framed.CompressionSettings().block_size(64 << 10).independent_blocks(False),
               framed.CompressionSettings().block_size(64 << 10).block_checksums(True).dictionary(9, dic)):
        plain = st.compress_many_device(tensors)
        checked = st.compress_many_device(tensors, verify=True)
        assert all(torch.equal(a, b) for a, b in zip(plain, checked))
        assert st.compress_many_device(tensors, verify=True, exact=True)[0].numel() == plain[0].numel()
    st = framed.CompressionSettings().block_size(64 << 10)
    frames = st.compress_many_device(tensors)
    assert framed.verify_frames_device(frames, tensors) == [(0, len(d)) for d in datas]
    hurt = [f.clone() for f in frames]
    hurt[0][len(frames[0]) // 2] ^= 0x04          # inside a block's payload
    hurt[4][-1] ^= 0x80                            # the content checksum
    got = framed.verify_frames_device(hurt, tensors)
    want = []
    for f, d in zip(hurt, datas):
        want.append(cases.frame_expect(dict(frame=bytes(f.cpu().numpy().tobytes()), dictionary=b"", expected=d)))
    assert got == want
    assert got[0][0] != 0 and got[4] == (cases.F_FRAME_CHECKSUM_FAIL, len(datas[4])) and got[1:4] == [(0, len(d)) for d in datas[1:4]]


def test_verify_raises_on_the_first_bad_frame(monkeypatch):
    """compress_many_device(verify=True) raises FrameError where the verify call does not say LZF_OK for a frame."""
    t = [dev(b"some bytes to compress, some bytes to compress")]
    monkeypatch.setattr(framed, "verify_frames_device", lambda frames, expected, dictionary=None, stream=None: [(ffi.MISMATCH, 3)])
    with pytest.raises(framed.FrameError) as ei:
        framed.CompressionSettings().compress_many_device(t, verify=True)
    assert ei.value.code == ffi.MISMATCH and str(ei.value) == "Mismatch"
