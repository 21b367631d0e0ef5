"""Child process of tests/test_gpu_size_latency.py: the size call's latency class through the ANALYSIS library (LZF_LIB_PATH), whose
knobs are read once per process — LZF_SIZE_SEG=force LZF_SIZE_SEG_MIN_IN=0 sends every input of the corpus through the class,
LZF_SIZE_FORCE=2 leaves out the one-wave kernel behind it, LZF_SIZE_FORCE=1 refuses its scratch.

  parity    status and out_len of every job are the oracle's, with the inputs at address residues 0, 1 and 15 and once on a side stream
            (results read after a stream sync only); every Ok job also equals what lzf_decompress_batch writes for the same job array
  who       results pre-filled with a sentinel: the class alone answers exactly the jobs it must, and leaves every other one untouched
  redzone   `out` points into poison with out_cap 64, `prefix` is NULL with prefix_len > 0, the results sit between zones: nothing but
            the results is written, and they do not depend on the bytes behind input_len (two poisons)
  refused   the scratch refused at the allocation (LZF_SIZE_FORCE=1: the branch a pool refusal takes): the same results from the one-wave
            kernel alone
Prints "size latency ok" at the end."""
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import device, ffi  # noqa: E402

S_CLASS = "latency: lzf_seg_parse_kernel + lzf_size_tile_kernel + lzf_size_finish_kernel + lzf_decoded_size_kernel<48,768>"
S_WAVE = "lzf_decoded_size_kernel<48,768>"
SENTINEL = 0x5A
ZONE = 4096
RESIDUES = (0, 1, 15)


def load():
    with open(os.environ["SIZE_LATENCY_CORPUS"], "rb") as f:
        return pickle.load(f)                                   # [(case, (status, len or None), finishes)]


def arena(blobs, residue=0, poison=0, gap=64):
    """The blobs in one device tensor, each at an address = residue (mod 16), `gap`+ bytes of poison behind each."""
    import torch
    offs, at = [], 256 + residue
    for b in blobs:
        offs.append(at); at = (at + len(b) + gap + 15) // 16 * 16 + residue
    h = np.full(at + gap, poison, dtype=np.uint8)
    for b, a in zip(blobs, offs):
        h[a:a + len(b)] = np.frombuffer(b, dtype=np.uint8)
    t = torch.from_numpy(h).cuda()
    assert t.data_ptr() % 256 == 0
    return t, np.array(offs, dtype=np.uint64), h


def size_jobs(cases, d_in, offs):
    j = np.zeros(len(cases), dtype=device.DJOB)
    j["input"] = np.uint64(d_in.data_ptr()) + offs
    j["input_len"] = [len(c["input"]) for c in cases]
    j["prefix_len"] = [c["prefix_len"] for c in cases]
    j["out_existing_len"] = [c["existing_len"] for c in cases]
    j["output_limit"] = [c["limit"] for c in cases]
    return j


def run_size(j, fill=0, stream=None):
    import torch
    n = len(j)
    d_res = torch.full((n * 16,), fill, dtype=torch.uint8, device="cuda")
    d_j = device.to_device(j, "cuda")
    torch.cuda.synchronize()
    device.decompressed_size_batch(d_j, d_res, n, stream=stream)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    return device.results_to_host(d_res, n).copy(), d_res.cpu().numpy().copy()


def check_results(corpus, res, what):
    for k, (c, exp, _) in enumerate(corpus):
        got = (int(res["status"][k]), int(res["out_len"][k]) if res["status"][k] == 0 else None)
        assert got == exp, (what, c["name"], got, exp)


def parity(corpus):
    import torch
    cases = [c for c, _, _ in corpus]
    for r in RESIDUES:
        d_in, offs, _ = arena([c["input"] for c in cases], residue=r, poison=0xC3)
        assert ((np.uint64(d_in.data_ptr()) + offs) % 16 == r).all()
        j = size_jobs(cases, d_in, offs)
        res, _ = run_size(j)
        assert device.last_size_launch() == S_CLASS, device.last_size_launch()
        check_results(corpus, res, f"residue {r}")
    side = torch.cuda.Stream()
    res, _ = run_size(j, stream=side)
    check_results(corpus, res, "side stream")
    # the decoder on the same job array: prefix bytes, the existing output in place, out_cap = what the oracle's answer needs
    caps = [(exp[1] if exp[0] == 0 else c["existing_len"] + min(c["limit"], 1 << 22) + len(c["input"])) + 64 for c, exp, _ in corpus]
    d_pre, pre_offs, _ = arena([c["prefix"] for c in cases])
    out_offs = np.cumsum([0] + [cap + 64 for cap in caps])
    h_out = np.zeros(int(out_offs[-1]), dtype=np.uint8)
    for c, a in zip(cases, out_offs):
        h_out[a:a + c["existing_len"]] = np.frombuffer(c["existing"], dtype=np.uint8)
    d_out = torch.from_numpy(h_out).cuda()
    j["prefix"] = np.uint64(d_pre.data_ptr()) + pre_offs
    j["out"] = np.uint64(d_out.data_ptr()) + out_offs[:-1].astype(np.uint64)
    j["out_cap"] = caps
    n = len(j)
    d_j = device.to_device(j, "cuda")
    r_size = torch.zeros(n * 16, dtype=torch.uint8, device="cuda"); r_dec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    device.decompressed_size_batch(d_j, r_size, n)
    device.decompress_batch(d_j, r_dec, n)
    torch.cuda.synchronize()
    rs, rd = device.results_to_host(r_size, n), device.results_to_host(r_dec, n)
    check_results(corpus, rs, "decode's job array")
    n_ok = 0
    for k, (c, exp, _) in enumerate(corpus):
        if exp[0] == 0:
            assert (int(rd["status"][k]), int(rd["out_len"][k])) == (0, int(rs["out_len"][k])), (c["name"], int(rd["status"][k]), int(rd["out_len"][k]))
            n_ok += 1
    print(f"parity: {n} jobs x {len(RESIDUES)} residues + side stream, {n_ok} Ok jobs equal the decoder")


def who(corpus):
    cases = [c for c, _, _ in corpus]
    d_in, offs, _ = arena([c["input"] for c in cases], residue=1)
    res, raw = run_size(size_jobs(cases, d_in, offs), fill=SENTINEL)
    assert device.last_size_launch() == S_CLASS
    raw = raw.reshape(len(cases), 16)
    n_fin = 0
    for k, (c, exp, fin) in enumerate(corpus):
        if fin:
            assert (int(res["status"][k]), int(res["out_len"][k])) == (0, exp[1]), ("not finished by the class", c["name"], raw[k].tolist())
            n_fin += 1
        else:
            assert (raw[k] == SENTINEL).all(), ("touched by the class", c["name"], exp, raw[k].tolist())
    assert 0 < n_fin < len(cases)
    print(f"who: the class alone finished {n_fin} of {len(cases)} jobs and left the others untouched")


def redzone(corpus):
    import torch
    cases = [c for c, _, _ in corpus]
    n = len(cases)
    answers = []
    for poison in (0xA5, 0x5A):
        d_in, offs, h_in = arena([c["input"] for c in cases], residue=15, poison=poison, gap=128)
        # [zone][results][zone][64 bytes every job's `out` points into][zone]
        h = np.full(ZONE + n * 16 + ZONE + 64 + ZONE, poison, dtype=np.uint8)
        d = torch.from_numpy(h).cuda()
        j = size_jobs(cases, d_in, offs)
        j["out"] = np.uint64(d.data_ptr() + ZONE + n * 16 + ZONE)
        j["out_cap"] = 64
        j["prefix"] = 0                                          # NULL, whatever prefix_len says
        d_j = device.to_device(j, "cuda")
        d_res = d[ZONE:ZONE + n * 16]
        torch.cuda.synchronize()
        device.decompressed_size_batch(d_j, d_res, n)
        torch.cuda.synchronize()
        assert device.last_size_launch() == S_CLASS
        after = d.cpu().numpy()
        assert (after[:ZONE] == poison).all() and (after[ZONE + n * 16:] == poison).all(), "written outside the results"
        assert (d_in.cpu().numpy() == h_in).all(), "an input or the bytes around it changed"
        res = device.results_to_host(d_res.clone(), n).copy()
        check_results(corpus, res, f"poison {poison:#x}")
        answers.append([(int(s), int(l)) for s, l in zip(res["status"], res["out_len"]) if s == 0])
    assert answers[0] == answers[1]
    print(f"redzone: {n} jobs, two poisons, nothing but the results written")


def refused(corpus):
    cases = [c for c, _, _ in corpus]
    d_in, offs, _ = arena([c["input"] for c in cases])
    res, _ = run_size(size_jobs(cases, d_in, offs))
    assert device.last_size_launch() == S_WAVE, device.last_size_launch()
    check_results(corpus, res, "scratch refused")
    print(f"refused: {len(cases)} jobs from the one-wave kernel alone")


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available()
    assert ffi.lib_path() == os.environ["LZF_LIB_PATH"]
    {"parity": parity, "who": who, "redzone": redzone, "refused": refused}[sys.argv[1]](load())
    print("size latency ok")
