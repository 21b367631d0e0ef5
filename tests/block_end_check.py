"""The block-end sweep on the GPU, one setting per process (the analysis library's knobs are read once); tests/test_gpu_block_ends.py
runs every setting as `python block_end_check.py WHAT LABEL` with the knobs in the environment and the corpus — block_end_cases.py's
jobs and the oracle's answers — in the file BLOCK_ENDS_CORPUS names.  Every setting prints "<label> ok: N cases".

    decode    lzf_decompress_batch over every job, ALIASED: one device copy of each block, every cut an input_len on it, so that the bytes
              behind a cut are the block's true continuation; every job's status is the oracle's, on Ok out_len and the bytes too, with
              out_cap the oracle's decoded length and poison intact around every output.  Then the CARVED sample through redzone.py: both
              input poisons, the zones.  N = all + carved.
    size      lzf_decompressed_size_batch over the aliased jobs.  With LZF_SIZE_FORCE=2 (no one-wave kernel behind the class) the results
              start as a sentinel: the class answers every Ok job itself, reserved = its tiles, and leaves every other job untouched.
    verify    lzf_decompress_verify_batch over block_end_cases.verify_jobs (expected bytes equal, and one byte flipped), the inputs
              aliased; the verdicts against verify_cases.expect and against the size call on the same job array; with the class forced,
              reserved = the tiles of every job that decodes.
    who_seg   lzf_debug_seg (the segmented pipeline alone, no pair kernel behind): done = 1 with the oracle's out_len and bytes for
              exactly the jobs seg_stage_cases.Model gives up nowhere; every other job not done and its result untouched.
    who_fed   lzf_debug_fed (the fed kernel alone): done = 1 for every Ok job of at least one byte, the others untouched."""
import ctypes as C
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import block_end_cases as B  # noqa: E402
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import device, ffi  # noqa: E402

POISON, SENTINEL, GUARD, SLACK = 0xEE, 0x5A, 64, 4096
VARIANT = "analysis variant (LZF_DECOMPRESS_KERNEL)"
S_CLASS = "latency: lzf_seg_parse_kernel + lzf_size_tile_kernel + lzf_size_finish_kernel + lzf_decoded_size_kernel<48,768>"
S_WAVE = "lzf_decoded_size_kernel<48,768>"
V_WAVE = "lzf_verify_kernel<48,768>"
V_CLASS = "latency: lzf_seg_parse_kernel + lzf_size_tile_kernel + lzf_verify_finish_kernel + lzf_verify_tile_kernel + " + V_WAVE
SEG_MAX_CALL, MAX_CALL, DEBUG_SEG_CALL = 1024, 4096, 256      # jobs per call (the pipeline ranks up to 1 024; lzf_debug_seg sizes its scratch for 4 MiB blocks)


def load():
    with open(os.environ["BLOCK_ENDS_CORPUS"], "rb") as f:
        return pickle.load(f)                                  # (blocks, jobs, verify jobs)


def cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


class Aliased:
    """The jobs on the device: ONE copy of every block (at a varying address residue, nothing but the next block's gap behind it), the
    prefixes behind them; every job's output in a slot of its own of exactly out_cap bytes between poisoned guards, the existing output
    in place.  mems: the memory at `out` per job instead (the verify call's expected bytes), which is then read-only."""

    def __init__(self, blocks, jobs, mems=None, caps=None):
        torch = cuda()
        self.jobs, self.n = jobs, len(jobs)
        off, at = [], 256
        for i, b in enumerate(blocks):
            off.append(at + (5 * i) % 16); at = (off[-1] + len(b) + 64 + 255) // 256 * 256
        pres = sorted({j["prefix"] for j in jobs})
        pre_off = {}
        for p in pres:
            pre_off[p] = at + 3; at = (at + 3 + len(p) + 64 + 255) // 256 * 256
        self.h_in = np.full(at + SLACK, 0xC3, np.uint8)
        for a, b in zip(off, blocks):
            self.h_in[a:a + len(b)] = np.frombuffer(b, np.uint8)
        for p, a in pre_off.items():
            self.h_in[a:a + len(p)] = np.frombuffer(p, np.uint8)
        self.d_in = torch.from_numpy(self.h_in).cuda()
        caps = [j["cap"] for j in jobs] if caps is None else caps
        self.out_off, to = np.zeros(self.n, np.int64), 256
        for i, cap in enumerate(caps):
            self.out_off[i] = to + GUARD + i % 16; to = (int(self.out_off[i]) + cap + (len(mems[i]) - cap if mems else 0) + GUARD + 15) // 16 * 16
        self.h_out0 = np.full(to + 256, POISON, np.uint8)
        for i, (q, j) in enumerate(zip(self.out_off.tolist(), jobs)):
            m = mems[i] if mems else j["existing"]
            self.h_out0[q:q + len(m)] = np.frombuffer(m, np.uint8)
        self.d_out = torch.from_numpy(self.h_out0).cuda()
        dj = np.zeros(self.n, dtype=device.DJOB)
        dj["input"] = np.uint64(self.d_in.data_ptr()) + np.array([off[j["block"]] for j in jobs], np.uint64)
        dj["input_len"] = [j["k"] for j in jobs]
        dj["prefix"] = [int(self.d_in.data_ptr()) + pre_off[j["prefix"]] if j["prefix"] else 0 for j in jobs]
        dj["prefix_len"] = [len(j["prefix"]) for j in jobs]
        dj["out"] = np.uint64(self.d_out.data_ptr()) + self.out_off.astype(np.uint64)
        dj["out_existing_len"] = [len(j["existing"]) for j in jobs]
        dj["out_cap"] = caps
        dj["output_limit"] = [j["limit"] for j in jobs]
        self.dj, self.caps = dj, caps
        self.max_in = max(j["k"] for j in jobs)
        # every byte a cut's continuation holds lies inside the input arena
        assert all(off[j["block"]] + len(j["blk"]) + SLACK <= len(self.h_in) for j in jobs)

    def call(self, fn, lo, hi, fill=0):
        """fn(d_jobs, d_res, n) over jobs [lo, hi) -> (results, their raw bytes)."""
        torch = cuda()
        n = hi - lo
        d_res = torch.full((n * 16,), fill, dtype=torch.uint8, device="cuda")
        d_j = device.to_device(self.dj[lo:hi], "cuda")
        torch.cuda.synchronize()
        fn(d_j, d_res, n)
        torch.cuda.synchronize()
        return device.results_to_host(d_res, n).copy(), d_res.cpu().numpy().reshape(n, 16).copy()

    def check_outputs(self, res, done=None, label=""):
        """Status, out_len and bytes of every job (done: only of the jobs it marks; the others' slots still hold what they held) and the
        guards; the inputs unchanged.  Returns the messages of what differs."""
        out = self.d_out.cpu().numpy()
        msgs = []
        for i, j in enumerate(self.jobs):
            say = lambda text: msgs.append(f"{label} [{j['name']}] end {j['end']}: {text}")      # noqa: E731
            q, cap, ex = int(self.out_off[i]), self.caps[i], len(j["existing"])
            erc, eout = j["exp"]
            if done is None or done[i]:
                st, ln = int(res["status"][i]), int(res["out_len"][i])
                if st != erc:
                    say(f"status {st}, oracle {erc}")
                elif st == 0 and ln != len(eout):
                    say(f"out_len {ln}, oracle {len(eout)}")
                elif st == 0 and out[q:q + ln].tobytes() != eout:
                    bad = np.nonzero(out[q:q + ln] != np.frombuffer(eout, np.uint8))[0]
                    say(f"output differs at {len(bad)} bytes, first {int(bad[0])} of {ln}")
            if out[q:q + ex].tobytes() != j["existing"]:
                say("the existing output was changed")
            if (out[q - GUARD:q] != POISON).any():
                say("bytes in front of the output were written")
            if (out[q + cap:q + cap + GUARD] != POISON).any():
                say("bytes behind out_cap were written")
        if not np.array_equal(self.d_in.cpu().numpy(), self.h_in):
            msgs.append(f"{label}: the input arena was written to")
        return msgs


def report(msgs):
    for text in msgs[:40]:
        print(text)
    assert not msgs, f"{len(msgs)} differences"


def by_end(jobs, pred):
    n = dict.fromkeys(range(1, 8), 0)
    for i, j in enumerate(jobs):
        n[j["end"]] += bool(pred(i))
    return n


# ---------------------------------------------------------------------------------------------------------------- decode
def decode_launch_ok(launch, n, max_in):
    torch = cuda()
    which = os.environ.get("LZF_DECOMPRESS_KERNEL", "")
    if which == "seg":
        return launch.startswith("segmented")
    if which == "fed":
        return launch.startswith("bitmap-fed")
    if which:
        return launch == VARIANT
    cus = torch.cuda.get_device_properties(0).multi_processor_count       # the product: by the rule of lzf_dispatch.h (inputs below 64 KiB: no pipeline, no fed path)
    assert max_in < 65536
    return launch == ("lzf_decompress_paired_kernel<4096,48,640>" if n <= 8 * cus else "lzf_decompress_paired_kernel<4096,24,384>" if n <= 64 * cus
                      else "lzf_decompress_batched_kernel<4096,16,256,staged>")


def child_decode(label):
    import redzone
    blocks, jobs, _ = load()
    al = Aliased(blocks, jobs)
    step = SEG_MAX_CALL if os.environ.get("LZF_DECOMPRESS_KERNEL") == "seg" else MAX_CALL
    res = np.zeros(al.n, device.RES)
    for lo in range(0, al.n, step):
        hi = min(al.n, lo + step)
        res[lo:hi], _ = al.call(lambda dj, dr, n: device.decompress_batch(dj, dr, n, max_input_len=al.max_in), lo, hi)
        launch = ffi.lib().lzf_last_decompress_launch().decode()
        assert decode_launch_ok(launch, hi - lo, al.max_in), (label, hi - lo, launch)
    report(al.check_outputs(res, label=label + ", aliased"))
    if os.environ.get("BLOCK_ENDS_ALIASED_ONLY"):              # (profiles/block_ends.txt: a library with a planted defect runs in the aliased layout alone)
        return al.n, launch
    some = B.carved(jobs)
    items = [dict(input=j["blk"][:j["k"]], prefix=j["prefix"], existing=j["existing"], limit=j["limit"], out_cap=j["cap"]) for j in some]
    redzone.check_decompress(items, [j["exp"] for j in some], label=label + ", carved", max_input_len=max(j["k"] for j in some))
    assert decode_launch_ok(ffi.lib().lzf_last_decompress_launch().decode(), len(some), max(j["k"] for j in some))
    return al.n + len(some), launch


# ---------------------------------------------------------------------------------------------------------------- size
def tiles(k):
    return (k + B.SEG_TILE - 1) // B.SEG_TILE


def child_size(label):
    blocks, jobs, _ = load()
    al = Aliased(blocks, jobs)
    alone = os.environ.get("LZF_SIZE_FORCE") == "2"
    res, raw = al.call(lambda dj, dr, n: device.decompressed_size_batch(dj, dr, n, max_input_len=al.max_in), 0, al.n, fill=SENTINEL if alone else 0)
    launch = device.last_size_launch()
    assert launch == (S_WAVE if os.environ.get("LZF_SIZE_SEG") == "off" else S_CLASS), launch
    msgs = []
    for i, j in enumerate(jobs):
        erc, eout = j["exp"]
        got = (int(res["status"][i]), int(res["out_len"][i]), int(res["reserved"][i]))
        if alone and erc != 0:
            if (raw[i] != SENTINEL).any():
                msgs.append(f"{label} [{j['name']}] end {j['end']}: an error job ({erc}) the class touched: {got}")
        elif got[0] != erc or (erc == 0 and got[1] != len(eout)):
            msgs.append(f"{label} [{j['name']}] end {j['end']}: (status, out_len) {got[:2]}, oracle {(erc, len(eout))}" + (": not answered by the class" if alone else ""))
        elif alone and got[2] != tiles(j["k"]):
            msgs.append(f"{label} [{j['name']}] end {j['end']}: reserved {got[2]}, not the job's {tiles(j['k'])} tiles")
    report(msgs)
    if alone:
        fin = by_end(jobs, lambda i: (raw[i] != SENTINEL).any())
        print(f"{label}: answered by the class itself, per end class: {fin}")
        assert all(fin[e] == sum(j["end"] == e and j["exp"][0] == 0 for j in jobs) for e in range(1, 8))
    return al.n, launch


# ---------------------------------------------------------------------------------------------------------------- verify
def child_verify(label):
    blocks, jobs, vjobs = load()
    js = [jobs[i] for i, _, _ in vjobs]
    cs = [B.verify_case(jobs[i], at) for i, at, _ in vjobs]
    al = Aliased(blocks, js, mems=[c["mem"] for c in cs], caps=[c["out_cap"] for c in cs])
    forced = os.environ.get("LZF_VERIFY_SEG") == "force"
    res, _ = al.call(lambda dj, dr, n: device.decompress_verify_batch(dj, dr, n, max_input_len=al.max_in), 0, al.n)
    launch = device.last_verify_launch()
    assert launch == (V_CLASS if forced else V_WAVE), launch
    size, _ = al.call(lambda dj, dr, n: device.decompressed_size_batch(dj, dr, n, max_input_len=al.max_in), 0, al.n)
    msgs = []
    for i, (c, (_, _, exp)) in enumerate(zip(cs, vjobs)):
        st = int(res["status"][i])
        got = (st, int(res["out_len"][i]) if st in (0, B.MISMATCH) else None)
        sz = (int(size["status"][i]), int(size["out_len"][i]))
        if got != exp:
            msgs.append(f"{label} [{c['name']}] end {js[i]['end']}: {got}, decode-then-compare {exp}")
        elif (got[0] == 0 and sz != got) or (got[0] == B.MISMATCH and sz[0] != 0) or (got[0] not in (0, B.MISMATCH) and sz[0] != got[0]):
            msgs.append(f"{label} [{c['name']}] end {js[i]['end']}: {got}, but the size call says {sz}")
        elif forced and got[0] in (0, B.MISMATCH) and int(res["reserved"][i]) != tiles(js[i]["k"]):
            msgs.append(f"{label} [{c['name']}] end {js[i]['end']}: reserved {int(res['reserved'][i])}, not the job's {tiles(js[i]['k'])} tiles: not answered by the class")
    if not np.array_equal(al.d_out.cpu().numpy(), al.h_out0) or not np.array_equal(al.d_in.cpu().numpy(), al.h_in):
        msgs.append(f"{label}: an input or an `out` was written to")
    report(msgs)
    return al.n, launch


# ---------------------------------------------------------------------------------------------------------------- who answered
def child_who_seg(label):
    import seg_stage_cases as S
    blocks, jobs, _ = load()
    al = Aliased(blocks, jobs)
    fn = ffi.lib().lzf_debug_seg
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 7 + [C.c_uint64, C.c_void_p]
    st = np.zeros(al.n, S.SEGJOB)
    res, raw = np.zeros(al.n, device.RES), np.zeros((al.n, 16), np.uint8)
    for lo in range(0, al.n, DEBUG_SEG_CALL):
        hi = min(al.n, lo + DEBUG_SEG_CALL)
        part = np.zeros(hi - lo, S.SEGJOB)
        res[lo:hi], raw[lo:hi] = al.call(lambda dj, dr, n: ffi.check(fn(dj.data_ptr(), dr.data_ptr(), n, 0, 8, part.ctypes.data, None, None, None, None, None, None, 0, None)),
                                         lo, hi, fill=SENTINEL)
        st[lo:hi] = part
    msgs = []
    for i, j in enumerate(jobs):
        # the model has no history: a job behind a prefix or existing output is held to the pipeline's stated rule (every DecodeError is left)
        gives = S.Model(dict(input=j["blk"][:j["k"]], limit=j["limit"], out_cap=j["cap"])).gives_up if not (j["prefix"] or j["existing"]) else "records"
        assert (gives is None) == (j["exp"][0] == 0), j["name"]
        if int(st["done"][i]) != int(gives is None):
            msgs.append(f"{label} [{j['name']}] end {j['end']}: done = {int(st['done'][i])}, the model gives up in {gives}")
        elif gives is not None and (raw[i] != SENTINEL).any():
            msgs.append(f"{label} [{j['name']}] end {j['end']}: not done, but a result was reported")
    msgs += al.check_outputs(res, done=st["done"], label=label)
    report(msgs)
    print(f"{label}: finished by the pipeline itself, per end class: {by_end(jobs, lambda i: st['done'][i])}")
    return al.n, "lzf_debug_seg"


def child_who_fed(label):
    from seg_stage_cases import SEGJOB
    blocks, jobs, _ = load()
    al = Aliased(blocks, jobs)
    fn = ffi.lib().lzf_debug_fed
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    st, geom = np.zeros(al.n, SEGJOB), np.zeros(4, np.uint32)
    res, raw = al.call(lambda dj, dr, n: ffi.check(fn(dj.data_ptr(), dr.data_ptr(), n, al.max_in, 0, st.ctypes.data, None, None, geom.ctypes.data)), 0, al.n, fill=SENTINEL)
    pieces = int(os.environ.get("LZF_FED_PIECES", "1"))
    assert int(geom[0]) == pieces and (pieces == 1 or int(geom[3]) != 0), geom.tolist()
    msgs = []
    for i, j in enumerate(jobs):
        must = j["exp"][0] == 0 and j["k"] >= 1                 # (an empty input is below the path's smallest input: the pair kernel's, by design)
        if int(st["done"][i]) != int(must):
            msgs.append(f"{label} [{j['name']}] end {j['end']}: done = {int(st['done'][i])}, oracle status {j['exp'][0]}")
        elif not must and (raw[i] != SENTINEL).any():
            msgs.append(f"{label} [{j['name']}] end {j['end']}: not done, but a result was reported")
    msgs += al.check_outputs(res, done=st["done"], label=label)
    report(msgs)
    print(f"{label}: finished by the fed kernel itself, per end class: {by_end(jobs, lambda i: st['done'][i])}")
    return al.n, "lzf_debug_fed"


CHILDREN = dict(decode=child_decode, size=child_size, verify=child_verify, who_seg=child_who_seg, who_fed=child_who_fed)

if __name__ == "__main__":
    what, label = sys.argv[1], sys.argv[2]
    if label != "product":
        assert ffi.lib_path() == os.environ["LZF_LIB_PATH"]
    n, launch = CHILDREN[what](label)
    print(f"[{launch}]")
    print(f"{label} ok: {n} cases")
