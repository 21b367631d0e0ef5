"""The piece hand-over of the bitmap-fed decompress kernel against the host model, on the built cases of fed_piece_cases.py (whose reach
test_fed_piece_cases_cpu.py proves without a GPU).  A call with more jobs than resident wavefronts cuts every job into pieces, and a job the fed
kernel does not finish is decoded again by the pair kernel behind it — so final bytes and statuses cannot show whether a hand-over worked.  Here
child processes load the analysis library and run the fed kernel ALONE through lzf_debug_fed (scratch, plan + parse, reset, the fed kernel by the
launch lines of the product call; no pair kernel), stopped in front of piece `stop_piece`:

  * geometry: the pieces asked for are the pieces used and the census gave an XCD mask — else forced pieces silently do nothing;
  * every hand-over: for 2, 3 and 16 pieces and every stop the job's parked flag, expect and o are the model's, out[existing_len, o) holds the
    bytes of the tokens below expect, the existing output and the poison around the slot are untouched, and a job still under way has done = 0
    and an untouched result;
  * who finished: with no stop every block the oracle decodes is finished by the fed kernel itself (done = 1, the oracle's out_len and bytes, flag
    kFedEnded), every damaged block is left (!done, result untouched, flag kFedEnded);
  * more jobs than slots (LZF_FED_SLOTS=1, 16 pieces, 2.3 jobs per slot: pieces really wait for their predecessors), with and without a launch order;
  * red zones: the full path with the pair kernel behind it, 2 and 16 pieces, inputs and prefixes at residues 0, 1, 15.
Every call carries 64 jobs or more — the corpus repeated, each copy with its own output slot — so that every XCD holds wavefronts wherever
workgroup 0 lands.  A hand-over wait that expires is not provoked: its rule is stated in the emulator and tested on the CPU."""
import ctypes as C
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import ffi  # noqa: E402
import fed_piece_cases as K  # noqa: E402
from seg_stage_cases import SEGJOB  # noqa: E402

pytestmark = pytest.mark.gpu

POISON, GUARD, SENTINEL = 0xEE, 64, 0xA5
FEDSTATE = np.dtype([("flag", "<u4"), ("expect", "<u4"), ("o", "<u4"), ("pad", "<u4")])      # fed_state (kernels.h)
MIN_JOBS = 64
STOPS = {2: (1, 2), 3: (1, 2, 3), 16: (1, 2, 3, 8, 15, 16)}
# A child's time limit: the sibling fed children (test_gpu_fed_decode_once.py, test_gpu_fed_windows.py) take 3 .. 4 s each on an MI355X, most of it
# the start of the process; a child here makes up to seven calls of under 3 ms and takes 2.2 .. 2.5 s (profiles/fed_piece_handover.txt).  A hand-over
# wait that expired would add seconds per piece, and the who-finished assertion would name the jobs.
CHILD_TIMEOUT = 120


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """The cases with the oracle's answers and the model per piece count, once for the module (the children read the file)."""
    cs = K.corpus()
    models = {p: [K.model(c, p) for c in cs] for p in K.PIECES}
    assert all(m.rc == 0 for ms in models.values() for m in ms)
    path = tmp_path_factory.mktemp("fed_pieces") / "corpus.pkl"
    path.write_bytes(pickle.dumps((cs, models)))
    return str(path)


def _child(what, corpus, *args, **env):
    from rust_lz_fear_amd import build
    e = dict(os.environ, FED_PIECES_CORPUS=corpus)
    for k in ("LZF_DECOMPRESS_KERNEL", "LZF_DECOMPRESS_ORDER", "LZF_FED_MIN_IN", "LZF_FED_PIECES", "LZF_FED_SLOTS", "LZF_FED_CARRY", "LZF_LIB_PATH"):
        e.pop(k, None)
    e.update(env, LZF_LIB_PATH=build.build_analysis_library(), LZF_FED_MIN_IN="1")
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what, *args], env=e, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    for line in r.stdout.splitlines():
        if line.startswith(("geometry", "fed pieces")):
            print(line)
    print(f"child {what} {' '.join(args)} {env}: {time.time() - t0:.1f} s")
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "fed pieces ok" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("pieces", K.PIECES)
def test_every_hand_over_and_who_finished(corpus, pieces):
    _child("handover", corpus, str(pieces), LZF_FED_PIECES=str(pieces))


@pytest.mark.parametrize("order", ["natural", "always"])
def test_more_jobs_than_slots(corpus, order):
    _child("slots", corpus, order, LZF_FED_PIECES="16", LZF_FED_SLOTS="1", LZF_DECOMPRESS_ORDER=order)


@pytest.mark.parametrize("pieces", [2, 16])
def test_red_zones(corpus, pieces):
    _child("redzone", corpus, str(pieces), LZF_DECOMPRESS_KERNEL="fed", LZF_FED_PIECES=str(pieces))


# ---------------------------------------------------------------------------------------------------------------- the children
def _load():
    with open(os.environ["FED_PIECES_CORPUS"], "rb") as f:
        return pickle.load(f)


def _debug_fed():
    fn = ffi.lib().lzf_debug_fed
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


class Placed:
    """n jobs (job i = case which[i]) on the device: inputs and prefixes shared per case at odd alignments, every job's output in a slot of its own
    at address residue rb of its case, poison around it, the existing output in place."""

    def __init__(self, cases, which):
        import torch
        from rust_lz_fear_amd import device
        self.cases, self.which, self.n = cases, which, len(which)
        in_off, pre_off, ti = [], [], 0
        for c in cases:
            in_off.append(ti); ti += (len(c["input"]) + 255) // 256 * 256 + 3
            pre_off.append(ti); ti += (len(c["prefix"]) + 255) // 256 * 256 + 5
        h_in = np.zeros(ti + 64, np.uint8)
        for a, p, c in zip(in_off, pre_off, cases):
            h_in[a:a + len(c["input"])] = np.frombuffer(c["input"], np.uint8)
            h_in[p:p + len(c["prefix"])] = np.frombuffer(c["prefix"], np.uint8)
        self.out_off, to = np.zeros(self.n, np.int64), 256
        for i, w in enumerate(which):
            self.out_off[i] = to + cases[w]["rb"]; to += (cases[w]["cap"] + 2 * GUARD + 16 + 255) // 256 * 256
        self.h_out0 = np.full(to + 256, POISON, np.uint8)
        for q, w in zip(self.out_off.tolist(), which):
            ex = cases[w]["existing"]
            self.h_out0[q:q + len(ex)] = np.frombuffer(ex, np.uint8)
        self.d_in = torch.from_numpy(h_in).cuda()
        self.d_out = torch.from_numpy(self.h_out0).cuda()
        assert self.d_out.data_ptr() % 256 == 0
        dj = np.zeros(self.n, dtype=device.DJOB)
        dj["input"] = np.uint64(self.d_in.data_ptr()) + np.array([in_off[w] for w in which], np.uint64)
        dj["input_len"] = [len(cases[w]["input"]) for w in which]
        dj["prefix"] = np.uint64(self.d_in.data_ptr()) + np.array([pre_off[w] for w in which], np.uint64)
        dj["prefix_len"] = [len(cases[w]["prefix"]) for w in which]
        dj["out"] = np.uint64(self.d_out.data_ptr()) + self.out_off.astype(np.uint64)
        dj["out_existing_len"] = [len(cases[w]["existing"]) for w in which]
        dj["out_cap"] = [cases[w]["cap"] for w in which]
        dj["output_limit"] = [cases[w]["limit"] for w in which]
        assert ((dj["out"] & 15) == [cases[w]["rb"] for w in which]).all()
        self.d_jobs = device.to_device(dj, "cuda")
        self.d_res = torch.empty(self.n * device.RES.itemsize, dtype=torch.uint8, device="cuda")
        self.max_in = max(len(c["input"]) for c in cases)

    def run(self, stop):
        """One call of lzf_debug_fed over fresh outputs and sentinel results -> dict of the host copies."""
        import torch
        from rust_lz_fear_amd import device
        self.d_out.copy_(torch.from_numpy(self.h_out0)); self.d_res.fill_(SENTINEL)
        torch.cuda.synchronize()
        st, fs = np.zeros(self.n, SEGJOB), np.zeros(self.n, FEDSTATE)
        perm, geom = np.zeros(self.n, np.uint32), np.zeros(4, np.uint32)
        t0 = time.time()
        ffi.check(_debug_fed()(self.d_jobs.data_ptr(), self.d_res.data_ptr(), self.n, self.max_in, stop, st.ctypes.data, fs.ctypes.data,
                               perm.ctypes.data, geom.ctypes.data))
        return dict(st=st, fs=fs, perm=perm, geom=[int(x) for x in geom], ms=(time.time() - t0) * 1e3, res_raw=self.d_res.cpu().numpy().reshape(self.n, -1).copy(),
                    res=device.results_to_host(self.d_res, self.n).copy(), out=self.d_out.cpu().numpy())


def check_geometry(d, pieces, label):
    g_pieces, slots, grid, mask = d["geom"]
    print(f"geometry {label}: pieces {g_pieces}, slots {slots}, grid {grid}, XCD mask 0x{mask:x}, call {d['ms']:.1f} ms")
    assert mask != 0, f"{label}: the census gave no XCD mask: every job stays whole, the pieces asked for do nothing"
    assert g_pieces == pieces, f"{label}: {pieces} pieces asked for, {g_pieces} used"


def check_states(pl, models, d, k, pieces, msgs):
    """Every job against the model's state after k pieces (k == pieces: the whole call).  Returns the jobs the fed kernel finished."""
    finished = 0
    for i, w in enumerate(pl.which):
        c, m = pl.cases[w], models[w]
        say = lambda text: msgs.append(f"[{c['name']}] job {i}, {pieces} pieces, stop {k}: {text}")      # noqa: E731
        s, f, q, ex = d["st"][i], d["fs"][i], int(pl.out_off[i]), len(c["existing"])
        out = d["out"]
        if not s["eligible"] or s["failed"]:
            say(f"eligible {s['eligible']}, failed {s['failed']}"); continue
        flag, expect, o, under_way = K.state_after(m, k)
        untouched = (d["res_raw"][i] == SENTINEL).all()
        if int(f["flag"]) != flag:
            say(f"flag 0x{int(f['flag']):x}, the model's 0x{flag:x} (the kernel's expect {f['expect']}, o {f['o']}; the model's piece {m.end_piece} ends the job, done {m.done})")
            continue
        written = ex
        if under_way:
            if (int(f["expect"]), int(f["o"])) != (expect, o):
                say(f"parked expect {f['expect']}, o {f['o']}; the model's {expect}, {o}"); continue
            ref = K.decode_below(c, expect)
            assert len(ref) == o
            if out[q + ex:q + o].tobytes() != ref[ex:]:
                bad = np.nonzero(out[q + ex:q + o] != np.frombuffer(ref[ex:], np.uint8))[0]
                say(f"out[{ex}, {o}) differs at {len(bad)} bytes, first {ex + int(bad[0])}")
            if s["done"] or not untouched:
                say(f"under way, but done {s['done']}, result {'untouched' if untouched else d['res'][i]}")
            written = o
        elif m.done:
            erc, eout = c["exp"]
            r = d["res"][i]
            if not s["done"] or int(r["status"]) != 0 or int(r["out_len"]) != len(eout):
                say(f"a valid job the fed kernel did not finish: done {s['done']}, status {r['status']}, out_len {r['out_len']} (oracle {len(eout)})"); continue
            if out[q:q + len(eout)].tobytes() != eout:
                bad = np.nonzero(out[q:q + len(eout)] != np.frombuffer(eout, np.uint8))[0]
                say(f"output differs at {len(bad)} bytes, first {int(bad[0])}")
            finished += 1
            written = len(eout)
        elif s["done"] or not untouched:
            say(f"a damaged job: done {s['done']}, result {'untouched' if untouched else d['res'][i]}")
        if out[q:q + ex].tobytes() != c["existing"]:
            say("the existing output was changed")
        if (out[q - GUARD:q] != POISON).any():
            say("bytes in front of the output slot were written")
        if (out[q + c["cap"]:q + c["cap"] + GUARD] != POISON).any():
            say("bytes behind the output slot were written")
        if m.done and written < c["cap"] and not under_way and (out[q + written:q + c["cap"]] != POISON).any():
            say("bytes behind out_len were written")
    return finished


def _report(msgs):
    for text in msgs[:40]:
        print(text)
    assert not msgs, f"{len(msgs)} differences"


def child_handover(pieces):
    pieces = int(pieces)
    cases, models = _load()
    copies = -(-MIN_JOBS // len(cases))
    which = [w for _ in range(copies) for w in range(len(cases))]      # (a case's copies land on different ranks, and so on different XCDs' groups, unless the corpus is a multiple of eight)
    assert len(which) >= MIN_JOBS
    pl = Placed(cases, which)
    msgs, n_valid = [], sum(models[pieces][w].done for w in which)
    assert 0 < n_valid < len(which)
    for k in STOPS[pieces]:
        d = pl.run(k)
        check_geometry(d, pieces, f"{pieces} pieces, stop {k}")
        fin = check_states(pl, models[pieces], d, k, pieces, msgs)
        print(f"fed pieces: {pieces} pieces, stop {k}: {len(which)} jobs, {fin} finished by the fed kernel, {sum(K.state_after(models[pieces][w], k)[3] for w in which)} parked")
    d = pl.run(0)
    check_geometry(d, pieces, f"{pieces} pieces, no stop")
    fin = check_states(pl, models[pieces], d, pieces, pieces, msgs)
    print(f"fed pieces: {pieces} pieces, no stop: {len(which)} jobs, {fin} of {n_valid} valid jobs finished by the fed kernel")
    _report(msgs)
    assert fin == n_valid
    print(f"fed pieces ok: hand-over, {pieces} pieces, stops {STOPS[pieces]} and none, {len(which)} jobs")


def child_slots(order):
    import torch
    cases, models = _load()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = int(2.3 * cu)
    which = [i % len(cases) for i in range(n)]
    pl = Placed(cases, which)
    d = pl.run(0)
    check_geometry(d, 16, f"more jobs than slots, order {order}")
    slots, grid = d["geom"][1], d["geom"][2]
    assert slots == cu and grid == slots < n, (slots, grid, cu, n)
    if order == "always":
        assert sorted(d["perm"].tolist()) == list(range(n)), "perm is not a permutation of the ranks"
        assert d["perm"].tolist() != list(range(n))
    else:
        assert (d["perm"] == 0xFFFFFFFF).all()
    msgs = []
    fin = check_states(pl, models[16], d, 16, 16, msgs)
    n_valid = sum(models[16][w].done for w in which)
    print(f"fed pieces: 16 pieces, {n} jobs on {slots} slots, order {order}: {fin} of {n_valid} valid jobs finished by the fed kernel")
    _report(msgs)
    assert fin == n_valid
    print(f"fed pieces ok: {n} jobs on {slots} slots, order {order}")


def child_redzone(pieces):
    import redzone
    cases, _ = _load()
    copies = -(-MIN_JOBS // len(cases))
    jobs = [c for _ in range(copies) for c in cases]
    items = [dict(input=c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"], out_cap=c["cap"]) for c in jobs]
    n = len(jobs)
    redzone.check_decompress(items, [c["exp"] for c in jobs], label=f"fed pieces, {pieces} pieces", max_input_len=max(len(c["input"]) for c in jobs),
                             in_low=[(0, 1, 15)[k % 3] for k in range(n)], prefix_low=[(0, 1, 15)[(k // 3) % 3] for k in range(n)],
                             out_low=[c["rb"] for c in jobs])
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    assert launch.startswith("bitmap-fed"), launch
    print(f"fed pieces ok: red zones, {pieces} pieces: {n} jobs, {launch}")


if __name__ == "__main__":
    {"handover": child_handover, "slots": child_slots, "redzone": child_redzone}[sys.argv[1]](*sys.argv[2:])
