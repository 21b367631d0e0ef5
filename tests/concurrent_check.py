"""Child process of tests/test_gpu_concurrent.py: two callers of the PRODUCT library at once, nothing forced.

  streams  LO HI    one thread, two caller streams behind one finite gate: pairs [LO, HI) of concurrent_cases.stream_pairs()
  threads  LO HI    two Python threads (ctypes releases the GIL), each with its own stream, started by a barrier: pairs [LO, HI) of
                    concurrent_cases.thread_pairs(); the slice that holds pair 0 also has the pair whose first thread fails on the host
  mix               four threads: D3, C2, F1, H2
  first-call        no warm-up: the first D4 call (the fed kernel's census) beside D3 calls back to back (the shared lanes are made),
                    then the first Z1 and V1 calls beside D3 (the per-device residencies)
  census WHAT       the analysis library (LZF_LIB_PATH): lzf_debug_fed's geom[1], geom[3] — slots and XCD mask — in an idle process
                    (WHAT = idle) or after a first D4 call taken beside D3 calls (WHAT = contended).  Reported, never asserted.

Every output buffer lies between red zones of poison (tests/redzone.py: ZONE, OUT_POISON, _layout); after every call the zones are
intact and statuses, lengths, bytes, tables and launch strings are the case file's — the oracle's.  Results are read with copies on
the caller's own stream after that stream alone was synchronised.  Every pair runs ROUNDS rounds; a pair of two long kinds must be
seen to overlap in at least one of them.  Prints one line per pair ("pair ...") and per kind alone ("alone ..."), then
"concurrent callers ok"."""
import ctypes as C
import os
import sys
import threading
import time
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402

import concurrent_cases as K  # noqa: E402
import redzone as R  # noqa: E402
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import device, ffi, framed  # noqa: E402

DEV = torch.device("cuda", 0)
ZONE, POISON = R.ZONE, R.OUT_POISON
ROUNDS = 3
GATE_MS = 40.0                               # the shortest gate; gate_ms adds to it what the two entry points may take on the host
JOIN_S = 60.0                                # a thread that has not come back by then has hung: the child fails and starts nothing more
BARRIER_S = 20.0                             # a thread waits this long at a barrier for the others (well below JOIN_S: a lone failure is no hang)
LONG_MS = 1.0                                # a long kind takes at least this alone


_STREAMS = {}


def stream(i):
    """The child's own streams, made once: 0 the gate, 1 .. 4 the callers (with the library's three lanes: 8 in the process)."""
    assert 0 <= i <= 4
    if i not in _STREAMS:
        _STREAMS[i] = torch.cuda.Stream()
    return _STREAMS[i]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def _arena(blobs, seed):
    """The blobs in one device tensor behind zones of poison, at the seeded residues of redzone._layout."""
    offs, total = R._layout([len(b) for b in blobs], ZONE, np.random.default_rng(seed))
    h = np.full(total, POISON, dtype=np.uint8)
    for a, b in zip(offs, blobs):
        h[a:a + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return torch.from_numpy(h).to(DEV), np.array(offs, dtype=np.uint64), h


def _first_bad(d_got, d_want, d_care=None):
    """Offset of the first byte that differs (where d_care says it matters), or None — computed on the current stream."""
    bad = d_got != d_want
    if d_care is not None:
        bad &= d_care
    if not bool(bad.any().item()):
        return None
    return int(bad.to(torch.uint8).argmax().item())


class Results:
    """n lzf_job_result between two zones."""

    def __init__(self, n, fill=0):
        self.n, self.fill = n, fill
        self.d = torch.empty(2 * ZONE + 16 * n, dtype=torch.uint8, device=DEV)
        self.view = self.d[ZONE:ZONE + 16 * n]

    def reset(self):
        self.d.fill_(POISON); self.view.fill_(self.fill)

    def fetch(self, what):
        h = self.d.cpu().numpy()
        assert (h[:ZONE] == POISON).all() and (h[ZONE + 16 * self.n:] == POISON).all(), f"{what}: written outside the results"
        return h[ZONE:ZONE + 16 * self.n].copy().view(device.RES)


class Call:
    """One library call of a case.  prepare() uploads once; reset() puts the poison back (current stream); enqueue(stream) calls the
    library; check(stream) reads back on `stream` — the caller has synchronised that stream and nothing else."""
    launch = None

    def __init__(self, case):
        self.case, self.kind, self.seed = case, case["kind"], case["seed"]
        self.name = f"{self.kind}/{self.seed}"
        self.launch = K.launch_of(self.kind, self.seed)
        self.prepare()

    def last_launch(self):
        fn = getattr(ffi.lib(), f"lzf_last_{self.launch[0]}_launch")
        return fn().decode()

    def check_launch(self):
        if self.launch is not None:
            assert self.last_launch() == self.launch[1], (self.name, self.last_launch(), self.launch[1])


# ------------------------------------------------------------------------------------------------------------------ decode family
class DecodeCall(Call):
    def prepare(self):
        c = self.case
        n = self.n = len(c["jobs"])
        pres = [j["prefix"] for j in c["jobs"]]
        self.d_in, in_offs, self.h_in = _arena(c["inputs"] + pres, 100 + self.seed)
        ni = len(c["inputs"])
        caps = [j["cap"] for j in c["jobs"]]
        uniform = c.get("uniform_cap")
        if uniform:                                              # D4: equal slots a fixed stride apart, everything built and compared on the device
            stride = ZONE + (uniform + 63) // 64 * 64
            out_offs = np.uint64(ZONE) + np.uint64(stride) * np.arange(n, dtype=np.uint64)
            total = stride * n + ZONE
            self.d_want = torch.full((total,), POISON, dtype=torch.uint8, device=DEV)
            self.d_care = torch.ones(total, dtype=torch.bool, device=DEV)
            w2, c2 = self.d_want[:stride * n].view(n, stride), self.d_care[:stride * n].view(n, stride)
            which = np.array([j["inp"] for j in c["jobs"]])
            for k, d in enumerate(c["plains"]):
                rows = torch.from_numpy(np.nonzero(which == k)[0]).to(DEV)
                w2[rows, ZONE:ZONE + len(d)] = _dev(np.frombuffer(d, dtype=np.uint8))
                c2[rows, ZONE + len(d):ZONE + uniform] = False
            self.d_template = None
        else:
            offs, total = R._layout(caps, ZONE, np.random.default_rng(200 + self.seed))
            out_offs = np.array(offs, dtype=np.uint64)
            h_t = np.full(total, POISON, dtype=np.uint8)
            h_w, h_c = h_t.copy(), np.ones(total, dtype=bool)
            for a, j, (st, p) in zip(offs, c["jobs"], c["expect"]):
                ex, want = j["existing"], c["plains"][p]
                h_t[a:a + len(ex)] = np.frombuffer(ex, dtype=np.uint8)
                h_w[a:a + len(want)] = np.frombuffer(want, dtype=np.uint8)
                h_c[a + len(want):a + j["cap"]] = False          # behind out_len, inside the slot: the job's own to scribble on
            self.d_template, self.d_want, self.d_care = _dev(h_t), _dev(h_w), torch.from_numpy(h_c).to(DEV)
        self.out_offs, self.caps = out_offs, caps
        self.d_out = torch.empty(total, dtype=torch.uint8, device=DEV)
        j = np.zeros(n, dtype=device.DJOB)
        j["input"] = np.uint64(self.d_in.data_ptr()) + in_offs[[x["inp"] for x in c["jobs"]]]
        j["input_len"] = [len(c["inputs"][x["inp"]]) for x in c["jobs"]]
        j["prefix"] = np.uint64(self.d_in.data_ptr()) + in_offs[ni:]
        j["prefix_len"] = [len(p) for p in pres]
        j["out"] = np.uint64(self.d_out.data_ptr()) + out_offs
        j["out_existing_len"] = [len(x["existing"]) for x in c["jobs"]]
        j["out_cap"] = caps
        j["output_limit"] = [x["limit"] for x in c["jobs"]]
        self.d_jobs = _dev(j)
        self.res = Results(n)

    def reset(self):
        if self.d_template is None:
            self.d_out.fill_(POISON)
        else:
            self.d_out.copy_(self.d_template)
        self.res.reset()

    def enqueue(self, stream):
        device.decompress_batch(self.d_jobs, self.res.view, self.n, stream=stream, max_input_len=self.case["max_input_len"])

    def check(self, stream):
        with torch.cuda.stream(stream):
            r = self.res.fetch(self.name)
            bad = _first_bad(self.d_out, self.d_want, self.d_care)
            in_ok = bool((self.d_in.cpu().numpy() == self.h_in).all())
        for k, (st, p) in enumerate(self.case["expect"]):
            assert (int(r["status"][k]), int(r["out_len"][k])) == (st, len(self.case["plains"][p])), (self.name, "job", k, int(r["status"][k]), int(r["out_len"][k]))
        if bad is not None:
            k = int(np.searchsorted(self.out_offs, bad, side="right")) - 1
            inside = k >= 0 and bad < int(self.out_offs[k]) + self.caps[k]
            raise AssertionError(f"{self.name}: output arena differs at offset {bad}: " + (f"job {k}'s bytes, position {bad - int(self.out_offs[k])}" if inside else f"a red zone behind job {k}'s slot"))
        assert in_ok, f"{self.name}: the input arena was written to"


class SizeCall(Call):
    verify = False

    def prepare(self):
        c = self.case
        n = self.n = len(c["jobs"])
        pres = [j["prefix"] for j in c["jobs"]]
        outs = c["outs"] if self.verify else []
        ni = len(c["inputs"])                                    # (blocks and expected bytes may be shared by several jobs: both are read-only)
        self.d_in, offs, self.h_in = _arena(c["inputs"] + pres + outs, 300 + self.seed)
        inp = [x["inp"] for x in c["jobs"]]
        j = np.zeros(n, dtype=device.DJOB)
        j["input"] = np.uint64(self.d_in.data_ptr()) + offs[inp]
        j["input_len"] = [len(c["inputs"][i]) for i in inp]
        j["prefix_len"] = [len(p) for p in pres]
        j["out_existing_len"] = [len(x["existing"]) for x in c["jobs"]]
        j["output_limit"] = [x["limit"] for x in c["jobs"]]
        if self.verify:
            j["prefix"] = np.uint64(self.d_in.data_ptr()) + offs[ni:ni + n]
            j["out"] = np.uint64(self.d_in.data_ptr()) + offs[ni + n:][inp]
            j["out_cap"] = [x["cap"] for x in c["jobs"]]
        else:                                                    # the size call looks at neither prefix nor out: both stay NULL
            j["out_cap"] = 64
        self.d_jobs = _dev(j)
        self.res = Results(n, fill=0x5A)

    def reset(self):
        self.res.reset()

    def enqueue(self, stream):
        fn = device.decompress_verify_batch if self.verify else device.decompressed_size_batch
        fn(self.d_jobs, self.res.view, self.n, stream=stream, max_input_len=self.case["max_input_len"])

    def check(self, stream):
        with torch.cuda.stream(stream):
            r = self.res.fetch(self.name)
            in_ok = bool((self.d_in.cpu().numpy() == self.h_in).all())
        for k, (st, ln) in enumerate(self.case["expect"]):
            got = (int(r["status"][k]), int(r["out_len"][k]) if ln is not None else None)
            assert got == (st, ln), (self.name, "job", k, got, (st, ln))
        assert in_ok, f"{self.name}: an input, a prefix or the expected bytes were written to"


class VerifyCall(SizeCall):
    verify = True


# ---------------------------------------------------------------------------------------------------------------- compress family
class CompressCall(Call):
    dry = False

    def prepare(self):
        c = self.case
        n = self.n = len(c["jobs"])
        tabs = [(k, j["table"]) for k, j in enumerate(c["jobs"]) if j["table"] is not None]
        self.d_in, offs, self.h_in = _arena([j["input"] for j in c["jobs"]], 400 + self.seed)
        j = np.zeros(n, dtype=device.CJOB)
        j["input"] = np.uint64(self.d_in.data_ptr()) + offs
        j["input_len"] = [len(x["input"]) for x in c["jobs"]]
        j["cursor"] = [x["cursor"] for x in c["jobs"]]
        j["out_cap"] = [x["cap"] for x in c["jobs"]]
        j["table_kind"] = [x["kind"] for x in c["jobs"]]
        self.tab_jobs = [k for k, _ in tabs]
        if tabs:                                                 # the carried tables, 16-aligned, between zones
            tsize = len(tabs[0][1])
            stride = (tsize + ZONE + 63) // 64 * 64
            h = np.full(ZONE + stride * len(tabs), POISON, dtype=np.uint8)
            w = h.copy()
            for i, (k, t) in enumerate(tabs):
                h[ZONE + i * stride:ZONE + i * stride + tsize] = np.frombuffer(t, dtype=np.uint8)
                w[ZONE + i * stride:ZONE + i * stride + tsize] = np.frombuffer(c["tables_after"][k], dtype=np.uint8)
            self.d_tab_template, self.d_tab_want = _dev(h), _dev(w)
            self.d_tab = torch.empty_like(self.d_tab_template)
            j["table"][self.tab_jobs] = np.uint64(self.d_tab.data_ptr()) + np.uint64(ZONE) + np.uint64(stride) * np.arange(len(tabs), dtype=np.uint64)
        if not self.dry:
            caps = [x["cap"] for x in c["jobs"]]
            o_offs, total = R._layout(caps, ZONE, np.random.default_rng(500 + self.seed))
            self.out_offs = np.array(o_offs, dtype=np.uint64)
            h_w, h_c = np.full(total, POISON, dtype=np.uint8), np.ones(total, dtype=bool)
            for a, x, (st, b) in zip(o_offs, c["jobs"], c["expect"]):
                ln = len(b) if st == 0 else 0
                if ln:
                    h_w[a:a + ln] = np.frombuffer(b, dtype=np.uint8)
                h_c[a + ln:a + x["cap"]] = False
            self.d_want, self.d_care = _dev(h_w), torch.from_numpy(h_c).to(DEV)
            self.d_out = torch.empty(total, dtype=torch.uint8, device=DEV)
            j["out"] = np.uint64(self.d_out.data_ptr()) + self.out_offs
        self.d_jobs = _dev(j)
        self.res = Results(n)

    def reset(self):
        if not self.dry:
            self.d_out.fill_(POISON)
        if self.tab_jobs:
            self.d_tab.copy_(self.d_tab_template)
        self.res.reset()

    def enqueue(self, stream):
        fn = device.compressed_size_batch if self.dry else device.compress_batch
        fn(self.d_jobs, self.res.view, self.n, kinds=self.case["kinds"], stream=stream)

    def check(self, stream):
        with torch.cuda.stream(stream):
            r = self.res.fetch(self.name)
            bad = None if self.dry else _first_bad(self.d_out, self.d_want, self.d_care)
            tab_bad = _first_bad(self.d_tab, self.d_tab_want) if self.tab_jobs else None
            in_ok = bool((self.d_in.cpu().numpy() == self.h_in).all())
        for k, (st, b) in enumerate(self.case["expect"]):
            ln = None if st != 0 else b if self.dry else len(b)
            got = (int(r["status"][k]), int(r["out_len"][k]) if ln is not None else None)
            assert got == (st, ln), (self.name, "job", k, got, (st, ln))
        if bad is not None:
            k = int(np.searchsorted(self.out_offs, bad, side="right")) - 1
            raise AssertionError(f"{self.name}: output arena differs from the oracle's bytes at offset {bad} (job {k}'s slot starts at {int(self.out_offs[max(k, 0)])})")
        assert tab_bad is None, f"{self.name}: the carried tables differ from the oracle's at byte {tab_bad} of their arena"
        assert in_ok, f"{self.name}: the input arena was written to"


class CompressedSizeCall(CompressCall):
    dry = True


# ------------------------------------------------------------------------------------------------------------------- the helpers
GUARD = 0x5A5A5A5A


class XxhCall(Call):
    def prepare(self):
        self.parts = []
        for c in self.case["calls"]:
            d = _dev(c["arena"])
            n = len(c["lens"])
            self.parts.append(dict(d=d, ptrs=_dev(np.uint64(d.data_ptr()) + c["offs"]), lens=_dev(c["lens"]), n=n,
                                   out=torch.empty(n + 64, dtype=torch.int32, device=DEV), want=c["hashes"]))

    def reset(self):
        for p in self.parts:
            p["out"].fill_(GUARD)

    def enqueue(self, stream):
        for p in self.parts:
            device.xxh32_batch(p["ptrs"], p["lens"], p["out"], p["n"], stream=stream)

    def check(self, stream):
        for i, p in enumerate(self.parts):
            with torch.cuda.stream(stream):
                got = p["out"].cpu().numpy().view(np.uint32)
            bad = np.nonzero(got[:p["n"]] != p["want"])[0]
            assert not len(bad), f"{self.name}: call {i}: {len(bad)} of {p['n']} hashes differ from the oracle's, first buffer {int(bad[0])}"
            assert (got[p["n"]:] == GUARD).all(), f"{self.name}: call {i}: out[] written behind its n entries"


class CopyCall(Call):
    def prepare(self):
        c = self.case
        self.d_src = _dev(c["src"])
        self.d_dst = torch.empty(c["total"], dtype=torch.uint8, device=DEV)
        self.d_want = _dev(K.copy_expect(c, POISON))
        self.a = (_dev(np.uint64(self.d_src.data_ptr()) + c["so"]), _dev(np.uint64(self.d_dst.data_ptr()) + c["do"]), _dev(c["lens"]))

    def reset(self):
        self.d_dst.fill_(POISON)

    def enqueue(self, stream):
        device.copy_ranges(*self.a, len(self.case["lens"]), self.case["max_len"], stream=stream)

    def check(self, stream):
        with torch.cuda.stream(stream):
            bad = _first_bad(self.d_dst, self.d_want)
        assert bad is None, f"{self.name}: destination differs at offset {bad}"


class TrimCall(Call):
    def prepare(self):
        rows = self.case["rows"]
        n = self.n = len(rows)
        j = np.zeros(n, dtype=device.DJOB)
        for name in device.DJOB.names:
            j[name] = [r[name] for r in rows]
        self.d_jobs, self.h_jobs = _dev(j), j
        want = np.zeros(n, dtype=device.DJOB)
        self.shifts = np.zeros(n, dtype=np.uint64)
        for k, r in enumerate(rows):
            t, self.shifts[k] = K.trim_expect(r)
            for name in device.DJOB.names:
                want[name][k] = t[name]
        self.want_jobs = want
        self.d_trim = torch.empty(2 * ZONE + 64 * n, dtype=torch.uint8, device=DEV)
        self.d_shift = torch.empty(2 * ZONE + 8 * n, dtype=torch.uint8, device=DEV)
        res = np.zeros(n, dtype=device.RES)
        res["status"] = [st for st, _ in self.case["results"]]; res["out_len"] = [ln for _, ln in self.case["results"]]
        self.h_res = res
        self.res = Results(n)

    def reset(self):
        self.d_trim.fill_(POISON); self.d_shift.fill_(POISON)
        self.res.reset()
        self.res.view.copy_(_dev(self.h_res))

    def enqueue(self, stream):
        device.history_trim_batch(self.d_jobs, self.d_trim[ZONE:], self.d_shift[ZONE:], self.n, stream=stream)
        device.history_restore_batch(self.res.view, self.d_shift[ZONE:], self.n, stream=stream)

    def check(self, stream):
        n = self.n
        with torch.cuda.stream(stream):
            r = self.res.fetch(self.name)
            t, s = self.d_trim.cpu().numpy(), self.d_shift.cpu().numpy()
            jobs_ok = bool((self.d_jobs.cpu().numpy().view(device.DJOB) == self.h_jobs).all())
        for a, body in ((t, 64 * n), (s, 8 * n)):
            assert (a[:ZONE] == POISON).all() and (a[ZONE + body:] == POISON).all(), f"{self.name}: written outside the trimmed jobs / the shifts"
        got = t[ZONE:ZONE + 64 * n].copy().view(device.DJOB)
        bad = np.nonzero(got != self.want_jobs)[0]
        assert not len(bad), (self.name, "trimmed job", int(bad[0]), got[bad[0]], self.want_jobs[bad[0]])
        assert (s[ZONE:ZONE + 8 * n].copy().view(np.uint64) == self.shifts).all(), f"{self.name}: shifts"
        for k, (st, ln) in enumerate(self.case["results"]):
            want = ln + int(self.shifts[k]) if st == 0 else ln
            assert (int(r["status"][k]), int(r["out_len"][k])) == (st, want), (self.name, "restored result", k)
        assert jobs_ok, f"{self.name}: the job array was written to"


# ---------------------------------------------------------------------------------------------------------- frames in device memory
def _slots(caps):
    """One poison arena, one view per capacity with a zone in front of and behind each."""
    offs = np.cumsum([ZONE] + [(c + ZONE + 63) // 64 * 64 for c in caps])
    arena = torch.empty(int(offs[-1]), dtype=torch.uint8, device=DEV)
    return arena, [arena[int(a):int(a) + c] for a, c in zip(offs[:-1], caps)], offs[:-1]


def _zones_ok(arena, offs, caps, lens):
    """On the current stream: is everything outside [slot, slot + len) of every slot still poison?"""
    keep = torch.ones(arena.numel(), dtype=torch.bool, device=DEV)
    for a, ln in zip(offs, lens):
        keep[int(a):int(a) + int(ln)] = False
    return _first_bad(arena, torch.full_like(arena, POISON), keep)


class FrameCall(Call):
    """The device frame drivers: they scan on the caller's stream and wait for it in mid-call — only another thread overlaps them."""

    def prepare(self):
        c, f = self.case, self.case["family"]
        self.frames = [_dev(np.frombuffer(x, dtype=np.uint8)) for x in c["frames"]]
        self.d_plain = [_dev(np.frombuffer(x, dtype=np.uint8)) for x in c["plains"]]
        self.ok = [k for k, d in enumerate(c["decoded"]) if d[0] == 0]
        if f == "frame_decompress":
            self.caps = device.frame_decompress_bound(self.frames)
        elif f == "frame_compress":
            s = framed.CompressionSettings().block_size(c["settings"]["block_size"]).independent_blocks(c["settings"]["independent_blocks"]) \
                .content_checksum(c["settings"]["content_checksum"])
            self.settings = s._struct(None)
            self.caps = [ffi.lib().lzf_frame_compress_bound(C.byref(self.settings), len(d)) for d in c["plains"]]
            self.d_expect = [_dev(np.frombuffer(x, dtype=np.uint8)) for _, x in c["expect"]]
        elif f == "stream_decompress":
            self.streams = [torch.cat([self.frames[k] for k in ks]) for ks in c["streams"]]
            self.d_expect = [torch.cat([self.d_plain[k] for k in ks]) for ks in c["streams"]]
            self.caps = device.stream_decompress_bound(self.streams)
        elif f == "frame_verify":
            self.d_wanted = [_dev(np.frombuffer(x, dtype=np.uint8)) for x in c["wanted"]]
            self.caps = []
        elif f == "frame_blocks":
            self.runs_of = [k for k in self.ok if c["frames"][k][4] & 0x20]          # independent blocks only
            self.caps = [len(c["plains"][k]) for k in self.runs_of]
        else:
            self.caps = []
        if self.caps:
            self.arena, self.outs, self.offs = _slots(self.caps)

    def reset(self):
        if self.caps:
            self.arena.fill_(POISON)
        self.got = None

    def enqueue(self, stream):
        f = self.case["family"]
        with torch.cuda.stream(stream):
            if f == "frame_decompress":
                self.got = device.frame_decompress_many(self.frames, self.outs, stream=stream)
            elif f == "frame_compress":
                self.got = device.frame_compress_many(self.settings, self.d_plain, self.outs, stream=stream)
            elif f == "stream_decompress":
                self.got = device.stream_decompress(self.streams, self.outs, stream=stream)
            elif f == "frame_verify":
                self.got = device.frame_verify(self.frames, self.d_wanted, stream=stream)
            elif f == "frame_size":
                self.got = device.frame_decompressed_size(self.frames, stream=stream)
            else:
                status, out_len, consumed, n_listed, entries = device.frame_block_index(self.frames, stream=stream)
                stream.synchronize()                             # (the runs are host copies of the index)
                self.index = (status.cpu().tolist(), out_len.cpu().tolist(), consumed.cpu().tolist(), n_listed.cpu().tolist(),
                              [np.ascontiguousarray(e.cpu().numpy()).view(device.FBLOCK) for e in entries])
                runs = [self.index[4][k] for k in self.runs_of]
                self.got = device.frame_decompress_blocks([self.frames[k] for k in self.runs_of], runs, self.outs, stream=stream)

    def check(self, stream):
        c, f, name = self.case, self.case["family"], self.name
        with torch.cuda.stream(stream):
            got = [t.cpu().tolist() for t in self.got]
        dec = c["decoded"]
        if f == "frame_decompress":
            lens = []
            for k, (st, b, used) in enumerate(dec):
                assert got[0][k] == st, (name, "frame", k, "status", got[0][k], st)
                if st == 0:
                    assert (got[1][k], got[2][k]) == (len(b), used), (name, "frame", k, got[1][k], got[2][k])
                lens.append(len(b) if st == 0 else self.caps[k])
            self._bytes(stream, [self.d_plain[k] if dec[k][0] == 0 else None for k in range(len(dec))], lens)
        elif f == "frame_compress":
            for k, (rc, fr) in enumerate(c["expect"]):
                assert (got[0][k], got[1][k]) == (rc, len(fr)), (name, "frame", k, got[0][k], got[1][k])
            self._bytes(stream, self.d_expect, [t.numel() for t in self.d_expect])
        elif f == "stream_decompress":
            for k, ks in enumerate(c["streams"]):
                assert (got[0][k], got[1][k], got[2][k], got[3][k]) == (0, self.d_expect[k].numel(), self.streams[k].numel(), len(ks)), (name, "stream", k, [g[k] for g in got])
            self._bytes(stream, self.d_expect, [t.numel() for t in self.d_expect])
        elif f == "frame_verify":
            for k, (st, at) in enumerate(c["expect"]):
                assert got[0][k] == st and (st not in (0, K.MISMATCH) or got[1][k] == at), (name, "frame", k, got[0][k], got[1][k], (st, at))
        elif f == "frame_size":
            for k, (st, b, used) in enumerate(dec):
                assert got[0][k] == st and (st != 0 or (got[1][k], got[2][k]) == (len(b), used)), (name, "frame", k, [g[k] for g in got])
        else:
            st_i, len_i, used_i, listed, entries = self.index
            for k, (st, b, used) in enumerate(dec):
                assert st_i[k] == st and (st != 0 or (len_i[k], used_i[k]) == (len(b), used)), (name, "index of frame", k)
                if st == 0:
                    e = entries[k]
                    assert listed[k] == len(e) == -(-len(b) // K.FRAME_BLOCK) and int(e["out_len"].sum()) == len(b), (name, "blocks of frame", k)
                    assert (e["out_off"] == np.arange(len(e), dtype=np.uint64) * np.uint64(K.FRAME_BLOCK)).all(), (name, "block offsets of frame", k)
            for i, k in enumerate(self.runs_of):
                assert (got[0][i], got[1][i]) == (0, len(c["plains"][k])), (name, "run of frame", k, got[0][i], got[1][i])
            self._bytes(stream, [self.d_plain[k] for k in self.runs_of], self.caps)

    def _bytes(self, stream, wants, lens):
        with torch.cuda.stream(stream):
            for k, (w, out) in enumerate(zip(wants, self.outs)):
                if w is not None:
                    bad = _first_bad(out[:w.numel()], w)
                    assert bad is None, f"{self.name}: output {k} differs at byte {bad}"
            bad = _zones_ok(self.arena, self.offs, self.caps, lens)
        assert bad is None, f"{self.name}: written outside an output's [0, out_len) at arena offset {bad}"


# ---------------------------------------------------------------------------------------------------------------- host buffers
class HostBatchCall(Call):
    def prepare(self):
        c = self.case
        self.d_items = [dict(input=comp, limit=len(d), out_cap=len(d) + len(comp) + 64) for d, (_, comp) in zip(c["plains"], c["comp"])]
        self.c_items = [dict(input=d) for d in c["plains"]]

    def reset(self):
        self.got = None

    def enqueue(self, stream):
        self.got = (ffi.decompress_blocks_host(self.d_items), ffi.compress_blocks_host(self.c_items))

    def check(self, stream):
        for k, (d, (rc, comp)) in enumerate(zip(self.case["plains"], self.case["comp"])):
            assert self.got[0][k] == (0, d), (self.name, "decoded block", k, self.got[0][k][0])
            assert self.got[1][k] == (rc, comp), (self.name, "compressed block", k, self.got[1][k][0])


class HostFramesCall(Call):
    def prepare(self):
        kw = self.case["settings"]
        self.settings = framed.CompressionSettings().block_size(kw["block_size"]).independent_blocks(kw["independent_blocks"]).content_checksum(kw["content_checksum"])
        self.caps = [len(d) + 65536 for d in self.case["plains"]]

    def reset(self):
        self.got = None

    def enqueue(self, stream):
        self.got = (self.settings.compress_many(self.case["plains"]), framed.decompress_frames(self.case["frames"], caps=self.caps))

    def check(self, stream):
        for k, (d, f) in enumerate(zip(self.case["plains"], self.case["frames"])):
            assert self.got[0][k] == f, (self.name, "frame", k, "differs from the oracle's")
            assert self.got[1][k] == (0, d), (self.name, "decoded frame", k, self.got[1][k][0])


FAMILY = {"decode": DecodeCall, "size": SizeCall, "verify": VerifyCall, "compress": CompressCall, "csize": CompressedSizeCall, "xxh": XxhCall,
          "copy": CopyCall, "trim": TrimCall, "host_batch": HostBatchCall, "host_frames": HostFramesCall}
_CALLS = {}


def call_of(ks):
    if ks not in _CALLS:
        case = K.build(*ks)
        _CALLS[ks] = FAMILY.get(case["family"], FrameCall)(case)
    return _CALLS[ks]


# ------------------------------------------------------------------------------------------------------------------- alone
ALONE_MS, ENQUEUE_MS, TOO_SHORT = {}, {}, []


def warm_up(ks):
    """The call alone, four times: checked every time; its time alone is the median of the last three (events around it on a side
    stream; wall time for the kinds that block the host)."""
    if ks in ALONE_MS:
        return
    call, s, times = call_of(ks), stream(1), []
    for _ in range(4):
        call.reset()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(s); call.enqueue(s); e1.record(s)
        ENQUEUE_MS[ks] = max(ENQUEUE_MS.get(ks, 0.0), (time.perf_counter() - t0) * 1e3)      # (the first call's includes whatever is made once, and the pool's growth)
        s.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        call.check(s); call.check_launch()
        times.append(wall if ks[0] in K.FRAME_KINDS + K.HOST_KINDS else e0.elapsed_time(e1))
    ms = sorted(times[1:])[1]
    ALONE_MS[ks] = ms
    print(f"alone {call.name}: {K.job_count(call.case)} jobs, {ms:.3f} ms")
    if ks[0] in K.LONG and ms < LONG_MS:                         # (asserted at the child's end: every figure is printed first)
        TOO_SHORT.append(f"{call.name} is a long kind and took {ms:.3f} ms alone: raise its job count in concurrent_cases.COUNTS")


# ------------------------------------------------------------------------------------------------------------------- (a) streams
_CYCLES_PER_MS = None


def gate(stream, ms):
    """A finite delay on `stream`: torch.cuda._sleep where this torch has it (calibrated once), else a chain of matmuls."""
    global _CYCLES_PER_MS
    if hasattr(torch.cuda, "_sleep"):
        if _CYCLES_PER_MS is None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(1000); torch.cuda.synchronize()
            e0.record(); torch.cuda._sleep(10_000_000); e1.record(); torch.cuda.synchronize()
            _CYCLES_PER_MS = 10_000_000 / e0.elapsed_time(e1)
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int(ms * _CYCLES_PER_MS))
    else:
        a = torch.randn(2048, 2048, device=DEV)
        with torch.cuda.stream(stream):
            for _ in range(int(ms * 4)):
                a = (a @ a).clamp_(-1, 1)


def _overlap(a, b):
    return a[0] < b[1] and b[0] < a[1]


POOL_MS_PER_GIB = 300.0


def gate_ms(pair):
    """An entry point never waits for the device, but it may take the host a while: hipMallocAsync, where the pool does not hand the
    call the block it used last time, waits for fresh device memory, and the time that takes grows with the request and differs from
    machine to machine — traced: 1.85 s for 7.6 GiB, 0.24 s per GiB (profiles/concurrent_callers.txt).  The gate covers three times the
    longest each entry point has taken so far in this process, its first call included, and 0.3 s per GiB of scratch the two calls ask
    the pool for (concurrent_cases.pool_request: 2.6 GiB for the size call of 4 096 jobs, under 1.4 GiB for every other kind)."""
    return GATE_MS + 3.0 * sum(ENQUEUE_MS[ks] for ks in pair) + POOL_MS_PER_GIB * sum(K.pool_request(*ks) for ks in pair) / 2 ** 30


def stream_pair(pair, streams):
    x, y = call_of(pair[0]), call_of(pair[1])
    g, s1, s2 = streams
    # each call once, ungated, on the stream it is about to use: the pool re-uses a block soonest on the stream that freed it
    for c, s in ((x, s1), (y, s2)):
        c.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.enqueue(s)
        ENQUEUE_MS[(c.kind, c.seed)] = max(ENQUEUE_MS[(c.kind, c.seed)], (time.perf_counter() - t0) * 1e3)
        s.synchronize()
        c.check(s)
    seen, closed_ms = [], gate_ms(pair)
    for rnd in range(ROUNDS):
        x.reset(); y.reset()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        base, opened = ev[0], torch.cuda.Event()
        base.record(g)
        gate(g, closed_ms)
        opened.record(g)
        s1.wait_event(opened); s2.wait_event(opened)
        t0 = time.perf_counter()
        ev[1].record(s1); x.enqueue(s1); ev[2].record(s1)
        t1 = time.perf_counter()
        x.check_launch()                                         # (set by the entry point, on the host: this thread's last call of its class)
        ev[3].record(s2); y.enqueue(s2); ev[4].record(s2)
        t2 = time.perf_counter()
        y.check_launch()
        # (an entry point that took about as long as the gate has waited for the device; one that took longer than ever before was slow on the host)
        assert not opened.query(), (f"{x.name} + {y.name}, round {rnd}: the gate of {closed_ms:.0f} ms opened before both entry points had returned: "
                                    f"{x.name} took {(t1 - t0) * 1e3:.2f} ms on the host, {y.name} {(t2 - t1) * 1e3:.2f} ms")
        # X on stream 1 alone, then Y on stream 2 alone; no device-wide synchronisation before the first comparison
        s1.synchronize()
        x.check(s1)
        s2.synchronize()
        y.check(s2)
        torch.cuda.synchronize()
        ix, iy = (base.elapsed_time(ev[1]), base.elapsed_time(ev[2])), (base.elapsed_time(ev[3]), base.elapsed_time(ev[4]))
        seen.append(_overlap(ix, iy))
    print(f"gate {x.name} + {y.name}: closed for {closed_ms:.0f} ms (entry points alone: up to {ENQUEUE_MS[pair[0]]:.2f} and {ENQUEUE_MS[pair[1]]:.2f} ms on the host)")
    report(pair, seen, [ix, iy])


def report(pair, seen, last):
    names = " + ".join(f"{k}/{s}" for k, s in pair)
    span, alone = max(b for _, b in last) - min(a for a, _ in last), sum(ALONE_MS[ks] for ks in pair)
    # (two threads released by one barrier meet whatever the library does: what the meeting was worth is the span against the sum)
    worth = "one after the other" if span >= 0.9 * alone else "side by side"
    print(f"pair {names}: overlapped in {sum(seen)} of {len(seen)} rounds; last round " + ", ".join(f"[{a:.3f}, {b:.3f}]" for a, b in last) +
          f" ms: {span:.3f} ms together, {alone:.3f} ms one after the other alone: {worth}")
    if all(k in K.LONG for k, _ in pair):
        assert any(seen), f"{names}: never overlapped in {len(seen)} rounds — the two calls ran one after the other"


def mode_streams(lo, hi):
    pairs = K.stream_pairs()[lo:hi]
    for ks in sorted({ks for p in pairs for ks in p}):
        warm_up(ks)
    for p in pairs:
        stream_pair(p, (stream(0), stream(1), stream(2)))


# ------------------------------------------------------------------------------------------------------------------- (b) threads
class Worker(threading.Thread):
    """Runs `body(self)`; an exception is kept with its traceback, and breaks the barriers the other threads of the group may be
    waiting at — they end with BrokenBarrierError at once, not at a time limit, and the failure is reported as what it is."""

    def __init__(self, body, name, barriers=()):
        super().__init__(name=name, daemon=True)
        self.body, self.barriers, self.error, self.interval = body, barriers, None, None

    def run(self):
        try:
            torch.cuda.set_device(0)
            self.body(self)
        except threading.BrokenBarrierError:
            self.error = "stopped at a barrier that another thread's failure (or the barrier's own time limit) broke\n"
        except BaseException:
            self.error = traceback.format_exc()
            for b in self.barriers:
                b.abort()


def run_threads(workers, what):
    for w in workers:
        w.start()
    deadline = time.monotonic() + JOIN_S
    for w in workers:
        w.join(max(deadline - time.monotonic(), 0.0))
    hung = [w.name for w in workers if w.is_alive()]
    errors = [f"--- {what}, thread {w.name}:\n{w.error}" for w in workers if w.error]
    if hung:
        print("\n".join(errors + [f"{what}: threads {hung} did not come back within {JOIN_S:.0f} s"]), flush=True)
        os._exit(3)                                               # nothing more is started on the device
    if errors:
        raise AssertionError("\n".join(errors))


def thread_group(group, fail_first=False):
    """len(group) threads, one call each; fail_first: thread 0 first makes a call that fails on the host with LZF_E_INVALID."""
    calls = [call_of(ks) for ks in group]
    streams = [stream(1 + i) for i in range(len(calls))]
    seen, lib = [], ffi.lib()
    lib.lzf_last_error.restype = C.c_char_p
    for rnd in range(ROUNDS):
        for c in calls:
            c.reset()
        torch.cuda.synchronize()
        start, called = threading.Barrier(len(calls)), threading.Barrier(len(calls))

        def body(w, i):
            c, s = calls[i], streams[i]
            before = lib.lzf_last_error()
            start.wait(BARRIER_S)
            if fail_first and i == 0:
                t = calls[0]
                rc = lib.lzf_history_trim_batch(t.d_jobs.data_ptr(), t.d_jobs.data_ptr(), t.d_shift.data_ptr(), t.n, s.cuda_stream)
                assert rc == ffi.E_INVALID, rc
                assert lib.lzf_last_error(), "LZF_E_INVALID without a text in lzf_last_error() of the thread that failed"
            t0 = time.perf_counter()
            with torch.cuda.stream(s):
                c.enqueue(s)
            s.synchronize()
            w.interval = (t0, time.perf_counter())
            called.wait(BARRIER_S)                                # the other thread has made its call — of another class, in most pairs
            if fail_first and i != 0:
                assert lib.lzf_last_error() == before, ("lzf_last_error() of a thread that made no failing call changed", before, lib.lzf_last_error())
            c.check_launch()
            c.check(s)
        workers = [Worker(lambda w, i=i: body(w, i), calls[i].name, (start, called)) for i in range(len(calls))]
        run_threads(workers, " + ".join(c.name for c in calls))
        iv = [w.interval for w in workers]
        seen.append(all(_overlap(iv[0], v) for v in iv[1:]))
    t0 = min(a for a, _ in iv)
    report(tuple(group), seen, [((a - t0) * 1e3, (b - t0) * 1e3) for a, b in iv])


def mode_threads(lo, hi):
    pairs = K.thread_pairs()[lo:hi]
    for ks in sorted({ks for p in pairs for ks in p}):
        warm_up(ks)
    for p in pairs:
        thread_group(p)
    if lo == 0:
        warm_up(("A3", 0)); warm_up(("D2", 1))
        thread_group((("A3", 0), ("D2", 1)), fail_first=True)
        print("error pair: LZF_E_INVALID and its text stayed in the thread that failed")


def mode_mix():
    for ks in K.THREAD_MIX:
        warm_up(ks)
    thread_group(K.THREAD_MIX)


# ------------------------------------------------------------------------------------------------------------------- (c) first call
def first_call(first, beside=("D3", 1), times=4):
    """No warm-up of `first`: its first call of the process runs in one thread while another makes `beside` calls back to back."""
    a, b = call_of(first), call_of(beside)
    sa, sb = stream(1), stream(2)
    a.reset(); b.reset()
    torch.cuda.synchronize()
    start = threading.Barrier(2)

    def body_a(w):
        start.wait(BARRIER_S)
        with torch.cuda.stream(sa):
            a.enqueue(sa)
        sa.synchronize()
        a.check_launch(); a.check(sa)

    def body_b(w):
        start.wait(BARRIER_S)
        for _ in range(times):
            with torch.cuda.stream(sb):
                b.enqueue(sb)
            sb.synchronize()
            b.check_launch(); b.check(sb)
            with torch.cuda.stream(sb):
                b.reset()
    run_threads([Worker(body_a, a.name, (start,)), Worker(body_b, b.name, (start,))], f"first {a.name} beside {b.name}")
    print(f"first call {a.name} beside {times} x {b.name}: results right")


def mode_first_call():
    first_call(("D4", 0))                                         # the census beside the making of the lanes
    first_call(("Z1", 0))
    first_call(("V1", 0))


def mode_census(what):
    """slots and XCD mask the fed kernel's census kept in this process (lzf_debug_fed, analysis library).  idle: the census is taken
    by lzf_debug_fed itself with nothing else on the device; contended: by a first D4 call beside D3 calls."""
    assert ffi.lib_path() == os.environ["LZF_LIB_PATH"]
    if what == "contended":
        first_call(("D4", 0))
    c = call_of(("D4", 1))
    c.reset()
    torch.cuda.synchronize()
    geom = (C.c_uint32 * 4)()
    fn = ffi.lib().lzf_debug_fed
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    ffi.check(fn(c.d_jobs.data_ptr(), c.res.view.data_ptr(), c.n, K.D4_BOUND, 0, None, None, None, geom))
    print(f"census {what}: pieces {geom[0]}, slots {geom[1]}, grid {geom[2]}, XCD mask {geom[3]:#x}")


if __name__ == "__main__":
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    t_start = time.perf_counter()
    mode, args = sys.argv[1], sys.argv[2:]
    if mode == "streams":
        mode_streams(int(args[0]), int(args[1]))
    elif mode == "threads":
        mode_threads(int(args[0]), int(args[1]))
    elif mode == "mix":
        mode_mix()
    elif mode == "first-call":
        mode_first_call()
    elif mode == "census":
        mode_census(args[0])
    else:
        raise SystemExit(f"unknown mode {mode}")
    print(f"child wall time {time.perf_counter() - t_start:.1f} s")
    assert not TOO_SHORT, "\n".join(TOO_SHORT)
    print("concurrent callers ok")
