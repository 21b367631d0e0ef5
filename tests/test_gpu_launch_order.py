"""The launch-order stage on the device against the host models of launch_order_cases.py, whose reach test_launch_order_cases_cpu.py proves
without a GPU.  Child processes load the analysis library and run one piece of the stage at a time through lzf_debug_order, which launches
through the launch lines of the batch calls (capi_order.h, fed_front):

  * the three ordering kernels over every size and estimate case: the permutation and the 1024-class rule (order_fault), never element by element;
  * lzf_decompress_cost_kernel: est[] equals cost_est for every case, address residue, len_shift and under two poisons behind the inputs;
  * the front of a fed call: est[] equals fed_est, the order holds, and for the in-step jobs est minus the bytes' share is the sequence count;
  * the compress probes: the probe jobs equal probe_jobs field by field, the dry run's status and out_len are the oracle's compress2 of the
    piece, its work lies between the sequences of the oracle's trace and that plus the piece's length, is the same in two runs, and the
    order by the device's own work values holds;
  * one leg through the batch calls with LZF_COMPRESS_ORDER=always and LZF_DECOMPRESS_ORDER=always: the results are the oracle's.

No figure asserted here comes from the device: equalities from the models, w from the sort's class count, the work bounds from the trace."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import launch_order_cases as Lc  # noqa: E402
import oracle_ffi as o  # noqa: E402
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import ffi, synth  # noqa: E402
from test_gpu_parse_staging import PATHS  # noqa: E402

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x1F)                      # behind every input: a length byte that never ends, then a token with 15 literals and a long match
SORT_BY_EST, SORT_BY_LEN, SORT_BY_COST, COST, FED, PROBES = range(6)      # lzf_debug_order's `what`


def _child(what, *args, **env):
    from rust_lz_fear_amd import build
    e = dict(os.environ, LZF_LIB_PATH=build.build_analysis_library(), **env)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what, *args], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "launch order ok" in r.stdout, r.stdout[-2000:]
    print(r.stdout.strip().splitlines()[-1], f"[{time.time() - t0:.1f} s]")
    return r.stdout


def test_the_three_sorts_keep_the_class_rule():
    _child("sorts")


def test_sampled_estimates_equal_the_model():
    _child("cost")


def test_fed_estimates_equal_the_model_and_order():
    _child("fed")


@pytest.mark.parametrize("piece,parts", Lc.PROBES)
def test_compress_probes(piece, parts):
    _child("probes", str(piece), str(parts))


@pytest.mark.parametrize("probe", ["65536,1", "4096,16"])
def test_ordered_batch_calls_give_the_oracles_results(probe):
    _child("e2e", LZF_COMPRESS_ORDER="always", LZF_DECOMPRESS_ORDER="always", LZF_COMPRESS_KERNEL="compact", LZF_DECOMPRESS_KERNEL="noseg", LZF_PROBE=probe)


def test_ordered_fed_call_gives_the_oracles_results():
    _child("e2e_fed", LZF_DECOMPRESS_ORDER="always", **PATHS["fed"])


# ---------------------------------------------------------------------------------------------------------------- the children
def _debug_order():
    fn = ffi.lib().lzf_debug_order
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def _run(what, d_jobs, n, h_in=None, a=0, b=0, parts=0):
    """One call of lzf_debug_order: (est, perm, probe jobs, probe results), each None where the piece does not give it."""
    from rust_lz_fear_amd import device
    est = np.full(n, 0xA5A5A5A5, np.uint32); perm = np.full(n, 0xA5A5A5A5, np.uint32)
    probes = np.zeros(n * parts, Lc.CJOB); pres = np.zeros(n * parts, device.RES)
    h_in = None if h_in is None else np.ascontiguousarray(h_in)
    ffi.check(_debug_order()(what, d_jobs.data_ptr() if d_jobs is not None else None, n, h_in.ctypes.data if h_in is not None else None, a, b,
                             est.ctypes.data, perm.ctypes.data, probes.ctypes.data if parts else None, pres.ctypes.data if parts else None))
    return (est if what in (COST, FED) else None, perm if what not in (COST, PROBES) else None, probes if what == PROBES else None,
            pres if what == PROBES else None)


def _djobs(input_len, inputs=None):
    from rust_lz_fear_amd import device
    dj = np.zeros(len(input_len), device.DJOB)
    dj["input_len"] = input_len
    if inputs is not None:
        dj["input"] = inputs
    return dj


def _cjobs(jobs):
    cj = np.zeros(len(jobs), Lc.CJOB)
    cj["input"] = [j["input"] for j in jobs]; cj["input_len"] = [j["input_len"] for j in jobs]; cj["cursor"] = [j["cursor"] for j in jobs]
    cj["table_kind"] = Lc.TABLE_U32
    return cj


def child_sorts():
    from rust_lz_fear_amd import device
    msgs, runs = [], 0

    def check(label, est, perm):
        nonlocal runs
        runs += 1
        fault = Lc.order_fault(est, perm)
        if fault:
            msgs.append(f"{label}: {fault}")

    for n in Lc.SORT_SIZES:
        for kind in Lc.SORT_KINDS:
            e = Lc.sort_estimates(kind, n)
            check(f"by estimate, n {n}, {kind}", e, _run(SORT_BY_EST, None, n, h_in=e)[1])
            check(f"by input length, n {n}, {kind}", e, _run(SORT_BY_LEN, device.to_device(_djobs(e.astype(np.uint64)), "cuda"), n)[1])
            for parts in (1, 3):
                jobs, reserved = Lc.cost_sort_jobs(e, parts, mixed=kind != "all equal")
                res = np.zeros(n * parts, device.RES)
                res["reserved"] = reserved; res["out_len"] = 0x7777; res["status"] = 3      # (the sort reads `reserved` alone)
                ce = Lc.cost_estimates(jobs, reserved, Lc.COST_PIECE, parts)
                check(f"by cost, n {n}, parts {parts}, {kind}", ce, _run(SORT_BY_COST, device.to_device(_cjobs(jobs), "cuda"), n, h_in=res, a=Lc.COST_PIECE, b=parts)[1])
        v = Lc.input_len_edges(n)
        check(f"by input length, n {n}, lengths of 0 and 2^31", v, _run(SORT_BY_LEN, device.to_device(_djobs(v), "cuda"), n)[1])
    for text in msgs[:40]:
        print(text)
    assert not msgs, f"{len(msgs)} orders break the rule"
    print(f"launch order ok: {runs} sorts through the three ordering kernels, sizes {Lc.SORT_SIZES}; behind the outlier the other jobs fall into "
          f"{Lc.outlier_classes()} class")


def _pool(items, fill, align=256, gap=512):
    """A host pool with every item (bytes, address residue) at that residue of a 256-byte line, `fill` everywhere else; gap: bytes of fill at
    least behind every item.  Returns (pool, offsets)."""
    offs, t = [], align
    for data, r in items:
        offs.append(t + r)
        t = (t + r + len(data) + gap + align - 1) // align * align
    pool = np.full(t + align, fill, np.uint8)
    for (data, _), a in zip(items, offs):
        pool[a:a + len(data)] = np.frombuffer(data, np.uint8)
    return pool, np.array(offs, np.uint64)


def child_cost():
    import torch
    from rust_lz_fear_amd import device
    cases = Lc.cost_cases()
    jobs = [(c, r) for c in cases for r in Lc.RESIDUES]
    n = len(jobs)
    want = {s: np.array([Lc.cost_est(c["input"], s, c["input_len"]) for c, _ in jobs], np.uint32) for s in Lc.LEN_SHIFTS}
    assert len({tuple(v.tolist()) for v in want.values()}) == 3                # (31 and 32 add nothing to these lengths; 0 and 2 do)
    msgs, got_by_poison = [], []
    for poison in POISONS:
        pool, offs = _pool([(c["input"] or b"", r) for c, r in jobs], poison)
        d_pool = torch.from_numpy(pool).cuda()
        assert d_pool.data_ptr() % 256 == 0
        ptr = np.uint64(d_pool.data_ptr()) + offs
        assert all(int(p) % 16 == r for p, (_, r) in zip(ptr, jobs))
        ptr[[i for i, (c, _) in enumerate(jobs) if c["input"] is None]] = 0
        d_jobs = device.to_device(_djobs([c["input_len"] for c, _ in jobs], ptr), "cuda")
        got = {}
        for s in Lc.LEN_SHIFTS:
            got[s] = _run(COST, d_jobs, n, a=s)[0]
            for i in np.nonzero(got[s] != want[s])[0].tolist():
                msgs.append(f"[{jobs[i][0]['name']}] residue {jobs[i][1]} len_shift {s} poison {poison:#x}: est {int(got[s][i])}, model {int(want[s][i])}")
        got_by_poison.append(got)
        assert (d_pool.cpu().numpy() == pool).all(), "the inputs' pool was written"
    for s in Lc.LEN_SHIFTS:
        if (got_by_poison[0][s] != got_by_poison[1][s]).any():
            msgs.append(f"len_shift {s}: the estimates depend on the bytes behind the inputs")
    for text in msgs[:40]:
        print(text)
    assert not msgs, f"{len(msgs)} estimates differ"
    print(f"launch order ok: {n} jobs ({len(cases)} cases x residues {Lc.RESIDUES}) x len_shift {Lc.LEN_SHIFTS} x 2 poisons: every estimate the model's")


def child_fed():
    import torch
    from rust_lz_fear_amd import device
    cases = Lc.fed_cases()
    n = len(cases)
    pool, offs = _pool([(c["input"], 3) for c in cases], 0xFF)
    d_pool = torch.from_numpy(pool).cuda()
    d_out = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda")
    dj = _djobs([c["input_len"] for c in cases], np.uint64(d_pool.data_ptr()) + offs)
    dj["out"] = [0 if c["null_out"] else d_out.data_ptr() + 64 for c in cases]
    dj["out_cap"] = 1024; dj["output_limit"] = 1 << 30
    dj["prefix"] = d_out.data_ptr(); dj["prefix_len"] = [c["prefix_len"] for c in cases]
    dj["out_existing_len"] = [c["out_existing_len"] for c in cases]
    d_jobs = device.to_device(dj, "cuda")
    msgs, exact = [], 0
    for min_in, shift in ((Lc.FED_MIN_IN, 2), (0, 32), (Lc.FED_MIN_IN, 0), (0, 31)):
        est, perm, _, _ = _run(FED, d_jobs, n, a=min_in, b=shift)
        for i, c in enumerate(cases):
            want, seqs = Lc.fed_est(c, min_in, shift)
            if int(est[i]) != want:
                msgs.append(f"[{c['name']}] min_in {min_in} len_shift {shift}: est {int(est[i])}, model {want}")
            if seqs is not None:
                exact += 1
                share = c["input_len"] >> shift if shift < 32 else 0
                if int(est[i]) - share != len(Lc._walk(c["input"])):
                    msgs.append(f"[{c['name']}] min_in {min_in} len_shift {shift}: est - share {int(est[i]) - share}, the block has {len(Lc._walk(c['input']))} sequences")
        fault = Lc.order_fault(est, perm)
        if fault:
            msgs.append(f"min_in {min_in} len_shift {shift}: {fault}")
    assert (d_out.cpu().numpy() == 0xEE).all(), "the front of a fed call wrote to an output"
    assert (d_pool.cpu().numpy() == pool).all(), "the inputs' pool was written"
    for text in msgs[:40]:
        print(text)
    assert not msgs, f"{len(msgs)} differences"
    print(f"launch order ok: {n} jobs x 4 settings of (min_in, len_shift): every estimate the model's, {exact} of them exact sequence counts, every order holds")


def _probe_data(name, n):
    if name == "zeros":
        return bytes(n)
    if name == "noise":
        return np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    start = {"mix": 30 << 20, "mix2": 101 << 20, "mix3": 12 << 20}[name]
    return synth.silesia_mix(start, start + n).tobytes()


def child_probes(piece, parts):
    import torch
    from rust_lz_fear_amd import device
    piece, parts = int(piece), int(parts)
    cases = Lc.probe_cases(piece, parts, _probe_data)
    n = len(cases)
    pool, offs = _pool([(c["data"], i % 16) for i, c in enumerate(cases)], 0xFF)
    d_pool = torch.from_numpy(pool).cuda()
    jobs = [dict(input=int(d_pool.data_ptr()) + int(a), input_len=len(c["data"]), cursor=c["cursor"]) for c, a in zip(cases, offs)]
    cj = _cjobs(jobs)
    cj["out"] = 0xDEAD0000; cj["out_cap"] = 5; cj["table"] = 0xBEEF0000; cj["flags"] = 1        # (what a probe must not inherit; nothing dereferences them)
    d_jobs = device.to_device(cj, "cuda")
    _, _, probes, pres = _run(PROBES, d_jobs, n, a=piece, b=parts, parts=parts)
    _, _, probes2, pres2 = _run(PROBES, d_jobs, n, a=piece, b=parts, parts=parts)
    want = Lc.probe_jobs(jobs, piece, parts)
    msgs, probed = [], 0
    for f in Lc.CJOB.names:
        for i in np.nonzero(probes[f] != want[f])[0].tolist():
            msgs.append(f"[{cases[i // parts]['name']}] piece {i % parts}: {f} = {int(probes[f][i]):#x}, model {int(want[f][i]):#x}")
    if probes.tobytes() != probes2.tobytes() or pres.tobytes() != pres2.tobytes():
        msgs.append("two runs give different probe jobs or probe results")
    for i in range(n * parts):
        if not want["input_len"][i]:
            continue
        c, j = cases[i // parts], jobs[i // parts]
        a = int(want["input"][i]) - j["input"]
        data = c["data"][a:a + piece]
        assert len(data) == piece and a >= j["cursor"]
        erc, eout, ev = o.compress2_trace(data)
        seqs = int((ev["type"] == o.EV_MATCH).sum())
        r = pres[i]
        print(f"{c['name']} piece {i % parts}: status {r['status']} out_len {r['out_len']} work {r['reserved']}; oracle {erc} {len(eout)}, {seqs} sequences")
        if int(r["status"]) != erc or int(r["out_len"]) != len(eout):
            msgs.append(f"[{c['name']}] piece {i % parts}: status {r['status']} out_len {r['out_len']}, oracle {erc} {len(eout)}")
        if not seqs <= int(r["reserved"]) <= seqs + piece:
            msgs.append(f"[{c['name']}] piece {i % parts}: work {r['reserved']} outside [{seqs}, {seqs + piece}]")
        probed += 1
    ce = Lc.cost_estimates(jobs, pres["reserved"], piece, parts)
    fault = Lc.order_fault(ce, _run(SORT_BY_COST, d_jobs, n, h_in=pres, a=piece, b=parts)[1])
    if fault:
        msgs.append(f"order by the device's own work values: {fault}")
    assert (d_pool.cpu().numpy() == pool).all(), "the inputs' pool was written"
    for text in msgs[:40]:
        print(text)
    assert not msgs, f"{len(msgs)} differences"
    print(f"launch order ok: piece {piece} x {parts}: {n} jobs, {n * parts} probe jobs the model's, {probed} probed pieces with the oracle's status, out_len and "
          f"work within the trace's bounds, estimates {[int(x) for x in ce]}")


def _decompress_items(blocks):
    """Decompress jobs for valid blocks and what the oracle decodes them to."""
    exp = []
    for c in blocks:
        rc, out = o.decompress_raw(c, limit=1 << 23, cap=(1 << 23) + 64)
        assert rc == 0
        exp.append(out)
    return [dict(input=c, limit=len(e), out_cap=len(e) + 64) for c, e in zip(blocks, exp)], exp


def child_e2e():
    piece, parts = (int(x) for x in os.environ["LZF_PROBE"].split(","))
    cases = Lc.probe_cases(piece, parts, _probe_data)
    items = [dict(input=c["data"], cursor=c["cursor"], out_cap=len(c["data"]) + len(c["data"]) // 200 + 64) for c in cases if c["cursor"] < len(c["data"])]
    res = ffi.compress_blocks_host(items)
    launch = ffi.lib().lzf_last_compress_launch().decode()
    assert launch.startswith("lzf_compress_compact_kernel"), launch
    blocks = []
    for it, (rc, out) in zip(items, res):
        erc, eout = o.compress2(it["input"], cursor=it["cursor"], cap=it["out_cap"])
        assert rc == erc and out == eout, (len(it["input"]), it["cursor"])
        if rc == 0 and it["cursor"] == 0:
            blocks.append((out, it["input"]))
    ditems, exp = _decompress_items([c["input"] for c in Lc.fed_cases()] + [c for c, _ in blocks])
    assert [e for e in exp[-len(blocks):]] == [d for _, d in blocks]
    dres = ffi.decompress_blocks_host(ditems)
    dlaunch = ffi.lib().lzf_last_decompress_launch().decode()
    assert dlaunch.startswith("lzf_decompress_paired_kernel"), dlaunch
    for it, e, (rc, out) in zip(ditems, exp, dres):
        assert rc == 0 and out == e, len(it["input"])
    print(f"launch order ok: {len(items)} compress jobs ordered by probes of {piece} x {parts} ({launch}), {len(ditems)} decompress jobs ordered by sampling ({dlaunch}): the oracle's results")


def child_e2e_fed():
    ditems, exp = _decompress_items([c["input"] for c in Lc.fed_cases()])
    dres = ffi.decompress_blocks_host(ditems)
    dlaunch = ffi.lib().lzf_last_decompress_launch().decode()
    assert dlaunch.startswith("bitmap-fed"), dlaunch
    for it, e, (rc, out) in zip(ditems, exp, dres):
        assert rc == 0 and out == e, len(it["input"])
    print(f"launch order ok: {len(ditems)} decompress jobs ordered by the parse's estimates ({dlaunch}): the oracle's results")


if __name__ == "__main__":
    {"sorts": child_sorts, "cost": child_cost, "fed": child_fed, "probes": child_probes, "e2e": child_e2e, "e2e_fed": child_e2e_fed}[sys.argv[1]](*sys.argv[2:])
