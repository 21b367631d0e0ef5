"""The copy stage of the batched decompress kernels (lz4_decompress_batch_phase.inc) class by class on the built edges of copy_stage_cases.py,
whose reach test_copy_stage_cases_cpu.py proves without a GPU.  Every forced kernel (analysis library: paired48, paired24, staged16, the fed kernel
whole and in three pieces) decodes the blocks built for its geometry, each block at the output residue (out & 15 = 0, 1, 15) it was built for,
prefix and existing output included; the product library decodes the blocks of every geometry by its own dispatch, one call per geometry.  Statuses, out_len and bytes — the
existing output too — are the oracle's and the poison around every output slot is untouched.  The same jobs go through the red-zone harness with
inputs and prefixes at residues 0, 1, 15.  Two instrumented builds report the pair kernel's rounds and batches and the fed kernel's batches per
job in results[].reserved: they equal the model's, job by job — for the fed kernel that is also the proof that it finished every valid job itself:
a job it gives up is decoded by the pair kernel <4096,24,384>, which reports its rounds there, and the CPU test holds every valid block of the fed
geometry to a round count in that kernel that differs from its batch count in the fed kernel."""
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
import oracle_ffi as o  # noqa: E402
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import ffi  # noqa: E402
import copy_stage_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xEE, 64
FORCED = {"paired48": dict(LZF_DECOMPRESS_KERNEL="paired48"), "paired24": dict(LZF_DECOMPRESS_KERNEL="paired24"),
          "staged16": dict(LZF_DECOMPRESS_KERNEL="staged16"),
          "fed": dict(LZF_DECOMPRESS_KERNEL="fed", LZF_FED_MIN_IN="1", LZF_FED_PIECES="1"),
          "fed3": dict(LZF_DECOMPRESS_KERNEL="fed", LZF_FED_MIN_IN="1", LZF_FED_PIECES="3")}
LAUNCH = {"paired48": "analysis variant", "paired24": "analysis variant", "staged16": "analysis variant", "fed": "bitmap-fed", "fed3": "bitmap-fed",
          "product": "lzf_decompress_paired_kernel<4096,48,640>"}
from rust_lz_fear_amd.build import COUNTER_BUILDS  # noqa: E402
ROUNDS_BUILD, BATCHES_BUILD = COUNTER_BUILDS      # the pair kernel's rounds with the fed kernel's batches; the pair kernel's batches


def build_corpus():
    """Per geometry the jobs (every case at every residue), what the oracle makes of them and the model's counts."""
    data = {}
    for g in K.GEOMS:
        jobs = []
        for rb in K.RESIDUES:
            cases, models, got = K.reach(g, rb)
            assert got >= K.edges(K.GEOMS[g])
            for c, m in zip(cases, models):
                e = o.decompress_raw(c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"], cap=c["cap"])
                assert e[0] == c["status"] == m.status and (e[0] != K.OK or e[1] == c["output"]), c["name"]
                jobs.append(dict(c, rb=rb, exp=e, nbatch=m.nbatch, rounds=m.rounds))
        assert len(jobs) <= K.JOBS_MAX
        data[g] = jobs
    return data


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """... once for the module (the children read the file)."""
    data = build_corpus()
    path = tmp_path_factory.mktemp("copy_stage") / "corpus.pkl"
    path.write_bytes(pickle.dumps(data))
    return str(path)


def _child(what, corpus, kernel, lib=None, count=""):
    from rust_lz_fear_amd import build
    env = dict(os.environ, COPY_STAGE_CORPUS=corpus, COPY_STAGE_COUNT=count)
    for k in ("LZF_DECOMPRESS_KERNEL", "LZF_FED_MIN_IN", "LZF_FED_PIECES", "LZF_FED_CARRY", "LZF_LIB_PATH"):
        env.pop(k, None)
    if kernel != "product":
        env.update(FORCED[kernel], LZF_LIB_PATH=lib or build.build_analysis_library())
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what, kernel], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "copy stage ok" in r.stdout, r.stdout[-2000:]
    print(r.stdout.strip().splitlines()[-1], f"[{time.time() - t0:.1f} s]")


@pytest.mark.parametrize("kernel", list(FORCED) + ["product"])
def test_bytes_statuses_and_existing_output(corpus, kernel):
    _child("bytes", corpus, kernel)


@pytest.mark.parametrize("kernel", ["paired48", "paired24", "staged16", "fed"])
def test_red_zones(corpus, kernel):
    _child("redzone", corpus, kernel)


@pytest.mark.parametrize("kernel,count", [("paired48", "rounds"), ("paired24", "rounds"), ("fed", "nbatch")])
def test_rounds_and_fed_batches_equal_the_model(corpus, kernel, count):
    from rust_lz_fear_amd import build
    _child("bytes", corpus, kernel, lib=build.build_library(defines=ROUNDS_BUILD), count=count)


@pytest.mark.parametrize("kernel", ["paired48", "paired24"])
def test_pair_kernel_batches_equal_the_model(corpus, kernel):
    from rust_lz_fear_amd import build
    _child("bytes", corpus, kernel, lib=build.build_library(defines=BATCHES_BUILD), count="nbatch")


# ---------------------------------------------------------------------------------------------------------------- the children
def _load(kernel):
    """The jobs built for the kernel's geometry; for the product library the jobs of every geometry, one call each."""
    with open(os.environ["COPY_STAGE_CORPUS"], "rb") as f:
        data = pickle.load(f)
    return [data[g] for g in K.GEOMS] if kernel == "product" else [data[kernel.rstrip("3")]]


def run_placed(jobs):
    """Every job through lzf_decompress_batch with its output at address residue job["rb"], poison around the slot.  Returns (results, host copy
    of the output arena, offsets of the outputs)."""
    import torch
    from rust_lz_fear_amd import device
    n = len(jobs)
    in_off, pre_off, out_off = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    ti, to = 0, 256
    for i, j in enumerate(jobs):
        in_off[i] = ti; ti += (len(j["input"]) + 255) // 256 * 256 + 3                      # odd input alignments
        pre_off[i] = ti; ti += (len(j["prefix"]) + 255) // 256 * 256 + 5
        out_off[i] = to + j["rb"]; to += (j["cap"] + 2 * GUARD + 16 + 255) // 256 * 256
    h_in = np.zeros(ti + 64, np.uint8)
    h_out = np.full(to + 256, POISON, np.uint8)
    for a, p, q, j in zip(in_off, pre_off, out_off, jobs):
        h_in[a:a + len(j["input"])] = np.frombuffer(j["input"], np.uint8)
        h_in[p:p + len(j["prefix"])] = np.frombuffer(j["prefix"], np.uint8)
        h_out[q:q + len(j["existing"])] = np.frombuffer(j["existing"], np.uint8)
    d_in, d_out = torch.from_numpy(h_in).cuda(), torch.from_numpy(h_out).cuda()
    assert d_out.data_ptr() % 256 == 0
    dj = np.zeros(n, dtype=device.DJOB)
    dj["input"] = np.uint64(d_in.data_ptr()) + in_off.astype(np.uint64)
    dj["input_len"] = [len(j["input"]) for j in jobs]
    dj["prefix"] = np.uint64(d_in.data_ptr()) + pre_off.astype(np.uint64)
    dj["prefix_len"] = [len(j["prefix"]) for j in jobs]
    dj["out"] = np.uint64(d_out.data_ptr()) + out_off.astype(np.uint64)
    dj["out_existing_len"] = [len(j["existing"]) for j in jobs]
    dj["out_cap"] = [j["cap"] for j in jobs]
    dj["output_limit"] = [j["limit"] for j in jobs]
    assert ((dj["out"] & 15) == [j["rb"] for j in jobs]).all()
    d_res = torch.zeros(n * device.RES.itemsize, dtype=torch.uint8, device="cuda")
    device.decompress_batch(device.to_device(dj, "cuda"), d_res, n, max_input_len=max(len(j["input"]) for j in jobs))
    torch.cuda.synchronize()
    return device.results_to_host(d_res, n).copy(), d_out.cpu().numpy(), out_off


def child_bytes(kernel):
    count = os.environ.get("COPY_STAGE_COUNT", "")
    msgs, counted, calls = [], 0, _load(kernel)
    for jobs in calls:
        counted += _check_call(kernel, jobs, count, msgs)
    for text in msgs[:40]:
        print(text)
    assert not msgs, f"{len(msgs)} differences"
    assert not count or counted >= 60
    jobs = sum(calls, [])
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    print(f"copy stage ok: {kernel}: {len(jobs)} jobs in {len(calls)} call(s), {sum(j['exp'][0] != 0 for j in jobs)} with an error, {counted} counts ({count or 'none'}) equal, {launch}")


def _check_call(kernel, jobs, count, msgs):
    """One call; the differences go to msgs.  Returns the number of counters compared."""
    res, out, out_off = run_placed(jobs)
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    assert launch.startswith(LAUNCH[kernel]), launch
    counted = 0
    for j, r, q in zip(jobs, res, out_off.tolist()):
        say = lambda text: msgs.append(f"[{j['name']}] rb {j['rb']}: {text}")      # noqa: E731
        erc, eout = j["exp"]
        if int(r["status"]) != erc:
            say(f"status {r['status']}, oracle {erc}"); continue
        end = q + j["cap"]
        if erc == K.OK:
            if int(r["out_len"]) != len(eout):
                say(f"out_len {r['out_len']}, oracle {len(eout)}"); continue
            got = out[q:q + len(eout)]
            if got.tobytes() != eout:
                w = np.nonzero(got != np.frombuffer(eout, np.uint8))[0]
                say(f"output differs at {len(w)} bytes, first {int(w[0])}, last {int(w[-1])} (existing_len {len(j['existing'])})")
            end = q + len(eout)
            if count:
                counted += 1
                print(f"{j['name']} rb {j['rb']}: reserved {int(r['reserved'])}, model {count} {j[count]}")
                if int(r["reserved"]) != j[count]:
                    say(f"reserved {int(r['reserved'])}, the model's {count} {j[count]}")
        elif out[q:q + len(j["existing"])].tobytes() != j["existing"]:
            say("the existing output of a failed job was changed")
        if (out[q - GUARD:q] != POISON).any():
            say("bytes in front of the output were written")
        if (out[end:end + GUARD] != POISON).any():
            say("bytes behind the output were written")
    return counted


def child_redzone(kernel):
    import redzone
    jobs, = _load(kernel)
    items = [dict(input=j["input"], prefix=j["prefix"], existing=j["existing"], limit=j["limit"], out_cap=j["cap"]) for j in jobs]
    n = len(jobs)
    redzone.check_decompress(items, [j["exp"] for j in jobs], label=f"copy stage, {kernel}", max_input_len=max(len(j["input"]) for j in jobs),
                             in_low=[(0, 1, 15)[k % 3] for k in range(n)], prefix_low=[(0, 1, 15)[(k // 3) % 3] for k in range(n)],
                             out_low=[j["rb"] for j in jobs])
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    assert launch.startswith(LAUNCH[kernel]), launch
    print(f"copy stage ok: red zones, {kernel}: {n} jobs, {launch}")


if __name__ == "__main__":
    {"bytes": child_bytes, "redzone": child_redzone}[sys.argv[1]](sys.argv[2])
