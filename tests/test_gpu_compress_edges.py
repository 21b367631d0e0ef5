"""Every compress kernel on the inputs of tests/compress_edge_cases.py: built for the candidate rules of raw::compress2 (distance
exactly 65535 / 65536 at every epoch phase, position 0 from an empty or a stale slot, the first position, the three ends of a
backtrack, the skip schedule, LSIC boundaries, the ends of a block, the U16 table), each proven to reach its rule in the reference by
the census of tests/test_compress_edge_cases_cpu.py.  A kernel that differs from the oracle here differs at the rule the job's class
names.  The analysis library's kernels run tests/compress_edge_check.py in a subprocess each; the product library, the red-zone
harness and the decode round trip run here."""
import os
import subprocess
import sys
import time

import pytest

import alignment_cases
import compress_edge_cases as ec
import compress_edge_check as chk
import oracle_ffi as o
import redzone
from rust_lz_fear_amd import build, ffi

pytestmark = pytest.mark.gpu

S_TEAM_ALL = "lzf_compress_team_kernel + lzf_compress_team_carry_kernel + lzf_compress_wave_kernel"


def _per_call():
    import torch
    return min(torch.cuda.get_device_properties(0).multi_processor_count, 128)


@pytest.mark.parametrize("kernel", ["team", "compact", "general", "ordered"])
def test_every_compress_kernel_on_the_edge_corpus(kernel):
    env = dict(os.environ, LZF_LIB_PATH=build.build_analysis_library())
    env.update({"LZF_COMPRESS_ORDER": "always"} if kernel == "ordered" else {"LZF_COMPRESS_KERNEL": kernel})
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "compress_edge_check.py")], env=env, capture_output=True, text=True, timeout=300)
    print(f"{kernel}: {time.time() - t0:.1f} s")
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-4000:]
    assert "edges ok" in r.stdout


def test_product_dispatch_on_the_edge_corpus():
    """No knobs: every fresh-table job in one call (more jobs than compute units: the compact kernel, U16 jobs to the general one), the
    U32 jobs again in calls of no more jobs than compute units (the team kernel), the carried tables as linked calls."""
    u32, u16, chains = chk.split(ec.corpus())
    bad = []
    assert len(u32) + len(u16) > 4 * _per_call()
    chk.fresh_calls(u32 + u16, len(u32) + len(u16), lambda s: s.startswith("lzf_compress_compact_kernel"), "product, one call", bad)
    chk.fresh_calls(u32, _per_call(), lambda s: s.startswith("lzf_compress_team_kernel"), "product, team-sized calls", bad, modes=("bound",))
    chk.chain_calls(chains, "product, linked calls", bad, lambda s: s == S_TEAM_ALL)
    assert not bad, (len(bad), bad[:20])


def test_red_zones_under_both_poisons():
    """Position 0 as a source, the first position, the backtrack that ends at the first byte of the input (the byte in front of it is
    poison here: 0x00 in one run, 0xFF in the other; the over-read inputs plant both in front of the copy), the ends of a block and the
    small LSIC jobs: nothing written outside [out, out + cap), results independent of the bytes around the input, equal to the oracle."""
    jobs = [j for j in ec.corpus() if j["chain"] is None and j["cls"] in ("empty slot", "first position", "backtrack", "block end", "lsic")]
    assert {j["cls"] for j in jobs} == {"empty slot", "first position", "backtrack", "block end", "lsic"}
    want = [(w["rc"], w["out"]) for w in ec.run_oracle(jobs, trace=False)]
    items = [dict(input=j["input"], cursor=j["cursor"], kind=j["kind"], out_cap=ec.bound(len(j["input"]))) for j in jobs]
    redzone.check_compress(items, expect=want, label="edge corpus, one call")
    assert chk.launch().startswith("lzf_compress_compact_kernel")
    n = _per_call()
    # ... and every U32 job again, the block ends of every n among them, in calls the team kernel takes
    small = [i for i, j in enumerate(jobs) if j["kind"] == o.TABLE_U32]
    assert sum(jobs[i]["cls"] == "block end" for i in small) >= 4 * 68
    for a in range(0, len(small), n):
        idx = small[a:a + n]
        redzone.check_compress([items[i] for i in idx], expect=[want[i] for i in idx], label=f"edge corpus, jobs {a}..")
        assert chk.launch().startswith("lzf_compress_team_kernel")


def test_oracle_blocks_with_offsets_at_the_limit_decode():
    """The oracle's blocks of the distance, empty-slot and LSIC classes (offsets 65534 / 65535 at every epoch phase, offset == position,
    length tails at every boundary) through the decompress dispatch: the inputs again."""
    jobs = [j for j in ec.corpus() if j["chain"] is None and j["kind"] == o.TABLE_U32 and j["cls"] in ("distance", "empty slot", "lsic")]
    comp = ec.run_oracle(jobs, trace=False)
    items = [dict(input=c["out"], prefix=j["input"][:j["cursor"]], limit=len(j["input"]) - j["cursor"], out_cap=len(j["input"]) - j["cursor"])
             for j, c in zip(jobs, comp)]
    assert sum(alignment_cases.max_offset(c["out"]) == 65535 for c in comp) >= 57
    for j, (rc, out) in zip(jobs, ffi.decompress_blocks_host(items)):
        assert rc == 0 and out == j["input"][j["cursor"]:], (j["cls"], j["name"], rc)

