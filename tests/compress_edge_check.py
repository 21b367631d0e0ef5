"""The corpus of tests/compress_edge_cases.py (inputs the oracle's trace proves to reach every candidate rule of compress2) through
whatever compress kernel LZF_COMPRESS_KERNEL / LZF_COMPRESS_ORDER select in the analysis library ("general": lzf_compress_wave_kernel,
"compact": lzf_compress_compact_kernel, default for calls of no more jobs than compute units: lzf_compress_team_kernel).  Run as a
script by tests/test_gpu_compress_edges.py (the choice is read once per process, hence the subprocess); that test also imports
`fresh_calls`, `chain_calls` and `compare` for the product library.

Fresh-table jobs: status and bytes == the oracle's at cap = the worst-case bound and cap = N, the LSIC class also at cap = C and C - 1.
Carried tables (stale slot, first position): call by call, and the table's bytes after every call == the oracle's."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import compress_edge_cases as ec  # noqa: E402
import oracle_ffi as o  # noqa: E402
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import ffi  # noqa: E402

U16_LAUNCH = "lzf_compress_wave_kernel<U16>"


def launch():
    return ffi.lib().lzf_last_compress_launch().decode()


def with_caps(jobs, mode, plain):
    """The jobs with out_cap per `mode`: "bound" (worst case), "N" (framed/compress.rs:242), "C" and "C-1" (the oracle's size)."""
    cap = {"bound": lambda j, p: ec.bound(len(j["input"])), "N": lambda j, p: len(j["input"]) - j["cursor"],
           "C": lambda j, p: len(p["out"]), "C-1": lambda j, p: max(len(p["out"]) - 1, 0)}[mode]
    return [dict(j, cap=cap(j, p)) for j, p in zip(jobs, plain)]


def compare(jobs, got, want, what, bad):
    for j, (rc, out), w in zip(jobs, got, want):
        if rc != w["rc"] or (rc == 0 and out != w["out"]):
            bad.append(f"{what}: {j['cls']} / {j['name']} (cursor {j['cursor']}, cap {j['cap']}, kind {j['kind']}): status {rc} / oracle {w['rc']}, "
                       f"{len(out)} / {len(w['out'])} bytes")


def fresh_calls(jobs, per_call, want_launch, what, bad, modes=("bound", "N")):
    """Fresh-table jobs of one table kind in calls of at most per_call jobs, once per cap mode."""
    plain = ec.run_oracle(jobs, trace=False)
    for mode in modes:
        capped = with_caps(jobs, mode, plain)
        want = plain if mode == "bound" else ec.run_oracle(capped, trace=False)
        for a in range(0, len(capped), per_call):
            part = capped[a:a + per_call]
            got = ffi.compress_blocks_host([dict(input=j["input"], cursor=j["cursor"], kind=j["kind"], out_cap=j["cap"]) for j in part])
            assert want_launch(launch()), (what, mode, launch())
            compare(part, got, want[a:a + per_call], f"{what}, cap = {mode}", bad)


def chain_calls(jobs, what, bad, want_launch=None):
    """The chains' calls in order — call k of every chain in one batch — on caller-owned U32 tables; the table after every call."""
    want = ec.run_oracle(jobs, trace=False)
    tables = {}
    for k in sorted({j["par"]["call"] for j in jobs}):
        part = [(j, w) for j, w in zip(jobs, want) if j["par"]["call"] == k]
        items = []
        for j, _ in part:
            t = tables.setdefault(j["chain"], ffi.U32Table())
            t.offset += j["offset_add"]
            items.append(dict(input=j["input"], cursor=j["cursor"], table=t, out_cap=ec.bound(len(j["input"]))))
        got = ffi.compress_blocks_host(items)
        assert want_launch is None or want_launch(launch()), (what, launch())
        compare([dict(j, cap=None) for j, _ in part], got, [w for _, w in part], f"{what}, call {k}", bad)
        for j, w in part:
            if bytes(tables[j["chain"]]) != w["table"]:
                bad.append(f"{what}: {j['name']}: the table after call {k} differs from the oracle's")


def split(jobs):
    return ([j for j in jobs if j["chain"] is None and j["kind"] == o.TABLE_U32], [j for j in jobs if j["chain"] is None and j["kind"] == o.TABLE_U16],
            [j for j in jobs if j["chain"] is not None])


def main():
    import torch
    per_call = min(torch.cuda.get_device_properties(0).multi_processor_count, 128)
    name = {"general": "lzf_compress_wave_kernel", "compact": "lzf_compress_compact_kernel"}.get(os.environ.get("LZF_COMPRESS_KERNEL", ""), "lzf_compress_team_kernel")
    u32, u16, chains = split(ec.corpus())
    bad = []
    fresh_calls(u32, per_call, lambda s: s.startswith(name), name, bad)
    fresh_calls(ec.of_class(u32, "lsic"), per_call, lambda s: s.startswith(name), name, bad, modes=("C", "C-1"))
    fresh_calls(u16, per_call, lambda s: s == U16_LAUNCH, U16_LAUNCH, bad)
    fresh_calls(ec.of_class(u16, "u16")[-1:] + [j for j in u16 if j["par"].get("of") == "lsic"], per_call, lambda s: s == U16_LAUNCH, U16_LAUNCH, bad, modes=("C", "C-1"))
    chain_calls(chains, name + ", carried tables", bad, lambda s: s.startswith(name))
    for line in bad[:40]:
        print(line)
    assert not bad, f"{len(bad)} differences from the oracle"
    print(f"edges ok: {len(u32)} U32 + {len(u16)} U16 fresh-table jobs, {len(chains)} calls on carried tables")


if __name__ == "__main__":
    main()
