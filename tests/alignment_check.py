"""The buffer-alignment sweep under the analysis library's knobs, and the helpers tests/test_gpu_alignment.py shares with it.

Run as a script by tests/test_gpu_alignment.py (the knobs are read once per process):

    alignment_check.py variant    T + E + H (and S under seg) through whatever LZF_DECOMPRESS_KERNEL forces: paired48, paired24,
                                  staged16, seg (LZF_SEG_MIN_IN=0), fed (LZF_FED_MIN_IN=1), fed with LZF_FED_PIECES=3 — the edge code of
                                  every kernel with tiny and handcrafted inputs that the product dispatch routes elsewhere
    alignment_check.py force      S under LZF_SEG_FORCE = noscratch | stager | resolver
    alignment_check.py pieces     the F batch of more jobs than the device holds workgroups of the fed kernel, nothing forced; with
                                  LZF_FED_VERBOSE=1 the library reports on stderr how many that is

Everything goes through redzone.check_decompress with explicit placement: both input poisons, 4 KiB zones intact, statuses and bytes
equal to the oracle's."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import alignment_cases as ac  # noqa: E402
import redzone  # noqa: E402
import rust_lz_fear_amd  # noqa: E402,F401
from rust_lz_fear_amd import ffi  # noqa: E402


def _check_pointers(shape, placement, compress=False):
    """The addresses the harness really used have the low bits the shape asked for; returns the 16 x 16 histogram of
    (input & 15, out & 15) of one run."""
    assert len(placement) == 2
    for p in placement:
        assert ((p["input"] & np.uint64(255)) == np.array(shape.in_low, dtype=np.uint64)).all()
        assert ((p["out"] & np.uint64(255)) == np.array(shape.out_low, dtype=np.uint64)).all()
        if not compress:
            has = np.array([len(it.get("prefix", b"")) > 0 for it in shape.items])
            assert ((p["prefix"] & np.uint64(255)) == np.array(shape.prefix_low, dtype=np.uint64))[has].all()
    return ac.residues(placement[0]["input"], placement[0]["out"])


def run_decompress(shape, label, max_input_len=None, alias_inputs=False):
    """One call of lzf_decompress_batch per input poison over every job of `shape`; (histogram, launch string)."""
    placement = []
    redzone.check_decompress(shape.items, shape.expect, label, max_input_len=max_input_len, in_low=shape.in_low, prefix_low=shape.prefix_low,
                             out_low=shape.out_low, alias_inputs=alias_inputs, placement=placement)
    if alias_inputs:                                                     # one upload per (input object, residue), not one per job
        assert placement[0]["input_buffers"] == len({(id(it["input"]), lo) for it, lo in zip(shape.items, shape.in_low)}) < len(shape.items)
    return _check_pointers(shape, placement), ffi.lib().lzf_last_decompress_launch().decode()


def run_compress(shape, label):
    placement = []
    redzone.check_compress(shape.items, shape.expect, label, in_low=shape.in_low, out_low=shape.out_low, placement=placement)
    return _check_pointers(shape, placement, compress=True), ffi.lib().lzf_last_compress_launch().decode()


def max_in(shape):
    return max(len(it["input"]) for it in shape.items)


def report(label, hist, calls):
    """One line per class for the log: how many jobs ran at each rb, and how evenly the (input & 15, out & 15) pairs were hit."""
    print(f"[alignment] {label}: {int(hist.sum())} jobs in {calls} calls; jobs per rb 0..15 {hist.sum(axis=0).tolist()}; "
          f"jobs per (input & 15, out & 15) pair min {int(hist.min())} max {int(hist.max())}", flush=True)


def sweep(shape, label, lo, hi, expect_launch, **kw):
    """Every job of `shape` in calls of lo < n <= hi jobs; each call's launch string must pass `expect_launch`.  Returns the
    histogram over all calls."""
    hist = np.zeros((16, 16), dtype=np.int64)
    parts = ac.chunks(shape, lo, hi)
    for k, part in enumerate(parts):
        h, launch = run_decompress(part, f"{label}, call {k} of {len(parts)} ({len(part.items)} jobs)", **kw)
        assert expect_launch(launch), (label, len(part.items), launch)
        hist += h
    assert hist.sum() >= len(shape.items)
    report(label, hist, len(parts))
    return hist


def _variant():
    which = os.environ["LZF_DECOMPRESS_KERNEL"]
    shape = ac.concat(ac.tiny(), ac.existing_prefix(), ac.handcrafted())
    if which == "seg":
        shape = ac.concat(shape, ac.segmented())
        want, hi = (lambda s: s.startswith("segmented")), 1024
    elif which == "fed":
        want, hi = (lambda s: s.startswith("bitmap-fed")), 4096
    else:
        assert which in ("paired48", "paired24", "staged16"), which
        want, hi = (lambda s: s == "analysis variant (LZF_DECOMPRESS_KERNEL)"), 4096
    hist = sweep(shape, "forced " + which + (" in %s pieces" % os.environ["LZF_FED_PIECES"] if "LZF_FED_PIECES" in os.environ else ""), 0, hi, want,
                 max_input_len=max_in(shape))
    assert (hist > 0).all()
    print("alignment variant ok:", which)


def _force():
    force = os.environ["LZF_SEG_FORCE"]
    shape = ac.segmented()
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = len(shape.items)
    assert n <= 1024
    # without scratch memory the pair kernel takes the whole call: its 48-byte form up to eight blocks per compute unit
    pair = "lzf_decompress_paired_kernel<4096,48,640>" if n <= 8 * cus else "lzf_decompress_paired_kernel<4096,24,384>"
    hist = sweep(shape, "LZF_SEG_FORCE=" + force, 0, 1024, (lambda s: s == pair) if force == "noscratch" else (lambda s: s.startswith("segmented")),
                 max_input_len=max_in(shape))
    assert (hist > 0).all()
    print("alignment force ok:", force)


def pieces_jobs(cus):
    return 24 * cus + 16


def _pieces():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shape = ac.fed(pieces_jobs(cus))
    hist, launch = run_decompress(shape, "bitmap-fed, more jobs than resident workgroups (analysis library)", max_input_len=max_in(shape), alias_inputs=True)
    assert launch.startswith("bitmap-fed"), launch
    assert (hist > 0).all()
    report("bitmap-fed in 16 pieces (analysis library)", hist, 1)
    print("alignment pieces ok:", len(shape.items), "jobs")


if __name__ == "__main__":
    {"variant": _variant, "force": _force, "pieces": _pieces}[sys.argv[1]]()
