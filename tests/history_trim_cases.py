"""The history trim (rust-lz-fear_amd/csrc/lzf_history_trim.h) restated in Python, and blocks built against a given history, for
tests/test_history_trim_cpu.py and tests/test_gpu_long_history.py.

The threshold is a parameter here (and only here): with a small one the property "trimmed job + restore == original job" is checked
against the oracle on histories of a few hundred KiB instead of gigabytes.  The header's own threshold is THRESHOLD."""
import struct

THRESHOLD = 1 << 30
KEEP = 65536
M64 = (1 << 64) - 1


def shift_of(existing, out_cap=M64, threshold=THRESHOLD):
    if existing < threshold or existing > out_cap:
        return 0
    return (existing - KEEP) & ~15


def trim(job, threshold=THRESHOLD):
    """job: dict(out, out_existing_len, out_cap, output_limit, ...).  Returns (trimmed job, shift); other keys are carried over."""
    s = shift_of(job["out_existing_len"], job["out_cap"], threshold)
    t = dict(job)
    if s:
        t["out"] = job["out"] + s if job["out"] else job["out"]
        t["out_existing_len"] = job["out_existing_len"] - s
        t["out_cap"] = job["out_cap"] - s
        t["output_limit"] = job["output_limit"] - s if job["output_limit"] > s else 0
    return t, s


def restore(status, out_len, shift):
    return (status, out_len + shift if status == 0 else out_len)


# ---- LZ4 sequences by hand ------------------------------------------------------------------------------------------------------
def _lsic(n):
    return b"\xff" * (n // 255) + bytes([n % 255])


def seq(literals=b"", offset=None, match=0):
    """One sequence: the literals, then (offset given) a match of `match` >= 4 bytes."""
    L, M = len(literals), (match - 4 if offset is not None else 0)
    tok = (min(L, 15) << 4) | min(M, 15)
    out = bytes([tok])
    if L >= 15:
        out += _lsic(L - 15)
    out += bytes(literals)
    if offset is not None:
        out += struct.pack("<H", offset)
        if M >= 15:
            out += _lsic(M - 15)
    return out
