"""Block-level cases of the decoded-size tests (test_decoded_size_cpu.py, test_gpu_decoded_size.py): inputs from tests/golden,
vectors.py and synth, expectations from the oracle's decompress_raw.  A case is dict(input, prefix_len, existing_len, limit);
its expectation (status, output.len() or None).  `prefix` / `existing` carry the bytes for callers that also decode."""
import json
import os

import numpy as np

import oracle_ffi as o
import vectors
from rust_lz_fear_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def mutate(rng, comp):
    """The mutation recipe of test_gpu_parity.test_decompress_malformed_inputs_same_error_kind, restated."""
    b = bytearray(comp)
    kind = rng.integers(0, 5)
    if kind == 0 and len(b) > 1:           # truncate
        del b[rng.integers(1, len(b)):]
    elif kind == 1 and len(b) > 0:         # flip a bit
        i = rng.integers(0, len(b)); b[i] ^= 1 << rng.integers(0, 8)
    elif kind == 2 and len(b) > 0:         # set a byte to 0 / 0xFF (zero offsets, LSIC runs)
        i = rng.integers(0, len(b)); b[i] = 0 if rng.integers(0, 2) else 0xFF
    elif kind == 3:                        # append garbage
        b += bytes(rng.integers(0, 256, rng.integers(1, 9), dtype=np.uint8))
    else:                                  # several bytes replaced
        for _ in range(4):
            if len(b):
                i = rng.integers(0, len(b)); b[i] = rng.integers(0, 256)
    return bytes(b)


def expect(case):
    """The oracle's status and, when Ok, output.len() (existing output included)."""
    prefix, existing = case.get("prefix", b""), case.get("existing", b"")
    cap = len(existing) + case["limit"] + len(case["input"]) + 64
    rc, out = o.decompress_raw(case["input"], prefix=prefix, existing=existing, limit=case["limit"], cap=cap)
    assert rc != o.OUT_CAPACITY
    return rc, (len(out) if rc == 0 else None)


def make_case(data, limit, prefix=b"", existing=b""):
    return dict(input=bytes(data), prefix_len=len(prefix), existing_len=len(existing), limit=limit, prefix=prefix, existing=existing)


def _case(data, limit, prefix=b"", existing=b""):
    c = make_case(data, limit, prefix, existing)
    return c, expect(c)


def block_cases():
    """[(name, case, (status, length))]: hc fixtures, valid blocks, mutated blocks (all five kinds), prefix / existing sweep."""
    out = []
    J = json.load(open(os.path.join(GOLD, "hc_blocks.json")))
    blob = open(os.path.join(GOLD, "hc_blocks.bin"), "rb").read()
    for k, b in enumerate(J["blocks"]):
        comp = blob[b["offset"]: b["offset"] + b["length"]]
        n = b["in"][0]
        for tag, data, limit in (("full", comp, n), ("limit-1", comp, n - 1), ("half", comp[: len(comp) // 2], n)):
            out.append((f"hc{k}/{tag}",) + _case(data, limit))
    valid = vectors.small_cases() + vectors.medium_cases()
    for name, d in valid:
        rc, comp = o.compress2(d)
        assert rc == 0
        out.append((f"valid/{name}",) + _case(comp, max(len(d), 1)))
    rng = np.random.default_rng(12345)
    base = [(n, d) for n, d in valid + [(f"librs{i}", s) for i, s in enumerate(vectors.LIB_RS_STRINGS)] if 0 < len(d) <= 300000]
    for name, d in base:
        comp = o.compress2(d)[1]
        for k in range(6):
            m = mutate(rng, comp)
            out.append((f"mutated/{name}/{k}",) + _case(m, len(d) if k % 2 == 0 else len(d) // 2 + 1))
    d = synth.gen_text_zipf(31, 50000).tobytes()
    dic, payload = d[:20000], d[20000:]
    rc, comp = o.compress2(dic + payload, cursor=len(dic))
    assert rc == 0
    out.append(("dict/prefix",) + _case(comp, len(payload), prefix=dic))
    out.append(("dict/existing",) + _case(comp, len(d), existing=dic))
    out.append(("dict/truncated",) + _case(comp, len(payload), prefix=dic[:100]))
    out.append(("dict/split",) + _case(comp, len(d), prefix=dic[:10000], existing=dic[10000:]))
    return out


def assert_all_kinds(cases):
    """The condition both tests state on the ORACLE's results before anything is compared."""
    kinds = {exp[0] for _, _, exp in cases}
    assert {0, 1, 2, 3, 4} <= kinds, kinds
