"""Red-zone harness for the GPU codec (test infrastructure, -m gpu).

The reference is `#![forbid(unsafe_code)]` (src/lib.rs:1) and its fuzz target's only property is "no crash, no out-of-bounds on
arbitrary bytes" (fuzz/fuzz_targets/decode.rs), with the documented overshoot bound output_limit + input.len()
(src/raw/decompress.rs:55-57).  A GPU kernel has no such language guarantee, so it is checked from outside: every job's
buffers are carved out of larger device allocations

    input arena :  ... [input bytes][ >= 4 KiB of IN-poison ] ...          the bytes behind input_len are poison A in one run, B in another
    output arena:  ... [4 KiB OUT-poison][existing | out_cap bytes][4 KiB OUT-poison] ...

through the device-pointer entry points of the C ABI (lzf_decompress_batch / lzf_compress_batch).  After the call every
OUT-poison zone must be untouched — a write in front of `out` or behind `out + out_cap` is a failure even when it lands in slack
the plain tests never look at — and statuses and Ok bytes must be identical under both IN-poisons: a result that depends on bytes
behind `input_len` is an over-read that matters.

The layout is seeded and random by default; in_low / prefix_low / out_low place every buffer at given low address bits instead
(tests/test_gpu_alignment.py: every kernel at every residue of `out & 15`), and `placement` hands back the device addresses used.
"""
import numpy as np
import torch

import rust_lz_fear_amd  # noqa: F401
from rust_lz_fear_amd import device, ffi

ZONE = 4096
OUT_POISON = 0xA5


def _layout(sizes, zone, rng, align_choices=(1, 2, 4, 8, 16, 64), low=None, base_low=0):
    """Offsets of buffers of `sizes` bytes, each behind `zone` bytes of poison and at a start address with varying low bits.

    Without `low` the start offsets are 64 * k + a * {0, 1, 2} with a drawn from {1, 2, 4, 8, 16} (64: no addend), one rng draw pair
    per buffer: the low six bits are one of {0, 1, 2, 4, 8, 16, 32}, so an arena on a 64-byte boundary gives `address & 15` in
    {0, 1, 2, 4, 8} only — residues 3, 5, 6, 7 and 9..15 are never reached by the random default.  `low` (one entry per buffer, an
    int in 0..255 or None for the random default) fixes `(base_low + offset) & 255` of that buffer instead and draws nothing from
    the rng for it; `base_low` is the arena base's own low eight bits (0 for a 256-aligned arena)."""
    offs, pos = [], 0
    for i, sz in enumerate(sizes):
        pos += zone
        lo = None if low is None else low[i]
        if lo is None:
            a = int(rng.choice(align_choices))
            pos = (pos + 63) // 64 * 64 + (a if a < 64 else 0) * int(rng.integers(0, 3))
        else:
            assert 0 <= int(lo) <= 255, lo
            pos = (pos + base_low + 255) // 256 * 256 - base_low + int(lo)
        offs.append(pos)
        pos += sz
    return offs, pos + zone


def _lows(low, n, what):
    """An explicit placement argument as a list of n entries (None: the random default for every buffer)."""
    if low is None:
        return [None] * n
    low = [None if v is None else int(v) for v in low]
    assert len(low) == n, f"{what}: {len(low)} entries for {n} jobs"
    return low


def _alias_slots(items, in_low, alias_inputs):
    """Which input buffer each job reads: one per job, or (alias_inputs) one per distinct (input object of the item, residue)."""
    if not alias_inputs:
        return list(range(len(items))), list(range(len(items)))
    slot_of, first = {}, []
    which = []
    for i, it in enumerate(items):
        k = (id(it["input"]), in_low[i])
        if k not in slot_of:
            slot_of[k] = len(first); first.append(i)
        which.append(slot_of[k])
    return which, first


def _place(sizes, lows, rng, dev, explicit):
    """Layout + arena: (offsets, total, arena tensor).  The arena base must be 256-aligned for explicit residues to be what was
    asked for; where it is not, its low bits are folded into the layout."""
    if not explicit:
        offs, total = _layout(sizes, ZONE, rng)
        return offs, total, None
    offs, total = _layout(sizes, ZONE, rng, low=lows)
    arena = torch.empty(total + 256, dtype=torch.uint8, device=dev)         # (256 spare bytes: the layout for a base that is not 256-aligned still fits)
    base_low = int(arena.data_ptr()) & 255
    if base_low:
        offs, t2 = _layout(sizes, ZONE, rng, low=lows, base_low=base_low)
        assert t2 <= total + 256
        total = t2
    for o, lo in zip(offs, lows):
        assert lo is None or (int(arena.data_ptr()) + o) & 255 == lo
    return offs, total, arena[:total]


def _upload(h, arena, dev):
    if arena is None:
        return torch.from_numpy(h).to(dev)
    arena.copy_(torch.from_numpy(h))
    return arena


def decompress_guarded(items, in_poison, seed=0, max_input_len=None, in_low=None, prefix_low=None, out_low=None, alias_inputs=False,
                       placement=None):
    """items as ffi.decompress_blocks_host.  Returns (results [(status, bytes incl. existing)], zones_ok, detail).

    in_low / prefix_low / out_low: the low eight address bits of every job's input, prefix and out (sequences of ints in 0..255, one
    per job); absent, the layout is the seeded random one.  alias_inputs: jobs whose `input` is the same object (at the same in_low)
    read one shared buffer.  placement: a dict that receives the device addresses used (uint64 arrays "input", "prefix", "out") and
    the number of input buffers uploaded ("input_buffers")."""
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(seed)
    n = len(items)
    ins = [bytes(it["input"]) for it in items]
    pres = [bytes(it.get("prefix", b"")) for it in items]
    exs = [bytes(it.get("existing", b"")) for it in items]
    limits = [it.get("limit") if it.get("limit") is not None else (1 << 63) - 1 for it in items]
    caps = []
    for it, ex, lim, d in zip(items, exs, limits, ins):
        cap = it.get("out_cap")
        caps.append(cap if cap is not None else len(ex) + min(lim, 1 << 26) + len(d) + 64)
    explicit_in = in_low is not None or prefix_low is not None
    in_low, prefix_low, out_low_l = _lows(in_low, n, "in_low"), _lows(prefix_low, n, "prefix_low"), _lows(out_low, n, "out_low")
    which, first = _alias_slots(items, in_low, alias_inputs)
    in_bufs = [ins[i] for i in first]
    in_offs, in_total, in_arena = _place([len(d) for d in in_bufs] + [len(p) for p in pres], [in_low[i] for i in first] + prefix_low, rng, dev, explicit_in)
    out_offs, out_total, out_arena = _place(caps, out_low_l, rng, dev, out_low is not None)
    nb = len(in_bufs)
    h_in = np.full(in_total, in_poison, dtype=np.uint8)
    for o, d in zip(in_offs, in_bufs + pres):
        h_in[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    h_out = np.full(out_total, OUT_POISON, dtype=np.uint8)
    for o, ex in zip(out_offs, exs):
        h_out[o:o + len(ex)] = np.frombuffer(ex, dtype=np.uint8)
    d_in = _upload(h_in, in_arena, dev)
    d_out = _upload(h_out, out_arena, dev)
    del h_out
    j = np.zeros(n, dtype=device.DJOB)
    j["input"] = np.uint64(d_in.data_ptr()) + np.array([in_offs[w] for w in which], dtype=np.uint64)
    j["input_len"] = [len(d) for d in ins]
    j["prefix"] = np.uint64(d_in.data_ptr()) + np.array(in_offs[nb:], dtype=np.uint64)
    j["prefix_len"] = [len(p) for p in pres]
    j["out"] = np.uint64(d_out.data_ptr()) + np.array(out_offs, dtype=np.uint64)
    j["out_existing_len"] = [len(e) for e in exs]
    j["out_cap"] = caps
    j["output_limit"] = limits
    if placement is not None:
        placement.update(input=j["input"].copy(), prefix=j["prefix"].copy(), out=j["out"].copy(), input_buffers=nb)
    d_j = device.to_device(j, dev)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    device.decompress_batch(d_j, d_res, n, max_input_len=max_input_len)
    torch.cuda.synchronize()
    res = device.results_to_host(d_res, n)
    got = d_out.cpu().numpy()
    # every byte outside the jobs' [out, out + cap) must still be poison
    mask = np.ones(out_total, dtype=bool)
    for o, cap in zip(out_offs, caps):
        mask[o:o + cap] = False
    bad = np.nonzero(mask & (got != OUT_POISON))[0]
    detail = ""
    if len(bad):
        first_bad = int(bad[0])
        k = int(np.searchsorted(np.array(out_offs), first_bad, side="right")) - 1
        where = "behind" if k >= 0 and first_bad >= out_offs[k] + caps[k] else "in front of"
        kk = k if where == "behind" else k + 1
        detail = f"{len(bad)} poisoned bytes overwritten; first at arena offset {first_bad}: {where} job {kk}'s output slot"
    # the input arena is read-only for the codec
    if not np.array_equal(d_in.cpu().numpy(), h_in):
        detail += " | the INPUT arena was written to"
    out = []
    for i in range(n):
        ln = int(min(res["out_len"][i], caps[i]))
        out.append((int(res["status"][i]), got[out_offs[i]:out_offs[i] + ln].tobytes()))
    return out, detail == "", detail


def compress_guarded(items, in_poison, seed=0, kinds=None, in_low=None, out_low=None, placement=None):
    """items as ffi.compress_blocks_host (input, cursor, kind, out_cap; fresh tables only).  Returns (results, zones_ok, detail).
    in_low / out_low / placement as in decompress_guarded."""
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(seed)
    n = len(items)
    ins = [bytes(it["input"]) for it in items]
    caps = [it["out_cap"] if it.get("out_cap") is not None else len(d) + len(d) // 255 + 64 for it, d in zip(items, ins)]
    in_offs, in_total, in_arena = _place([len(d) for d in ins], _lows(in_low, n, "in_low"), rng, dev, in_low is not None)
    out_offs, out_total, out_arena = _place(caps, _lows(out_low, n, "out_low"), rng, dev, out_low is not None)
    h_in = np.full(in_total, in_poison, dtype=np.uint8)
    for o, d in zip(in_offs, ins):
        h_in[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    d_in = _upload(h_in, in_arena, dev)
    if out_arena is None:
        d_out = torch.full((out_total,), OUT_POISON, dtype=torch.uint8, device=dev)
    else:
        d_out = out_arena.fill_(OUT_POISON)
    j = np.zeros(n, dtype=device.CJOB)
    j["input"] = np.uint64(d_in.data_ptr()) + np.array(in_offs, dtype=np.uint64)
    j["input_len"] = [len(d) for d in ins]
    j["cursor"] = [it.get("cursor", 0) for it in items]
    j["out"] = np.uint64(d_out.data_ptr()) + np.array(out_offs, dtype=np.uint64)
    j["out_cap"] = caps
    j["table_kind"] = [it.get("kind", ffi.TABLE_U32) for it in items]
    if placement is not None:
        placement.update(input=j["input"].copy(), out=j["out"].copy())
    if kinds is None:
        kinds = 0
        for it in items:
            kinds |= ffi.KINDS_U16 if it.get("kind", ffi.TABLE_U32) == ffi.TABLE_U16 else ffi.KINDS_U32
    d_j = device.to_device(j, dev)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    device.compress_batch(d_j, d_res, n, kinds)
    torch.cuda.synchronize()
    res = device.results_to_host(d_res, n)
    got = d_out.cpu().numpy()
    mask = np.ones(out_total, dtype=bool)
    for o, cap in zip(out_offs, caps):
        mask[o:o + cap] = False
    bad = np.nonzero(mask & (got != OUT_POISON))[0]
    detail = ""
    if len(bad):
        first = int(bad[0])
        k = int(np.searchsorted(np.array(out_offs), first, side="right")) - 1
        detail = f"{len(bad)} poisoned bytes overwritten; first at arena offset {first}, near job {k}'s output slot (cap {caps[max(k, 0)]})"
    if not np.array_equal(d_in.cpu().numpy(), h_in):
        detail += " | the INPUT arena was written to"
    out = []
    for i in range(n):
        st = int(res["status"][i])
        out.append((st, got[out_offs[i]:out_offs[i] + int(res["out_len"][i])].tobytes() if st == ffi.OK else b""))
    return out, detail == "", detail


def _first_diff(a, b):
    m = min(len(a), len(b))
    x = np.nonzero(np.frombuffer(a, dtype=np.uint8, count=m) != np.frombuffer(b, dtype=np.uint8, count=m))[0]
    return int(x[0]) if len(x) else m


def check_decompress(items, expect=None, label="", max_input_len=None, in_low=None, prefix_low=None, out_low=None, alias_inputs=False,
                     placement=None):
    """Both IN-poisons: zones intact, statuses and Ok bytes identical under both, and (when given) equal to `expect`
    [(status, bytes) from the oracle].  Returns the results.  in_low / prefix_low / out_low / alias_inputs as in
    decompress_guarded; `placement`, a list, receives one dict of device addresses per run."""
    kw = dict(max_input_len=max_input_len, in_low=in_low, prefix_low=prefix_low, out_low=out_low, alias_inputs=alias_inputs)
    pa, pb = {}, {}
    ra, ok_a, da = decompress_guarded(items, 0x00, seed=1, placement=pa, **kw)
    rb, ok_b, db = decompress_guarded(items, 0xFF, seed=2, placement=pb, **kw)
    if placement is not None:
        placement += [pa, pb]

    def at(i):
        return f"job {i} (input & 15 = {int(pa['input'][i]) & 15}, out & 15 = {int(pa['out'][i]) & 15})"
    assert ok_a, f"{label}: red zone violated (input poison 0x00): {da}"
    assert ok_b, f"{label}: red zone violated (input poison 0xFF): {db}"
    for i, ((sa, ba), (sb, bb)) in enumerate(zip(ra, rb)):
        assert sa == sb, f"{label}: {at(i)} status depends on the bytes behind input_len ({sa} vs {sb})"
        if sa == 0:
            assert ba == bb, f"{label}: {at(i)} output depends on the bytes behind input_len"
    if expect is not None:
        for i, ((s, b), (es, eb)) in enumerate(zip(ra, expect)):
            assert s == es, f"{label}: {at(i)} status {s}, oracle {es}"
            if s == 0:
                assert b == eb, f"{label}: {at(i)} bytes differ from the oracle's, first at output offset {_first_diff(b, eb)} of {len(eb)}"
    return ra


def check_compress(items, expect=None, label="", in_low=None, out_low=None, placement=None):
    pa, pb = {}, {}
    ra, ok_a, da = compress_guarded(items, 0x00, seed=3, in_low=in_low, out_low=out_low, placement=pa)
    rb, ok_b, db = compress_guarded(items, 0xFF, seed=4, in_low=in_low, out_low=out_low, placement=pb)
    if placement is not None:
        placement += [pa, pb]
    assert ok_a, f"{label}: red zone violated (input poison 0x00): {da}"
    assert ok_b, f"{label}: red zone violated (input poison 0xFF): {db}"
    for i, (a, b) in enumerate(zip(ra, rb)):
        assert a == b, f"{label}: job {i} result depends on the bytes behind input_len"
    if expect is not None:
        for i, ((s, b), (es, eb)) in enumerate(zip(ra, expect)):
            assert s == es and (s != 0 or b == eb), (f"{label}: job {i} (input & 15 = {int(pa['input'][i]) & 15}, out & 15 = "
                                                      f"{int(pa['out'][i]) & 15}) differs from the oracle ({s} vs {es})")
    return ra
