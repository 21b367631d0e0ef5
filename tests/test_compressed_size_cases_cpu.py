"""CPU: the cases of tests/compressed_size_cases.py are what they claim to be.  Every expectation comes from the oracle; the census
below reads the oracle's own output (its sequences, statuses and tables) and proves that each class is reached in the reference —
the case meant to end in OutputFull does, the chains' later blocks match into their history, the epoch case crosses 64 KiB with a
live candidate.  The frame-level expectations are the lengths of the oracle's frames."""
import os
import re

import compressed_size_cases as cc
import oracle_ffi as o
from rust_lz_fear_amd import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def by_cls(cls):
    return [c for c in cc.cases() if c["cls"] == cls]


def one(cls):
    (c,) = by_cls(cls)
    return c, cc.expectations(c["name"])


def test_every_class_is_present_and_every_job_has_an_expectation():
    want = {"tiny", "lsic", "repeat256", "caps", "template", "u16", "chain", "epoch", "residues", "big", "mixed", "promise"}
    assert {c["cls"] for c in cc.cases()} == want
    n_jobs = 0
    for c in cc.cases():
        exp = cc.expectations(c["name"])
        assert len(exp) == len(c["calls"])
        for call, (res, tables, plain) in zip(c["calls"], exp):
            assert len(res) == len(call) == len(plain) and set(tables) == set(c["tables"])
            n_jobs += len(call)
            assert max(len(j["input"]) for j in call) <= 5000 * 1024 and sum(len(j["input"]) for j in call) <= 6 << 20
    assert n_jobs == 5394, n_jobs


def test_tiny_inputs():
    c, ((res, _, _),) = one("tiny")
    seen = set()
    for j, (rc, n) in zip(c["calls"][0], res):
        ln, cur = len(j["input"]), j["cursor"]
        seen.add((ln, "end" if cur == ln else "zero" if cur == 0 else "mid", j["kind"]))
        assert rc == o.OK
        assert n == (0 if cur == ln else 1 + ln - cur), (ln, cur, n)          # nothing, or one token and the literals
    for kind in (cc.U32, cc.U16):
        assert {(0, "end", kind), (1, "zero", kind), (1, "end", kind), (12, "zero", kind), (12, "mid", kind), (12, "end", kind),
                (13, "zero", kind), (13, "mid", kind), (13, "end", kind)} <= seen


def test_lsic_edges_are_reached():
    c, ((res, _, plain),) = one("lsic")
    lits, matches = set(), set()
    for (rc, n), out in zip(res, plain):
        assert rc == o.OK and n == len(out)
        first = cc.sequences(out)[0]
        lits.add(first[1]); matches.add(first[3])
    assert {14, 15, 269, 270} <= lits and {18, 19, 273, 274} <= matches
    assert len(res) == 16


def test_repeat256_is_one_match_of_65535_bytes():
    c, ((res, _, plain),) = one("repeat256")
    seqs = cc.sequences(plain[0])
    assert res[0][0] == o.OK and [s[3] for s in seqs] == [65535, 0] and seqs[0][2] == 256


def test_capacities():
    c, ((res, _, plain),) = one("caps")
    exact = len(plain[0])
    assert [j["cap"] for j in c["calls"][0][:4]] == [exact, exact - 1, 0, None]
    assert res[0] == (o.OK, exact) and res[3] == (o.OK, exact)
    assert res[1][0] == o.OUTPUT_FULL and res[2] == (o.OUTPUT_FULL, 0)
    last = cc.sequences(plain[0])[-1]
    assert res[1][1] == last[0] and 0 < last[0] < exact                  # everything in front of the last literals
    assert [r[0] for r in res[4:]] == [o.OUTPUT_FULL, o.OUTPUT_FULL, o.OK] and c["calls"][0][4]["kind"] == cc.U16


def test_template_jobs_match_into_the_dictionary_and_leave_the_template_alone():
    c, ((res, tables, plain),) = one("template")
    assert tables["tmpl"] == c["tables"]["tmpl"]["init"] and any(tables["tmpl"])
    j = c["calls"][0][0]
    assert j["readonly"] and j["cursor"] == len(cc.DICT)
    pos, into_dict = 0, 0
    for s in cc.sequences(plain[0]):
        pos += s[1]
        if s[3] and s[2] > pos:
            into_dict += 1
        pos += s[3]
    assert into_dict >= 1 and res[0][0] == o.OK
    assert res[2] == (o.OK, len(plain[2])) and c["calls"][0][2]["slot"] is None


def test_u16_limits():
    c, ((res, _, _),) = one("u16")
    assert [len(j["input"]) for j in c["calls"][0]] == [65535, 65536]
    assert res[0][0] == o.OK and res[0][1] > 0 and res[1] == (o.CONTRACT, 0)


def test_chains_match_into_their_history_and_carry_their_tables():
    for c in by_cls("chain"):
        exp = cc.expectations(c["name"])
        before = c["tables"]["t"]["init"]
        for k, (call, (res, tables, plain)) in enumerate(zip(c["calls"], exp)):
            assert res[0][0] == o.OK and tables["t"] != before
            before = tables["t"]
            if k == 0:
                continue
            pos, back = 0, 0
            for s in cc.sequences(plain[0]):
                pos += s[1]
                if s[3] and s[2] > pos:
                    back += 1                                            # the source lies in front of the cursor: the block before
                pos += s[3]
            assert back >= 1, (c["name"], k)
        offsets = [int.from_bytes(t["t"][-8:], "little") for _, t, _ in exp]
        assert offsets == ([0, 0] if len(exp) == 2 else [0, 0, 65536])
    assert sorted(len(c["calls"]) for c in by_cls("chain")) == [2, 3]


def test_epoch_cases_cross_64k_with_a_live_candidate():
    c, ((res, _, plain),) = one("epoch")
    assert [len(j["input"]) for j in c["calls"][0]] == [65536 + 40, 131072 + 40]
    for (rc, n), out, edges in zip(res, plain, ((65536,), (65536, 131072))):
        assert rc == o.OK
        pos, crossed = 0, set()
        for s in cc.sequences(out):
            pos += s[1]
            for e in edges:
                if s[3] and pos >= e and pos - s[2] < e:
                    crossed.add(e)
            pos += s[3]
        assert crossed == set(edges)


def test_residues_big_mixed_and_promise():
    c, ((res, _, _),) = one("residues")
    assert sorted(j["in_low"] for j in c["calls"][0] if j["kind"] == cc.U32) == list(range(16))
    assert len({r for r, j in zip(res, c["calls"][0]) if j["kind"] == cc.U32}) == 1
    c, ((res, _, _),) = one("big")
    assert len(res) == 5000 and all(len(j["input"]) == 1024 for j in c["calls"][0]) and all(rc == o.OK and 0 < n < 1024 for rc, n in res)
    c, ((res, _, _),) = one("mixed")
    kinds = [j["kind"] for j in c["calls"][0]]
    assert len(res) == 300 and kinds.count(cc.U16) == 100 and all(rc == o.OK for rc, _ in res)
    c, ((res, tables, _),) = one("promise")
    assert c["kinds"] == cc.KINDS_U32 | cc.KINDS_FRESH_ONLY and c["contract"] == [(0, 2)]
    assert [r[0] for r in res] == [o.OK, o.OK, o.CONTRACT, o.OK] and res[2][1] == 0 and tables["w"] == c["tables"]["w"]["init"]


def test_frame_expectations_are_the_oracle_frames_lengths():
    """4 bytes of EndMark, 4 more with a content checksum, whatever its value; a stored middle block counts its raw length."""
    datas = cc.frame_inputs()
    assert [len(d) for d in datas] == [0, 1, 65536, 65537, 2 * 65536 + 30000]
    n = 0
    for kw, with_size in cc.flag_combos():
        for d in datas:
            got = cc.oracle_frame_len(kw, d, with_size)
            other = cc.oracle_frame_len(dict(kw, content_checksum=not kw["content_checksum"]), d, with_size)
            assert got - other == (4 if kw["content_checksum"] else -4)
            n += 1
    assert n == 160
    kw = dict(independent_blocks=True, block_checksums=False, content_checksum=False, block_size=cc.FRAME_BS)
    rc, frame = o.frame_compress(datas[4], o.make_settings(**kw))
    words = []
    p = 7
    while True:
        w = int.from_bytes(frame[p:p + 4], "little")
        if w == 0:
            break
        words.append(w); p += 4 + (w & 0x7FFFFFFF)
    assert [w >> 31 for w in words] == [0, 1, 0] and words[1] & 0x7FFFFFFF == 65536


def test_the_four_entry_points_are_declared_and_bound():
    hip = open(os.path.join(ROOT, "include", "lzfear_hip.h")).read()
    frame = open(os.path.join(ROOT, "include", "lzfear_frame.h")).read()
    for n in ("lzf_compressed_size_batch", "lzf_compressed_size_batch_host"):
        assert re.search(r"\bint %s\(" % n, hip) and n in ffi.EXPORTS
    for n in ("lzf_frame_compressed_size_device", "lzf_frame_compress_stream_size_device"):
        assert re.search(r"\bint %s\(" % n, frame) and n in ffi.FRAME_EXPORTS
    assert "#define LZFEAR_ABI_VERSION 2" in hip
    rust = open(os.path.join(ROOT, "bindings", "rust", "lz-fear-hip-sys", "src", "lib.rs")).read()
    for n in ("lzf_compressed_size_batch", "lzf_compressed_size_batch_host", "lzf_frame_compressed_size_device", "lzf_frame_compress_stream_size_device"):
        assert "pub fn %s(" % n in rust
    from rust_lz_fear_amd import device, framed
    for f in (device.compressed_size_batch, device.frame_compressed_size, device.stream_compressed_size, ffi.compressed_sizes_host,
              framed.CompressionSettings.compressed_sizes_device):
        assert callable(f)
