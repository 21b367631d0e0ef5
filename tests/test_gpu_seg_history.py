"""The segmented decompress pipeline (lz4_seg_*.hip) on jobs WITH HISTORY — existing output and prefixes — stage by stage on the built
edges of seg_history_cases.py, whose reach test_seg_history_cases_cpu.py proves without a GPU.  The conventions are test_gpu_seg_stages.py's:
for each ring (LZF_SEG_RING = 32, 64, 128 KiB) a child process runs lzf_debug_seg (analysis library, min_in = 0) up to the scan (5), the records
stage (6) and the resolve stage (8), the outputs at address residues 0 and 9 and the prefixes at odd ones, and compares what the stages left
with the host model: the tiles' first batch and first output byte (the first tile's is E), ntok and outb, every record word for word, the literals
in place after the records stage and nothing else written — not below out + E, not beyond —, then for every intact case eligible, not failed, DONE
(no case is left to the pair kernel, under any ring or residue), out_len = E + the decoded length, the oracle's bytes, history and prefix as they
were, the poison around every output untouched.  A damaged case fails in the stage the model names, is never done, and the pipeline reports no
result for it.  The corpus then goes through the forced pipeline (statuses always, out_len and bytes of every Ok job are the oracle's) and
the red-zone harness; and the product library decodes linked-block frames and a dictionary frame of 256 KiB blocks through both frame drivers."""
import ctypes as C
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
import seg_history_cases as H  # noqa: E402
import seg_stage_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu

POISON, RES_POISON = 0xEE, 0x5A
GUARD = 64
STAGE_NO = {"scan": 5, "records": 6}
UPTO = (5, 6, 8)
PREFIX_LOW = (1, 3, 5, 7, 9, 11, 13, 15, 2)                # address residues (mod 16) of the prefixes, case by case


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    cases, models = H.all_cases(), H.models()
    exp = [o.decompress_raw(c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"], cap=c["out_cap"]) for c in cases]
    for c, e in zip(cases, exp):
        assert e[0] == c["status"] and (e[0] != S.OK or e[1] == c["output"]), c["name"]
    for m in models:
        m.P.memo = {}
    path = tmp_path_factory.mktemp("seg_history") / "corpus.pkl"
    path.write_bytes(pickle.dumps((cases, models, exp)))
    return str(path)


def _child(what, corpus, *args, analysis=True, **env):
    from rust_lz_fear_amd import build
    e = dict(os.environ, SEG_HISTORY_CORPUS=corpus, **env)
    if analysis:
        e["LZF_LIB_PATH"] = build.build_analysis_library()
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what, *args], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "seg history ok" in r.stdout, r.stdout[-2000:]
    print(r.stdout.strip().splitlines()[-1], f"[{time.time() - t0:.1f} s]")
    return r.stdout


@pytest.mark.parametrize("ring", S.RINGS)
def test_stage_dumps_equal_the_model(corpus, ring):
    _child("dumps", corpus, LZF_SEG_RING=str(ring))


@pytest.mark.parametrize("ring", S.RINGS)
def test_forced_pipeline_decodes_like_the_oracle(corpus, ring):
    _child("decode", corpus, LZF_DECOMPRESS_KERNEL="seg", LZF_SEG_MIN_IN="0", LZF_SEG_RING=str(ring))


@pytest.mark.parametrize("ring", S.RINGS)
def test_red_zones(corpus, ring):
    _child("redzone", corpus, LZF_DECOMPRESS_KERNEL="seg", LZF_SEG_MIN_IN="0", LZF_SEG_RING=str(ring))


def test_linked_and_dictionary_frames_through_both_drivers(corpus):
    _child("frames", corpus, analysis=False)


# ---------------------------------------------------------------------------------------------------------------- the children
def _load():
    with open(os.environ["SEG_HISTORY_CORPUS"], "rb") as f:
        return pickle.load(f)


def _debug_seg():
    fn = ffi.lib().lzf_debug_seg
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 7 + [C.c_uint64, C.c_void_p]
    return fn


def run_debug_seg(cases, rb, upto, max_recs):
    """lzf_debug_seg over `cases`: every output at address residue rb with its existing bytes in place and poison around it, every prefix at
    an odd residue of its own.  Returns a dict of the host copies."""
    import torch
    from rust_lz_fear_amd import device
    n = len(cases)
    in_off = np.zeros(n, np.int64); pre_off = np.zeros(n, np.int64); out_off = np.zeros(n, np.int64)
    ti, to = 0, 256
    for i, c in enumerate(cases):
        in_off[i] = ti; ti += (len(c["input"]) + 255) // 256 * 256 + 3
    ti = (ti + 255) // 256 * 256
    for i, c in enumerate(cases):
        pre_off[i] = ti + PREFIX_LOW[i % len(PREFIX_LOW)]; ti += (len(c["prefix"]) + 16 + 255) // 256 * 256
        out_off[i] = to + rb; to += (c["out_cap"] + 2 * GUARD + 16 + 255) // 256 * 256
    h_in = np.full(ti + 64, 0xC3, np.uint8)
    for a, p, c in zip(in_off, pre_off, cases):
        h_in[a:a + len(c["input"])] = np.frombuffer(c["input"], np.uint8)
        h_in[p:p + len(c["prefix"])] = np.frombuffer(c["prefix"], np.uint8)
    h_out = np.full(to + 256, POISON, np.uint8)
    for a, c in zip(out_off, cases):
        h_out[a:a + len(c["existing"])] = np.frombuffer(c["existing"], np.uint8)
    d_in = torch.from_numpy(h_in).cuda()
    d_out = torch.from_numpy(h_out).cuda()
    assert d_out.data_ptr() % 256 == 0 and d_in.data_ptr() % 256 == 0
    dj = np.zeros(n, dtype=device.DJOB)
    dj["input"] = np.uint64(d_in.data_ptr()) + in_off.astype(np.uint64)
    dj["input_len"] = [len(c["input"]) for c in cases]
    dj["prefix"] = np.uint64(d_in.data_ptr()) + pre_off.astype(np.uint64)
    dj["prefix_len"] = [len(c["prefix"]) for c in cases]
    dj["out"] = np.uint64(d_out.data_ptr()) + out_off.astype(np.uint64)
    dj["out_existing_len"] = [len(c["existing"]) for c in cases]
    dj["out_cap"] = [c["out_cap"] for c in cases]
    dj["output_limit"] = [c["limit"] for c in cases]
    assert ((dj["out"] & 15) == rb).all() and (dj["prefix"] & 1).sum() >= n // 2
    d_dj = device.to_device(dj, "cuda")
    d_res = torch.full((n * device.RES.itemsize,), RES_POISON, dtype=torch.uint8, device="cuda")
    fn = _debug_seg()
    geom = np.zeros(4, np.uint32)
    ffi.check(fn(d_dj.data_ptr(), d_res.data_ptr(), n, 0, 1, None, None, None, None, None, None, None, 0, geom.ctypes.data))
    maxch, maxtile, cw, rec_cap = (int(x) for x in geom)
    st = np.zeros(n, S.SEGJOB)
    ttok = np.zeros((n, maxtile), np.uint32); tout = np.zeros((n, maxtile), np.uint32)
    recs = np.zeros((min(rec_cap, max_recs), 4), np.uint32)
    d_out.copy_(torch.from_numpy(h_out)); d_res.fill_(RES_POISON)
    torch.cuda.synchronize()
    ffi.check(fn(d_dj.data_ptr(), d_res.data_ptr(), n, 0, upto, st.ctypes.data, None, None, None, ttok.ctypes.data, tout.ctypes.data,
                 recs.ctypes.data, recs.nbytes, geom.ctypes.data))
    return dict(st=st, tile_tok=ttok, tile_out=tout, recs=recs, rec_cap=rec_cap, res_raw=d_res.cpu().numpy().copy(),
                res=device.results_to_host(d_res, n).copy(), out=d_out.cpu().numpy(), out_off=out_off,
                inputs_intact=bool((d_in.cpu().numpy() == h_in).all()))


def check_dump(cases, models, d, R, rb, upto, stats):
    msgs = []
    if not d["inputs_intact"]:
        msgs.append(f"R {R} rb {rb} upto {upto}: the inputs or prefixes were written to")
    for i, (c, m) in enumerate(zip(cases, models)):
        say = lambda text: msgs.append(f"[{c['name']}] R {R} rb {rb} upto {upto}: {text}")      # noqa: E731
        s, ly, E = d["st"][i], m.layout, m.E
        if not s["eligible"]:
            say("not eligible"); continue
        if int(s["nch"]) != m.nch or int(s["ntile"]) != m.ntile:
            say(f"nch {s['nch']} ntile {s['ntile']}, model {m.nch} {m.ntile}"); continue
        gives = m.gives_up
        failed = gives is not None and STAGE_NO[gives] <= upto
        if int(s["failed"]) != int(failed):
            say(f"failed = {s['failed']}, model: gives up in {gives}"); continue
        raw = d["res_raw"][i * 16:(i + 1) * 16]
        off = int(d["out_off"][i])
        for name, got, exp in (("tile_tok", d["tile_tok"][i, :m.ntile], ly.tile_tok), ("tile_out", d["tile_out"][i, :m.ntile], ly.tile_out)):
            bad = np.nonzero(got.astype(np.int64) != exp)[0]
            if len(bad):
                say(f"{name} differs at {len(bad)} tiles, first {int(bad[0])}: {int(got[bad[0]])}, model {int(exp[bad[0]])}")
        if gives != "scan" and (int(s["ntok"]) != ly.ntok or int(s["outb"]) != ly.outb):
            say(f"ntok {s['ntok']} outb {s['outb']}, model {ly.ntok} {ly.outb}")
        if gives == "scan" and (int(s["ntok"]) != 0 or int(s["rec_off"]) != 0):
            say("records allotted")
        ok_case = c["status"] == S.OK
        total = len(c["output"]) if ok_case else 0
        out = d["out"][off:off + total]
        if upto >= 6 and not failed:
            r0 = int(s["rec_off"])
            if r0 + ly.ntok > len(d["recs"]):
                say(f"records at {r0} + {ly.ntok}: beyond the host copy"); continue
            rm, nrec, nex, nbd = S.check_records(ly, d["recs"][r0:r0 + ly.ntok], R, rb)
            for text in rm:
                say(text)
            stats["records"] += nrec; stats["exact"] += nex; stats["bounded"] += nbd
        # the history is what it was, whatever the stage
        if d["out"][off:off + E].tobytes() != c["existing"]:
            say("the existing output was changed")
        if upto == 6 and ok_case:
            lit = np.zeros(ly.outb, bool)
            act = np.nonzero(ly.act & (ly.L > 0))[0]
            for a, b in zip(ly.lo[act].tolist(), ly.mo[act].tolist()):
                lit[a:b] = True
            want = np.where(lit, np.frombuffer(c["output"], np.uint8), POISON)
            bad = np.nonzero(out[E:] != want[E:])[0]
            if len(bad):
                say(f"after the records stage {len(bad)} output bytes are neither their literal nor untouched, first {E + int(bad[0])}")
        if upto < 6 and (d["out"][off + E:off + c["out_cap"] + GUARD] != POISON).any():
            say("output written before the records stage")
        done = upto >= 8 and gives is None
        if int(s["done"]) != int(done):
            say(f"done = {s['done']}" + (": the resolve pair left the job to the pair kernel" if done else ""))
        if not done:
            if (raw != RES_POISON).any():
                say("a result was reported")
        else:
            res = d["res"][i]
            if int(res["status"]) != 0 or int(res["out_len"]) != total:
                say(f"status {res['status']} out_len {res['out_len']}, oracle 0 {total}")
            elif out.tobytes() != c["output"]:
                w = np.nonzero(out != np.frombuffer(c["output"], np.uint8))[0]
                say(f"output differs at {len(w)} bytes, first {int(w[0])}, last {int(w[-1])} (E {E})")
            stats["done"] += 1
        end = off + (total if ok_case else c["out_cap"])
        if (d["out"][off - GUARD:off] != POISON).any():
            say("bytes in front of the output were written")
        if (d["out"][end:end + GUARD] != POISON).any():
            say("bytes behind the output were written")
    return msgs


def child_dumps():
    cases, models, _ = _load()
    R = int(os.environ["LZF_SEG_RING"])
    stats = dict(records=0, exact=0, bounded=0, done=0)
    msgs = []
    max_recs = sum(m.layout.ntok + 64 for m in models)
    intact = sum(c["status"] == S.OK for c in cases)
    for rb in S.RESIDUES:
        for upto in UPTO:
            d = run_debug_seg(cases, rb, upto, max_recs)
            msgs += check_dump(cases, models, d, R, rb, upto, stats)
    for text in msgs[:40]:
        print(text)
    assert not msgs, f"{len(msgs)} differences"
    assert stats["done"] == intact * len(S.RESIDUES), (stats["done"], intact)
    print(f"seg history ok: ring {R}, {len(cases)} cases ({intact} intact, all done by the pipeline) x {len(S.RESIDUES)} residues x stages {UPTO}: "
          f"{stats['records']} records compared, levels {stats['exact']} exact / {stats['bounded']} bounded")


def _items(cases):
    return [dict(input=c["input"], prefix=c["prefix"], existing=c["existing"], limit=c["limit"], out_cap=c["out_cap"]) for c in cases]


def child_decode():
    cases, _, exp = _load()
    res = ffi.decompress_blocks_host(_items(cases))
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    assert launch.startswith("segmented") and f"<{os.environ['LZF_SEG_RING']}>" in launch, launch
    nerr = 0
    for c, (erc, eout), (rc, out) in zip(cases, exp, res):
        print(f"{c['name']}: status {rc} out_len {len(out)}, oracle {erc} {len(eout)}")
        assert rc == erc, (c["name"], rc, erc)
        if rc == 0:
            assert len(out) == len(eout) and out == eout, c["name"]
        else:
            nerr += 1
    print(f"seg history ok: {len(cases)} jobs, {nerr} with an error,", launch)


def child_redzone():
    import redzone
    cases, _, exp = _load()
    keep = [i for i, c in enumerate(cases) if c["status"] == S.OK]
    redzone.check_decompress(_items([cases[i] for i in keep]), [exp[i] for i in keep], label="seg history",
                             out_low=[S.RESIDUES[k % 2] for k in range(len(keep))], prefix_low=[PREFIX_LOW[k % len(PREFIX_LOW)] for k in range(len(keep))])
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    assert launch.startswith("segmented"), launch
    print("seg history ok:", len(keep), "jobs", launch)


def frame_blocks(frame):
    """(position of the data, size, stored) of every block of an LZ4 frame with a dictionary id or not, no content size."""
    flg = frame[4]
    p = 4 + 2 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0) + 1
    out = []
    while True:
        w = int.from_bytes(frame[p:p + 4], "little"); p += 4
        if w == 0:
            return out
        out.append((p, w & 0x7FFFFFFF, bool(w >> 31)))
        p += (w & 0x7FFFFFFF) + (4 if flg & 16 else 0)


def child_frames():
    import torch
    from rust_lz_fear_amd import framed, synth
    BS = 256 << 10
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()      # noqa: E731
    dct = synth.gen_text_zipf(3, 65536).tobytes()
    texts = [synth.gen_text_zipf(10 + k, 5 * BS).tobytes() for k in range(4)]      # (whole blocks: the last launch of a lock-step run is of large blocks too)
    linked = [o.frame_compress(t, o.make_settings(block_size=BS, independent_blocks=False))[1] for t in texts[:3]]
    dfr = o.frame_compress(texts[3], o.make_settings(block_size=BS, dictionary=dct, dictionary_id=7))[1]
    for f in linked + [dfr]:
        bl = frame_blocks(f)
        assert len(bl) == 5 and all(sz >= (64 << 10) and not stored for _, sz, stored in bl), [b[1:] for b in bl]     # inside the pipeline's window
    # the third block of a linked frame damaged: a sequence of no literals and offset 0 at its start
    bad = bytearray(linked[0]); p3 = frame_blocks(linked[0])[2][0]; bad[p3:p3 + 3] = b"\x00\x00\x00"
    bad = bytes(bad)
    erc, eout, eused = o.frame_decompress(bad)
    assert erc != 0 and len(eout) == 2 * BS and eout == texts[0][:2 * BS], (erc, len(eout))
    for frames, d in ((linked + [bad], b""), ([dfr], dct)):
        exp = [o.frame_decompress(f, dictionary=d) for f in frames]
        got = framed.decompress_frames_device([dev(f) for f in frames], dictionary=dev(d) if d else None)
        launch = ffi.lib().lzf_last_decompress_launch().decode()
        got = [(st, t.cpu().numpy().tobytes(), used) for st, t, used in got]
        host = framed.decompress_frames(frames, dictionary=d, caps=[len(e[1]) + BS + 64 for e in exp], with_consumed=True)
        for k, (e, g, h) in enumerate(zip(exp, got, host)):
            assert g[0] == e[0] and g[1] == e[1], (k, g[0], e[0], len(g[1]), len(e[1]))
            assert h[0] == e[0] and h[1] == e[1], (k, h[0], e[0], len(h[1]), len(e[1]))
            if e[0] == 0:
                assert g[2] == e[2] and h[2] == e[2], (k, g[2], h[2], e[2])
        assert exp[0][0] == 0 and exp[0][1] == (texts[0] if not d else texts[3])
        print(f"{len(frames)} frames, dictionary {len(d)}: {launch}")
        assert launch.startswith("segmented"), launch
    print("seg history ok: 3 linked frames + a damaged one, 1 dictionary frame, both drivers")


if __name__ == "__main__":
    {"dumps": child_dumps, "decode": child_decode, "redzone": child_redzone, "frames": child_frames}[sys.argv[1]](*sys.argv[2:])
