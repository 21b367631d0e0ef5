"""The segmented decompress pipeline (lz4_seg_*.hip) stage by stage on the built edges of seg_stage_cases.py, whose reach
test_seg_stage_cases_cpu.py proves without a GPU.  For each ring (LZF_SEG_RING = 32, 64, 128 KiB) a child process runs lzf_debug_seg
(analysis library, min_in = 0) up to the seam stage (3), the scan (5), the records stage (6) and the resolve stage (8), the outputs at address
residues 0 and 9, and compares what the stages left with the host model: chunk and tile counts, every chunk's exit, vfrom and bit row, the stitched
token map, the tiles' first batch and first output byte, every record word for word (padding included), the dependency levels (equal where
the model is exact, within its bounds elsewhere), the literals in place after the records stage and nothing else written, then done / status /
out_len / bytes and untouched poison around every output.  A damaged case fails in the stage the model names, not earlier, is never done, and
the pipeline reports no result for it.  The same corpus goes through the forced pipeline under each ring and (the seam cases) through the forced
fed path, whole and in three pieces: statuses always, out_len and bytes of every Ok job are the oracle's (the ABI leaves out_len open on an
error); the red-zone harness runs the intact cases once per ring."""
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
import seg_stage_cases as S  # noqa: E402
from test_gpu_parse_staging import PATHS  # noqa: E402

pytestmark = pytest.mark.gpu

POISON, RES_POISON = 0xEE, 0x5A
GUARD = 64                                  # poisoned bytes looked at in front of and behind every output
STAGE_NO = {"seam": 3, "tilesum": 4, "scan": 5, "records": 6}
UPTO = (3, 5, 6, 8)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """The cases, their models and what the oracle makes of them, once for the module (the children read the file)."""
    cases, models = S.all_cases(), S.models()
    exp = [o.decompress_raw(c["input"], limit=c["limit"], cap=c["out_cap"]) for c in cases]
    for c, e in zip(cases, exp):
        assert e[0] == c["status"] and (e[0] != S.OK or e[1] == c["output"]), c["name"]
    for m in models:
        m.P.memo = {}                       # (the token cache is not needed again)
    path = tmp_path_factory.mktemp("seg_stages") / "corpus.pkl"
    path.write_bytes(pickle.dumps((cases, models, exp)))
    return str(path)


def _child(what, corpus, *args, **env):
    from rust_lz_fear_amd import build
    e = dict(os.environ, LZF_LIB_PATH=build.build_analysis_library(), SEG_STAGES_CORPUS=corpus, **env)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what, *args], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "seg stages ok" in r.stdout, r.stdout[-2000:]
    print(r.stdout.strip().splitlines()[-1], f"[{time.time() - t0:.1f} s]")
    return r.stdout


@pytest.mark.parametrize("ring", S.RINGS)
def test_stage_dumps_equal_the_model(corpus, ring):
    _child("dumps", corpus, LZF_SEG_RING=str(ring))


@pytest.mark.parametrize("ring", S.RINGS)
def test_forced_pipeline_decodes_like_the_oracle(corpus, ring):
    _child("decode", corpus, "all", "segmented", LZF_DECOMPRESS_KERNEL="seg", LZF_SEG_MIN_IN="0", LZF_SEG_RING=str(ring))


@pytest.mark.parametrize("path", ["fed", "fed3"])
def test_seam_cases_through_the_fed_path(corpus, path):
    _child("decode", corpus, "seam", "bitmap-fed", **PATHS[path])


@pytest.mark.parametrize("ring", S.RINGS)
def test_red_zones(corpus, ring):
    _child("redzone", corpus, LZF_DECOMPRESS_KERNEL="seg", LZF_SEG_MIN_IN="0", LZF_SEG_RING=str(ring))


# ---------------------------------------------------------------------------------------------------------------- the children
def _load():
    with open(os.environ["SEG_STAGES_CORPUS"], "rb") as f:
        return pickle.load(f)


def _debug_seg():
    fn = ffi.lib().lzf_debug_seg
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 7 + [C.c_uint64, C.c_void_p]
    return fn


def run_debug_seg(cases, rb, upto, max_recs, min_in=0):
    """lzf_debug_seg over `cases` with every output at address residue rb; max_recs: records of the arena to copy out.  Returns a dict of the
    host copies."""
    import torch
    from rust_lz_fear_amd import device
    n = len(cases)
    in_off = np.zeros(n, np.int64); out_off = np.zeros(n, np.int64)
    ti, to = 0, 256
    for i, c in enumerate(cases):
        in_off[i] = ti; ti += (len(c["input"]) + 255) // 256 * 256 + 3                  # odd input alignments
        out_off[i] = to + rb; to += (c["out_cap"] + 2 * GUARD + 16 + 255) // 256 * 256
    h_in = np.zeros(ti + 64, np.uint8)
    for a, c in zip(in_off, cases):
        h_in[a:a + len(c["input"])] = np.frombuffer(c["input"], np.uint8)
    d_in = torch.from_numpy(h_in).cuda()
    d_out = torch.full((to + 256,), POISON, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 256 == 0
    dj = np.zeros(n, dtype=device.DJOB)
    dj["input"] = np.uint64(d_in.data_ptr()) + in_off.astype(np.uint64)
    dj["input_len"] = [len(c["input"]) for c in cases]
    dj["out"] = np.uint64(d_out.data_ptr()) + out_off.astype(np.uint64)
    dj["out_cap"] = [c["out_cap"] for c in cases]
    dj["output_limit"] = [c["limit"] for c in cases]
    assert ((dj["out"] & 15) == rb).all()
    d_dj = device.to_device(dj, "cuda")
    d_res = torch.full((n * device.RES.itemsize,), RES_POISON, dtype=torch.uint8, device="cuda")
    fn = _debug_seg()
    geom = np.zeros(4, np.uint32)
    ffi.check(fn(d_dj.data_ptr(), d_res.data_ptr(), n, min_in, 1, None, None, None, None, None, None, None, 0, geom.ctypes.data))
    maxch, maxtile, cw, rec_cap = (int(x) for x in geom)
    assert cw == S.CHUNK // 32
    st = np.zeros(n, S.SEGJOB)
    bits = np.zeros((n, maxch, cw), np.uint32)
    xexit = np.zeros((n, maxch), np.uint32); vfrom = np.zeros((n, maxch), np.uint32)
    ttok = np.zeros((n, maxtile), np.uint32); tout = np.zeros((n, maxtile), np.uint32)
    recs = np.zeros((min(rec_cap, max_recs), 4), np.uint32)
    d_out.fill_(POISON); d_res.fill_(RES_POISON)
    torch.cuda.synchronize()
    ffi.check(fn(d_dj.data_ptr(), d_res.data_ptr(), n, min_in, upto, st.ctypes.data, bits.ctypes.data, xexit.ctypes.data, vfrom.ctypes.data,
                 ttok.ctypes.data, tout.ctypes.data, recs.ctypes.data, recs.nbytes, geom.ctypes.data))
    return dict(st=st, bits=bits, xexit=xexit, vfrom=vfrom, tile_tok=ttok, tile_out=tout, recs=recs, rec_cap=rec_cap, maxch=maxch, maxtile=maxtile,
                res_raw=d_res.cpu().numpy().copy(), res=device.results_to_host(d_res, n).copy(), out=d_out.cpu().numpy(), out_off=out_off)


def check_dump(cases, models, d, R, rb, upto, stats):
    """Everything lzf_debug_seg left behind at `upto` against the model.  Returns the messages of what differs."""
    msgs = []
    spans = []
    for i, (c, m) in enumerate(zip(cases, models)):
        say = lambda text: msgs.append(f"[{c['name']}] R {R} rb {rb} upto {upto}: {text}")      # noqa: E731
        s, n = d["st"][i], m.n
        if not s["eligible"]:
            say("not eligible"); continue
        if int(s["nch"]) != m.nch or int(s["ntile"]) != m.ntile:
            say(f"nch {s['nch']} ntile {s['ntile']}, model {m.nch} {m.ntile}")
            continue
        gives = m.gives_up
        failed = gives is not None and STAGE_NO[gives] <= upto
        if int(s["failed"]) != int(failed):
            say(f"failed = {s['failed']}, model: gives up in {gives}")
            continue
        raw = d["res_raw"][i * 16:(i + 1) * 16]
        off = int(d["out_off"][i])
        seam = m.seam
        # ---- parse and seam: every chunk's exit, vfrom, the stitched map
        upto_h = m.nch if not seam.failed else max(seam.walks)           # (a walk that fails leaves the chunks from there on open)
        for h in range(m.nch):
            if int(d["xexit"][i, h]) != seam.xexit[h]:
                say(f"exit of chunk {h}: {d['xexit'][i, h]}, model {seam.xexit[h]}"); break
            if h < upto_h and int(d["vfrom"][i, h]) != seam.vfrom[h]:
                say(f"vfrom of chunk {h}: {d['vfrom'][i, h]:#x}, model {seam.vfrom[h]:#x} ({seam.outcome[h]})"); break
        rows = np.stack([np.packbits(seam.marks[h], bitorder="little").view(np.uint32) for h in range(m.nch)])
        bad = np.nonzero((d["bits"][i, :m.nch] != rows).any(axis=1))[0]
        if len(bad):                                                     # (a walked chunk's marks are rewritten from its overlap to the merge)
            say(f"the bit rows of {len(bad)} chunks differ from the model's, first chunk {int(bad[0])} ({seam.outcome[int(bad[0])]})")
        if not seam.failed:
            got = S.device_token_map(n, m.nch, d["vfrom"][i], d["bits"][i])
            diff = np.nonzero(got != seam.stitched())[0]
            if len(diff):
                say(f"token map differs at {len(diff)} positions, first {int(diff[0])}")
            stats["chunks"] += m.nch
        ly = m.layout
        # ---- tiles and scan
        if upto >= 5 and ly is not None and gives not in ("seam", "tilesum"):
            for name, got, exp in (("tile_tok", d["tile_tok"][i, :m.ntile], ly.tile_tok), ("tile_out", d["tile_out"][i, :m.ntile], ly.tile_out)):
                bad = np.nonzero(got.astype(np.int64) != exp)[0]
                if len(bad):
                    say(f"{name} differs at {len(bad)} tiles, first {int(bad[0])}: {int(got[bad[0]])}, model {int(exp[bad[0]])}")
            if not failed and (int(s["ntok"]) != ly.ntok or int(s["outb"]) != ly.outb):
                say(f"ntok {s['ntok']} outb {s['outb']}, model {ly.ntok} {ly.outb}")
        allotted = int(s["ntok"]) != 0 or int(s["rec_off"]) != 0
        if (upto < 5 or gives in ("seam", "tilesum", "scan")) and allotted:
            say(f"records allotted (ntok {s['ntok']}, rec_off {s['rec_off']})")
        if upto >= 5 and allotted:
            spans.append((int(s["rec_off"]), int(s["ntok"]) + 64))
        # ---- records
        out = d["out"][off:off + len(c.get("output", b""))]
        if upto >= 6 and not failed:
            r0 = int(s["rec_off"])
            if r0 + ly.ntok > len(d["recs"]):
                say(f"records at {r0} + {ly.ntok}: beyond the host copy"); continue
            rm, nrec, nex, nbd = S.check_records(ly, d["recs"][r0:r0 + ly.ntok], R, rb)
            for text in rm:
                say(text)
            stats["records"] += nrec; stats["exact"] += nex; stats["bounded"] += nbd
        if upto in (6,) and not failed and c["status"] == S.OK:
            # the literals are in place and nothing else is written
            lit = np.zeros(ly.outb, bool)
            act = np.nonzero(ly.act & (ly.L > 0))[0]
            for a, b in zip(ly.lo[act].tolist(), ly.mo[act].tolist()):
                lit[a:b] = True
            want = np.where(lit, np.frombuffer(c["output"], np.uint8), POISON)
            bad = np.nonzero(out != want)[0]
            if len(bad):
                say(f"after the records stage {len(bad)} output bytes are neither their literal nor untouched, first {int(bad[0])}")
        if upto < 6 and (d["out"][off - GUARD:off + c["out_cap"] + GUARD] != POISON).any():
            say("output written before the records stage")
        # ---- resolve
        done = upto >= 8 and gives is None
        if int(s["done"]) != int(done):
            say(f"done = {s['done']}" + (": the resolve pair gave the job up" if done else ""))
        if not done:
            if (raw != RES_POISON).any():
                say("a result was reported")
        else:
            res = d["res"][i]
            if int(res["status"]) != 0 or int(res["out_len"]) != len(c["output"]):
                say(f"status {res['status']} out_len {res['out_len']}, oracle 0 {len(c['output'])}")
            elif out.tobytes() != c["output"]:
                w = np.nonzero(out != np.frombuffer(c["output"], np.uint8))[0]
                say(f"output differs at {len(w)} bytes, first {int(w[0])}, last {int(w[-1])}")
        end = off + (len(c["output"]) if c["status"] == S.OK else c["out_cap"])
        if (d["out"][off - GUARD:off] != POISON).any():
            say("bytes in front of the output were written")
        if (d["out"][end:end + GUARD] != POISON).any():
            say("bytes behind the output were written")
    spans.sort()
    for (a, na), (b, _) in zip(spans, spans[1:]):
        if a + na > b:
            msgs.append(f"R {R} rb {rb} upto {upto}: record ranges overlap ({a} + {na} > {b})")
    if spans and spans[-1][0] + spans[-1][1] > d["rec_cap"]:
        msgs.append(f"R {R} rb {rb} upto {upto}: records beyond the arena")
    return msgs


def child_dumps():
    cases, models, _ = _load()
    R = int(os.environ["LZF_SEG_RING"])
    stats = dict(chunks=0, records=0, exact=0, bounded=0)
    msgs = []
    max_recs = sum(m.layout.ntok + 64 for m in models if m.layout is not None)       # (every job that passes the scan takes ntok + 64)
    for rb in S.RESIDUES:
        for upto in UPTO:
            d = run_debug_seg(cases, rb, upto, max_recs)
            msgs += check_dump(cases, models, d, R, rb, upto, stats)
    for text in msgs[:40]:
        print(text)
    assert not msgs, f"{len(msgs)} differences"
    print(f"seg stages ok: ring {R}, {len(cases)} cases x {len(S.RESIDUES)} residues x stages {UPTO}: {stats['chunks']} chunk outcomes, "
          f"{stats['records']} records compared, levels {stats['exact']} exact / {stats['bounded']} bounded")


def _pick(cases, exp, which):
    keep = [i for i, c in enumerate(cases) if which == "all" or c["name"].startswith("seam:") or "seam walk" in c["name"]]
    return [cases[i] for i in keep], [exp[i] for i in keep]


def child_decode(which, prefix):
    cases, _, exp = _load()
    cases, exp = _pick(cases, exp, which)
    items = [dict(input=c["input"], limit=c["limit"], out_cap=c["out_cap"]) for c in cases]
    res = ffi.decompress_blocks_host(items)
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    assert launch.startswith(prefix), launch
    ring = os.environ.get("LZF_SEG_RING")
    assert ring is None or f"<{ring}>" in launch, launch
    nerr = same = 0
    for c, (erc, eout), (rc, out) in zip(cases, exp, res):
        print(f"{c['name']}: status {rc} out_len {len(out)}, oracle {erc} {len(eout)}")
        assert rc == erc, (c["name"], rc, erc)
        if rc == 0:
            assert len(out) == len(eout) and out == eout, c["name"]
        else:                                  # (lzfear_hip.h: out_len is unspecified on an error — counted, not required)
            nerr += 1; same += len(out) == len(eout)
    print(f"seg stages ok: {len(items)} jobs, {nerr} with an error ({same} with the oracle's out_len),", launch)


def child_redzone():
    import redzone
    cases, _, exp = _load()
    keep = [i for i, c in enumerate(cases) if c["status"] == S.OK]
    items = [dict(input=cases[i]["input"], limit=cases[i]["limit"], out_cap=cases[i]["out_cap"]) for i in keep]
    redzone.check_decompress(items, [exp[i] for i in keep], label="seg stages", out_low=[S.RESIDUES[k % 2] for k in range(len(keep))])
    launch = ffi.lib().lzf_last_decompress_launch().decode()
    assert launch.startswith("segmented"), launch
    print("seg stages ok:", len(items), "jobs", launch)


if __name__ == "__main__":
    {"dumps": child_dumps, "decode": child_decode, "redzone": child_redzone}[sys.argv[1]](*sys.argv[2:])
